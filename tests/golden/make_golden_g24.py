#!/usr/bin/env python3
"""Generate tests/golden/g24_lstm_trainer.npz by RUNNING THE REFERENCE's LSTM-RL value networks under autograd and its ``Trainer``.

TEST INFRASTRUCTURE ONLY.  Run from the repo root:  python tests/golden/make_golden_g24.py

G23's recipe (make_golden_g23.py) for the recurrent family: the reference is imported through make_golden.py's harness; only numbers
(inputs and what the reference produced) and short names are written.  Four small networks whose widths are multiples neither of 32 nor of
8 -- ``lstm_rl.ValueNetwork1`` (H = 19, mlp 41-27-1) and ``ValueNetwork2`` (mlp1 40-33, H = 19, mlp 41-27-1), each on 13 and 15 columns --
seeded by G19's ``draw_weights`` (N(0, 0.25) matrices, N(0, 0.1) biases; recorded as the seed and the SHA-256 of the float32 bytes).
Per network:

  inputs0..2, values0..2   three minibatches (inputs [B, n, cols], values [B, 1]) with (B, n) = (7, 5), (33, 3), (4, 1): uniform numbers
                           in [-1, 1), float32; a sample's rows are evaluated in the order they lie in.  No ReLU of the float64 module
                           reads an input within 2^-16 of zero on them (tests/test_value_lstm_grad_cpu.py checks the fixture for it)
  grads, loss              the reference's .grad of every parameter, flat in the sorted order of the state_dict keys, after
                           MSELoss(model(inputs0), values0).backward() on the seeded weights, and that loss
  trained, average         the parameters (same order) after the reference's ``Trainer.optimize_batch(3)`` at learning rate 0.01 over the
                           three minibatches in order (a preset ``data_loader`` whose ``__iter__`` yields the next minibatch each time it
                           is asked) and the average loss it returned
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402,F401  (imports the reference through _refharness)
from golden_io import save_cases  # noqa: E402
from make_golden_g19 import draw_weights  # noqa: E402
from make_golden_g23 import SHAPES, InOrder, flat  # noqa: E402

F32 = np.float32
H, MLP1, MLP = 19, [40, 33], [41, 27, 1]
NETWORKS = [(1, 13), (1, 15), (2, 13), (2, 15)]


def build(network, cols):
    from crowd_nav.policy import lstm_rl

    if network == 1:
        return lstm_rl.ValueNetwork1(cols, 6, MLP, H)
    return lstm_rl.ValueNetwork2(cols, 6, MLP1, MLP, H)


def generate():
    import torch
    from crowd_nav.utils.trainer import Trainer

    cases = []
    for i, (network, cols) in enumerate(NETWORKS):
        model = build(network, cols)
        seed = 2400 + i
        digest = draw_weights(model, seed, calm=False)
        rng = np.random.default_rng(2430 + i)      # (2424 + i put a ReLU input of lstm2_13 4e-9 from zero: float32 and float64 took it on different sides)
        batches = [(torch.from_numpy(rng.uniform(-1, 1, (B, n, cols)).astype(F32)), torch.from_numpy(rng.uniform(-1, 1, (B, 1)).astype(F32)))
                   for B, n in SHAPES]
        model.zero_grad()
        loss = torch.nn.MSELoss()(model(batches[0][0]), batches[0][1])
        loss.backward()
        grads = flat(model, "grad")
        trainer = Trainer(model, [], torch.device("cpu"), 1)
        trainer.set_learning_rate(0.01)
        trainer.data_loader = InOrder(batches)
        average = trainer.optimize_batch(3)
        sd = model.state_dict()
        case = dict(net=f"lstm{network}_{cols}", network=network, cols=cols, hidden=H, seed=seed, sha256=digest,
                    weights_keys=sorted(str(k) for k in sd), weights_shapes=[list(sd[k].shape) for k in sorted(sd)],
                    grads=grads, loss=float(loss.item()), trained=flat(model, "param"), average=float(average), learning_rate=0.01)
        for b, (x, v) in enumerate(batches):
            case[f"inputs{b}"], case[f"values{b}"] = x.numpy(), v.numpy()
        cases.append(case)
    return cases


if __name__ == "__main__":
    cases = generate()
    for c in cases:
        print(f"{c['net']}: {len(c['grads'])} parameters, loss {c['loss']:.6f}, average of three steps {c['average']:.6f}, "
              f"max |grad| {float(np.max(np.abs(c['grads']))):.3e}, finite: {bool(np.all(np.isfinite(c['trained'])))}")
    path = save_cases("g24_lstm_trainer", cases)
    print("g24_lstm_trainer:", len(cases), "cases ->", path, os.path.getsize(path), "bytes")
