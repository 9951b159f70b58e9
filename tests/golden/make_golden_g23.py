#!/usr/bin/env python3
"""Generate tests/golden/g23_trainer.npz by RUNNING THE REFERENCE's value networks under autograd and its ``Trainer``.

TEST INFRASTRUCTURE ONLY.  Run from the repo root:  python tests/golden/make_golden_g23.py

The reference is imported through make_golden.py's harness; only numbers (inputs and what the reference produced) and short names are
written.  Five small networks whose widths are multiples neither of 32 nor of 8 -- SARL mlp1 (40, 33), mlp2 (33, 20), attention
(36, 30, 1), mlp3 (41, 27, 1) with and without the global state, for 13 and 15 columns, and a CADRL (37, 29, 1) on 13 columns --, seeded
by G19's ``draw_weights`` (N(0, 0.25) matrices, N(0, 0.1) biases, SARL's attention output layer times 0.1 so that the softmax without
maximum subtraction overflows nowhere; recorded as the seed and the SHA-256 of the float32 bytes).  Per network:

  inputs0..2, values0..2   three minibatches (inputs [B, n, cols] -- CADRL: [B, cols], one human's row per sample -- and values [B, 1])
                           with (B, n) = (7, 5), (33, 3), (4, 1): uniform numbers in [-1, 1), float32
  grads, loss              the reference's .grad of every parameter, flat in the sorted order of the state_dict keys, after
                           MSELoss(model(inputs0), values0).backward() on the seeded weights, and that loss
  trained, average         the parameters (same order) after the reference's ``Trainer.optimize_batch(3)`` at learning rate 0.01 over the
                           three minibatches in order -- fed through a preset ``data_loader`` object whose ``__iter__`` yields the next
                           minibatch each time it is asked -- and the average loss it returned
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402,F401  (imports the reference through _refharness)
from golden_io import save_cases  # noqa: E402
from make_golden_g19 import draw_weights  # noqa: E402

F32 = np.float32
SHAPES = ((7, 5), (33, 3), (4, 1))
SARL_WIDTHS = dict(mlp1_dims=[40, 33], mlp2_dims=[33, 20], attention_dims=[36, 30, 1], mlp3_dims=[41, 27, 1])
CADRL_WIDTHS = [37, 29, 1]
NETWORKS = [("sarl", 13, True), ("sarl", 13, False), ("sarl", 15, True), ("sarl", 15, False), ("cadrl", 13, False)]


class InOrder:
    """A preset data_loader: every iter() yields the next minibatch of the list."""

    def __init__(self, batches):
        self.batches, self.at = batches, 0

    def __iter__(self):
        batch = self.batches[self.at]
        self.at += 1
        return iter([batch])


def build(name, cols, with_global):
    from crowd_nav.policy import cadrl, sarl

    if name == "cadrl":
        return cadrl.ValueNetwork(cols, CADRL_WIDTHS)
    return sarl.ValueNetwork(cols, 6, SARL_WIDTHS["mlp1_dims"], SARL_WIDTHS["mlp2_dims"], SARL_WIDTHS["mlp3_dims"], SARL_WIDTHS["attention_dims"],
                             with_global, 1.0, 4)


def flat(model, what):
    sd = dict(model.named_parameters())
    return np.concatenate([(sd[k].grad if what == "grad" else sd[k].detach()).numpy().astype(F32).reshape(-1) for k in sorted(sd)])


def generate():
    import torch
    from crowd_nav.utils.trainer import Trainer

    cases = []
    for i, (name, cols, with_global) in enumerate(NETWORKS):
        model = build(name, cols, with_global)
        seed = 2300 + i
        digest = draw_weights(model, seed, calm=name == "sarl")
        rng = np.random.default_rng(2323 + i)
        batches = []
        for B, n in SHAPES:
            shape = (B, cols) if name == "cadrl" else (B, n, cols)
            batches.append((torch.from_numpy(rng.uniform(-1, 1, shape).astype(F32)), torch.from_numpy(rng.uniform(-1, 1, (B, 1)).astype(F32))))
        model.zero_grad()
        loss = torch.nn.MSELoss()(model(batches[0][0]), batches[0][1])
        loss.backward()
        grads = flat(model, "grad")
        trainer = Trainer(model, [], torch.device("cpu"), 1)
        trainer.set_learning_rate(0.01)
        trainer.data_loader = InOrder(batches)
        average = trainer.optimize_batch(3)
        sd = model.state_dict()
        case = dict(net=f"{name}_{cols}_{int(with_global)}", policy=name, cols=cols, with_global=with_global, seed=seed, calm=name == "sarl", sha256=digest,
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
    path = save_cases("g23_trainer", cases)
    print("g23_trainer:", len(cases), "cases ->", path, os.path.getsize(path), "bytes")
