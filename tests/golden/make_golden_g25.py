#!/usr/bin/env python3
"""Generate tests/golden/g25_om_trainer.npz by RUNNING THE REFERENCE's value networks on rows with occupancy-map columns under autograd
and its ``Trainer``.

TEST INFRASTRUCTURE ONLY.  Run from the repo root:  python tests/golden/make_golden_g25.py

G23's and G24's recipe (make_golden_g23.py, make_golden_g24.py) for the two families whose rows carry a human's occupancy map behind its
rotated columns (OM-SARL, OM-LSTM-RL: ``input_dim = cols + om_cols``): the reference is imported through make_golden.py's harness; only
numbers (inputs and what the reference produced) and short names are written.  Seven networks at G23's SARL widths and G24's LSTM widths
(multiples neither of 32 nor of 8), seeded by G19's ``draw_weights`` (recorded as the seed and the SHA-256 of the float32 bytes):

  sarl.ValueNetwork       with the global state at (cols, om_cols) = (13, 48) and (15, 18), without it at (13, 18)
  lstm_rl.ValueNetwork1   at (13, 48) and (15, 18)
  lstm_rl.ValueNetwork2   at (13, 18) and (15, 48)

Per network:

  inputs0..2, values0..2   three minibatches (inputs [B, n, cols + om_cols], values [B, 1]) with (B, n) = (7, 5), (33, 3), (4, 1), float32.
                           The rotated columns are uniform in [-1, 1); the map columns are sparse, as real maps are: each is 0 with
                           probability 3 / 4, else uniform in [-1, 1) -- about a third of the map columns of the four-row minibatch are 0 in
                           every row, and the exact gradient of their weights is 0 there.  The rows' seed (rows_seed) is the first of its sequence for which no ReLU of
                           the reference's module reads an input within 2^-14 of zero on any of the three -- the reference's LSTM forward is
                           float32 only; tests/test_value_om_grad_cpu.py checks the fixture for 2^-16 in float64, and that no whole tensor's
                           gradient vanishes but the one that does by construction
  grads, loss              the reference's .grad of every parameter, flat in the sorted order of the state_dict keys, after
                           MSELoss(model(inputs0), values0).backward() on the seeded weights, and that loss
  trained, average         the parameters (same order) after the reference's ``Trainer.optimize_batch(3)`` at learning rate 0.01 over the
                           three minibatches in order (the preset ``data_loader`` of G23) and the average loss it returned
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402,F401  (imports the reference through _refharness)
from golden_io import save_cases  # noqa: E402
from make_golden_g19 import draw_weights  # noqa: E402
from make_golden_g23 import SARL_WIDTHS, SHAPES, InOrder, flat  # noqa: E402
from make_golden_g24 import MLP, MLP1, H  # noqa: E402

F32 = np.float32
KINK_MARGIN = 2.0 ** -14
# (policy, network | with_global, cols, om_cols)
NETWORKS = [("sarl", 1, 13, 48), ("sarl", 1, 15, 18), ("sarl", 0, 13, 18), ("lstm", 1, 13, 48), ("lstm", 1, 15, 18), ("lstm", 2, 13, 18),
            ("lstm", 2, 15, 48)]


def build(policy, which, width):
    from crowd_nav.policy import lstm_rl, sarl

    if policy == "sarl":
        return sarl.ValueNetwork(width, 6, SARL_WIDTHS["mlp1_dims"], SARL_WIDTHS["mlp2_dims"], SARL_WIDTHS["mlp3_dims"],
                                 SARL_WIDTHS["attention_dims"], bool(which), 1.0, 4)
    if which == 1:
        return lstm_rl.ValueNetwork1(width, 6, MLP, H)
    return lstm_rl.ValueNetwork2(width, 6, MLP1, MLP, H)


def rows(rng, B, n, cols, om_cols):
    """[B, n, cols + om_cols]: uniform rotated columns, then map columns that are 0 with probability 3 / 4"""
    rot = rng.uniform(-1, 1, (B, n, cols))
    maps = rng.uniform(-1, 1, (B, n, om_cols)) * (rng.uniform(0, 1, (B, n, om_cols)) < 0.25)
    return np.concatenate([rot, maps], axis=2).astype(F32)


def relu_margin(model, x):
    """the smallest |input of a ReLU| in the forward of `model` on x"""
    import copy

    import torch

    m = copy.deepcopy(model)
    least = [float("inf")]

    def hook(_, inputs, __):
        least[0] = min(least[0], float(inputs[0].detach().abs().min()))

    for mod in m.modules():
        if isinstance(mod, torch.nn.ReLU):
            mod.register_forward_hook(hook)
    with torch.no_grad():
        m(x)
    return least[0]


def generate():
    import torch
    from crowd_nav.utils.trainer import Trainer

    cases = []
    for i, (policy, which, cols, om_cols) in enumerate(NETWORKS):
        model = build(policy, which, cols + om_cols)
        seed = 2500 + i
        digest = draw_weights(model, seed, calm=policy == "sarl")
        for rows_seed in range(2530 + 100 * i, 2530 + 100 * i + 50):
            rng = np.random.default_rng(rows_seed)
            batches = [(torch.from_numpy(rows(rng, B, n, cols, om_cols)), torch.from_numpy(rng.uniform(-1, 1, (B, 1)).astype(F32))) for B, n in SHAPES]
            if min(relu_margin(model, x) for x, _ in batches) >= KINK_MARGIN:
                break
        else:
            raise SystemExit(f"no rows away from the ReLUs' kinks for network {i}")
        model.zero_grad()
        loss = torch.nn.MSELoss()(model(batches[0][0]), batches[0][1])
        loss.backward()
        grads = flat(model, "grad")
        trainer = Trainer(model, [], torch.device("cpu"), 1)
        trainer.set_learning_rate(0.01)
        trainer.data_loader = InOrder(batches)
        average = trainer.optimize_batch(3)
        sd = model.state_dict()
        name = f"om_sarl_{cols}_{om_cols}_{which}" if policy == "sarl" else f"om_lstm{which}_{cols}_{om_cols}"
        case = dict(net=name, policy=policy, network=which if policy == "lstm" else 0, with_global=bool(which) if policy == "sarl" else False, cols=cols,
                    om_cols=om_cols, hidden=H, seed=seed, calm=policy == "sarl", rows_seed=rows_seed, sha256=digest,
                    weights_keys=sorted(str(k) for k in sd), weights_shapes=[list(sd[k].shape) for k in sorted(sd)],
                    grads=grads, loss=float(loss.item()), trained=flat(model, "param"), average=float(average), learning_rate=0.01)
        for b, (x, v) in enumerate(batches):
            case[f"inputs{b}"], case[f"values{b}"] = x.numpy(), v.numpy()
        cases.append(case)
    return cases


if __name__ == "__main__":
    cases = generate()
    for c in cases:
        dead = int(np.sum(~np.any(c["inputs2"][:, :, c["cols"]:] != 0, axis=(0, 1))))
        print(f"{c['net']}: {len(c['grads'])} parameters, rows seed {c['rows_seed']}, {dead} map columns of minibatch 2 all zero, loss {c['loss']:.6f}, "
              f"average of three steps {c['average']:.6f}, max |grad| {float(np.max(np.abs(c['grads']))):.3e}, "
              f"finite: {bool(np.all(np.isfinite(c['trained'])))}")
    path = save_cases("g25_om_trainer", cases)
    print("g25_om_trainer:", len(cases), "cases ->", path, os.path.getsize(path), "bytes")
