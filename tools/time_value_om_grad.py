#!/usr/bin/env python3
"""Time the whole optimisation step of crowd_nav/utils/trainer.py on the GPU for the networks with occupancy-map columns: OM-SARL (mlp1
150-100, mlp2 100-50, attention 100-100-1, mlp3 150-100-100-1, with the global state) and OM-LSTM-RL's two networks (hidden 50, mlp
150-100-100-1; network 2 with mlp1 150-100-100-50) at the reference's widths, on rows of 13 + 48 columns (the reference's 4 x 4 x 3 map),
seeded weights and minibatches whose map columns are three quarters zero.  Three variants:

  "autograd"  torch's zero_grad + forward + MSELoss + backward + optimizer.step() on this project's module, the loss read back per
              minibatch -- the only path these networks had before the map modes
  "device"    ``set_gradient("device_om" | "device_lstm_om")`` with ``set_update("torch")``: the blob packed on the device, the
              loss-and-gradient entry (two launches), torch's SGD(momentum 0.9) step over the views of the flat tensor, the loss read back
  "fused"     the same gradient mode with ``set_update("device")``: cs_value_net_train_step_om | _lstm_om, two launches, nothing read back
              but once per optimize_batch call

One ``Trainer.optimize_batch(1)`` between two device events: median, minimum and maximum over --reps repetitions.

Usage:  python tools/time_value_om_grad.py [--reps 30] [--warmup 5] [--only autograd|device|fused] [--out profiles/value_om_grad.txt]
With --only one variant runs alone, for a profiler run of its own.  Without a GPU the script fails."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLS, OM_COLS = 13, 48
SARL = dict(mlp1=[150, 100], mlp2=[100, 50], attention=[100, 100, 1], mlp3=[150, 100, 100, 1])
LSTM = dict(hidden=50, mlp1=[150, 100, 100, 50], mlp=[150, 100, 100, 1])
VARIANTS = ("autograd", "device", "fused")


class Same:
    """A data_loader whose every iteration yields the one minibatch"""

    def __init__(self, item):
        self.item = item

    def __iter__(self):
        return iter([self.item])


def step_times(trainer, reps, warmup):
    import torch

    for _ in range(warmup):
        trainer.optimize_batch(1)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        trainer.optimize_batch(1)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=VARIANTS)
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch

    from social_navigation_pyenvs_amd import _lib
    from social_navigation_pyenvs_amd.crowd_nav.policy import lstm_rl, sarl, value_net
    from social_navigation_pyenvs_amd.crowd_nav.utils.trainer import Trainer

    _lib.require_gpu()
    K = COLS + OM_COLS
    lines = [f"device: {_lib.device_name(0)}", f"rows of {COLS} + {OM_COLS} columns"]
    nets = {
        "OM-SARL": (lambda: sarl.ValueNetwork(K, 6, SARL["mlp1"], SARL["mlp2"], SARL["mlp3"], SARL["attention"], True), "device_om", SARL,
                    ["100x5", "4096x5"]),
        "OM-LSTM-RL network 1": (lambda: lstm_rl.ValueNetwork1(K, 6, LSTM["mlp"], LSTM["hidden"]), "device_lstm_om", LSTM, ["100x5", "4096x5", "100x25"]),
        "OM-LSTM-RL network 2": (lambda: lstm_rl.ValueNetwork2(K, 6, LSTM["mlp1"], LSTM["mlp"], LSTM["hidden"]), "device_lstm_om", LSTM,
                                 ["100x5", "4096x5", "100x25"]),
    }
    variants = [args.only] if args.only else list(VARIANTS)
    for name, (make, gradient, widths, shapes) in nets.items():
        lines.append(f"{name} {widths}, {sum(p.numel() for p in make().parameters())} parameters")
        for shape in shapes:
            B, n = (int(x) for x in shape.split("x"))
            rs = np.random.RandomState(B + n)
            rows = np.concatenate([rs.uniform(-1, 1, (B, n, COLS)), rs.uniform(-1, 1, (B, n, OM_COLS)) * (rs.uniform(0, 1, (B, n, OM_COLS)) < 0.25)], axis=2)
            x = torch.as_tensor(rows.astype(np.float32), device="cuda")
            t = torch.as_tensor(rs.uniform(-1, 1, (B, 1)).astype(np.float32), device="cuda")
            lines.append(f"  B = {B}, n = {n}:")
            res = {}
            for variant in variants:
                g = torch.Generator().manual_seed(7)
                model = make()
                with torch.no_grad():
                    for prm in model.parameters():
                        prm.copy_(torch.randn(prm.shape, generator=g) * 0.1)
                model = model.cuda()
                trainer = Trainer(model, [], torch.device("cuda"), B)
                trainer.set_learning_rate(1e-5)        # (many steps on one minibatch: small enough to stay finite)
                if variant != "autograd":
                    trainer.set_gradient(gradient, net=value_net.DeviceNet(model, COLS, om_cols=OM_COLS))
                    trainer.set_update("device" if variant == "fused" else "torch")
                trainer.data_loader = Same((x, t))
                res[variant] = step_times(trainer, args.reps, args.warmup)
                med, lo, hi = res[variant]
                lines.append(f"    {variant:9s} step   median {med * 1e3:9.1f} us   min {lo * 1e3:9.1f}   max {hi * 1e3:9.1f}")
            if len(res) == 3:
                lines.append(f"    autograd / device: {res['autograd'][0] / res['device'][0]:.2f}   autograd / fused: {res['autograd'][0] / res['fused'][0]:.2f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
