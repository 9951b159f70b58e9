#!/usr/bin/env python3
"""Time the whole optimisation step of crowd_nav/utils/trainer.py on the GPU in its two update modes, for SARL (mlp1 150-100, mlp2
100-50, attention 100-100-1, mlp3 150-100-100-1, with the global state) and LSTM-RL's network 1 (hidden 50, mlp 150-100-100-1) at the
reference's widths, seeded weights and minibatches.  Both run the device gradient mode ("device" / "device_lstm"):

  "torch"   the blob packed on the device, the loss-and-gradient entry (two launches), torch's SGD(momentum 0.9) step over the views of the
            flat tensor, the loss read back per minibatch -- the path before the fused step, the yardstick
  "device"  cs_value_net_train_step[_lstm]: the gradient kernel, then one kernel that sums the gradient, takes the step and rewrites the
            blob; the loss added to a float64 on the device and read once per optimize_batch call

  step      one ``Trainer.optimize_batch(1)`` between two device events: median, minimum and maximum over --reps repetitions
  run       ``Trainer.optimize_batch(100)``, 100 consecutive minibatches, in wall time (the device idle before and after): the same three
            over --runs repetitions, per step

Usage:  python tools/time_value_step.py [--shapes 100x5 4096x5] [--reps 30] [--runs 5] [--warmup 5] [--only torch|device] [--out profiles/value_step.txt]
With --only one mode runs alone, for a `rocprofv3 --kernel-trace --stats -- python tools/time_value_step.py --only device` run of its own.
Without a GPU the script fails."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SARL = dict(mlp1=[150, 100], mlp2=[100, 50], attention=[100, 100, 1], mlp3=[150, 100, 100, 1])
LSTM1 = dict(hidden=50, mlp=[150, 100, 100, 1])
CONSECUTIVE = 100


class Same:
    """A data_loader whose every iteration yields the one minibatch"""

    def __init__(self, item):
        self.item = item

    def __iter__(self):
        return iter([self.item])


def stats(xs):
    return statistics.median(xs), min(xs), max(xs)


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
    return stats(ms)


def run_times(trainer, runs):
    import torch

    ms = []
    for _ in range(runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        trainer.optimize_batch(CONSECUTIVE)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / CONSECUTIVE)
    return stats(ms[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["100x5", "4096x5"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=("torch", "device"))
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch

    from social_navigation_pyenvs_amd import _lib
    from social_navigation_pyenvs_amd.crowd_nav.policy import lstm_rl, sarl
    from social_navigation_pyenvs_amd.crowd_nav.utils.trainer import Trainer

    _lib.require_gpu()
    lines = [f"device: {_lib.device_name(0)}"]
    nets = {
        "SARL": (lambda: sarl.ValueNetwork(13, 6, SARL["mlp1"], SARL["mlp2"], SARL["mlp3"], SARL["attention"], True), "device", SARL),
        "LSTM-RL network 1": (lambda: lstm_rl.ValueNetwork1(13, 6, LSTM1["mlp"], LSTM1["hidden"]), "device_lstm", LSTM1),
    }
    modes = [args.only] if args.only else ["torch", "device"]
    for name, (make, gradient, widths) in nets.items():
        lines.append(f"{name} {widths}, {sum(p.numel() for p in make().parameters())} parameters")
        for shape in args.shapes:
            B, n = (int(x) for x in shape.split("x"))
            rs = np.random.RandomState(B + n)
            x = torch.as_tensor(rs.uniform(-1, 1, (B, n, 13)).astype(np.float32), device="cuda")
            t = torch.as_tensor(rs.uniform(-1, 1, (B, 1)).astype(np.float32), device="cuda")
            lines.append(f"  B = {B}, n = {n}:")
            res = {}
            for mode in modes:
                g = torch.Generator().manual_seed(7)
                model = make()
                with torch.no_grad():
                    for prm in model.parameters():
                        prm.copy_(torch.randn(prm.shape, generator=g) * 0.1)
                trainer = Trainer(model.cuda(), [], torch.device("cuda"), B)
                trainer.set_learning_rate(1e-5)        # (hundreds of steps on one minibatch: small enough to stay finite)
                trainer.set_gradient(gradient)
                trainer.set_update(mode)
                trainer.data_loader = Same((x, t))
                res[mode] = (step_times(trainer, args.reps, args.warmup), run_times(trainer, args.runs))
                for what, (med, lo, hi) in zip(("step", f"run of {CONSECUTIVE}, per step"), res[mode]):
                    lines.append(f"    update {mode!r:9s} {what:24s} median {med * 1e3:9.1f} us   min {lo * 1e3:9.1f}   max {hi * 1e3:9.1f}")
            if len(res) == 2:
                lines.append(f"    torch / device: step {res['torch'][0][0] / res['device'][0][0]:.2f}, run {res['torch'][1][0] / res['device'][1][0]:.2f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
