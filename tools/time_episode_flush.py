#!/usr/bin/env python3
"""Time ``EpisodeBuffer.flush`` (cs_episode_flush: three launches) against the same result composed from torch operations on the same
device, interleaved in one process: 4096 worlds, max_steps 100, states [5, 13] and [25, 13], episode lengths uniform in 20..100, outcomes
ReachGoal / Collision / Timeout at 45 / 35 / 20 %, targets="returns", in two situations -- every world done in one flush, and a quarter of
the worlds done.

  kernel   buf.flush(memory, done, code) between two device events; the cursors are put back (a [W] device copy) outside the events
  torch    kept lengths -> cumsum -> the kept (world, step) pairs by nonzero (which reads their number back: the sizes of everything
           behind it depend on it) -> ring slots -> a float64 return scan (reversed cumsum of r_t gamma^(t dt v) over gamma^(i dt v)) ->
           gather -> index_copy_ of states and values -> position, count, the six figures, the cursors

Reported per situation: median / minimum / maximum microseconds per flush over --reps repetitions, GB/s over 2 K F 4 bytes (K rows read
and written), and torch / kernel.  Both paths' memories are compared once per shape (states must be equal; the values' largest distance in
float32 ulps is printed: the torch scan divides where the kernel sums directly).

Usage:  python tools/time_episode_flush.py [--worlds 4096] [--reps 30] [--warmup 3] [--out profiles/episode_flush.txt]
Without a GPU the script fails."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, GAMMA, DT, V = 100, 0.9, 0.25, 1.0


def torch_flush(buf, memory, done, code, figures):
    """EpisodeBuffer.flush(memory, done, code, V, "returns") out of torch operations"""
    import torch

    W, cap, dev = buf.W, memory.capacity, buf.states.device
    length = buf.cursor.long()
    kept = torch.where(done & ((code == 2) | (code == 3)) & (buf.overflow == 0), length, torch.zeros_like(length))
    off = torch.cumsum(kept, 0) - kept
    K = kept.sum()
    t = torch.arange(buf.T, device=dev)
    disc = torch.pow(torch.tensor(GAMMA, dtype=torch.float64, device=dev), t.double() * DT * V)              # [T]
    x = torch.where(t[None, :] < length[:, None], buf.rewards.double() * disc[None, :], torch.zeros((), dtype=torch.float64, device=dev))
    togo = torch.flip(torch.cumsum(torch.flip(x, (1,)), 1), (1,))                                             # sum over t >= i
    values = (togo / disc[None, :]).float()
    g = off[:, None] + t[None, :]
    lands = (t[None, :] < kept[:, None]) & (g >= K - cap)
    rows = lands.reshape(-1).nonzero()[:, 0]                                                                  # synchronises
    slot = ((memory._position + g) % cap).reshape(-1)[rows]
    memory.states.view(cap + 1, -1).index_copy_(0, slot, buf.states.view(W * buf.T, -1)[rows])
    memory.values.index_copy_(0, slot, values.reshape(-1, 1)[rows])
    memory._position = (memory._position + K) % cap
    memory._count = torch.clamp(memory._count + K, max=cap)
    memory._len = None
    figures += torch.stack([done.sum().double(), (done & (code == 2)).sum().double(), (done & (code == 3)).sum().double(),
                            (done & (code == 4)).sum().double(), (length.double() * DT)[done & (code == 2)].sum(), togo[:, 0][done].sum()])
    buf.cursor.masked_fill_(done, 0)
    buf.overflow.masked_fill_(done, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch

    from social_navigation_pyenvs_amd import _lib
    from social_navigation_pyenvs_amd.crowd_nav.utils.episodes import EpisodeBuffer
    from social_navigation_pyenvs_amd.crowd_nav.utils.memory import ReplayMemory

    _lib.require_gpu()
    W = args.worlds
    lines = [f"device: {_lib.device_name(0)}", f"{W} worlds, max_steps {T}, lengths uniform in 20..100, gamma {GAMMA}, time step {DT}, "
             f"{args.reps} repetitions interleaved, microseconds per flush"]
    rng = np.random.default_rng(2630)
    lengths = torch.as_tensor(rng.integers(20, 101, W).astype(np.int32), device="cuda")
    code = torch.as_tensor(rng.choice([2, 3, 4], W, p=[0.45, 0.35, 0.2]).astype(np.int32), device="cuda")
    everyone = torch.ones(W, dtype=torch.bool, device="cuda")
    quarter = torch.as_tensor(rng.random(W) < 0.25, device="cuda")
    for shape in ((5, 13), (25, 13)):
        F = shape[0] * shape[1]
        buf = EpisodeBuffer(W, T, GAMMA, DT)
        buf.append(torch.zeros((W,) + shape, device="cuda"), torch.zeros(W, device="cuda"))
        buf.states.uniform_(-2, 2)
        buf.rewards.copy_(torch.as_tensor(rng.choice(np.array([0.0, -0.0125, -0.00625, 1.0, -0.25], np.float32), (W, T)), device="cuda"))
        capacity = W * T
        mems = {"kernel": ReplayMemory(capacity), "torch": ReplayMemory(capacity)}
        for m in mems.values():
            m._attach(shape, torch.float32, buf.states.device)
        figures = torch.zeros(6, dtype=torch.float64, device="cuda")
        run = {"kernel": lambda done: buf.flush(mems["kernel"], done, code, V, "returns"),
               "torch": lambda done: torch_flush(buf, mems["torch"], done, code, figures)}
        for name, done in (("every world done", everyone), ("a quarter of the worlds done", quarter)):
            K = int(lengths[done & (code != 4)].sum().item())
            nbytes = 2 * K * F * 4
            ms = {"kernel": [], "torch": []}
            for rep in range(args.warmup + args.reps):
                for which in ("kernel", "torch"):
                    buf.cursor.copy_(lengths)
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    run[which](done)
                    b.record()
                    torch.cuda.synchronize()
                    if rep >= args.warmup:
                        ms[which].append(a.elapsed_time(b))
            lines.append(f"state {list(shape)} (F = {F}), {name}: K = {K} samples, {nbytes / 1e6:.1f} MB read + written")
            med = {}
            for which in ("kernel", "torch"):
                med[which] = statistics.median(ms[which])
                lines.append(f"    {which:7s} median {med[which] * 1e3:9.1f} us   min {min(ms[which]) * 1e3:9.1f}   max {max(ms[which]) * 1e3:9.1f}"
                             f"   {nbytes / (med[which] * 1e-3) / 1e9:8.1f} GB/s")
            lines.append(f"    torch / kernel: {med['torch'] / med['kernel']:.2f}")
        # both paths flushed the same episodes the same number of times from position 0: the same memory
        a, b = mems["kernel"], mems["torch"]
        same = torch.equal(a.states, b.states) and int(a._position.item()) == int(b._position.item()) and len(a) == len(b)
        bits = lambda v: torch.where(v.view(torch.int32) < 0, -(v.view(torch.int32) & 0x7FFFFFFF), v.view(torch.int32)).long()
        lines.append(f"state {list(shape)}: states, position and length of the two memories equal: {same}; values differ by at most "
                     f"{int((bits(a.values) - bits(b.values)).abs().max().item())} float32 ulp; figures (kernel) {buf._figures.tolist()[:4]}, "
                     f"(torch) {figures.tolist()[:4]}")
        del buf, mems
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
