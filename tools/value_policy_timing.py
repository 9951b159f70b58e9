#!/usr/bin/env python3
"""Device time of the value-based robot decision (CADRL, SARL; csrc/value_net.hip) at 4096 worlds x 81 actions x {5, 25} humans, measured
in one process on the same worlds and weights:

    kernel    cs_value_net_decide alone on the look-ahead rows (the network kernel + the per-world pick)
    decide    BatchedSocialNavGym.act_device(policy): cs_peek + cs_lookahead + the kernel
    torch     the baseline: the same policy.model run by torch in float32 under no_grad on the same rows, then min / argmax in torch

Warm device, HIP events around every single run, `kernel` and `torch` alternated, median of --repeats each, and the spread (min, max,
interquartile range) of the baseline.  FLOP are the useful ones (2 x in x out per Linear layer and row; the padding of widths to the
tile is not counted), the fraction is against the 157 TFLOP/s float32 matrix peak.  Writes profiles/value_policy_timing.json and prints it.

    python tools/value_policy_timing.py [--worlds 4096] [--humans 5 25] [--policies cadrl sarl] [--repeats 20] [--out FILE]
    python tools/value_policy_timing.py --precision f32 bf16   # both arithmetics, alternated inside every repeat; one record each
    python tools/value_policy_timing.py --trace-only        # a few act_device decisions, for a kernel trace of `decide`
    python tools/value_policy_timing.py --om [--precision f32 bf16]   # the OM-SARL row: cs_value_net_decide_om against
                                                            # cs_value_net_decide_om_bf16 on the look-ahead rows and the 48-column
                                                            # maps of the next humans, both in HBM, alternated inside every repeat; text lines
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
for _d in ("tools", "tests", os.path.join("tests", "golden")):
    sys.path.insert(0, os.path.join(ROOT, _d))

PEAK_F32_MATRIX = 157e12


def _env(n, W):
    from policy_no_train_bench import _config

    from social_navigation_pyenvs_amd.social_gym.social_nav_gym import BatchedSocialNavGym

    env = BatchedSocialNavGym(_config(n), W)
    env.reset(phase="test", first_case=11, device=True)
    for _ in range(3):
        env.step_device(env.act_device("sfm_helbing"))
    return env


def _policy(name, env):
    import torch
    from test_value_policy_cpu import make_policy, seeded_weights      # the default policy.config and G16's weight scale: one copy, the tests'

    pol = make_policy(name)
    seeded_weights(pol.model, 1700)
    pol.set_phase("test")
    pol.set_device(torch.device("cuda"))
    pol.time_step = env.robot_time_step
    return pol


def useful_flop(pol, rows, groups):
    """2 x in x out per Linear layer: per (action, human) row for the pairwise chains, per (world, action) for SARL's mlp3."""
    import torch.nn as nn

    lin = lambda seq: sum(2 * m.in_features * m.out_features for m in seq if isinstance(m, nn.Linear))
    m = pol.model
    if hasattr(m, "value_network"):
        return rows * lin(m.value_network)
    return rows * (lin(m.mlp1) + lin(m.mlp2) + lin(m.attention)) + groups * lin(m.mlp3)


def torch_decide(pol, rot, rew, disc, chunk):
    import torch

    W, A, n, cols = rot.shape
    out = torch.empty((W, A), dtype=torch.float32, device=rot.device)
    with torch.no_grad():
        for w0 in range(0, W, chunk):
            x = rot[w0:w0 + chunk].reshape(-1, n, cols)
            v = pol.model(x)[..., 0].min(dim=-1).values if pol.name == "CADRL" else pol.model(x)[:, 0]
            out[w0:w0 + chunk] = v.view(-1, A)
        values = rew + disc * out
        return values, torch.argmax(values, dim=1)


def om_rows(a):
    """The OM-SARL row: the float32 and the bf16 decision kernel (each with the per-world pick) on the same look-ahead rows, rewards and
    maps [W, n, 48] of the next humans, all in HBM, the default network with seeded weights; the arithmetics of --precision alternated
    inside every repeat.  Prints, per crowd size, the median (min .. max) of each and how often the two pick the same action."""
    import numpy as np
    import om_cases
    import torch
    from test_value_om_cpu import om_policy

    from social_navigation_pyenvs_amd import _lib
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    entries = {"f32": ("cs_value_net_decide_om", value_net.decide_om), "bf16": ("cs_value_net_decide_om_bf16", getattr(value_net, "decide_om_bf16", None))}
    warm = 5
    print(f"OM-SARL decision, 48 map columns: {a.worlds} worlds x 81 actions, {a.repeats} repetitions after {warm} warm-up, ms per decision of all "
          f"worlds (median, min .. max); device {_lib.device_name(0)}; library {os.environ.get('CROWDSTEP_LIB', 'product build')}")
    for n in a.humans:
        env = _env(n, a.worlds)
        W = env.W
        pol = om_policy()
        om_cases.draw_weights(pol.model, 1700)
        pol.set_phase("test")
        pol.set_device(torch.device("cuda"))
        pol.time_step = env.robot_time_step
        with torch.cuda.stream(env.device_stream()):
            for _ in range(3):
                env.act_device(pol)                 # (builds the action table for the batch's robot speed)
            acts = pol.device_action_space()
            rot, rew = env.lookahead_device(acts)
            maps = env.occupancy_maps_device(*pol.om_grid(), which="next").contiguous()
            rob = env.cw.d_robot.torch().view(W, 13)[:, [0, 1, 3, 4, 8, 10, 11, 12, 2]].contiguous()
            net = pol.device_net()
            if "bf16" in a.precision:
                net.refresh_wide("bf16")
            stream = env.device_stream().cuda_stream
            out = {p: (torch.zeros((W, 81), device="cuda"), torch.zeros(W, dtype=torch.int32, device="cuda"), torch.zeros((W, 2), device="cuda")) for p in a.precision}

            def kernel(prec):
                vals, pick, act = out[prec]
                entries[prec][1](net, W, 81, n, rot.data_ptr(), maps.data_ptr(), rew.data_ptr(), acts.data_ptr(), rob.data_ptr(), 9, pol.gamma,
                                 env.robot_time_step, None, vals.data_ptr(), pick.data_ptr(), act.data_ptr(), stream)

            def timed(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1)

            for _ in range(warm):
                for prec in a.precision:
                    kernel(prec)
            t = {p: [] for p in a.precision}
            for _ in range(a.repeats):
                for prec in a.precision:
                    t[prec].append(timed(lambda: kernel(prec)))
            torch.cuda.synchronize()
            flop = useful_flop(pol, W * 81 * n, W * 81)
            print(f"n = {n}: {flop / 2e9:.2f} G multiply-adds, {rot.numel() * 4 / 1e6:.0f} MB of look-ahead rows and {maps.numel() * 4 / 1e6:.1f} MB of maps per decision")
            for prec in a.precision:
                med = float(np.median(t[prec]))
                print(f"  {prec:<5} {entries[prec][0]:<32} {med:8.3f}  ({min(t[prec]):.3f} .. {max(t[prec]):.3f})  {flop / (med * 1e-3) / 1e12:.1f} TFLOP/s")
            if len(a.precision) == 2:
                f, h = t["f32"], t["bf16"]
                same = float((out["f32"][1] == out["bf16"][1]).float().mean())
                finite = bool(torch.isfinite(out["f32"][0]).all() and torch.isfinite(out["bf16"][0]).all())
                print(f"  f32 / bf16 = {np.median(f) / np.median(h):.2f} in the medians; bf16's slowest repeat {'beats' if max(h) < min(f) else 'DOES NOT beat'} "
                      f"f32's fastest; the two pick the same action in {100 * same:.2f} % of the worlds (all values finite: {finite})")
        env.close()


def main():
    import numpy as np
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=4096)
    ap.add_argument("--humans", type=int, nargs="+", default=[5, 25])
    ap.add_argument("--policies", nargs="+", default=["cadrl", "sarl"])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--torch-chunk", type=int, default=1024, help="worlds per torch forward (the whole batch's intermediates at once need tens of GB)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "value_policy_timing.json"))
    ap.add_argument("--precision", nargs="+", default=["f32"], choices=["f32", "bf16"], help="decision arithmetics to time, alternated inside every repeat")
    ap.add_argument("--no-torch", action="store_true", help="skip the torch baseline (an A/B of two libraries needs only the kernels)")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--om", action="store_true", help="the OM-SARL row instead: the float32 and the bf16 wide-row kernel on rows and maps in HBM")
    a = ap.parse_args()

    from social_navigation_pyenvs_amd import _lib
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    _lib.require_gpu()
    if a.om:
        return om_rows(a)
    results = []
    for n in a.humans:
        env = _env(n, a.worlds)
        W = env.W
        for name in a.policies:
            pol = _policy(name, env)
            with torch.cuda.stream(env.device_stream()):
                for _ in range(3):
                    env.act_device(pol)
                if a.trace_only:
                    torch.cuda.synchronize()
                    continue
                acts = pol.device_action_space()
                rot, rew = env.lookahead_device(acts)
                rob = env.cw.d_robot.torch().view(W, 13)[:, [0, 1, 3, 4, 8, 10, 11, 12, 2]].contiguous()
                disc = torch.pow(torch.tensor(pol.gamma, dtype=torch.float64, device="cuda"), env.robot_time_step * rob[:, 7].double()).float()[:, None]
                vals = torch.zeros((W, 81), device="cuda")
                pick = torch.zeros(W, dtype=torch.int32, device="cuda")
                act = torch.zeros((W, 2), device="cuda")
                stream = env.device_stream().cuda_stream

                def kernel(prec):
                    pol.set_decision_precision(prec)
                    value_net.decide(pol.device_net(), W, 81, n, rot.data_ptr(), rew.data_ptr(), acts.data_ptr(), rob.data_ptr(), 9, pol.gamma,
                                     env.robot_time_step, None, vals.data_ptr(), pick.data_ptr(), act.data_ptr(), stream, precision=prec)

                def decide(prec):
                    pol.set_decision_precision(prec)
                    env.act_device(pol)

                def timed(fn):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    return e0.elapsed_time(e1)

                run_torch = lambda: torch_decide(pol, rot, rew, disc, a.torch_chunk)
                for _ in range(3):
                    for prec in a.precision:
                        kernel(prec)
                        decide(prec)
                    if not a.no_torch:
                        run_torch()
                tv, tp = run_torch()
                scale = torch.clamp(tv.abs().max(dim=1).values, min=1.0)
                rel, same = {}, {}
                for prec in a.precision:
                    kernel(prec)
                    rel[prec] = float(((vals - tv).abs().max(dim=1).values / scale).max())
                    same[prec] = float((pick.long() == tp).float().mean())
                tk, td, tt = {p: [] for p in a.precision}, {p: [] for p in a.precision}, []
                for _ in range(a.repeats):
                    for prec in a.precision:
                        tk[prec].append(timed(lambda: kernel(prec)))
                    if not a.no_torch:
                        tt.append(timed(run_torch))
                    for prec in a.precision:
                        td[prec].append(timed(lambda: decide(prec)))
                pol.set_decision_precision("f32")
                flop = useful_flop(pol, W * 81 * n, W * 81)
                q = lambda xs, p: float(np.percentile(xs, p))
                for prec in a.precision:
                    k, d = tk[prec], td[prec]
                    r = dict(policy=name, precision=prec, worlds=W, actions=81, humans=n, repeats=a.repeats, useful_gflop=flop / 1e9,
                             kernel_ms=q(k, 50), kernel_min_ms=min(k), kernel_max_ms=max(k),
                             decide_ms=q(d, 50), decide_min_ms=min(d), decide_max_ms=max(d),
                             kernel_tflops=flop / (q(k, 50) * 1e-3) / 1e12,
                             kernel_fraction_of_f32_matrix_peak=flop / (q(k, 50) * 1e-3) / PEAK_F32_MATRIX,
                             worst_rel_value_diff_vs_torch=rel[prec], same_pick_fraction=same[prec],
                             tile_rows=os.environ.get("CROWDSTEP_VN_TILE", "default"), device=_lib.device_name(0),
                             library=os.environ.get("CROWDSTEP_LIB", "product build"))
                    if tt:
                        r.update(torch_ms=q(tt, 50), torch_min_ms=min(tt), torch_max_ms=max(tt), torch_iqr_ms=q(tt, 75) - q(tt, 25),
                                 torch_chunk_worlds=a.torch_chunk, torch_tflops=flop / (q(tt, 50) * 1e-3) / 1e12, speedup_vs_torch=q(tt, 50) / q(k, 50),
                                 kernel_not_slower_than_torch=bool(q(k, 50) <= q(tt, 50) + (max(tt) - min(tt))))
                    print(json.dumps(r), flush=True)
                    results.append(r)
        env.close()
    if results and a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
