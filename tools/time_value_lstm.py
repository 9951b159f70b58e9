#!/usr/bin/env python3
"""Time LSTM-RL's decision on the GPU: 4096 worlds x 81 actions x n humans, seeded inputs, device events, no reference.

  (i)   cs_value_net_decide_lstm (sort + LSTM + MLP + pick, csrc/value_net_lstm.hip)
  (ii)  cs_value_net_decide with SARL's default network on the same tensor, for scale
  (iii) what a user has without the kernel: the same torch module on the GPU, evaluated by PyTorch on the same rows, the per-action sort
        done with torch ops (argsort of column 11, flip, take_along_dim), compute_action_value and the arg-max

With --om the rows are OM-LSTM-RL's (lstm_rl.with_om = true: 48 map columns behind the 13 rotated ones) and three more lines are timed:
  (iv)  cs_value_net_decide_lstm_om with the reference's pairing and with the own pairing, the maps already in HBM
  (v)   cs_occupancy_maps on the next humans of all worlds, on its own
  (vi)  the wide torch module on the GPU: the sort as in (iii), the maps gathered in action 0's order and concatenated by torch ops

With --precision f32 bf16 only the recurrent kernel's arithmetics are timed: cs_value_net_decide_lstm and cs_value_net_decide_lstm_bf16
(LstmRL.set_recurrent_precision) on the same tensors, ALTERNATED repetition by repetition in this one process, so that clocks and
neighbours are the same for both; the line ends with the ratio of the medians and the share of worlds in which the two pick the same action.
With --om --precision f32 bf16 it is OM-LSTM-RL's kernel instead: cs_value_net_decide_lstm_om and cs_value_net_decide_lstm_om_bf16
(OMLstmRL.set_mapped_precision) alternated in the same way, once per pairing of rows and maps, the maps already in HBM; the line also says
whether the bf16 median lies below the float32 median by more than the float32 runs' own min .. max spread.

With --input tensor fused the decision starts from the worlds' own rows (LstmRL.set_recurrent_input): "tensor" is cs_lookahead into a tensor
allocated once plus cs_value_net_decide_lstm[_bf16] -- the two calls the fused entry replaces --, "fused" is cs_value_net_decide_lstm_worlds[_bf16];
ALTERNATED repetition by repetition, once per arithmetic of --precision (float32 without it).  The line says whether the fused median lies
beyond the tensor sequence's own min .. max spread, on which side, and whether the action values are bit-equal.  --input does not combine
with --om or --only (refused).

Usage:  python tools/time_value_lstm.py [--worlds 4096] [--humans 5 25] [--network 1] [--reps 20] [--warmup 5]
        [--only lstm|sarl|torch|om|maps|omtorch] [--om] [--precision f32 bf16] [--input tensor fused] [--out profiles/lstm_rl_decision.txt]
        python tools/time_value_lstm.py --input tensor fused --precision f32 bf16 --network 1 --out profiles/lstm_rl_fused_decision.txt   (then --network 2)
        python tools/time_value_lstm.py --om --precision f32 bf16 --network 1 --out profiles/om_lstm_rl_bf16_decision.txt   (then --network 2)
With --only one variant runs alone, for a `rocprofv3 --kernel-trace --stats -- python tools/time_value_lstm.py --only lstm` run of its own.
Times are per decision of all worlds: median, minimum and maximum over --reps repetitions, each between two device events.  The work per
decision is counted from the shapes.  Without a GPU the script fails."""
import argparse
import configparser
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POLICY = {
    "rl": {"gamma": "0.9"},
    "om": {"cell_num": "4", "cell_size": "1", "om_channel_size": "3"},
    "action_space": {"kinematics": "holonomic", "speed_samples": "5", "rotation_samples": "16", "sampling": "exponential", "query_env": "true"},
    "sarl": {"mlp1_dims": "150, 100", "mlp2_dims": "100, 50", "attention_dims": "100, 100, 1", "mlp3_dims": "150, 100, 100, 1",
             "multiagent_training": "true", "with_om": "false", "with_global_state": "true", "with_theta_and_omega_visible": "false"},
    "lstm_rl": {"global_state_dim": "50", "mlp1_dims": "150, 100, 100, 50", "mlp2_dims": "150, 100, 100, 1", "multiagent_training": "true",
                "with_om": "false", "with_interaction_module": "false"},
}


def make_policy(name, network=1, with_om=False):
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.policy.policy_factory import policy_factory

    cfg = configparser.RawConfigParser()
    cfg.read_dict(POLICY)
    cfg.set("lstm_rl", "with_interaction_module", "true" if network == 2 else "false")
    cfg.set("lstm_rl", "with_om", "true" if with_om else "false")
    pol = policy_factory[name]()
    pol.configure(cfg)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for prm in pol.model.parameters():
            prm.copy_(torch.randn(prm.shape, generator=g) * 0.1)
    pol.set_device(torch.device("cuda"))
    return pol


def work_per_decision(model, W, A, n, cols):
    """(multiply-adds, bytes read of the look-ahead tensor) of one decision of all worlds, from the shapes"""
    lin = lambda seq: sum(m.in_features * m.out_features for m in seq if hasattr(m, "in_features"))
    per_row = (lin(model.mlp1) if hasattr(model, "mlp1") else 0) + 4 * model.lstm.hidden_size * (model.lstm.input_size + model.lstm.hidden_size)
    return W * A * (n * per_row + lin(model.mlp)), W * A * n * cols * 4


def gate_work(model):
    """multiply-adds of the gates per row"""
    return 4 * model.lstm.hidden_size * (model.lstm.input_size + model.lstm.hidden_size)


def timed(fn, reps, warmup):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def timed_alternated(fns, reps, warmup):
    """`timed` for several callables taking turns: {key: (median, min, max)}; repetition r runs every callable once, in order"""
    import torch

    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {key: [] for key in fns}
    for _ in range(reps):
        for key, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms[key].append(a.elapsed_time(b))
    return {key: (statistics.median(v), min(v), max(v)) for key, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=4096)
    ap.add_argument("--humans", type=int, nargs="+", default=[5, 25])
    ap.add_argument("--network", type=int, default=1, choices=(1, 2))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=("lstm", "sarl", "torch", "om", "maps", "omtorch"))
    ap.add_argument("--om", action="store_true")
    ap.add_argument("--precision", nargs="+", choices=("f32", "bf16"), help="time the recurrent kernel in these arithmetics, alternated")
    ap.add_argument("--input", nargs="+", choices=("tensor", "fused"), help="time LSTM-RL's decision from the worlds' rows with these inputs, alternated")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.input and (args.om or args.only):
        ap.error("--input times LSTM-RL's decision from the worlds' rows alone: it does not combine with --om or --only")

    import torch

    from social_navigation_pyenvs_amd import _lib
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net
    from social_navigation_pyenvs_amd.crowd_nav.policy.cadrl import build_action_space_array

    _lib.require_gpu()
    W, cols, gamma, dt = args.worlds, 13, 0.9, 0.25
    acts = torch.as_tensor(build_action_space_array(1.0).astype(np.float32), device="cuda")
    A = acts.shape[0]
    lstm, sarl = make_policy("lstm_rl_device", args.network), make_policy("sarl")
    nets = {"lstm": value_net.DeviceNet(lstm.model, cols), "sarl": value_net.DeviceNet(sarl.model, cols)}
    if args.om:
        wide = make_policy("om_lstm_rl", args.network, with_om=True)
        C, grid = wide.map_columns(), wide.om_grid()
        for order in ("reference", "own"):
            nets["om " + order] = value_net.DeviceNet(wide.model, cols, C, grid, order)
    for net in nets.values():
        net.refresh()
    if args.precision and "bf16" in args.precision:
        nets["lstm"].refresh_recurrent("bf16")
        for key, net in nets.items():
            if key.startswith("om "):
                net.refresh_mapped("bf16")
    stream = torch.cuda.current_stream().cuda_stream
    lines = [f"LSTM-RL decision, network {args.network}: {W} worlds x {A} actions, {args.reps} repetitions after {args.warmup} warm-up, ms per decision "
             f"of all worlds (median, min .. max); device {torch.cuda.get_device_name(0)}"]
    for n in args.humans:
        g = torch.Generator(device="cuda").manual_seed(100 + n)
        rot = torch.rand((W, A, n, cols), generator=g, device="cuda") * 4 - 2
        rot[..., 11] = torch.rand((W, A, n), generator=g, device="cuda") * 5 + 0.3
        rew = torch.rand((W, A), generator=g, device="cuda") - 0.25
        rob = torch.tensor([0, 0, 0, 0, 0.3, 5, 5, 1.0, 0], device="cuda").repeat(W, 1).contiguous()
        vals = torch.empty((W, A), device="cuda")
        pick = torch.empty(W, dtype=torch.int32, device="cuda")
        act = torch.empty((W, 2), device="cuda")
        tail = (rew.data_ptr(), acts.data_ptr(), rob.data_ptr(), rob.shape[1], gamma, dt, None, vals.data_ptr(), pick.data_ptr(), act.data_ptr(), stream)
        disc = torch.pow(torch.tensor(gamma, device="cuda"), dt * rob[:, 7])

        def by_torch(chunk=512):
            with torch.no_grad():
                best = torch.empty(W, dtype=torch.int64, device="cuda")
                for w0 in range(0, W, chunk):
                    x = rot[w0:w0 + chunk].reshape(-1, n, cols)
                    idx = torch.flip(torch.argsort(x[:, :, 11], dim=1, stable=True), dims=[1])
                    x = torch.take_along_dim(x, idx[:, :, None], dim=1)
                    v = lstm.model(x)[:, 0].view(-1, A)
                    best[w0:w0 + chunk] = torch.argmax(rew[w0:w0 + chunk] + disc[w0:w0 + chunk, None] * v, dim=1)
                return best

        variants = {
            "lstm": ("(i)   cs_value_net_decide_lstm", lambda: value_net.decide_lstm(nets["lstm"], W, A, n, 1, rot.data_ptr(), *tail)),
            "sarl": ("(ii)  cs_value_net_decide, SARL", lambda: value_net.decide(nets["sarl"], W, A, n, rot.data_ptr(), *tail)),
            "torch": ("(iii) torch module on the GPU", by_torch),
        }
        if args.om:
            nxt = torch.rand((W, n, 4), generator=g, device="cuda") * 4 - 2
            maps = value_net.maps_of(nxt, 2, grid, stream)
            scratch = torch.empty_like(maps)

            def wide_by_torch(chunk=512):
                with torch.no_grad():
                    best = torch.empty(W, dtype=torch.int64, device="cuda")
                    for w0 in range(0, W, chunk):
                        x = rot[w0:w0 + chunk]
                        idx = torch.flip(torch.argsort(x[..., 11], dim=2, stable=True), dims=[2])
                        x = torch.take_along_dim(x, idx[..., None], dim=2)
                        m = torch.take_along_dim(maps[w0:w0 + chunk], idx[:, 0, :, None], dim=1)            # action 0's order, by position
                        x = torch.cat([x, m[:, None].expand(-1, A, -1, -1)], dim=3).reshape(-1, n, cols + C)
                        v = wide.model(x)[:, 0].view(-1, A)
                        best[w0:w0 + chunk] = torch.argmax(rew[w0:w0 + chunk] + disc[w0:w0 + chunk, None] * v, dim=1)
                    return best

            om_tail = (rot.data_ptr(), maps.data_ptr()) + tail
            variants.update({
                "om": ("(iv)  cs_value_net_decide_lstm_om", lambda: value_net.decide_lstm_om(nets["om reference"], W, A, n, 1, *om_tail)),
                "om own": ("(iv)  ... with the own pairing", lambda: value_net.decide_lstm_om(nets["om own"], W, A, n, 1, *om_tail)),
                "maps": ("(v)   cs_occupancy_maps", lambda: value_net.occupancy_maps(W, n, nxt.data_ptr(), 4, 2, *grid, scratch.data_ptr(), stream)),
                "omtorch": ("(vi)  wide torch module on the GPU", wide_by_torch),
            })
        macs, nbytes = work_per_decision(lstm.model, W, A, n, cols)
        lines.append(f"n = {n}: {macs / 1e9:.2f} G multiply-adds, {nbytes / 1e6:.0f} MB of look-ahead rows per decision")
        if args.input:
            # synthetic worlds as cs_lookahead takes them: the humans 2 - 5 m from their robot, the goal 5 m away
            ang, dist = torch.rand((W, n), generator=g, device="cuda") * 6.2831853, torch.rand((W, n), generator=g, device="cuda") * 3 + 2
            rob_w = rob.clone()
            rob_w[:, 0:2] = torch.rand((W, 2), generator=g, device="cuda") * 4 - 2
            rob_w[:, 5:7] = rob_w[:, 0:2] + torch.tensor([4.0, 3.0], device="cuda")
            cur = torch.empty((W, n, 5), device="cuda")
            cur[..., 0], cur[..., 1] = rob_w[:, None, 0] + dist * torch.cos(ang), rob_w[:, None, 1] + dist * torch.sin(ang)
            cur[..., 2:4], cur[..., 4] = torch.rand((W, n, 2), generator=g, device="cuda") * 2 - 1, 0.3
            nxt = torch.cat([cur[..., 0:2] + cur[..., 2:4] * dt, cur[..., 2:4]], dim=2).contiguous()
            lib = _lib.load()
            world_tail = (rob_w.data_ptr(), rob_w.shape[1], gamma, dt, None)
            outputs = (vals.data_ptr(), pick.data_ptr(), act.data_ptr(), stream)
            by_rows = {"f32": ("cs_value_net_decide_lstm", value_net.decide_lstm), "bf16": ("cs_value_net_decide_lstm_bf16", value_net.decide_lstm_bf16)}
            by_worlds = {"f32": ("cs_value_net_decide_lstm_worlds", value_net.decide_lstm_worlds),
                         "bf16": ("cs_value_net_decide_lstm_worlds_bf16", value_net.decide_lstm_worlds_bf16)}
            for p in args.precision or ["f32"]:
                def tensor_path(p=p):       # (the tensor and the rewards are allocated once: only the two library calls are timed)
                    _lib.check(lib.cs_lookahead(W, n, A, 0, acts.data_ptr(), nxt.data_ptr(), cur.data_ptr(), rob_w.data_ptr(), rob_w.shape[1], dt,
                                                rot.data_ptr(), rew.data_ptr(), stream))
                    by_rows[p][1](nets["lstm"], W, A, n, 1, rot.data_ptr(), rew.data_ptr(), acts.data_ptr(), *world_tail, *outputs)

                def fused_path(p=p):
                    by_worlds[p][1](nets["lstm"], W, A, n, False, 1, acts.data_ptr(), nxt.data_ptr(), cur.data_ptr(), *world_tail, None, *outputs)

                paths = {"tensor": ("cs_lookahead + " + by_rows[p][0], tensor_path), "fused": (by_worlds[p][0], fused_path)}
                got = timed_alternated({k: paths[k][1] for k in args.input}, args.reps, args.warmup)
                seen = {}
                for k in args.input:
                    med, lo, hi = got[k]
                    lines.append(f"  {p:5s} {k:7s} {paths[k][0]:46s} {med:9.3f}  ({lo:.3f} .. {hi:.3f})")
                    paths[k][1]()
                    torch.cuda.synchronize()
                    seen[k] = vals.clone()
                if len(got) == 2:
                    (t_med, t_lo, t_hi), f_med = got["tensor"], got["fused"][0]
                    gap, spread = t_med - f_med, t_hi - t_lo
                    word = "WITHIN the spread" if abs(gap) <= spread else ("faster beyond the spread" if gap > 0 else "SLOWER beyond the spread")
                    lines.append(f"  {p:5s} tensor / fused = {t_med / f_med:.2f} in the medians; the tensor sequence's median minus the fused one is {gap:+.3f} ms, and its "
                                 f"runs spread over {spread:.3f} ms: fused is {word}; the action values are "
                                 f"{'bit-equal' if torch.equal(seen['tensor'].view(torch.int32), seen['fused'].view(torch.int32)) else 'DIFFERENT'}; "
                                 f"{nbytes / 1e6:.0f} MB of rows neither written nor read")
            continue
        if args.precision and args.om:
            wmacs, _ = work_per_decision(wide.model, W, A, n, cols + C)
            entries = {"f32": ("cs_value_net_decide_lstm_om", value_net.decide_lstm_om), "bf16": ("cs_value_net_decide_lstm_om_bf16", value_net.decide_lstm_om_bf16)}
            for order in ("reference", "own"):
                run = lambda entry: (lambda: entry(nets["om " + order], W, A, n, 1, *om_tail))
                got = timed_alternated({p: run(entries[p][1]) for p in args.precision}, args.reps, args.warmup)
                lines.append(f"  {cols} + {C} columns, the {order} pairing, {wmacs / 1e9:.2f} G multiply-adds")
                picks = {}
                for p in args.precision:
                    med, lo, hi = got[p]
                    lines.append(f"  {p:5s} {entries[p][0]:34s} {med:9.3f}  ({lo:.3f} .. {hi:.3f})  {2 * wmacs / med / 1e9:.1f} TFLOP/s")
                    run(entries[p][1])()
                    torch.cuda.synchronize()
                    picks[p] = pick.clone()
                if len(got) == 2:
                    agree = float((picks["f32"] == picks["bf16"]).float().mean())
                    (f_med, f_lo, f_hi), b_med = got["f32"], got["bf16"][0]
                    lines.append(f"  f32 / bf16 = {f_med / b_med:.2f} in the medians; the bf16 median is {f_med - b_med:.3f} ms below the float32 one, whose runs "
                                 f"spread over {f_hi - f_lo:.3f} ms: {'beyond' if f_med - b_med > f_hi - f_lo else 'WITHIN'} the spread; the two pick the same "
                                 f"action in {100 * agree:.2f} % of the worlds")
            continue
        if args.precision:
            entries = {"f32": ("cs_value_net_decide_lstm", value_net.decide_lstm), "bf16": ("cs_value_net_decide_lstm_bf16", value_net.decide_lstm_bf16)}
            run = lambda entry: (lambda: entry(nets["lstm"], W, A, n, 1, rot.data_ptr(), *tail))
            got = timed_alternated({p: run(entries[p][1]) for p in args.precision}, args.reps, args.warmup)
            picks = {}
            for p in args.precision:
                med, lo, hi = got[p]
                lines.append(f"  {p:5s} {entries[p][0]:32s} {med:9.3f}  ({lo:.3f} .. {hi:.3f})  {2 * macs / med / 1e9:.1f} TFLOP/s")
                run(entries[p][1])()
                torch.cuda.synchronize()
                picks[p] = pick.clone()
            if len(got) == 2:
                agree = float((picks["f32"] == picks["bf16"]).float().mean())
                lines.append(f"  f32 / bf16 = {got['f32'][0] / got['bf16'][0]:.2f} in the medians; the two pick the same action in {100 * agree:.2f} % of the worlds")
            continue
        results = {}
        for key, (label, fn) in variants.items():
            if args.only and key.split()[0] != args.only:
                continue
            try:
                results[key] = timed(fn, args.reps, args.warmup)
                med, lo, hi = results[key]
                extra = f"  {2 * macs / med / 1e9:.1f} TFLOP/s, {nbytes / med / 1e6:.0f} GB/s of rows" if key == "lstm" else ""
                lines.append(f"  {label:34s} {med:9.3f}  ({lo:.3f} .. {hi:.3f}){extra}")
            except Exception as e:          # (MIOpen may refuse the module: said plainly, the other variants still run)
                lines.append(f"  {label:34s} did not run: {type(e).__name__}: {str(e).splitlines()[0][:120]}")
        if "lstm" in results and "torch" in results:
            value_net.decide_lstm(nets["lstm"], W, A, n, 1, rot.data_ptr(), *tail)      # (the SARL run wrote the same outputs since)
            torch.cuda.synchronize()
            agree = float((by_torch() == pick.long()).float().mean())
            lines.append(f"  (iii) / (i) = {results['torch'][0] / results['lstm'][0]:.1f}; the two pick the same action in {100 * agree:.2f} % of the worlds")
        if "om" in results and "lstm" in results:
            wmacs, _ = work_per_decision(wide.model, W, A, n, cols + C)
            lines.append(f"  (iv) / (i) = {results['om'][0] / results['lstm'][0]:.2f} in time; {wmacs / macs:.2f} in multiply-adds ({wmacs / 1e9:.2f} G), "
                         f"{gate_work(wide.model) / gate_work(lstm.model):.2f} in the gates alone; (iv) runs at {2 * wmacs / results['om'][0] / 1e9:.1f} TFLOP/s")
        if "om" in results and "omtorch" in results:
            value_net.decide_lstm_om(nets["om reference"], W, A, n, 1, *om_tail)
            torch.cuda.synchronize()
            agree = float((wide_by_torch() == pick.long()).float().mean())
            lines.append(f"  (vi) / (iv) = {results['omtorch'][0] / results['om'][0]:.1f}; the two pick the same action in {100 * agree:.2f} % of the worlds")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
