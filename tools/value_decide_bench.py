#!/usr/bin/env python3
"""Device time and peak memory of one value-network decision (CADRL, SARL) with its two inputs, at 4096 worlds x 81
actions x {5, 25} humans, in one process on the same worlds and weights:

    tensor   cs_lookahead writes rotated [W][81][n][13] to HBM, cs_value_net_decide reads it back (k_lookahead + k_value_net + k_value_pick)
    fused    cs_value_net_decide_worlds generates the rows in LDS (k_value_net_worlds + k_value_pick)

Per input: `kernels_ms`, the library calls alone on fixed device inputs (for "tensor" also its two halves), and `act_ms`, the whole
``act_device(policy)`` (cs_peek, the gathers, the allocations, the kernels); `peak_bytes`, what torch's allocator holds at most during
one ``act_device`` beyond what it held before.  Warm device, HIP events around every single run, the inputs alternated inside every
repeat, median with minimum and maximum.  The two inputs' values are compared bit for bit first.  Prints one JSON line per case.

    python tools/value_decide_bench.py [--worlds 4096] [--humans 5 25] [--policies cadrl sarl] [--repeats 20] [--inputs tensor fused]
    CROWDSTEP_LIB=<another build> python tools/value_decide_bench.py --inputs tensor      # the tensor path of a build without the fused entry

`--state` times the value network on the worlds' CURRENT state instead (cs_value_net_state, k_value_net_state): `kernel_ms`, the library
call alone on fixed device inputs (rows written and not written); `value_device_ms`, the whole ``env.value_device(policy)`` (the gathers,
the allocations, the kernel); and `torch_forward_ms`, the only way to the same numbers without the kernel: the torch module's float32
forward under no_grad on the same rows on the same device (the rows given: torch has no ``rotate`` for the worlds' tensors).

    python tools/value_decide_bench.py --state [--worlds 4096] [--humans 5 25] [--policies cadrl sarl] [--repeats 20]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
for _d in ("tools", "tests", os.path.join("tests", "golden")):
    sys.path.insert(0, os.path.join(ROOT, _d))


def _timed(fn):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def state_rows(a):
    """The `--state` cases: one JSON line per (humans, policy)."""
    import numpy as np
    import torch
    from value_policy_timing import _env, _policy

    from social_navigation_pyenvs_amd import _lib
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    _lib.require_gpu()
    for n in a.humans:
        env = _env(n, a.worlds)
        W = env.W
        for name in a.policies:
            pol = _policy(name, env)
            with torch.cuda.stream(env.device_stream()):
                stream = env.device_stream().cuda_stream
                net = pol.state_net()
                _, cur, rob = env._worlds_on_side_stream(env._device_loop_state(), peek=False)
                vals = torch.zeros(W, device="cuda")
                rows = torch.zeros((W, n, 13), device="cuda")

                def kernel(with_rows):
                    value_net.state_values(net, W, n, False, cur.data_ptr(), rob.data_ptr(), 9, None, pol.gamma, 0.0,
                                           rows.data_ptr() if with_rows else None, vals.data_ptr(), stream)

                def forward():
                    with torch.no_grad():
                        out = pol.model(rows)
                        return out[..., 0].min(dim=-1).values if pol.name == "CADRL" else out[:, 0]

                for _ in range(3):
                    kernel(True), kernel(False), env.value_device(pol), forward()
                torch.cuda.synchronize()
                want = forward().double()
                rel = float((vals.double() - want).abs().max() / want.abs().max().clamp(min=1.0))
                t = dict(kernel_ms=[], kernel_without_rows_ms=[], value_device_ms=[], torch_forward_ms=[])
                for _ in range(a.repeats):
                    t["kernel_ms"].append(_timed(lambda: kernel(True)))
                    t["kernel_without_rows_ms"].append(_timed(lambda: kernel(False)))
                    t["value_device_ms"].append(_timed(lambda: env.value_device(pol)))
                    t["torch_forward_ms"].append(_timed(forward))
                stat = lambda xs: dict(median=float(np.median(xs)), min=float(min(xs)), max=float(max(xs)))
                print(json.dumps(dict(state=True, policy=name, worlds=W, humans=n, repeats=a.repeats, relative_error_against_torch=rel,
                                      device=_lib.device_name(0), **{k: stat(v) for k, v in t.items()})), flush=True)
        env.close()


def main():
    import numpy as np
    import torch
    from value_policy_timing import _env, _policy

    ap = argparse.ArgumentParser()
    ap.add_argument("--state", action="store_true", help="time cs_value_net_state / value_device beside the torch forward on the same rows")
    ap.add_argument("--worlds", type=int, default=4096)
    ap.add_argument("--humans", type=int, nargs="+", default=[5, 25])
    ap.add_argument("--policies", nargs="+", default=["cadrl", "sarl"])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inputs", nargs="+", default=["tensor", "fused"], choices=["tensor", "fused"])
    a = ap.parse_args()
    if a.state:
        return state_rows(a)

    from social_navigation_pyenvs_amd import _lib
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    _lib.require_gpu()
    lib, P = _lib.load(), C.c_void_p
    for n in a.humans:
        env = _env(n, a.worlds)
        W, A, dt = env.W, 81, env.robot_time_step
        for name in a.policies:
            pol = _policy(name, env)
            with torch.cuda.stream(env.device_stream()):
                stream = env.device_stream().cuda_stream
                acts, net = pol.device_action_space(), pol.device_net()
                nxt, cur, rob = env._worlds_on_side_stream(env._device_loop_state())
                vals = {k: torch.zeros((W, A), device="cuda") for k in a.inputs}
                pick = torch.zeros(W, dtype=torch.int32, device="cuda")
                act = torch.zeros((W, 2), device="cuda")
                rot = torch.empty((W, A, n, 13), device="cuda") if "tensor" in a.inputs else None
                rew = torch.empty((W, A), device="cuda")

                def lookahead():
                    _lib.check(lib.cs_lookahead(C.c_int(W), C.c_int(n), C.c_int(A), C.c_int(0), P(acts.data_ptr()), P(nxt.data_ptr()), P(cur.data_ptr()),
                                                P(rob.data_ptr()), C.c_int(9), C.c_float(dt), P(rot.data_ptr()), P(rew.data_ptr()), P(stream)))

                def network():
                    value_net.decide(net, W, A, n, rot.data_ptr(), rew.data_ptr(), acts.data_ptr(), rob.data_ptr(), 9, pol.gamma, dt, None,
                                     vals["tensor"].data_ptr(), pick.data_ptr(), act.data_ptr(), stream)

                def fused():
                    value_net.decide_worlds(net, W, A, n, False, acts.data_ptr(), nxt.data_ptr(), cur.data_ptr(), rob.data_ptr(), 9, pol.gamma, dt, None,
                                            None, vals["fused"].data_ptr(), pick.data_ptr(), act.data_ptr(), stream)

                kernels = {"tensor": lambda: (lookahead(), network()), "fused": fused}

                def act_device(how):
                    if hasattr(pol, "set_decision_input"):
                        pol.set_decision_input(how)
                    env.act_device(pol)

                def timed(fn):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    return e0.elapsed_time(e1)

                def peak(how):
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    before = torch.cuda.memory_allocated()
                    act_device(how)
                    torch.cuda.synchronize()
                    return torch.cuda.max_memory_allocated() - before

                for _ in range(3):
                    for how in a.inputs:
                        kernels[how]()
                        act_device(how)
                torch.cuda.synchronize()
                same = None
                if len(a.inputs) == 2:
                    same = bool(torch.equal(vals["tensor"].view(torch.int32), vals["fused"].view(torch.int32)))
                t = {(how, what): [] for how in a.inputs for what in ("kernels", "act")}
                halves = {"lookahead": [], "network": []}
                for _ in range(a.repeats):
                    for how in a.inputs:
                        t[how, "kernels"].append(timed(kernels[how]))
                    if "tensor" in a.inputs:
                        halves["lookahead"].append(timed(lookahead))
                        halves["network"].append(timed(network))
                    for how in a.inputs:
                        t[how, "act"].append(timed(lambda: act_device(how)))
                stat = lambda xs: dict(median=float(np.median(xs)), min=float(min(xs)), max=float(max(xs)))
                r = dict(policy=name, worlds=W, actions=A, humans=n, repeats=a.repeats, values_bitwise_equal=same,
                         rot_bytes=W * A * n * 13 * 4, input_bytes=int(nxt.numel() + cur.numel() + rob.numel()) * 4,
                         device=_lib.device_name(0), library=os.environ.get("CROWDSTEP_LIB", "product build"))
                for how in a.inputs:
                    r[how] = dict(kernels_ms=stat(t[how, "kernels"]), act_ms=stat(t[how, "act"]), peak_bytes=int(peak(how)))
                if "tensor" in a.inputs:
                    r["tensor"].update(lookahead_ms=stat(halves["lookahead"]), network_and_pick_ms=stat(halves["network"]))
                if hasattr(pol, "set_decision_input"):
                    pol.set_decision_input("tensor")
                print(json.dumps(r), flush=True)
        env.close()


if __name__ == "__main__":
    main()
