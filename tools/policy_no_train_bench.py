#!/usr/bin/env python3
"""Device time of the batched no-train robot policies (BatchedSocialNavGym.act_device, csrc/policy_no_train.hip) against the Gym step
they feed, measured in the same process on the same worlds:

    act        act_device(policy) alone
    step       step_device(action_buffer()) alone
    act+step   act_device -> step_device, the evaluation loop of a baseline
    fused      act_step_device(policy): the same Gym step as one library call (one launch where the step build decides in its head);
               left out when the loaded library has no cs_gym_step_policy (an older build through CROWDSTEP_LIB: the A side of an A/B)

Everything runs inside ``with torch.cuda.stream(env.device_stream())`` (no cross-stream waits); device events bracket `--iters`
iterations after `--warmup` ones; the figure is the mean per iteration.  act+step and fused are measured `--repeats` times, alternating,
and reported as min / median / max.  Prints one JSON line per (worlds, humans, policy); --out appends them to a file.

    python tools/policy_no_train_bench.py [--worlds 4096] [--humans 5 25] [--policies sfm_moussaid bp] [--iters 200] [--repeats 5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _config(n):
    import configparser

    cfg = configparser.RawConfigParser()
    cfg.read_dict({
        "env": {"time_limit": 50, "time_step": 0.0125, "robot_time_step": 0.25, "val_size": 100, "test_size": 100, "randomize_attributes": "false"},
        "reward": {"success_reward": 1, "collision_penalty": -0.25, "discomfort_dist": 0.2, "discomfort_penalty_factor": 0.5},
        "sim": {"train_val_sim": "hybrid_scenario", "test_sim": "hybrid_scenario", "square_width": 10, "circle_radius": 7, "human_num": n,
                "traffic_length": 14, "traffic_height": 3},
        "humans": {"visible": "true", "policy": "sfm_guo", "radius": 0.3, "v_pref": 1, "sensor": "coordinates"},
        "robot": {"visible": "false", "policy": "none", "radius": 0.3, "v_pref": 1, "sensor": "coordinates"},
    })
    return cfg


def measure(env, fn, warmup, iters):
    import torch

    for _ in range(warmup):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=4096)
    ap.add_argument("--humans", type=int, nargs="+", default=[5, 25])
    ap.add_argument("--policies", nargs="+", default=["sfm_moussaid", "sfm_helbing", "ssp"])
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--visible", action="store_true", help="the robot as the last row of every world")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.policy_no_train.policy_factory import policy_factory
    from social_navigation_pyenvs_amd import _lib
    from social_navigation_pyenvs_amd.social_gym.social_nav_gym import BatchedSocialNavGym

    has_fused = hasattr(_lib.load(), "cs_gym_step_policy")
    build_id = None
    if hasattr(_lib.load(), "cs_build_id"):
        import ctypes as C

        _lib.load().cs_build_id.restype = C.c_char_p
        build_id = _lib.load().cs_build_id().decode()
    mmm = lambda xs: dict(min=round(min(xs), 2), median=round(sorted(xs)[len(xs) // 2], 2), max=round(max(xs), 2))
    for n in args.humans:
        env = BatchedSocialNavGym(_config(n), args.worlds, robot_visible=args.visible)
        env.reset(phase="test", first_case=0, device=True)
        buf = env.action_buffer()
        with torch.cuda.stream(env.device_stream()):
            for name in args.policies:
                pol = policy_factory[name]()
                act = measure(env, lambda: env.act_device(pol), args.warmup, args.iters)
                step = measure(env, lambda: env.step_device(buf), args.warmup, args.iters)
                both, fused = [], []
                for _ in range(max(1, args.repeats)):
                    both.append(measure(env, lambda: (env.act_device(pol), env.step_device(buf)), args.warmup, args.iters))
                    if has_fused:
                        fused.append(measure(env, lambda: env.act_step_device(pol), args.warmup, args.iters))
                row = dict(label=args.label, worlds=args.worlds, humans=n, visible=bool(args.visible), policy=name, act_us=round(act, 2),
                           step_us=round(step, 2), act_step_us=mmm(both), act_over_step=round(act / step, 3),
                           build_id=build_id)
                if has_fused:
                    row.update(fused_us=mmm(fused), fused_variant=env.act_step_variant().split(" grid")[0])
                line = json.dumps(row)
                print(line, flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(line + "\n")
        env.close()


if __name__ == "__main__":
    main()
