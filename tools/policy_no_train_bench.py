#!/usr/bin/env python3
"""Device time of the batched no-train robot policies (BatchedSocialNavGym.act_device, csrc/policy_no_train.hip) against the Gym step
they feed, measured in the same process on the same worlds:

    act        act_device(policy) alone
    step       step_device(action_buffer()) alone
    act+step   act_device -> step_device, the evaluation loop of a baseline

Everything runs inside ``with torch.cuda.stream(env.device_stream())`` (no cross-stream waits); device events bracket `--iters`
iterations after `--warmup` ones; the figure is the mean per iteration.  Prints one JSON line per (worlds, humans, policy).

    python tools/policy_no_train_bench.py [--worlds 4096] [--humans 5 25] [--policies sfm_moussaid bp] [--iters 200]
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
    args = ap.parse_args()
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.policy_no_train.policy_factory import policy_factory
    from social_navigation_pyenvs_amd.social_gym.social_nav_gym import BatchedSocialNavGym

    for n in args.humans:
        env = BatchedSocialNavGym(_config(n), args.worlds)
        env.reset(phase="test", first_case=0, device=True)
        buf = env.action_buffer()
        with torch.cuda.stream(env.device_stream()):
            for name in args.policies:
                pol = policy_factory[name]()
                act = measure(env, lambda: env.act_device(pol), args.warmup, args.iters)
                step = measure(env, lambda: env.step_device(buf), args.warmup, args.iters)
                both = measure(env, lambda: (env.act_device(pol), env.step_device(buf)), args.warmup, args.iters)
                print(json.dumps(dict(worlds=args.worlds, humans=n, policy=name, act_us=round(act, 2), step_us=round(step, 2),
                                      act_step_us=round(both, 2), act_over_step=round(act / step, 3))), flush=True)


if __name__ == "__main__":
    main()
