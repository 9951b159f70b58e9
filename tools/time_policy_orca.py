#!/usr/bin/env python3
"""Device time of the batched ORCA robot policy (BatchedSocialNavGym.act_device(ORCA), csrc/policy_orca.hip: a wavefront per world) on
resident hybrid_scenario worlds in their dense phase, beside what it is compared with, in the same process on the same worlds:

    orca        act_device(ORCA()): one launch of cs_policy_orca
    moussaid    act_device("sfm_moussaid"): the costliest of the other no-train policies (cs_policy_no_train, the same mapping)
    step        step_device(action_buffer()): the Gym step the decision feeds
    robot_lane  cs_robot_model_velocities with CS_ORCA through CrowdWorlds.robot_model_step(dt, just_velocities=True): the robot's ORCA
                MOTION MODEL, one LANE per world (k_orca_robot_step[_fast]) -- nearly the same arithmetic per world (it reads the crowd's
                state rows and update_goals_orca's preferred velocity), so it is the yardstick for the mapping.  It rewrites the robots'
                velocities, so the robot rows are put back after every measurement of it.

The worlds are stepped `--presteps` times with the ORCA robot first.  Everything runs inside ``with torch.cuda.stream(env.device_stream())``;
device events bracket `--iters` calls after `--warmup` ones and the figure is the mean per call.  The four are measured `--repeats` times,
alternating, and reported as min / median / max in microseconds.  Prints one JSON line per (worlds, humans); --out appends them to a file.

    python tools/time_policy_orca.py [--worlds 4096] [--humans 5 25] [--presteps 40] [--iters 200] [--repeats 5] [--out profiles/policy_orca.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from policy_no_train_bench import _config, measure  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", type=int, default=4096)
    ap.add_argument("--humans", type=int, nargs="+", default=[5, 25])
    ap.add_argument("--presteps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import ctypes as C

    import torch

    from social_navigation_pyenvs_amd import _lib
    from social_navigation_pyenvs_amd.crowd_nav.policy_no_train.orca import ORCA
    from social_navigation_pyenvs_amd.social_gym.social_nav_gym import BatchedSocialNavGym

    _lib.load().cs_build_id.restype = C.c_char_p
    build_id = _lib.load().cs_build_id().decode()
    mmm = lambda xs: dict(min=round(min(xs), 2), median=round(sorted(xs)[len(xs) // 2], 2), max=round(max(xs), 2))
    for n in args.humans:
        env = BatchedSocialNavGym(_config(n), args.worlds)
        env.reset(phase="test", first_case=0, device=True)
        buf = env.action_buffer()
        pol = ORCA()
        with torch.cuda.stream(env.device_stream()):
            for _ in range(args.presteps):                 # into the crowd's dense phase, the robot deciding with ORCA
                env.step_device(env.act_device(pol))
            env.act_device(pol)                            # the action the timed steps consume
            env.cw.set_robot_model("orca")
            rows = env.cw.d_robot.torch()
            saved = rows.clone()
            dt = env.robot_time_step

            def robot_lane():
                t = measure(env, lambda: env.cw.robot_model_step(dt, just_velocities=True), args.warmup, args.iters)
                rows.copy_(saved)
                return t

            # the three decisions leave the worlds where they are: they alternate on the dense worlds; the step moves them on (and resets the
            # worlds that end), so its rounds follow behind
            arms = dict(orca=lambda: measure(env, lambda: env.act_device(pol), args.warmup, args.iters),
                        moussaid=lambda: measure(env, lambda: env.act_device("sfm_moussaid"), args.warmup, args.iters),
                        robot_lane=robot_lane)
            times = {k: [] for k in list(arms) + ["step"]}
            for _ in range(max(1, args.repeats)):
                for k, fn in arms.items():
                    times[k].append(fn())
            env.act_device(pol)
            for _ in range(max(1, args.repeats)):
                times["step"].append(measure(env, lambda: env.step_device(buf), args.warmup, args.iters))
        row = dict(worlds=args.worlds, humans=n, presteps=args.presteps, iters=args.iters, repeats=args.repeats,
                   act_orca_us=mmm(times["orca"]), act_sfm_moussaid_us=mmm(times["moussaid"]), step_us=mmm(times["step"]),
                   robot_model_orca_one_lane_per_world_us=mmm(times["robot_lane"]),
                   orca_over_robot_lane=round(sorted(times["orca"])[len(times["orca"]) // 2] / sorted(times["robot_lane"])[len(times["robot_lane"]) // 2], 3),
                   build_id=build_id)
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        env.close()


if __name__ == "__main__":
    main()
