#!/usr/bin/env python3
"""Generate tests/golden/g27_social_momentum_blocks.npz by RUNNING THE REFERENCE's ``MotionModelManager("social_momentum")`` over several
consecutive ``update_humans`` calls with ``parallel_traffic_humans_respawn`` on.

TEST INFRASTRUCTURE ONLY.  Run from the repo root:  python tests/golden/make_golden_g27.py

The reference is imported through make_golden.py's harness; only numbers are written.  A case is one sequence of K calls on a corridor of
humans walking towards -x: per-human radius, safety space and a desired speed drawn from a continuous range, goal lists of length 1 to 3 (one
human stands within its radius of a first goal, so its list rotates in the first call), two humans just outside the 3 m zone of their goal
so that BOTH respawn in the same call, one human beyond +bound_y and one beyond -bound_y.  With a considered robot, the robot is moved by hand
before every call (position += action dt, velocity = action: what robot.step(ActionXY) does) and is, in one case, the rightmost entity with
the largest radius + safety space.  Per case:

  n, dt, robot_visible, respawn_bounds, calls
  radius, safety, vd [n]              the humans' constants
  in_pos, in_vel [n, 2], in_goals [n, 3, 2] (NaN-padded)   the state before the first call
  robot0 [6], action [2]              px, py, vx, vy, radius, safety space of the robot before its first move; its constant action
  out_pos, out_vel [K, n, 2], out_goals [K, n, 3, 2], out_robot [K, 6], respawned [K, n]   after (the robot: as seen by) every call
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (imports the reference through _refharness)
from golden_io import save_cases  # noqa: E402

DT = 0.25
BOUNDS = [7.0, 1.5]
GOAL_X = -9.0
# (seed, n, robot_visible, calls, robot far right with the largest margin)
CASES = [(2701, 6, False, 8, False), (2702, 6, True, 8, False), (2703, 12, True, 6, True), (2704, 12, False, 6, False), (2705, 3, True, 6, True)]


def corridor(rng, n):
    pts = []
    while len(pts) < n:
        p = np.array([rng.uniform(-4.0, 5.0), rng.uniform(-1.4, 1.4)])
        if all(np.linalg.norm(p - q) > 1.0 for q in pts):
            pts.append(p)
    pts = np.array(pts)
    # two humans just outside the 3 m zone of their goal (both enter it in one call), above the others; two outside the y bounds
    pts[0] = [GOAL_X + 3.05, 0.6]
    pts[n - 1] = [GOAL_X + 3.12, -0.7]
    if n >= 6:
        pts[2, 1], pts[3, 1] = 1.9, -1.8
        pts[4] = [GOAL_X + 3.6, 0.0]      # enters the zone a few calls later, alone
    return pts


def generate():
    ns = mg.ns
    cases = []
    for seed, n, robot_visible, calls, robot_far in CASES:
        rng = np.random.default_rng(seed)
        pts = corridor(rng, n)
        humans = {}
        for i in range(n):
            p = pts[i]
            goals = [[GOAL_X, float(p[1])]]
            length = 1 + (i + seed) % 3
            if length >= 2:
                goals.append([GOAL_X, float(-p[1])])
            if length == 3:
                goals.append([float(-GOAL_X), float(p[1])])
            if i == 1:            # within its radius of a first goal: the list rotates in the first call, the corridor goal becomes the head
                goals = [[float(p[0] + 0.1), float(p[1])]] + goals[:2]
            humans[i] = {"pos": [float(p[0]), float(p[1])], "yaw": float(np.pi), "goals": goals,
                         "des_speed": float(rng.uniform(0.6, 1.4)), "radius": float(rng.uniform(0.25, 0.45))}
        cfg = {"headless": True, "motion_model": "social_momentum", "runge_kutta": False, "robot_visible": robot_visible, "grid": False,
               "humans": humans, "walls": []}
        if robot_visible:
            cfg["robot"] = {"pos": [9.0, 0.3] if robot_far else [1.0, 0.1], "yaw": 0.0, "radius": 0.5 if robot_far else 0.3,
                            "goals": [[-8.0, 0.0]]}
        sim = ns.sim.SocialNavSim(cfg, scenario="custom_config", parallelize_humans=False)
        mm = sim.motion_model_manager
        assert bool(mm.consider_robot) == robot_visible
        mm.parallel_traffic_humans_respawn = True
        mm.respawn_bounds = list(BOUNDS)
        for h in mm.humans:
            h.safety_space = float(rng.uniform(0.0, 0.08))
            h.linear_velocity = np.array([-h.desired_speed, 0.0])
        action = np.array([-0.35, 0.05]) if not robot_far else np.array([-0.2, -0.1])
        robot0 = np.zeros(6)
        if robot_visible:
            sim.robot.safety_space = 0.12 if robot_far else 0.02
            sim.robot.linear_velocity = np.zeros(2)
            robot0 = np.array([*sim.robot.position, *sim.robot.linear_velocity, sim.robot.radius, sim.robot.safety_space], dtype=float)

        def snap():
            g = np.full((n, 3, 2), np.nan)
            for i, h in enumerate(mm.humans):
                g[i, :len(h.goals)] = np.array(h.goals, dtype=float)
            return (np.array([h.position for h in mm.humans], dtype=float), np.array([h.linear_velocity for h in mm.humans], dtype=float), g)

        in_pos, in_vel, in_goals = snap()
        out_pos, out_vel, out_goals, out_robot, respawned = [], [], [], [], []
        for k in range(calls):
            if robot_visible:
                sim.robot.position = np.array(sim.robot.position, dtype=float) + action * DT
                sim.robot.linear_velocity = action.copy()
                out_robot.append(np.array([*sim.robot.position, *sim.robot.linear_velocity, sim.robot.radius, sim.robot.safety_space], dtype=float))
            else:
                out_robot.append(np.zeros(6))
            x_before = np.array([h.position[0] for h in mm.humans]) + np.array([h.linear_velocity[0] for h in mm.humans]) * DT
            mm.update_humans(0.0, DT)
            p, v, g = snap()
            out_pos.append(p); out_vel.append(v); out_goals.append(g)
            respawned.append(p[:, 0] > x_before + 1.0)
        respawned = np.array(respawned)
        cases.append(dict(n=n, dt=DT, robot_visible=robot_visible, respawn_bounds=list(BOUNDS), calls=calls,
                          radius=np.array([h.radius for h in mm.humans], dtype=float),
                          safety=np.array([h.safety_space for h in mm.humans], dtype=float),
                          vd=np.array([h.desired_speed for h in mm.humans], dtype=float),
                          in_pos=in_pos, in_vel=in_vel, in_goals=in_goals, robot0=robot0, action=action,
                          out_pos=np.array(out_pos), out_vel=np.array(out_vel), out_goals=np.array(out_goals), out_robot=np.array(out_robot),
                          respawned=respawned))
    return cases


if __name__ == "__main__":
    cases = generate()
    for c in cases:
        per_call = c["respawned"].sum(axis=1)
        print(f"n {c['n']} robot {c['robot_visible']}: {c['calls']} calls, respawns per call {per_call.tolist()}")
    assert any(c["respawned"].sum(axis=1).max() >= 2 for c in cases), "no call with two respawns"
    path = save_cases("g27_social_momentum_blocks", cases)
    print("g27_social_momentum_blocks:", len(cases), "cases ->", path, os.path.getsize(path), "bytes")
