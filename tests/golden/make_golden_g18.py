#!/usr/bin/env python3
"""Generate tests/golden/g18_policy_no_train.npz by RUNNING THE REFERENCE's no-train robot policies.

TEST INFRASTRUCTURE ONLY.  Run from the repo root:  python tests/golden/make_golden_g18.py

The reference is imported through make_golden.py's harness; only numbers (inputs and what the reference produced) and, for the
HSFM probe, the exception class and message the reference raised are written.  Case kinds:

  decisions every BlindPlanner / SimpleSocialPlanner / SFMHelbing / SFMGuo / SFMMoussaid .predict call of reference episodes
            (SocialNavSim.set_robot_policy(name, crowdnav_policy=True) + run_k_steps): circular crossing and parallel traffic, robot
            visible / invisible, 5 and 25 humans.  robot = FullState (px, py, vx, vy, radius, gx, gy, v_pref, theta), obs [n][5],
            time_step, action (vx, vy).  Stacked into one case (stack()).
  edges     synthetic predict calls: robot within its radius of the goal and exactly on it, ssp surface distances straddling 0.2,
            overlapping bodies (the k1 / k2 contact terms), a Moussaid pair with equal velocities, no humans at all, random states.
  episode   whole run_k_steps(additional_info=True) episodes: every output (human_states, robot_states, collision, time_to_goal,
            success, truncated), with the initial rows and goal lists the simulator started from.
  hsfm      the exception the reference raises when an HSFM robot policy drives its simulator.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (imports the reference through _refharness)
from golden_io import save_cases  # noqa: E402

ns = mg.ns
SUPPORTED = ["bp", "ssp", "sfm_helbing", "sfm_guo", "sfm_moussaid"]
HSFM = ["hsfm_farina", "hsfm_guo", "hsfm_moussaid", "hsfm_new", "hsfm_new_guo", "hsfm_new_moussaid"]


def full_state_array(s):
    return np.array([s.px, s.py, s.vx, s.vy, s.radius, s.gx, s.gy, s.v_pref, s.theta], np.float64)


def obs_array(humans):
    return np.array([[h.px, h.py, h.vx, h.vy, h.radius] for h in humans], np.float64).reshape(len(humans), 5)


def make_sim(scenario, n, human_policy, robot_visible, dt, seed):
    np.random.seed(seed)
    if scenario == "circular_crossing":
        cfg = dict(circle_radius=7 if n > 5 else 4, n_actors=n, randomize_human_positions=n > 5, randomize_human_attributes=False)
    else:
        cfg = dict(traffic_length=14, traffic_height=5 if n > 5 else 3, n_actors=n, randomize_human_attributes=False)
    cfg.update(insert_robot=True, human_policy=human_policy, headless=True, robot_visible=robot_visible)
    sim = ns.sim.SocialNavSim(cfg, scenario)
    sim.set_time_step(dt)        # (a module global of the reference: set for every simulator made here)
    return sim, cfg


def initial(sim):
    mm = sim.motion_model_manager
    return dict(init_humans=np.array([[*h.position, h.yaw, *h.linear_velocity, *h.body_velocity, h.angular_velocity, h.radius, h.mass,
                                       *h.goals[0], h.desired_speed] for h in sim.humans], np.float64),
                init_goals=[[list(map(float, g)) for g in h.goals] for h in sim.humans],
                init_robot=np.array(sim.robot.get_safe_state(), np.float64),
                init_robot_goals=[list(map(float, g)) for g in sim.robot.goals])


def decisions():
    cases = []
    k = 0
    for pol in SUPPORTED:
        for scenario in ("circular_crossing", "parallel_traffic"):
            for visible in (False, True):
                for n in (5, 25):
                    k += 1
                    sim, cfg = make_sim(scenario, n, "sfm_guo", visible, 1 / 60, 1800 + k)
                    sim.set_robot_policy(pol, crowdnav_policy=True)
                    policy = sim.robot.policy
                    orig = policy.predict

                    def predict(state, _o=orig, _p=pol, _s=scenario, _v=visible, _n=n):
                        a = _o(state)
                        cases.append(dict(kind="decision", policy=_p, scenario=_s, robot_visible=_v, n=_n, robot=full_state_array(state.self_state),
                                          obs=obs_array(state.human_states), time_step=float(policy.time_step), action=np.array([a.vx, a.vy], np.float64)))
                        return a
                    policy.predict = predict
                    sim.run_k_steps(120, additional_info=True, stop_when_collision_or_goal=True, save_states_time_step=1 / 60)
    return cases


def edge_cases():
    State, Obs = ns.state.FullState, ns.state.ObservableState
    from crowd_nav.utils.state import JointState
    from crowd_nav.policy_no_train.policy_factory import policy_factory
    rng = np.random.default_rng(1818)
    cases = []

    def run(tag, pol, robot, humans):
        p = policy_factory[pol]()
        p.time_step = 0.25
        st = JointState(State(*robot), [Obs(*h) for h in humans])
        a = p.predict(st)
        cases.append(dict(kind="edge", tag=tag, policy=pol, n=len(humans), robot=np.array(robot[:9], np.float64).reshape(9),
                          obs=np.array(humans, np.float64).reshape(len(humans), 5), time_step=0.25, action=np.array([a.vx, a.vy], np.float64)))

    far = [[4.0, 4.0, 0.1, -0.2, 0.3], [-3.0, 2.0, 0.5, 0.0, 0.4]]
    for pol in SUPPORTED:
        run("on_goal", pol, [1.0, 2.0, 0.3, -0.1, 0.3, 1.0, 2.0, 1.0, 0.0], far)
        run("within_radius", pol, [1.0, 2.0, 0.3, -0.1, 0.3, 1.1, 2.15, 1.0, 0.0], far)
        run("no_humans", pol, [0.5, -1.0, 0.2, 0.4, 0.3, 3.0, 4.0, 1.0, 0.0], [])
        for j in range(2):   # overlapping bodies: the k1 / k2 contact terms
            d = 0.45 + 0.1 * j
            run("overlap", pol, [0.0, 0.0, 0.3, 0.2, 0.3, 5.0, 1.0, 1.0, 0.0], [[d * 0.8, d * 0.6, -0.4, 0.1, 0.3]] + far)
    for sgn in (-1, 1):        # ssp: surface distance 0.2 -/+ 1e-4 and 1e-3
        for eps in (1e-4, 1e-3):
            dist = 0.3 + 0.3 + 0.2 + sgn * eps
            run("ssp_threshold", "ssp", [0.0, 0.0, 0.0, 0.0, 0.3, 5.0, 0.0, 1.0, 0.0], [[dist * 0.6, dist * 0.8, 0.0, 0.0, 0.3]] + far)
    for v in ((0.3, 0.4), (0.0, 0.0), (-0.7, 0.2)):   # Moussaid: robot and human with equal velocities
        run("moussaid_equal_velocity", "sfm_moussaid", [0.0, 0.0, v[0], v[1], 0.3, 5.0, 1.0, 1.0, 0.0], [[1.2, 0.5, v[0], v[1], 0.3]])
    for pol in SUPPORTED:      # random states, 0 .. 25 humans
        for _ in range(30):
            n = int(rng.choice([1, 3, 5, 25]))
            robot = [*rng.uniform(-4, 4, 2), *rng.uniform(-1, 1, 2), rng.uniform(0.2, 0.4), *rng.uniform(-5, 5, 2), rng.uniform(0.5, 1.5), 0.0]
            humans = [[*rng.uniform(-5, 5, 2), *rng.uniform(-1, 1, 2), rng.uniform(0.3, 0.5)] for _ in range(n)]
            run("random", pol, robot, humans)
    return cases


def episodes():
    """12 episodes: long ones (700 updates, long enough for a robot to reach its goal) saved every robot time step, short ones
    (160 / 120 updates) saved every update -- the rows the float64 replay of the CPU suite checks the flags on."""
    cases = []
    plan = []
    for k, pol in enumerate(SUPPORTED):
        plan.append((pol, "circular_crossing", 5, True, False, 0.25, 700, 1901 + k))
        plan.append((pol, "parallel_traffic", 5, False, True, 0.0125, 160, 1911 + k))
    plan.append(("sfm_helbing", "circular_crossing", 7, False, False, 0.0125, 120, 1921))
    plan.append(("ssp", "circular_crossing", 7, False, True, 0.25, 700, 1922))
    for pol, scenario, n, visible, stop, save, steps, seed in plan:
        sim, cfg = make_sim(scenario, n, "sfm_helbing" if seed % 2 else "sfm_guo", visible, 0.0125, seed)
        init = initial(sim)
        sim.set_robot_policy(pol, crowdnav_policy=True)
        hs, rs, col, ttg, succ, trunc = sim.run_k_steps(steps, additional_info=True, stop_when_collision_or_goal=stop, save_states_time_step=save)
        cases.append(dict(kind="episode", policy=pol, scenario=scenario, n=n, robot_visible=visible, human_policy=cfg["human_policy"],
                          seed=seed, config=cfg, steps=steps, stop=stop, save_states_time_step=save, dt=0.0125, human_states=np.array(hs),
                          robot_states=np.array(rs), collision=bool(col), time_to_goal=None if ttg is None else float(ttg), success=bool(succ),
                          truncated=bool(trunc), **init))
        print(pol, scenario, n, visible, stop, save, hs.shape, col, ttg, succ, trunc, flush=True)
    return cases


def hsfm_probe():
    cases = []
    for pol in HSFM:
        sim, _ = make_sim("circular_crossing", 5, "sfm_guo", False, 1 / 60, 1700)
        try:
            sim.set_robot_policy(pol, crowdnav_policy=True)
            sim.run_k_steps(20, additional_info=True, save_states_time_step=1 / 60)
            cases.append(dict(kind="hsfm", policy=pol, error=None, message=None))
        except Exception as e:   # noqa: BLE001 (what the reference raises IS the record)
            cases.append(dict(kind="hsfm", policy=pol, error=type(e).__name__, message=str(e)))
    return cases


def stack(kind, rows):
    """The predict calls of one kind as ONE case of stacked arrays (a case per call costs a zip entry and an .npy header per array):
    robot [N][9], time_step [N], action [N][2], n [N], obs [sum n][5] (call i owns rows offset[i] .. offset[i] + n[i]), and per call the
    index of its policy in `policies`, its tag / scenario, robot visibility."""
    n = np.array([r["n"] for r in rows], np.int32)
    return dict(kind=kind, policies=SUPPORTED, policy_index=np.array([SUPPORTED.index(r["policy"]) for r in rows], np.int8), n=n,
                offset=np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int32), robot=np.stack([r["robot"] for r in rows]),
                obs=np.concatenate([r["obs"] for r in rows]), time_step=np.array([r["time_step"] for r in rows]),
                action=np.stack([r["action"] for r in rows]), tags=[r.get("tag") or r.get("scenario") for r in rows],
                robot_visible=np.array([bool(r.get("robot_visible", False)) for r in rows]))


if __name__ == "__main__":
    rows = decisions()
    print("decisions:", len(rows), flush=True)
    cases = [stack("decisions", rows), stack("edges", edge_cases())]
    cases += episodes()
    cases += hsfm_probe()
    print("g18_policy_no_train:", len(cases), "cases ->", save_cases("g18_policy_no_train", cases))
