"""CPU suite of the no-train CrowdNav robot policies (crowd_nav/policy_no_train, csrc/policy_no_train.hip).

A float64 restatement of the five policies, written from the reference's formulas (blind_planner.py, simple_social_planner.py,
sfm_*.py, forces.py), reproduces every action of golden G18 (recorded from the reference) and the robot half of its run_k_steps
episodes; the factory, the C entry point's argument checks and the unchanged humans-only simulator need no device either."""
import ctypes as C
import math

import numpy as np
import pytest

from golden_io import load_cases

PARAMS = {
    "sfm_helbing": dict(relaxation_time=0.5, Ai=2000.0, Bi=0.08, k1=120000.0, k2=240000.0, mass=80.0),
    "sfm_guo": dict(relaxation_time=0.5, Ai=2000.0, Bi=0.08, Ci=120.0, Di=0.6, k1=120000.0, k2=240000.0, mass=80.0),
    "sfm_moussaid": dict(relaxation_time=0.5, Ei=360.0, agent_lambda=2.0, gamma=0.35, ns=2.0, ns1=3.0, k1=120000.0, k2=240000.0, mass=80.0),
}
REFERENCE_KEYS = ["none", "bp", "ssp", "orca", "socialforce", "sfm_helbing", "sfm_guo", "sfm_moussaid", "hsfm_farina", "hsfm_guo",
                  "hsfm_moussaid", "hsfm_new", "hsfm_new_guo", "hsfm_new_moussaid"]


def _wrap(a):
    if a > math.pi:
        a -= 2 * math.pi
    if a < -math.pi:
        a += 2 * math.pi
    return a


def policy_f64(policy, robot, obs, time_step):
    """Action (vx, vy) of `policy` for robot = (px, py, vx, vy, radius, gx, gy, v_pref, theta) and obs [n][5] rows, in float64."""
    px, py, vx, vy, rr, gx, gy, vd = (float(x) for x in robot[:8])
    obs = np.asarray(obs, np.float64).reshape(-1, 5)
    to_goal = math.atan2(gy - py, gx - px)
    if policy == "bp":
        return np.array([math.cos(to_goal) * vd, math.sin(to_goal) * vd])
    if policy == "ssp":
        for h in obs:
            if math.sqrt((h[0] - px) ** 2 + (h[1] - py) ** 2) - h[4] - rr <= 0.2:
                return np.zeros(2)
        return np.array([math.cos(to_goal) * vd, math.sin(to_goal) * vd])
    p = PARAMS[policy]
    v = np.array([vx, vy])
    pos = np.array([px, py])
    goal_vec = np.array([gx, gy]) - pos
    gd = math.sqrt(goal_vec @ goal_vec)
    desired = p["mass"] * (goal_vec / gd * vd - v) / p["relaxation_time"] if gd > rr else np.zeros(2)
    social = np.zeros(2)
    for h in obs:
        diff = pos - h[:2]
        d = np.linalg.norm(diff)
        nij = diff / d
        overlap = max(0.0, rr + h[4] - d)
        hv = h[2:4]
        if policy == "sfm_moussaid":
            inter = p["agent_lambda"] * (v - hv) - nij
            inorm = np.linalg.norm(inter)
            iij = inter / inorm
            # np.arctan2 as the reference calls it: an equal-velocity pair has |theta| ~ 1e-16 and its sign is decided there
            th = _wrap(np.arctan2(nij[1], nij[0]) - np.arctan2(iij[1], iij[0]) + math.pi)
            hij = np.array([-iij[1], iij[0]])
            F = p["gamma"] * inorm
            social = social - (p["Ei"] * math.exp(-d / F) * (math.exp(-(p["ns1"] * F * th) ** 2) * iij
                                                           + np.sign(th) * math.exp(-(p["ns"] * F * th) ** 2) * hij)
                             + p["k1"] * overlap * iij + p["k2"] * overlap * ((hv - v) @ hij) * hij)
        else:
            tij = np.array([-nij[1], nij[0]])
            rd = rr + h[4] - d
            normal = p["Ai"] * math.exp(rd / p["Bi"]) + p["k1"] * overlap
            tangent = p["k2"] * overlap * ((hv - v) @ tij)
            if policy == "sfm_guo":
                tangent = tangent + p["Ci"] * math.exp(rd / p["Di"])
            social = social + (normal * nij + tangent * tij)
    nv = v + (desired + social) / p["mass"] * time_step
    sp = math.sqrt(nv @ nv)
    return nv / sp * vd if sp > vd else nv


def unpack(case):
    """One dict per predict call of a stacked G18 case (make_golden_g18.stack: the calls' arrays stacked, obs rows by offset)."""
    out = []
    for i, (o, n) in enumerate(zip(case["offset"], case["n"])):
        out.append(dict(kind=case["kind"], policy=case["policies"][case["policy_index"][i]], tag=case["tags"][i], n=int(n),
                        robot=case["robot"][i], obs=case["obs"][o:o + n], time_step=float(case["time_step"][i]), action=case["action"][i]))
    return out


def _decisions():
    return [d for c in load_cases("g18_policy_no_train") if c["kind"] in ("decisions", "edges") for d in unpack(c)]


def test_g18_actions_restated_in_float64():
    cases = _decisions()
    assert len(cases) > 450 and {c["kind"] for c in cases} == {"decisions", "edges"}
    assert {c["policy"] for c in cases} == {"bp", "ssp", "sfm_helbing", "sfm_guo", "sfm_moussaid"}
    worst = 0.0
    for c in cases:
        got = policy_f64(c["policy"], c["robot"], c["obs"], c["time_step"])
        err = float(np.max(np.abs(got - c["action"])))
        assert err <= 1e-12, (c["policy"], c.get("tag"), err)
        worst = max(worst, err)
    # the at-goal convention: atan2(0, 0) = 0, the action is (v_pref, 0), not NaN
    on_goal = [c for c in cases if c.get("tag") == "on_goal" and c["policy"] == "bp"]
    assert on_goal and np.array_equal(on_goal[0]["action"], [on_goal[0]["robot"][7], 0.0])


def _is_multiple(x, d, tol=1e-7):
    m = x % d
    return abs(m) <= tol or abs(d - m) <= tol


def _replay_robot(c):
    """The robot's half of a G18 episode from the recorded human rows: decisions at robot time steps, pose between them, goal
    rotation, and -- with every update saved -- the collision / success / truncated flags."""
    dt, save = c["dt"], c["save_states_time_step"]
    stride = int(round(save / dt))
    hs, rs = c["human_states"], c["robot_states"]
    radii = c["init_humans"][:, 8]
    r0 = c["init_robot"]
    pos, vel, rr = r0[0:2].copy(), r0[3:5].copy(), float(r0[8])
    goals = [list(g) for g in c["init_robot_goals"]]
    rows = [np.array([pos[0], pos[1], r0[2], vel[0], vel[1], r0[7], goals[0][0], goals[0][1]])]
    collision = success = truncated = False
    ttg = None
    u = 0
    while len(rows) < len(rs):
        u += 1
        t_prev = (u - 1) * dt
        if _is_multiple(t_prev, 0.25):
            assert (u - 1) % stride == 0
            obs = np.concatenate([hs[(u - 1) // stride][:, [0, 1, 3, 4]], radii[:, None]], axis=1)
            a = policy_f64(c["policy"], [pos[0], pos[1], vel[0], vel[1], rr, goals[0][0], goals[0][1], 1.0, r0[2]], obs, 0.25)
            pos = pos + a * dt
            vel = a.copy()
            if np.linalg.norm(pos - np.array(goals[0])) < rr and len(goals) > 1:
                goals.append(goals.pop(0))
        else:
            pos = pos + vel * dt
        if _is_multiple(u * dt, save):
            rows.append(np.array([pos[0], pos[1], r0[2], vel[0], vel[1], r0[7], goals[0][0], goals[0][1]]))
        if stride == 1:
            hp = hs[u][:, 0:2]
            if np.any(np.linalg.norm(hp - pos, axis=1) < radii + rr):
                collision = True
            if not np.array_equal(rows[-1][6:8], rows[-2][6:8]):
                ttg, success = u * dt, True
            if u == c["steps"] and not collision and not success:
                truncated = True
    return np.array(rows), (collision, ttg, success, truncated)


def test_g18_episodes_robot_rows_and_flags_restated():
    eps = [c for c in load_cases("g18_policy_no_train") if c["kind"] == "episode"]
    assert len(eps) >= 12
    assert {c["save_states_time_step"] for c in eps} == {0.0125, 0.25} and {c["stop"] for c in eps} == {True, False}
    outcomes = set()
    for c in eps:
        rows, flags = _replay_robot(c)
        err = float(np.max(np.abs(rows - c["robot_states"])))
        assert err < 1e-9, (c["policy"], c["seed"], err)
        if c["save_states_time_step"] == c["dt"]:
            assert flags[0] == c["collision"] and flags[2] == c["success"] and flags[3] == c["truncated"], (c["policy"], c["seed"], flags)
            assert (flags[1] is None) == (c["time_to_goal"] is None)
            if flags[1] is not None:
                assert abs(flags[1] - c["time_to_goal"]) < 1e-12
        outcomes.add("collision" if c["collision"] else ("success" if c["success"] else "truncated"))
    assert outcomes == {"collision", "success", "truncated"}   # the recorded episodes are informative


def test_factory_keys_and_unsupported_reasons():
    from social_navigation_pyenvs_amd.crowd_nav.policy_no_train.policy_factory import SUPPORTED, policy_factory

    assert sorted(policy_factory) == sorted(REFERENCE_KEYS)
    assert policy_factory["none"]() is None
    for name in SUPPORTED:
        p = policy_factory[name]()
        assert p.name == name and p.kinematics == "holonomic" and p.trainable is False and p.last_state is None
    assert policy_factory["bp"]().multiagent_training is True and policy_factory["sfm_guo"]().multiagent_training is None
    for name in ("orca", "socialforce"):
        with pytest.raises(NotImplementedError, match="rvo2" if name == "orca" else "socialforce"):
            policy_factory[name]()
    probe = {c["policy"]: c for c in load_cases("g18_policy_no_train") if c["kind"] == "hsfm"}
    assert sorted(probe) == sorted(k for k in REFERENCE_KEYS if k.startswith("hsfm"))
    for name, c in probe.items():
        assert c["error"] == "AttributeError", c         # G18 (d): the reference itself fails
        with pytest.raises(NotImplementedError) as e:
            policy_factory[name]()
        assert c["message"] in str(e.value)


def test_parameters_pack_into_agent_slots():
    from social_navigation_pyenvs_amd.crowd_nav.policy_no_train.policy import CS_PNT_MASS, pack_params
    from social_navigation_pyenvs_amd.crowd_nav.policy_no_train.policy_factory import policy_factory

    m = pack_params(policy_factory["sfm_moussaid"]().params)
    assert m[0] == 0.5 and m[9] == 360 and m[12] == 2.0 and m[13] == np.float32(0.35) and m[14] == 2.0 and m[15] == 3.0
    assert m[10] == 120000 and m[11] == 240000 and m[CS_PNT_MASS] == 80
    g = pack_params(policy_factory["sfm_guo"]().params)
    assert g[1] == 2000 and g[3] == np.float32(0.08) and g[5] == 120 and g[7] == np.float32(0.6)
    assert policy_factory["bp"]().packed_params() is None


def test_entry_point_rejects_bad_arguments_without_a_device():
    import __graft_entry__ as g

    g.build()
    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    fake = C.c_void_p(64)          # never dereferenced: every call below fails its argument checks first
    prm = (C.c_float * 21)(*([0.5] + [1.0] * 19 + [80.0]))
    ok = dict(policy=2, W=4, n=5, robot=fake, obs=fake, cols=5, params=prm, act=fake)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cs_policy_no_train(C.c_int(a["policy"]), C.c_int(a["W"]), C.c_int(a["n"]), a["robot"], a["obs"], C.c_int(a["cols"]),
                                      C.c_float(0.25), a["params"], a["act"], None)

    for bad in (dict(policy=5), dict(policy=-1), dict(W=0), dict(W=-3), dict(n=-1), dict(cols=6), dict(cols=13), dict(robot=None),
                dict(obs=None), dict(act=None), dict(params=None)):
        assert call(**bad) == _lib.CS_ERR_ARG, bad
    with pytest.raises(ValueError, match="unknown no-train policy"):
        _lib.check(call(policy=7))


def _sim(monkeypatch):
    """A headless circle crossing whose crowd step is replaced by a deterministic host stand-in (no device)."""
    from social_navigation_pyenvs_amd.social_gym.social_nav_sim import SocialNavSim

    np.random.seed(5)
    sim = SocialNavSim(dict(circle_radius=4, n_actors=3, insert_robot=True, human_policy="sfm_guo", headless=True), "circular_crossing")
    mm = sim.motion_model_manager
    calls = []

    def fake_update(t, dt, post_update=True):
        calls.append((t, dt))
        mm.states[:len(sim.humans), 0] += 1.0
        mm.states[:len(sim.humans), 3] = 0.5

    monkeypatch.setattr(mm, "update_humans", fake_update)
    return sim, calls


def test_simulator_without_policy_keeps_its_humans_only_contract(monkeypatch):
    sim, calls = _sim(monkeypatch)
    x0 = sim.motion_model_manager.get_human_states()[:, 0].copy()
    robot0 = sim.robot.get_safe_state()
    out = sim.run_k_steps(4, additional_info=True, stop_when_collision_or_goal=True, save_states_time_step=0.25)
    assert isinstance(out, np.ndarray) and out.shape == (4, 3, 8)       # states BEFORE each update, no final state, no flags
    x = x0
    for k in range(4):
        assert np.array_equal(out[k][:, 0], x)
        x = x + 1.0
    assert [dt for _, dt in calls] == [sim.sampling_time] * 4
    assert np.array_equal(sim.robot.get_safe_state(), robot0)           # nobody moved the robot
    sim.update()
    assert sim.n_updates == 5 and np.array_equal(sim.robot.get_safe_state(), robot0)
    # a human motion model for the robot (crowdnav_policy=False) does not switch the update path either
    sim.set_robot_policy("sfm_guo", crowdnav_policy=False)
    assert not sim._policy_drives_robot()


def test_set_robot_policy_arguments(monkeypatch):
    sim, _ = _sim(monkeypatch)
    with pytest.raises(NotImplementedError):
        sim.set_robot_policy("sarl", crowdnav_policy=True, model_dir="/nonexistent")
    for name in ("orca", "hsfm_farina"):
        with pytest.raises(NotImplementedError):
            sim.set_robot_policy(name, crowdnav_policy=True)
    sim.set_robot_policy("bp", crowdnav_policy=True)
    assert sim._policy_drives_robot() and sim.robot.policy.time_step == 0.25 and sim.robot.desired_speed == 1
    with pytest.raises(ValueError, match="multiple of environment sampling time"):
        sim.run_k_steps(3, additional_info=True, save_states_time_step=0.01)
    with pytest.raises(ValueError, match="additional info"):
        sim.run_k_steps(3, additional_info=False, stop_when_collision_or_goal=True, save_states_time_step=sim.sampling_time)
