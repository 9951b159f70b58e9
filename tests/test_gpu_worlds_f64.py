"""GPU: float64 worlds (cs_step_f64, cs_update_humans_parallel_f64, cs_peek_f64; batched.CrowdWorlds64; the "f64" world precision of the
facade) against the goldens the reference recorded and against the float64 C oracle.  The code under test is never a yardstick.

The bars.  One substep: 1e-12 + 16 s, a fused block: 1e-10 + 16 s, where 1e-12 is the project's float64 bar (tests/test_oracle_golden.py),
and s is how far the ORACLE's own output moves when every incoming position is moved one ulp (np.nextafter): what float64 itself
determines of the case.  16 = a pair force chains about four library calls of a couple of ulps each.  A case with s > 1e-9 is one float64
does not determine: it is left out, and at most 5 % of a fixture's cases may be.  Errors are measured as tests/test_oracle_golden.py
measures them for the same fixture (relative to max(1, |reference|) for G1 and G13, absolute for G2, G7); s in the same measure."""
import numpy as np
import pytest

from golden_io import load_cases

pytestmark = pytest.mark.gpu

UNDETERMINED = 1e-9
MAX_LEFT_OUT = 0.05
MARGIN = 16.0


# ------------------------------------------------------------------------------------------------------------------ helpers
def _nudge(S):
    """Every position one ulp up."""
    S = np.array(S, dtype=np.float64, copy=True)
    S[..., 0:2] = np.nextafter(S[..., 0:2], np.inf)
    return S


def _err(got, ref, relative):
    """Worst difference over the entries the reference holds finite; an entry it holds non-finite must be non-finite here too."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    fin = np.isfinite(ref)
    if not np.all(np.isfinite(got[fin])) or np.any(np.isfinite(got[~fin])):
        return np.inf
    if not fin.any():
        return 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(got[fin] - ref[fin])
        if relative:
            d = d / np.maximum(1.0, np.abs(ref[fin]))
    return float(d.max())


def _record(group, err, bar):
    from parity_util import REPORT, record

    record(group, err, bar)
    r = REPORT[group]
    if err / bar >= r.get("worst_ratio", 0.0):
        r["worst_ratio"], r["bar_of_worst_ratio"] = err / bar, bar


def _check(group, what, err, s, floor, stats):
    """One comparison at the bar floor + 16 s; returns False (and counts it) when float64 does not determine the case."""
    stats["cases"] += 1
    if not (s <= UNDETERMINED):
        stats["left_out"] += 1
        return False
    bar = floor + MARGIN * s
    print(f"{group} {what}: err {err:.3e} s {s:.3e} bar {bar:.3e}")
    _record(group, err, bar)
    stats["worst_ratio"] = max(stats["worst_ratio"], err / bar)
    if not err <= bar:   # (every case of a fixture is measured before the test fails: _finish lists them all)
        stats["failed"].append(f"{what}: error {err:.3e} above {floor:.0e} + 16 x {s:.3e}")
        return False
    return True


def _stats():
    return {"cases": 0, "left_out": 0, "worst_ratio": 0.0, "failed": []}


def _finish(group, stats):
    print(f"{group}: {stats}")
    assert not stats["failed"], f"{group}: {len(stats['failed'])} of {stats['cases']} cases above their bar:\n" + "\n".join(stats["failed"])
    assert stats["left_out"] <= MAX_LEFT_OUT * stats["cases"], f"{group}: {stats['left_out']} of {stats['cases']} cases left out"


def _worlds(S, goals, P, safety, obstacles, type_, peq, **kw):
    from social_navigation_pyenvs_amd.batched import CrowdWorlds64

    return CrowdWorlds64(S, goals, P, safety, obstacles, type=type_, all_params_equal=peq, **kw)


# ------------------------------------------------------------------------------------------------------------------ (a) one substep
@pytest.mark.parametrize("group", ["g1_direct", "g1_episode"])
def test_one_substep_against_the_reference_records(group):
    """Every G1 case through cs_update_humans_parallel_f64 (out of place, the cases of one shape as the worlds of one launch):
    state_out and state_in_after at 1e-12 + 16 s, goals_out and the goal columns exactly."""
    from oracle import crowd_oracle as orc

    cases = load_cases(group)
    shapes = {}
    for k, c in enumerate(cases):
        obs = c.get("obstacles")
        key = (c["type"], c["state_in"].shape, c["goals_in"].shape, None if obs is None else obs.shape, bool(c["all_params_equal"]),
               bool(c["last_is_robot"]), float(c["dt"]))
        shapes.setdefault(key, []).append(k)
    stats = _stats()
    for (type_, _, _, oshape, peq, rob, dt), idx in shapes.items():
        cs = [cases[k] for k in idx]
        S = np.stack([c["state_in"] for c in cs]); G = np.stack([c["goals_in"] for c in cs])
        P = np.stack([c["params"] for c in cs]); saf = np.stack([c["safety"] for c in cs])
        obs = None if oshape is None else np.stack([c["obstacles"] for c in cs])
        cw = _worlds(S, G, P, saf, obs, type_, peq, robot_row=rob)
        out = cw.get_states(cw.update_humans_parallel(dt, in_place=False))
        after, goals = cw.get_states(), cw.get_goals()
        for j, (k, c) in enumerate(zip(idx, cs)):
            args = (c["goals_in"], c.get("obstacles"), c["params"], c["dt"], c["safety"], c["all_params_equal"], c["last_is_robot"])
            with np.errstate(all="ignore"):
                r0, a0, _ = orc.update_humans(c["type"], c["state_in"], *args)
                r1, a1, _ = orc.update_humans(c["type"], _nudge(c["state_in"]), *args)
            s = max(_err(r1, r0, True), _err(a1, a0, True))
            err = max(_err(out[j], c["state_out"], True), _err(after[j], c["state_in_after"], True))
            if _check(group, f"case {k} type {c['type']} n {c['n']}", err, s, 1e-12, stats):
                np.testing.assert_array_equal(goals[j], c["goals_out"])                                   # rotated goals (NaN == NaN)
                n = c["n"]
                np.testing.assert_array_equal(out[j][:n, 10:12], c["state_out"][:n, 10:12])
                np.testing.assert_array_equal(after[j][:n, 10:12], c["state_in_after"][:n, 10:12])
    assert stats["cases"] == {"g1_direct": 234, "g1_episode": 108}[group]
    _finish(group, stats)


# ------------------------------------------------------------------------------------------------------------------ (b) fused blocks
def _block_case(group, what, c, stats, relative, floor=1e-10, robot=None, robot_visible=False, n_substeps=None, respawn=None, rp=None):
    from oracle import crowd_oracle as orc

    respawn = bool(c["respawn"]) if respawn is None else respawn
    if rp is None:
        rp = (list(c["respawn_bounds"]) + [0.0]) if respawn else (0.0, 0.0, 0.0)
    nsub = c["n_substeps"] if n_substeps is None else n_substeps
    args = (c["in_goals"], c.get("in_obstacles"), c["in_params"], c["dt"], nsub, c["in_safety"], c["all_params_equal"])
    kw = dict(robot_visible=robot_visible, robot=robot, respawn=respawn, respawn_par=rp)
    with np.errstate(all="ignore"):
        r0, g0, _ = orc.step_block(c["type"], c["in_states"], *args, **kw)
        r1, g1, _ = orc.step_block(c["type"], _nudge(c["in_states"]), *args, **{**kw, "robot": None if robot is None else _nudge(robot)})
    s = max(_err(r1, r0, relative), _err(g1, g0, relative))
    cw = _worlds(c["in_states"], c["in_goals"], c["in_params"], c["in_safety"], c.get("in_obstacles"), c["type"], c["all_params_equal"],
                 robot_row=robot_visible, robot=robot, respawn_bounds=(rp[0], rp[1]) if respawn else None)
    cw.step(c["dt"], nsub)
    S, goals = cw.get_states()[0], cw.get_goals()[0]
    err = max(_err(S, c["out_states"], relative), _err(goals, c["out_goals"], relative))
    return _check(group, what, err, s, floor, stats)


def test_fused_blocks_g2_walls():
    """G2: 36 blocks of 20 fused substeps (walls, 5 / 25 / 8 humans, respawns) against the reference's records, absolute as
    tests/test_oracle_golden.py measures them.  35 blocks: worst error 2.7e-12 m at a bar of 9.0e-10 (case 34), otherwise <= 2.5e-15;
    case 32 (hsfm_new_guo, the reference's own omega diverged, s = 2.7e8) is left out.

    Moussaid's law multiplies a lateral term by sign(theta_ij), and with everybody at rest theta_ij = wrap(atan2(n) - atan2(i) + pi) is the
    rounding of the two atan2 values (+-1e-16).  The kernel takes them correctly rounded (csrc/atan2_cr.h), as the
    reference's C library does, and lands on the reference's side: case 35 (hsfm_new_moussaid, 8 humans starting at rest), 7.7e-10 m off with the
    device library's atan2, is within 1e-15 of the record."""
    stats = _stats()
    cases = load_cases("g2_block")
    for k, c in enumerate(cases):
        _block_case("g2_block", f"case {k} {c['kind']} {c['model']} n {c['n']}", c, stats, relative=False)
    assert stats["cases"] == len(cases) == 36
    _finish("g2_block", stats)


def test_fused_blocks_g13_sizes():
    stats = _stats()
    cases = load_cases("g13_block_sizes")
    for k, c in enumerate(cases):
        _block_case("g13_block_sizes", f"case {k} {c['kind']} {c['model']}", c, stats, relative=True)
    assert stats["cases"] == len(cases) == 36 and {c["n"] for c in cases} == {10, 25, 50}
    _finish("g13_block_sizes", stats)


def test_blocks_that_miss_1e5_in_float32_pass_in_float64():
    """The golden 20-substep blocks on which the float32 instantiation of the oracle ends outside north_star's 1e-5 (float32 state at
    k1 = 120 kN/m) -- found here with the oracle, not listed by hand: seven of them -- meet the float64 bar wherever float64 determines
    the block (five; in the other two the reference's own omega has diverged, hsfm_new* pushed into contact, and s is 1e7 .. 1e8)."""
    from oracle import crowd_oracle as orc

    missed = passed = 0
    for group, relative in (("g2_block", False), ("g13_block_sizes", True)):
        stats = _stats()
        for k, c in enumerate(load_cases(group)):
            rp = (list(c["respawn_bounds"]) + [0.0]) if c["respawn"] else (0.0, 0.0, 0.0)
            up = lambda x: None if x is None else np.asarray(x, np.float32).astype(np.float64)
            args = (c["type"], up(c["in_states"]), up(c["in_goals"]), up(c.get("in_obstacles")), up(c["in_params"]), c["dt"], c["n_substeps"],
                    up(c["in_safety"]), c["all_params_equal"])
            with np.errstate(all="ignore"):
                r32 = orc.step_block(*args, respawn=c["respawn"], respawn_par=rp, dtype=np.float32)[0]
                r64 = orc.step_block(*args, respawn=c["respawn"], respawn_par=rp)[0]
            if np.max(np.abs(r32[:, [0, 1, 3, 4]] - r64[:, [0, 1, 3, 4]])) > 1e-5:
                missed += 1
                passed += int(_block_case(group + "_f32_misses", f"case {k} {c['kind']} {c['model']}", c, stats, relative))
    assert passed >= 4 and missed - passed <= 2, (missed, passed)


def test_respawn_g7():
    stats = _stats()
    cases = load_cases("g7_respawn")
    for k, c in enumerate(cases):
        rv = bool(c["robot_visible"])
        robot = c["in_states"][-1].copy() if rv else None
        rsafety = float(c["robot"][3])
        if rv:
            assert c["in_safety"][-1] == rsafety    # the robot's margin travels in the safety array
        _block_case("g7_respawn", f"case {k}", c, stats, relative=False, robot=robot, robot_visible=rv, n_substeps=1, respawn=True,
                    rp=list(c["respawn_bounds"]) + [rsafety])
        assert np.any(np.abs(c["out_states"][:, 0] - c["in_states"][:, 0]) > 1.0)   # the fixture really contains respawns
    assert stats["cases"] == len(cases) and stats["left_out"] == 0
    _finish("g7_respawn", stats)


def _gym_env(c):
    from test_facade_cpu import make_env

    env = make_env(c["model"], c["scenario"], c["human_num"], c["robot_visible"], c["headed_obs"])
    if c["safety_space"] > 0:
        env.set_safety_space(c["safety_space"])
    env.reset(phase=c["phase"], test_case=c["test_case"])
    return env


def test_gym_blocks_g3_with_the_recorded_actions():
    """mm_states of G3 over the 10 Gym steps: every step's 20 fused substeps with the robot's recorded action, from the recorded state
    (parameters, margins and the robot's constants from the host generators, which are bit-exact on G6).  316 of 320 steps compared, worst
    error / bar 2.3e-5; steps 0 of cases 27, 28, 30 (Moussaid at rest) are skipped by name, one step is left out.

    Moussaid's law multiplies a lateral term by sign(theta_ij), and with everybody at rest theta_ij = wrap(atan2(n) - atan2(i) + pi) is the
    rounding of the two atan2 values (+-1e-16).  The kernel takes them correctly rounded (csrc/atan2_cr.h), as the
    reference's C library does, and lands on the reference's side: case 29 step 0 (sfm_moussaid at rest), 1.0e-8 m off with the device library's atan2,
    is within 1e-15 of the record."""
    from oracle import crowd_oracle as orc

    stats, skipped = _stats(), []
    for ci, c in enumerate(load_cases("g3_gym")):
        env = _gym_env(c)
        mm = env.motion_model_manager
        rv = bool(c["robot_visible"])
        respawn = bool(mm.parallel_traffic_humans_respawn)
        bounds = tuple(float(x) for x in mm.respawn_bounds) if respawn else None
        rb0 = np.asarray(env.robot.get_safe_state(), dtype=np.float64)
        n = len(mm.humans)
        for k in range(len(c["actions"])):
            S = np.array(c["mm_states"][k], dtype=np.float64)
            rb = rb0.copy()
            rb[[0, 1, 2, 3, 4]] = c["robot_states"][k]
            if rv:
                S[-1] = rb
            a = np.asarray(c["actions"][k], dtype=np.float64)
            args = (c["mm_goals"][k], mm.obstacles, mm.params, env.time_step, env.time_step_factor, mm.safety_space, bool(mm.all_equal_humans))
            kw = dict(robot_visible=rv, action=a, respawn=respawn, respawn_par=(bounds + (0.0,)) if respawn else (0.0, 0.0, 0.0))
            with np.errstate(all="ignore"):
                r0 = orc.step_block(int(mm.sfm_type), S, *args, robot=rb, **kw)[0]
                r1 = orc.step_block(int(mm.sfm_type), _nudge(S), *args, robot=_nudge(rb), **kw)[0]
            s = _err(r1[:n], r0[:n], False)
            ref = c["mm_states"][k + 1]
            if _err(r0[:n, 0:8], ref[:n, 0:8], False) > 1e-10:
                # the oracle itself does not reproduce the record: Moussaid's sign(theta_ij) with everybody at rest -- theta_ij is +-1e-16
                # rounding noise in the reference and its sign picks a side at random (tests/test_gpu_facade.py skips
                # the same step) -- skipped by name
                assert c["model"].endswith("moussaid") and k == 0, (ci, c["model"], k)
                skipped.append((ci, c["model"], c["scenario"], k))
                continue
            cw = _worlds(S, c["mm_goals"][k], mm.params, mm.safety_space, mm.obstacles, int(mm.sfm_type), bool(mm.all_equal_humans),
                         robot_row=rv, robot=rb, respawn_bounds=bounds)
            cw.step(env.time_step, env.time_step_factor, a)
            got = cw.get_states()[0]
            err = _err(got[:n, 0:8], ref[:n, 0:8], False)
            if _check("g3_gym", f"case {ci} {c['model']} {c['scenario']} step {k}", err, s, 1e-10, stats):
                np.testing.assert_array_equal(cw.get_goals()[0], c["mm_goals"][k + 1])
                np.testing.assert_allclose(cw.get_robot()[0][[0, 1, 3, 4]], c["robot_states"][k + 1][[0, 1, 3, 4]], rtol=0, atol=1e-12)
    print("g3_gym skipped (Moussaid at rest, the oracle does not reproduce the record):", skipped)
    assert stats["cases"] + len(skipped) == 320 and len(skipped) <= 8
    _finish("g3_gym", stats)


# ------------------------------------------------------------------------------------------------------------------ (c) edges
_DEFAULT_P = {}


def _params(type_):
    """The reference's default parameter row of a model, from the recorded cases."""
    if not _DEFAULT_P:
        for c in load_cases("g1_direct"):
            _DEFAULT_P.setdefault(c["type"], c["params"][0].copy())
    return _DEFAULT_P[type_]


def _synthetic(seed, W, rows, robot, G, type_, per_agent, walls, reach=True):
    """W worlds of `rows` rows on a jittered 0.9 m lattice (neighbours in contact now and then), goal lists of 1..G goals NaN padded,
    one human per world standing on its first goal (a goal switch inside the block), optional polygon walls with NaN segments."""
    rng = np.random.default_rng(seed)
    n = rows - int(robot)
    side = int(np.ceil(np.sqrt(rows)))
    cell = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)[:rows] * 0.9
    S = np.zeros((W, rows, 13))
    S[..., 0:2] = cell[None] + rng.uniform(-0.12, 0.12, (W, rows, 2)) - side * 0.45
    S[..., 2] = rng.uniform(-np.pi, np.pi, (W, rows))
    S[..., 5:7] = rng.uniform(-0.6, 0.6, (W, rows, 2))
    if type_ >= 3:
        c, s = np.cos(S[..., 2]), np.sin(S[..., 2])
        S[..., 3], S[..., 4] = c * S[..., 5] - s * S[..., 6], s * S[..., 5] + c * S[..., 6]
        S[..., 7] = rng.uniform(-1, 1, (W, rows))
    else:
        S[..., 3:5] = rng.uniform(-0.6, 0.6, (W, rows, 2))
        S[..., 5:8] = 0.0
    S[..., 8] = rng.uniform(0.25, 0.4, (W, rows)); S[..., 9] = 75.0; S[..., 12] = rng.uniform(0.7, 1.3, (W, rows))
    goals = np.full((W, n, G, 2), np.nan)
    for w in range(W):
        for i in range(n):
            k = 1 + (w + i) % G
            goals[w, i, :k] = rng.uniform(-6, 6, (k, 2))
        if reach and n > 0:
            i = w % n
            goals[w, i] = rng.uniform(-6, 6, (G, 2))                                       # a full list: the rotation shows
            goals[w, i, 0] = S[w, i, 0:2] + 0.5 * S[w, i, 8] * np.array([0.6, -0.8])      # within the radius: switches at once
    S[:, :n, 10:12] = goals[:, :, 0]
    P = np.broadcast_to(_params(type_), (W, n, 20)).copy()
    if per_agent:
        P *= rng.uniform(0.9, 1.1, P.shape)
    safety = rng.uniform(0.0, 0.05, (W, rows))
    obs = None
    if walls:
        O, Smax = 3, 5
        obs = np.full((W, O, Smax, 2, 2), np.nan)
        for w in range(W):
            for o in range(O):
                k = 2 + (w + o) % 4                                                         # 2..5 segments, the rest NaN
                pts = rng.uniform(-1, 1, (k + 1, 2)) + np.array([(o - 1) * 5.0, 6.5 + o])
                obs[w, o, :k, 0], obs[w, o, :k, 1] = pts[:-1], pts[1:]
        if walls == "shared":
            obs = obs[0]
    rb = None
    if robot:
        rb = S[:, -1].copy()
        rb[:, 3:5] = rng.uniform(-0.5, 0.5, (W, 2))
        S[:, -1] = rb
    return S, goals, P, safety, obs, rb


def _oracle_block(type_, S, goals, P, safety, obs, peq, dt, nsub, robot, action, respawn=False, rp=(0.0, 0.0, 0.0)):
    from oracle import crowd_oracle as orc

    with np.errstate(all="ignore"):
        return orc.step_block(type_, S, goals, obs, P, dt, nsub, safety, peq, robot_visible=robot is not None, robot=robot, action=action,
                              respawn=respawn, respawn_par=rp)


EDGE_CASES = [
    # rows, robot, W, G, type, per-agent parameters, walls, substeps
    (1, False, 1, 1, 0, False, None, 1), (2, False, 3, 2, 1, True, None, 20), (2, True, 5, 1, 3, False, None, 20),
    (5, False, 65, 3, 2, False, "shared", 1), (5, True, 3, 2, 4, True, "per_world", 20), (25, False, 5, 2, 3, False, None, 20),
    (25, True, 3, 3, 5, False, "shared", 20), (25, False, 3, 1, 6, True, "per_world", 1), (63, False, 5, 2, 7, False, None, 1),
    (63, True, 3, 3, 8, True, None, 1), (64, False, 65, 2, 0, False, None, 1), (64, True, 3, 2, 1, False, "shared", 20),
    (64, False, 1, 3, 8, False, "per_world", 20), (5, False, 5, 3, 7, False, "shared", 20), (25, True, 65, 2, 2, True, None, 1),
    (5, True, 1, 3, 6, False, None, 20),
]


@pytest.mark.parametrize("rows,robot,W,G,type_,per_agent,walls,nsub", EDGE_CASES)
def test_edges_against_the_oracle(rows, robot, W, G, type_, per_agent, walls, nsub):
    """Synthetic worlds, several per launch (W = 65: a partial last workgroup), with the robot moved by a held action."""
    S, goals, P, safety, obs, rb = _synthetic(1000 + rows * 7 + W, W, rows, robot, G, type_, per_agent, walls)
    peq = not per_agent
    dt = 0.0125
    action = None if rb is None else np.tile([0.3, -0.2], (W, 1))
    r0, g0, b0 = _oracle_block(type_, S, goals, P, safety, obs, peq, dt, nsub, rb, action)
    r1, g1, _ = _oracle_block(type_, _nudge(S), goals, P, safety, obs, peq, dt, nsub, None if rb is None else _nudge(rb), action)
    cw = _worlds(S, goals, P, safety, obs, type_, peq, robot_row=robot, robot=rb)
    cw.step(dt, nsub, action)
    got, gg = cw.get_states(), cw.get_goals()
    stats = _stats()
    group = "f64_edges"
    for w in range(W):
        s = max(_err(r1[w], r0[w], True), _err(g1[w], g0[w], True))
        err = max(_err(got[w], r0[w], True), _err(gg[w], g0[w], True))
        _check(group, f"rows {rows} robot {robot} W {W} type {type_} nsub {nsub} world {w}", err, s, 1e-12 if nsub == 1 else 1e-10, stats)
    if rb is not None:
        np.testing.assert_allclose(cw.get_robot(), b0, rtol=0, atol=1e-13)
    if G > 1:
        n = rows - int(robot)
        for w in range(W):                                         # the human standing on its goal rotated its list
            np.testing.assert_array_equal(gg[w, w % n, G - 1], goals[w, w % n, 0])
    _finish(group, stats)


@pytest.mark.parametrize("type_,per_agent,walls", [(0, False, "shared"), (4, True, "per_world"), (8, False, None)])
def test_peek_inplace_batch_and_nan_invariants(type_, per_agent, walls):
    """Peek leaves state and goals bitwise untouched and equals a one-substep step; in place equals out of place bitwise; a world alone
    has the bits it has in any batch; a NaN row stays in its world."""
    W, rows, G, dt = 6, 26, 3, 0.0125
    S, goals, P, safety, obs, rb = _synthetic(77 + type_, W, rows, True, G, type_, per_agent, walls)
    peq = not per_agent
    mk = lambda sel=slice(None): _worlds(S[sel], goals[sel], P[sel], safety[sel], obs if (obs is None or obs.ndim == 4) else obs[sel], type_, peq,
                                         robot_row=True, robot=rb[sel])
    # peek
    cw = mk()
    s_before, g_before = cw.get_states(), cw.get_goals()
    nxt = cw.peek(dt)
    np.testing.assert_array_equal(cw.get_states().view(np.uint64), s_before.view(np.uint64))
    np.testing.assert_array_equal(cw.get_goals().view(np.uint64), g_before.view(np.uint64))
    cw.step(dt, 1)
    st, gl = cw.get_states(), cw.get_goals()
    n = rows - 1
    want = np.concatenate([st[:, :n, [0, 1, 2, 3, 4, 7]], gl[:, :, 0]], axis=-1)
    np.testing.assert_array_equal(nxt.view(np.uint64), want.view(np.uint64))
    # in place == out of place (cs_update_humans_parallel_f64: the state's last row is the robot row)
    a, b = mk(), mk()
    out = b.get_states(b.update_humans_parallel(dt, in_place=False))
    a.update_humans_parallel(dt, in_place=True)
    np.testing.assert_array_equal(a.get_states().view(np.uint64), out.view(np.uint64))
    np.testing.assert_array_equal(a.get_goals().view(np.uint64), b.get_goals().view(np.uint64))
    # a world alone has the bits it has in the batch
    full = mk()
    full.step(dt, 20, np.tile([0.2, 0.1], (W, 1)))
    for w in (0, 3, 5):
        alone = mk(slice(w, w + 1))
        alone.step(dt, 20, np.array([[0.2, 0.1]]))
        np.testing.assert_array_equal(alone.get_states()[0].view(np.uint64), full.get_states()[w].view(np.uint64))
        np.testing.assert_array_equal(alone.get_goals()[0].view(np.uint64), full.get_goals()[w].view(np.uint64))
    # a NaN row stays in its world
    S2 = S.copy()
    S2[2, 4, :] = np.nan
    sick = _worlds(S2, goals, P, safety, obs, type_, peq, robot_row=True, robot=rb)
    sick.step(dt, 20, np.tile([0.2, 0.1], (W, 1)))
    got, ref = sick.get_states(), full.get_states()
    others = [w for w in range(W) if w != 2]
    np.testing.assert_array_equal(got[others].view(np.uint64), ref[others].view(np.uint64))
    assert np.isnan(got[2, 4, 0])


def test_respawn_with_the_per_world_switch():
    """Parallel-traffic respawns inside a fused block, switched per world: against the oracle run with and without the rule."""
    type_, W, rows, G, dt, nsub = 3, 5, 9, 1, 0.0125, 20
    S, goals, P, safety, obs, rb = _synthetic(5, W, rows, True, G, type_, False, None, reach=False)
    n = rows - 1
    goals[:, :, 0, 0] = -7.0; goals[:, :, 0, 1] = S[:, :n, 1]
    goals[:, ::3, 0, 0] = S[:, :n:3, 0] - 2.5          # every third human within 3 m of its goal: respawns
    S[:, :n, 10:12] = goals[:, :, 0]
    bounds = (7.0, 1.5)
    on = np.array([1, 0, 1, 1, 0])
    action = np.tile([0.1, 0.0], (W, 1))
    cw = _worlds(S, goals, P, safety, obs, type_, True, robot_row=True, robot=rb, respawn_bounds=bounds, respawn_worlds=on)
    cw.step(dt, nsub, action)
    got, gg = cw.get_states(), cw.get_goals()
    stats = _stats()
    for w in range(W):
        sel = slice(w, w + 1)
        kw = dict(respawn=bool(on[w]), rp=(bounds[0], bounds[1], float(safety[w, -1])))
        # (the oracle adds respawn_par[2] to the robot's radius: the margin the device reads from the safety array)
        r0, g0, _ = _oracle_block(type_, S[sel], goals[sel], P[sel], safety[sel], obs, True, dt, nsub, rb[sel], action[sel], **kw)
        r1, g1, _ = _oracle_block(type_, _nudge(S[sel]), goals[sel], P[sel], safety[sel], obs, True, dt, nsub, _nudge(rb[sel]), action[sel], **kw)
        s = max(_err(r1, r0, True), _err(g1, g0, True))
        err = max(_err(got[w], r0[0], True), _err(gg[w], g0[0], True))
        _check("f64_respawn", f"world {w} respawn {on[w]}", err, s, 1e-10, stats)
        assert bool(np.any(got[w, :n, 0] > 6.9)) == bool(on[w])
    _finish("f64_respawn", stats)


# ------------------------------------------------------------------------------------------------------------------ (d) the point of it
_EPISODE_WORLDS = {}


def _crossing_worlds(model):
    """8 circular-crossing worlds x 25 humans from the host generators (float64)."""
    if model not in _EPISODE_WORLDS:
        from test_facade_cpu import make_env

        rows = []
        for case in range(8):
            env = make_env(model, "circle_crossing", 25, False)
            env.reset(phase="test", test_case=case)
            mm = env.motion_model_manager
            rows.append((np.array(mm.states), np.array(mm.goals), np.array(mm.params), np.array(mm.safety_space), int(mm.sfm_type),
                         bool(mm.all_equal_humans)))
        S, G, P, saf = (np.stack([r[i] for r in rows]) for i in range(4))
        _EPISODE_WORLDS[model] = (S, G, P, saf, rows[0][4], rows[0][5])
    return _EPISODE_WORLDS[model]


@pytest.mark.parametrize("model", ["hsfm_farina", "sfm_helbing"])
def test_an_episode_stays_on_the_float64_trajectory(model):
    """2000 substeps (a 25 s episode) in blocks of 20.  The device's float64 positions stay within 1000 x the oracle's own divergence
    from a start one ulp off at the same substep count (its running maximum: the device injects a rounding difference at every substep,
    the nudged oracle once), and that bound ends below 1e-3 x what the float32 oracle has drifted from the float64 one."""
    from oracle import crowd_oracle as orc

    S, G, P, saf, type_, peq = _crossing_worlds(model)
    dt, nsub, blocks = 0.0125, 20, 100
    run = lambda S0, dtype: orc.StepBlockRunner(type_, S0, G, None, P, saf, peq, dtype=dtype)
    ref, ulp = run(S, np.float64), run(_nudge(S), np.float64)
    with np.errstate(all="ignore"):
        f32 = run(S.astype(np.float32), np.float32)
    cw = _worlds(S, G, P, saf, None, type_, peq)
    envelope = worst_ratio = d32 = 0.0
    for b in range(blocks):
        ref.run(dt, nsub); ulp.run(dt, nsub)
        with np.errstate(all="ignore"):
            f32.run(dt, nsub)
        cw.step(dt, nsub)
        envelope = max(envelope, float(np.max(np.abs(ulp.S[..., 0:2] - ref.S[..., 0:2]))))
        dev = float(np.max(np.abs(cw.get_states()[..., 0:2] - ref.S[..., 0:2])))
        d32 = float(np.max(np.abs(f32.S[..., 0:2].astype(np.float64) - ref.S[..., 0:2])))
        bound = 1000.0 * envelope
        worst_ratio = max(worst_ratio, dev / bound)
        if (b + 1) % 20 == 0:
            print(f"{model} substep {(b + 1) * nsub}: device {dev:.3e}  one-ulp oracle {envelope:.3e}  float32 oracle {d32:.3e}")
        assert dev <= bound, f"{model}: substep {(b + 1) * nsub}: device {dev:.3e} m off the oracle, bound {bound:.3e}"
    _record("f64_episode_" + model, dev, bound)
    assert bound < 1e-3 * d32, f"{model}: 1000 x one-ulp divergence {bound:.3e} is not below 1e-3 x the float32 drift {d32:.3e}"


# ------------------------------------------------------------------------------------------------------------------ (e) facade
def test_array_seam_f64_g1():
    """update_humans_parallel(..., precision="f64"): the reference signature, numpy float64 in / out, in-place side effects, at the bars of (a)."""
    from oracle import crowd_oracle as orc
    from social_navigation_pyenvs_amd.social_gym.src.forces_parallel import update_humans_parallel

    stats = _stats()
    for k, c in list(enumerate(load_cases("g1_episode")))[::6]:
        S, G = c["state_in"].copy(), c["goals_in"].copy()
        out = update_humans_parallel(c["type"], S, G, c.get("obstacles"), c["params"], c["dt"], c["safety"], c["all_params_equal"],
                                     c["last_is_robot"], precision="f64")
        assert out.dtype == np.float64 and out.shape == c["state_out"].shape
        args = (c["goals_in"], c.get("obstacles"), c["params"], c["dt"], c["safety"], c["all_params_equal"], c["last_is_robot"])
        with np.errstate(all="ignore"):
            r0, a0, _ = orc.update_humans(c["type"], c["state_in"], *args)
            r1, a1, _ = orc.update_humans(c["type"], _nudge(c["state_in"]), *args)
        s = max(_err(r1, r0, True), _err(a1, a0, True))
        err = max(_err(out, c["state_out"], True), _err(S, c["state_in_after"], True))
        if _check("f64_seam_g1", f"case {k}", err, s, 1e-12, stats):
            np.testing.assert_array_equal(G, c["goals_out"])
    _finish("f64_seam_g1", stats)
    with pytest.raises(ValueError):
        update_humans_parallel(9, S, G, None, c["params"], 0.0125, c["safety"], precision="f64")


def test_manager_update_and_peek_f64_g4():
    """MotionModelManager with precision "f64": get_next_human_observable_states on G4 at the one-substep bar, nothing committed;
    update_humans equals the block of one substep."""
    from oracle import crowd_oracle as orc
    from test_facade_cpu import make_env

    stats = _stats()
    for k, c in enumerate(load_cases("g4_peek")):
        env = make_env(c["model"], c["scenario"], 6, c["robot_visible"])
        env.set_world_precision("f64")
        env.reset(phase="test", test_case=c["test_case"])
        mm = env.motion_model_manager
        assert mm.precision == "f64"
        mm.states[...] = c["states_before"]
        mm.goals[...] = c["goals_before"]
        mm._sync_goal_lists_from_array()
        if c["robot_visible"]:
            rb = c["states_before"][-1]
            env.robot.position, env.robot.linear_velocity = rb[0:2].copy(), rb[3:5].copy()
        nxt4 = mm.get_next_human_observable_states(0.25)
        nxt8 = mm.get_next_human_observable_states(0.25, theta_and_omega_visible=True)
        n = nxt4.shape[0]
        for key, got, want, cols in (("states_before", nxt4, c["next4"], [0, 1, 2, 3]), ("states_mid", nxt8, c["next8"], [0, 1, 3, 4, 6, 7])):
            args = (c["goals_before"], None, c["params"], c["dt"], c["safety"], c["all_params_equal"], c["robot_visible"])
            with np.errstate(all="ignore"):
                r0 = orc.update_humans(c["type"], c[key], *args)[0]
                r1 = orc.update_humans(c["type"], _nudge(c[key]), *args)[0]
            s = _err(r1[:n], r0[:n], True)
            _check("f64_facade_g4", f"case {k} {c['model']} {key}", _err(got[:, cols], want[:, cols], True), s, 1e-12, stats)
        np.testing.assert_allclose(mm.states[:, [0, 1, 2, 5, 6, 7]], c["states_after"][:, [0, 1, 2, 5, 6, 7]], atol=1e-12)  # restored
        np.testing.assert_allclose(mm.goals, c["goals_after"], atol=0, equal_nan=True)
        # update_humans (one substep through the manager) == update_humans_block of one substep, bit for bit
        before, gbefore = mm.states.copy(), mm.goals.copy()
        mm.update_humans(0.0, 0.0125, post_update=False)
        one = mm.states.copy()
        mm.states[...] = before; mm.goals[...] = gbefore; mm._sync_goal_lists_from_array()
        respawn = mm.parallel_traffic_humans_respawn
        mm.parallel_traffic_humans_respawn = False
        mm.update_humans_block(0.0125, 1, None)
        mm.parallel_traffic_humans_respawn = respawn
        np.testing.assert_array_equal(one[:n].view(np.uint64), mm.states[:n].view(np.uint64))
    _finish("f64_facade_g4", stats)


def _obs_array(ob, headed):
    return np.array([[o.px, o.py, o.vx, o.vy, o.radius] + ([o.theta, o.omega] if headed else []) for o in ob])


def test_gym_loop_f64_g3():
    """SocialNavGym.step with set_world_precision("f64"), FREE RUNNING over the 10 recorded Gym steps (200 substeps, no
    re-synchronisation): rewards and flags match the record, the observations stay within 1e-10 + 16 s of it, s = the oracle's own
    one-ulp divergence over the same steps.  280 steps compared, worst error / bar 1.3e-5; cases 28 and 30
    (Moussaid at rest: the oracle's own free run leaves the record at step 0) are skipped by name.

    Moussaid's law multiplies a lateral term by sign(theta_ij), and with everybody at rest theta_ij = wrap(atan2(n) - atan2(i) + pi) is the
    rounding of the two atan2 values (+-1e-16).  The kernel takes them correctly rounded (csrc/atan2_cr.h), as the
    reference's C library does, and lands on the reference's side: case 29 (sfm_moussaid at rest) follows the record through all ten steps."""
    from oracle import crowd_oracle as orc
    from social_navigation_pyenvs_amd.crowd_nav.utils.action import ActionXY

    stats, skipped = _stats(), []
    for ci, c in enumerate(load_cases("g3_gym")):
        env = _gym_env(c)
        env.set_world_precision("f64")
        mm = env.motion_model_manager
        n, rv = len(mm.humans), bool(c["robot_visible"])
        respawn = bool(mm.parallel_traffic_humans_respawn)
        rp = (float(mm.respawn_bounds[0]), float(mm.respawn_bounds[1]), 0.0) if respawn else (0.0, 0.0, 0.0)
        rb = np.asarray(env.robot.get_safe_state(), dtype=np.float64)
        S0 = np.array(mm.states)
        if rv:
            S0[-1] = rb
        o = [[S0, np.array(mm.goals), rb.copy()], [_nudge(S0), np.array(mm.goals), _nudge(rb)]]
        determined, prev_bar = True, 0.0
        for k in range(len(c["actions"])):
            a = c["actions"][k]
            for side in o:
                with np.errstate(all="ignore"):
                    side[0], side[1], side[2] = orc.step_block(int(mm.sfm_type), side[0], side[1], mm.obstacles, mm.params, env.time_step,
                                                               env.time_step_factor, mm.safety_space, bool(mm.all_equal_humans), robot_visible=rv,
                                                               robot=side[2], action=np.asarray(a, dtype=np.float64), respawn=respawn, respawn_par=rp)
            s = _err(o[1][0][:n, [0, 1, 3, 4]], o[0][0][:n, [0, 1, 3, 4]], False)
            if determined and _err(o[0][0][:n, [0, 1, 3, 4]], c["mm_states"][k + 1][:n, [0, 1, 3, 4]], False) > 1e-10 + MARGIN * s:
                # the oracle's own free run leaves the record: Moussaid's sign(theta_ij ~ 0) with everybody at rest at step 0 picks a side
                # at random in the reference -- the rest of such an episode is skipped by name
                assert c["model"].endswith("moussaid"), (ci, c["model"], k)
                skipped.append((ci, c["model"], c["scenario"], k))
                determined = False
            ob, reward, term, trunc, info = env.step(ActionXY(float(a[0]), float(a[1])))
            if not determined:
                continue
            got = _obs_array(ob, c["headed_obs"])
            err = _err(got[:, :4], c["obs"][k + 1][:, :4], False)
            determined = _check("f64_gym_g3", f"case {ci} {c['model']} {c['scenario']} step {k}", err, s, 1e-10, stats)
            if determined:
                # the reward is a function of the state BEFORE the substeps with slope < 1 in the positions: within that state's bar
                assert abs(reward - c["rewards"][k]) <= 1e-12 + prev_bar and (term, trunc) == (bool(c["terminated"][k]), bool(c["truncated"][k]))
                prev_bar = 1e-10 + MARGIN * s
                assert type(info[0]).__name__ == c["infos"][k]
                np.testing.assert_allclose([*env.robot.position, *env.robot.linear_velocity], c["robot_states"][k + 1][[0, 1, 3, 4]], atol=1e-12)
        assert mm.precision == "f64" and env.motion_model_manager is mm
    print("f64_gym_g3 skipped from (case, model, scenario, step) on:", skipped)
    assert stats["cases"] >= 200 and len(skipped) <= 8
    _finish("f64_gym_g3", stats)


def test_default_precision_is_bitwise_the_float32_worlds(monkeypatch):
    """With the default precision the manager's results are, bit for bit, those of CrowdWorlds driven directly (what the parent commit ran)."""
    from social_navigation_pyenvs_amd.batched import CrowdWorlds
    from test_facade_cpu import make_env

    monkeypatch.delenv("CROWDSTEP_PRECISION", raising=False)
    for model, scenario, rv in (("hsfm_farina", "circle_crossing", True), ("sfm_guo", "parallel_traffic", False)):
        env = make_env(model, scenario, 7, rv)
        env.reset(phase="test", test_case=11)
        mm = env.motion_model_manager
        assert mm.precision == "f32"
        S = mm.states.copy()
        rb = np.asarray(env.robot.get_safe_state())
        if rv:
            S[-1] = rb
        bounds = mm.respawn_bounds if mm.parallel_traffic_humans_respawn else None
        cw = CrowdWorlds(S, mm.goals, mm.params, mm.safety_space, mm.obstacles, type=mm.sfm_type, all_params_equal=mm.all_equal_humans,
                         robot_row=rv, robot=rb, respawn_bounds=bounds)
        cw.step(0.0125, 20, np.array([[0.3, -0.1]], np.float32))
        direct = cw.get_states()[0]
        peek_direct = cw.peek(0.25)[0]
        mm.update_humans_block(0.0125, 20, (0.3, -0.1))
        n = len(mm.humans)
        np.testing.assert_array_equal(mm.states[:n, 0:8].astype(np.float32).view(np.uint32), direct[:n, 0:8].view(np.uint32))
        peek = mm.get_next_human_observable_states(0.25, theta_and_omega_visible=True)
        np.testing.assert_array_equal(peek.astype(np.float32).view(np.uint32), peek_direct.view(np.uint32))
