"""The social-momentum block oracle on the reference's recorded calls (golden G27), and the conditions of tests/social_momentum_cases.py
proved without a device: the oracle alone leaves at most half the cap undecided on every shape the GPU suite runs, and the decision rule
catches every mutated restatement on those very inputs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
sys.path.insert(0, os.path.dirname(__file__))
from golden_io import load_cases  # noqa: E402

import social_momentum_cases as smc  # noqa: E402
from oracle import crowd_oracle as orc  # noqa: E402

K_A = 4


def test_block_oracle_matches_golden_g27():
    """Every recorded update_humans call of the reference (respawn rule on, robot moved by hand between the calls) from ONE block of the oracle."""
    doubles = singles = rotations = 0
    for ci, c in enumerate(load_cases("g27_social_momentum_blocks")):
        K, n, rv = c["calls"], c["n"], c["robot_visible"]
        rb = None
        if rv:
            rb = np.zeros((1, 13)); rb[0, 0:2] = c["robot0"][0:2]; rb[0, 3:5] = c["robot0"][2:4]; rb[0, 8] = c["robot0"][4]
        out = orc.social_momentum_block(c["in_pos"][None], c["in_vel"][None], c["radius"][None], c["safety"][None], c["vd"][None],
                                        c["in_goals"][None], c["dt"], K, robot=rb, robot_visible=rv, robot_safety=c["robot0"][5],
                                        action=c["action"][None] if rv else None, respawn=[True], respawn_bounds=c["respawn_bounds"])
        for k in range(K):
            np.testing.assert_allclose(out["pos"][k, 0], c["out_pos"][k], rtol=0, atol=1e-13, err_msg=f"case {ci} call {k}")
            np.testing.assert_allclose(out["vel"][k, 0], c["out_vel"][k], rtol=0, atol=1e-13, err_msg=f"case {ci} call {k}")
            if rv:
                np.testing.assert_allclose(out["robot"][k, 0][[0, 1, 3, 4]], c["out_robot"][k][0:4], rtol=0, atol=1e-13)
            np.testing.assert_array_equal(out["respawned"][k, 0], c["respawned"][k])
            for i in range(n):
                want = c["out_goals"][k, i]
                L = int(np.sum(~np.isnan(want[:, 0])))
                got = out["goals"][k, 0, i]
                np.testing.assert_array_equal(got[:L], want[:L])
                # the reference's list after a respawn holds ONE goal (:418); the oracle, like the parallel arrays of :422 that golden G7 pins,
                # holds that goal in every slot: the same list under rotation
                rest = got[L:]
                assert np.all(np.isnan(rest)) or (L == 1 and np.all(rest == got[0])), (ci, k, i, got, want)
        per_call = c["respawned"].sum(axis=1)
        doubles += int(np.sum(per_call >= 2)); singles += int(np.sum(per_call == 1))
        rotations += int(np.array_equal(c["out_goals"][0, 1, 0], c["in_goals"][1, 1]))      # human 1's list rotated in the first call
    assert doubles == 5 and singles >= 3 and rotations == 5, (doubles, singles, rotations)


def _cases():
    out = [(f"rows{rows}-{robot}", (lambda rows=rows, robot=robot: smc.random_case(rows, robot)), K_A)
           for rows in smc.ROWS for robot in smc.ROBOTS if not (rows == 1 and robot != "none")]
    out += [("traffic", smc.traffic_case, 3), ("traffic-no-robot", lambda: smc.traffic_case(robot=False), 3),
            ("goal-edge", smc.goal_edge_case, 3), ("boxed", smc.boxed_case, 3), ("exact", smc.exact_case, 1),
            ("rows13-unicycle", lambda: smc.random_case(13, "moving", kinematics=1), K_A),
            ("rows13-invisible", lambda: smc.random_case(13, "invisible"), K_A),
            ("rows13-invisible-unicycle", lambda: smc.random_case(13, "invisible", kinematics=1), K_A),
            ("rows33-invisible", lambda: smc.random_case(33, "invisible"), K_A)]
    out += [(f"rows13-A{A}", (lambda A=A: dict(smc.random_case(13, "moving", seed=A), n_actions=A)), 2) for A in (1, 7, 20, 64)]
    return out


CASES = _cases()


@pytest.mark.parametrize("name,build,K", CASES, ids=[c[0] for c in CASES])
def test_oracle_alone_leaves_at_most_half_the_cap_undecided(name, build, K):
    und, total = smc.undecided_share(build(), K)
    print(f"{name}: {und} of {total} undecided on the oracle's own trajectory ({100.0 * und / max(total, 1):.2f} %)")
    assert und <= 0.5 * smc.CAP * total, (name, und, total)


def test_built_cases_hold_their_conditions():
    """What the docstrings of traffic_case, goal_edge_case, boxed_case and exact_case promise, on the oracle."""
    c = smc.traffic_case()
    n = c["n"]
    ref = smc.oracle_block(c, 2)
    want = {0: [1, 4], 1: [1, 4], 2: [], 3: [1, 4, 5], 4: []}
    for w, who in want.items():
        assert np.flatnonzero(ref["respawned"][0, w]).tolist() == who, (w, ref["respawned"][0, w])
    in_zone = np.linalg.norm(ref["pos"][0, 2] - ref["goals"][0, 2, :, 0], axis=-1) < 3
    assert in_zone[[1, 4]].all()                                           # flag off: in the zone and left alone
    assert ref["robot"][0, 0, 0] > ref["pos"][0, 0, [0, 2, 3, 5], 0].max() and ref["robot"][0, 0, 0] > 7.0   # the robot is the maximum x
    rs = c["S"][1, :, 8].astype(np.float64) + c["safety"][1].astype(np.float64)
    assert rs[n] > rs[:n].max()
    step = 2 * float(rs[n])
    assert abs(ref["pos"][0, 1, 4, 0] - ref["pos"][0, 1, 1, 0] - step) < 1e-12   # the second lands one step behind the first
    assert abs(ref["pos"][0, 0, 1, 0] - (float(F32_(9.5)) - 0.4 * 0.25 + 2 * float((c["S"][0, :, 8].astype(np.float64) + c["safety"][0]).max()))) < 1e-6
    assert c["S"][0, 1, 1] > 1.5 and c["S"][0, 4, 1] < -1.5 and ref["pos"][0, 0, 1, 1] == 1.5 and ref["pos"][0, 0, 4, 1] == -1.5
    assert abs(c["S"][1, 1, 1]) < 1.5 and abs(ref["pos"][0, 1, 1, 1]) < 1.5
    assert not ref["respawned"][1].any()

    c = smc.goal_edge_case()
    ref = smc.oracle_block(c, 2)
    g0 = c["goals"].astype(np.float64)
    for i in range(c["n"]):
        L = 1 + i // 2
        rot1 = i % 2 == 0 and L > 1
        assert np.array_equal(ref["goals"][0, :, i, 0], g0[:, i, 1] if rot1 else g0[:, i, 0]), i
        if L == 3 and i % 2 == 0:                                         # rotates again on the next substep
            assert np.array_equal(ref["goals"][1, :, i, 0], g0[:, i, 2]) and np.array_equal(ref["goals"][1, :, i, 2], g0[:, i, 1]), i
        else:
            assert np.array_equal(ref["goals"][1, :, i], ref["goals"][0, :, i], equal_nan=True), i

    c = smc.boxed_case()
    ref = smc.oracle_block(c, 3)
    assert ref["chosen"][0, 0, 0] == -1 and np.all(ref["vel"][0, 0, 0] == 0) and ref["margin"][0, 0, 0] >= smc.MARGIN
    assert ref["chosen"][0, 1, 0] >= 0 and np.all(ref["chosen"][0, :, 1:] >= 0)
    assert ref["chosen"][2, 0, 0] >= 0                                    # the neighbours have walked away: it chooses again

    c = smc.exact_case()
    ref = smc.oracle_block(c, 1)
    assert np.flatnonzero(ref["gap"][0, 0, 0] >= 0).tolist() == [0, 10] and ref["rewards"][0, 0, 0, 0] == ref["rewards"][0, 0, 0, 10]
    assert ref["gap"][0, 1, 0, 0] == 0.0 and ref["chosen"][0, 1, 0] == 0 and ref["chosen"][0, 0, 0] == 0
    # the same two decisions in float32 arithmetic, operation by operation as the kernel forms them
    f = np.float32
    u = smc.unit_actions(20).astype(f)
    r0, r10 = [f(1) / np.sqrt((f(0) - (f(0) + u[k, 0] * f(1) * f(0.25))) ** 2 + (f(5) - (f(0) + u[k, 1] * f(1) * f(0.25))) ** 2) for k in (0, 10)]
    assert r0 == r10
    ex, ey = (f(1.25) + f(0) * f(0.25)) - (f(0) + u[0, 0] * f(1) * f(0.25)), f(0) - (f(0) + u[0, 1] * f(1) * f(0.25))
    assert np.sqrt(ex * ex + ey * ey) == f(0.5) + f(0.5)


F32_ = np.float32


def _mutant_cases():
    return {"random": smc.random_case(7, "moving", W=6), "random13": smc.random_case(13, "rest", W=4), "traffic": smc.traffic_case(),
            "goal-edge": smc.goal_edge_case(), "exact": smc.exact_case()}


def _violations(case, S, g, K):
    """The per-substep check of the GPU suite on a restatement's records: substep k against the oracle restarted from record k - 1."""
    prev_S, prev_g, R = case["S"], case["goals"], case["robot"]
    bad = []
    for k in range(K):
        ref = smc.oracle_block(case, 1, S=prev_S, goals=prev_g, robot=R)
        r = smc.check_record(case, ref, 0, S[k], g[k])
        bad += [(k,) + v for v in r["violations"]]
        prev_S, prev_g = S[k], g[k]
        if R is not None and case["action"] is not None:
            R = R.copy(); R[:, [0, 1, 3, 4]] = S[k][:, case["n"], [0, 1, 3, 4]] if case["visible"] else R[:, [0, 1, 3, 4]]
    return bad


def test_rule_accepts_the_plain_restatement():
    for name, case in _mutant_cases().items():
        S, g = smc.restated_block(case, 3)
        assert _violations(case, S, g, 3) == [], name


@pytest.mark.parametrize("mutant", smc.MUTANTS)
def test_rule_catches_mutant(mutant):
    """Each deliberate mistake breaks the rule on a DECIDED human of at least one case."""
    caught = {}
    for name, case in _mutant_cases().items():
        S, g = smc.restated_block(case, 3, mutant)
        bad = [v for v in _violations(case, S, g, 3) if v[3]]
        if bad:
            caught[name] = bad[0]
    print(mutant, "caught on", caught)
    assert caught, mutant
