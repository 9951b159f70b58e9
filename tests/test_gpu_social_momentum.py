"""k_sm_step (csrc/social_momentum.hip) against the float64 block oracle on every world, substep and respawn: the shapes, the rule and the
bars are those of tests/social_momentum_cases.py, whose conditions tests/test_social_momentum_cases_cpu.py proves without a device.
Every batch is a few hundred lanes and a handful of launches."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import parity_util  # noqa: E402
import social_momentum_cases as smc  # noqa: E402

pytestmark = pytest.mark.gpu
K_A = 4
UNTOUCHED = [2, 5, 6, 7, 8, 9, 12]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _snapshot(cw, case):
    return cw.get_states(), cw.get_goals(), (cw.get_robot() if case["robot"] is not None else None)


def _same_bits(a, b, what):
    for x, y, name in zip(a, b, ("states", "goals", "robot")):
        if x is not None:
            assert np.array_equal(_bits(x), _bits(y)), f"{what}: {name} differ in {int(np.sum(_bits(x) != _bits(y)))} words"


def _singles(case, K, layout="aos", check=True, group=None):
    """K launches of one substep; each record against ONE oracle substep restarted from the GPU's previous record.  Returns the last snapshot
    and the figures."""
    cw = smc.make_worlds(case, layout=layout)
    n = case["n"]
    prev = (case["S"], case["goals"], case["robot"])
    fig = dict(decided=0, undecided=0, worst_pos=0.0, worst_robot=0.0)
    for k in range(K):
        cw.step(case["dt"], 1, case["action"])
        S, g, R = _snapshot(cw, case)
        if check:
            ref = smc.oracle_block(case, 1, S=prev[0], goals=prev[1], robot=prev[2])
            r = smc.check_record(case, ref, 0, S, g)
            assert not r["violations"], f"substep {k + 1}: {len(r['violations'])} violations, first {r['violations'][:3]}"
            assert np.array_equal(_bits(S[:, :, UNTOUCHED]), _bits(case["S"][:, :, UNTOUCHED])), f"substep {k + 1}: a constant column changed"
            for name in ("decided", "undecided"):
                fig[name] += r[name]
            fig["worst_pos"] = max(fig["worst_pos"], r["worst_pos"])
            if R is not None:
                # the true robot's record against the float64 formula (fused_substeps_vs_oracle's robot bars: 2e-6, the yaw 1e-6)
                want = ref["robot"][0]
                e = float(np.abs(R[:, [0, 1, 3, 4]] - want[:, [0, 1, 3, 4]]).max())
                dyaw = np.abs(R[:, 2] - want[:, 2]); dyaw = np.minimum(dyaw, np.abs(2 * np.pi - dyaw))
                assert e < 2e-6 and dyaw.max() < 1e-6, f"substep {k + 1}: the robot's record, {e:.2e} / yaw {dyaw.max():.2e}"
                assert np.array_equal(_bits(R[:, 5:]), _bits(case["robot"][:, 5:]))
                if case["visible"]:
                    assert np.array_equal(_bits(S[:, n, [0, 1, 3, 4]]), _bits(R[:, [0, 1, 3, 4]])), "the robot's row is not the robot"
                if case["action"] is None:
                    assert np.array_equal(_bits(R), _bits(case["robot"])), "a robot without an action moved"
                fig["worst_robot"] = max(fig["worst_robot"], e)
        prev = (S, g, R)
    if check:
        total = fig["decided"] + fig["undecided"]
        print(f"{group or 'social momentum'}: {fig['decided']} decided humans compared, {fig['undecided']} of {total} undecided "
              f"({100.0 * fig['undecided'] / max(total, 1):.2f} %), worst position error {fig['worst_pos']:.2e}, robot {fig['worst_robot']:.2e}")
        assert fig["undecided"] <= smc.CAP * total, (fig, "the cap is a condition on the inputs: change them, not the cap")
        if group:
            parity_util.record(group, fig["worst_pos"], smc.POS_BAR)
            parity_util.REPORT[group].update(decided=fig["decided"], undecided=fig["undecided"])
    return prev, fig


def _fused(case, K, layout="aos"):
    cw = smc.make_worlds(case, layout=layout)
    cw.step(case["dt"], K, case["action"])
    return _snapshot(cw, case)


# ---------------------------------------------------------------------------------------------------- a. per substep against the oracle
SHAPES = [(rows, robot) for rows in smc.ROWS for robot in smc.ROBOTS if not (rows == 1 and robot != "none")]


@pytest.mark.parametrize("rows,robot", SHAPES)
def test_every_world_and_substep_against_the_oracle(rows, robot):
    """W = 2 * (64 // rows) + 1 worlds: a full block, a second block and a partly filled last one; rows 7 / 21 leave one lane of the wavefront
    idle, 22 twenty, 32 none, 33 and up hold one world per block.  (One row that is a visible robot is a world without humans: not a case.)"""
    _singles(smc.random_case(rows, robot), K_A, group=f"social momentum vs f64 oracle: {rows} rows, robot {robot}")


# ---------------------------------------------------------------------------------------------------- b. fused = single, bit for bit
FUSED = {
    "visible-moving-7": lambda: smc.random_case(7, "moving"),
    "visible-unicycle-13": lambda: smc.random_case(13, "moving", kinematics=1),
    "invisible-33": lambda: smc.random_case(33, "invisible"),
    "invisible-unicycle-13": lambda: smc.random_case(13, "invisible", kinematics=1),
    "respawn-mixed-flags-7": lambda: smc.traffic_case(7),
    "respawn-mixed-flags-13": lambda: smc.traffic_case(13),
    "respawn-mixed-flags-33": lambda: smc.traffic_case(33),
    "respawn-no-robot-7": lambda: smc.traffic_case(7, robot=False),
    "goal-rotations": smc.goal_edge_case,
}


@pytest.mark.parametrize("name", list(FUSED))
def test_fused_launch_equals_single_launches(name):
    """One launch of nsub = K gives the states, goal lists and robot rows of K launches of nsub = 1 (which test a pins on the oracle)."""
    case = FUSED[name]()
    K = 3 if case["respawn"] is not None else K_A      # (the traffic worlds: the substeps the CPU file proves the cap for)
    # (the per-substep check rides along wherever the CPU file proves the cap for the inputs: everything but the wide traffic worlds)
    single, _ = _singles(case, K, check=name not in ("respawn-mixed-flags-13", "respawn-mixed-flags-33"), group=f"social momentum vs f64 oracle: {name}")
    _same_bits(_fused(case, K), single, name)
    if case["respawn"] is not None:
        x, x0 = single[0][:, :, 0], case["S"][:, :, 0]
        assert np.all(x[[0, 1, 3]][:, [1, 4]] > x0[[0, 1, 3]][:, [1, 4]] + 10.0), "the flagged worlds' humans 1 and 4 respawn"
        assert np.all(x[2, [1, 4]] < -4.0), "a world with its flag off respawned somebody"


# ---------------------------------------------------------------------------------------------------- c. respawn against the oracle
@pytest.mark.parametrize("robot", [True, False])
def test_respawn_against_the_oracle(robot):
    """traffic_case: two and three humans of a world respawn in one substep at lw = 0 and lw > 0, beside a world whose flag is off; the robot is
    the maximum x of one world and the maximum radius + safety space of another; y beyond both bounds.  The step after is compared too."""
    case = smc.traffic_case(7, robot=robot)
    cw = smc.make_worlds(case)
    cw.step(case["dt"], 1, case["action"])
    S = cw.get_states()
    n = case["n"]
    landed = S[:, :n, 0] > 6.9
    assert [np.flatnonzero(landed[w]).tolist() for w in range(5)] == [[1, 4], [1, 4], [], [1, 4, 5], []]
    assert np.array_equal(np.abs(S[[0, 0, 3, 3], [1, 4, 1, 4], 1]), np.full(4, 1.5, np.float32))
    _singles(case, 3, group=f"social momentum respawn vs f64 oracle (robot {robot})")


# ---------------------------------------------------------------------------------------------------- d. layout
@pytest.mark.parametrize("rows", [13, 33])
def test_soa_layout_gives_the_bits_of_aos(rows):
    case = smc.random_case(rows, "moving")
    aos, _ = _singles(case, K_A, check=False)
    soa, _ = _singles(case, K_A, layout="soa", check=False)
    _same_bits(soa, aos, f"soa vs aos, {rows} rows")
    _same_bits(_fused(case, K_A, layout="soa"), aos, f"fused soa vs aos, {rows} rows")


# ---------------------------------------------------------------------------------------------------- e. action count
@pytest.mark.parametrize("A", [1, 7, 20, 64])
def test_action_count_against_the_oracle(A):
    case = dict(smc.random_case(13, "moving", seed=A), n_actions=A)
    last, fig = _singles(case, 2, group=f"social momentum vs f64 oracle: {A} actions")
    sp = np.linalg.norm(last[0][:, :case["n"], 3:5].astype(np.float64), axis=-1)
    assert np.all((np.abs(sp - case["S"][:, :case["n"], 12]) < 2e-6) | (sp == 0))


def test_too_many_actions_are_refused_and_nothing_moves():
    case = smc.random_case(13, "moving")
    cw = smc.make_worlds(case, n_actions=65)
    before = _snapshot(cw, case)
    with pytest.raises(ValueError, match="sm_n_actions must be <= 64"):
        cw.step(case["dt"], 1, case["action"])
    with pytest.raises(ValueError, match="sm_n_actions must be <= 64"):
        cw.peek(case["dt"])
    _same_bits(_snapshot(cw, case), before, "after the refused launches")
    _same_bits(before, (case["S"], case["goals"], case["robot"]), "what was uploaded")


# ---------------------------------------------------------------------------------------------------- f. goals and the empty action set
def test_goal_edges_rotate_on_consecutive_substeps_of_a_fused_launch():
    """At a distance equal to the radius in float32 the list stays, one float32 inside it rotates; three-goal lists rotate twice in two
    substeps of ONE launch; every single substep follows the oracle."""
    case = smc.goal_edge_case()
    ref = smc.oracle_block(case, 2)
    S, g, _ = _fused(case, 2)
    want = ref["goals"][1].astype(np.float32)
    assert np.array_equal(_bits(g), _bits(want)) and np.array_equal(_bits(S[:, :, 10:12]), _bits(want[:, :, 0]))
    g0 = case["goals"]
    assert np.array_equal(_bits(g[:, 4]), _bits(g0[:, 4][:, [2, 0, 1]])) and np.array_equal(_bits(g[:, 5]), _bits(g0[:, 5]))   # twice / not at all
    assert np.array_equal(_bits(g[:, 2]), _bits(g0[:, 2][:, [1, 0, 2]])) and np.array_equal(_bits(g[:, 3]), _bits(g0[:, 3]))   # once / not at all
    _singles(case, 3, group="social momentum goal edges vs f64 oracle")


def test_boxed_in_human_stops_with_a_positive_zero_and_chooses_again():
    case = smc.boxed_case()
    cw = smc.make_worlds(case)
    cw.step(case["dt"], 1)
    S = cw.get_states()
    assert np.array_equal(_bits(S[0, 0, 3:5]), np.zeros(2, np.uint32)), S[0, 0, 3:5]          # exactly (+0, +0)
    assert np.linalg.norm(S[1, 0, 3:5]) > 0.49 and np.all(np.linalg.norm(S[:, 1:, 3:5], axis=-1) > 1.0)
    last, fig = _singles(case, 3, group="social momentum boxed-in human vs f64 oracle")
    assert np.linalg.norm(last[0][0, 0, 3:5]) > 0.49 and fig["undecided"] == 0                # everybody reactive, a choice by the rule again


def test_exact_threshold_and_exact_tie():
    """exact_case: a distance that EQUALS the threshold leaves the action free (strict <), and of two rewards equal bit for bit the first wins."""
    case = smc.exact_case()
    last, fig = _singles(case, 1, group="social momentum exact edges vs f64 oracle")
    assert fig["undecided"] == 0
    assert np.array_equal(_bits(last[0][:, 0, 3:5]), _bits(np.array([[1.0, 0.0], [1.0, 0.0]], np.float32)))


# ---------------------------------------------------------------------------------------------------- g. peek
@pytest.mark.parametrize("rows", [7, 33])
def test_peek_is_the_next_state_and_commits_nothing(rows):
    """cs_peek on W worlds with a pending goal rotation, respawn bounds set and humans inside the 3 m zone: the step's next state (of a step
    without the respawn rule: post_update=False), nothing written, nobody respawned."""
    case = smc.random_case(rows, "rest")
    n = case["n"]
    S, goals = case["S"].copy(), case["goals"].copy()
    goals[:, 0, 1] = S[:, 0, 0:2] + np.float32(1.0)
    goals[:, 0, 0] = S[:, 0, 0:2] + np.float32(0.1)                     # human 0: within its radius of the head, the second goal 1.4 m away
    if n > 1:
        goals[:, 1, 0] = S[:, 1, 0:2] + np.float32(1.5)                 # human 1: inside the 3 m zone
    S[:, :n, 10:12] = goals[:, :, 0]
    case = dict(case, S=S, goals=goals)
    armed = dict(case, respawn=np.ones(case["W"], np.int32), bounds=(7.0, 1.5))
    cw = smc.make_worlds(armed)
    before = _snapshot(cw, armed)
    nxt = cw.peek(case["dt"])
    _same_bits(_snapshot(cw, armed), before, "after the peek")
    plain = smc.make_worlds(case)
    plain.step(case["dt"], 1)
    P = plain.get_states()
    assert np.array_equal(_bits(nxt), _bits(P[:, :n][:, :, [0, 1, 2, 3, 4, 7, 10, 11]]))
    assert not np.array_equal(_bits(P[:, 0, 10:12]), _bits(S[:, 0, 10:12]))                 # the rotation was pending and the peek shows it
    ref = smc.oracle_block(case, 1)
    r = smc.check_record(case, ref, 0, P, plain.get_goals())
    assert not r["violations"], r["violations"][:3]
    cw.step(case["dt"], 1)                                             # the same worlds DO respawn when they step
    assert np.all(cw.get_states()[:, 0, 0] > nxt[:, :, 0].max(axis=1) + 0.4)
