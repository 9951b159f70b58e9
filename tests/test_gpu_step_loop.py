"""The substep loop of the plain one-wavefront builds (MAXT = 64, LEAN = 1, compile-time row count: sfmstep_kernel.h ONE_REGION): the loop
runs inside ONE exec region of the valid lanes, and the refreshed linear velocity R(theta) bv is carried from a substep's tail to the next
substep's part A instead of being formed again.  What that can break, at the smallest shapes that can break it:

  * wavefronts that are partly (or almost wholly) outside the region: 25 rows at W = 1, 2, 3 (two worlds per wavefront);
  * the trip structure of the loop: any substep count, a launch of k substeps = k launches of one, a launch split in two;
  * the rare events of a substep -- the respawn rule (which overwrites the body velocity the carried value was formed from) and the
    goal switch -- on consecutive substeps of one wavefront;
  * substep 0 of a launch whose incoming rows hold a stored velocity that is NOT R(theta) bv;
  * the other builds the change reaches (10 / 20 / 30 / 50 rows).

Every parity check is per substep against the f64 oracle from the same f32 inputs at the 1e-5 bar of tests/parity_util.py.
"""
import os

import numpy as np
import pytest

from oracle import crowd_oracle as orc
from parity_util import f32, fused_substeps_vs_oracle

pytestmark = pytest.mark.gpu

DT = 0.0125
N = 25
VARIANT_25 = "MAXT=64,OCC=1,ROWS_CT=25,LEAN=1"


def _hybrid(W, n, model, seed0):
    from social_navigation_pyenvs_amd import scenarios as sc

    S, goals, P, rb = sc.hybrid_worlds(W, n, model, seed0=seed0)
    return f32(S), f32(goals), f32(P), rb, (np.arange(W) % 2 == 1).astype(np.int32)


def _worlds(S, goals, P, rb, rw, model):
    from social_navigation_pyenvs_amd.batched import CrowdWorlds

    return CrowdWorlds(S, goals, P, None, None, type=model, all_params_equal=True, respawn_bounds=rb, respawn_worlds=rw)


def _walking(W, n, model, seed0):
    """Hybrid worlds two Gym steps in (distinct velocities, headings that turn): (states, goals, P, rb, rw) as float32."""
    S, goals, P, rb, rw = _hybrid(W, n, model, seed0)
    cw = _worlds(S, goals, P, rb, rw, model)
    for _ in range(2):
        cw.step(DT, 20)
    return cw.get_states(), cw.get_goals(), P, rb, rw


def _per_substep(S, goals, P, rb, rw, model, nsub, variant, what):
    from social_navigation_pyenvs_amd.batched import SFMS

    cw = _worlds(S, goals, P, rb, rw, model)
    assert variant in cw.step_variant(), cw.step_variant()
    res = fused_substeps_vs_oracle(cw, SFMS.index(model), S, goals, P, None, None, DT, nsub, True, respawn=rw, respawn_bounds=rb,
                                   group="substep loop in one exec region, per substep", what=what)
    assert res["substeps"] == nsub * S.shape[0]
    assert res["within"] >= res["substeps"] - res["ill_conditioned"], (what, res)
    return cw, res


@pytest.mark.parametrize("W", [1, 2, 3])
@pytest.mark.parametrize("model", ["hsfm_farina", "sfm_helbing", "hsfm_guo"])
def test_partly_empty_wavefronts_every_substep(W, model):
    """25 rows, two worlds per wavefront: W = 1 leaves lanes 25-63 outside the region, W = 2 the 14 idle lanes, W = 3 a second wavefront
    with one world.  12 fused substeps, each against the f64 oracle restarted from the GPU's own previous rows."""
    S, goals, P, rb, rw = _walking(W, N, model, seed0=411)
    _per_substep(S, goals, P, rb, rw, model, 12, VARIANT_25, f"25 rows W={W} {model}")


@pytest.mark.parametrize("model", ["hsfm_farina", "sfm_guo"])
def test_trip_structure(model):
    """Substep counts 0, 1, 2, 3, 5.  Record k of step_trace = the state after k + 1 chained launches of one substep, and a launch of five
    substeps = a launch of two followed by a launch of three: BITWISE (a launch boundary writes the row out and reads it back, forms
    sin / cos of the same heading and the refreshed velocity from the same operands; the build before this change satisfies both bit for
    bit on the GPU: checked there before this test was written).  A count of 0 is refused by the entry point and leaves the worlds alone."""
    W = 3
    S, goals, P, rb, rw = _walking(W, N, model, seed0=523)
    cw0 = _worlds(S, goals, P, rb, rw, model)
    assert VARIANT_25 in cw0.step_variant(), cw0.step_variant()
    with pytest.raises(ValueError):
        cw0.step(DT, 0)
    np.testing.assert_array_equal(cw0.get_states(), S)
    np.testing.assert_array_equal(cw0.get_goals(), goals)
    for nsub in (1, 2, 3, 5):
        traced = _worlds(S, goals, P, rb, rw, model)
        trace = traced.step_trace(DT, nsub)                                # [nsub, W, rows, 12]
        chained = _worlds(S, goals, P, rb, rw, model)
        for k in range(nsub):
            chained.step(DT, 1)
            got = chained.get_states()
            np.testing.assert_array_equal(trace[k][..., 0:8], got[..., 0:8], err_msg=f"nsub={nsub}: record {k} vs {k + 1} launches of one")
            np.testing.assert_array_equal(trace[k][..., 8:10], got[..., 10:12], err_msg=f"nsub={nsub}: goal columns of record {k}")
        np.testing.assert_array_equal(traced.get_states(), chained.get_states())
        np.testing.assert_array_equal(traced.get_goals(), chained.get_goals())
    whole, split = _worlds(S, goals, P, rb, rw, model), _worlds(S, goals, P, rb, rw, model)
    whole.step(DT, 5)
    split.step(DT, 2); split.step(DT, 3)
    np.testing.assert_array_equal(whole.get_states(), split.get_states())
    np.testing.assert_array_equal(whole.get_goals(), split.get_goals())


def _lonely(S, goals, w, count, what):
    """`count` humans of world w whose `what` ('goal' / 'self') is farthest from everybody else: events staged on them disturb nobody."""
    n = S.shape[1]
    at = goals[w, :, 0] if what == "goal" else S[w, :, 0:2]
    d = np.linalg.norm(at[:, None] - S[w, None, :, 0:2], axis=-1)
    d[np.arange(n), np.arange(n)] = np.inf
    order = np.argsort(-d.min(axis=1))
    return [int(i) for i in order[:count]], float(d.min(axis=1)[order[count - 1]])


@pytest.mark.parametrize("model", ["hsfm_farina", "sfm_guo"])
def test_respawns_and_goal_switches_on_consecutive_substeps(model):
    """A circle world (two-goal lists) and a traffic world (respawn rule on) in ONE wavefront.  Two humans of the traffic world walk into the
    respawn zone (|p - goal| < 3) in substep 1 and in substep 2 (counted from 0), two of the circle world reach their goal (|goal - p| <= r,
    tested on the incoming position) at the head of substep 1 and of substep 2.  The walking speed is 0.9 m/s = 0.01125 m per substep and
    every threshold is staged >= 5 mm away from a decision, against ~1 mm of drift by the forces over three substeps.  Five fused substeps:
    states and goal columns per substep against the oracle, the events in the substeps they were staged for, and the goal lists the
    epilogue commits against the oracle's: exactly where the list is a rotation of its inputs (the circle world) and for every x; the y
    of a respawned human's goal is its own float32 y (motion_model_manager.py:418) and is held to the 1e-5 bar."""
    from social_navigation_pyenvs_amd.batched import SFMS

    S, goals, P, rb, rw = _hybrid(2, N, model, seed0=637)
    S, goals = S.astype(np.float64), goals.astype(np.float64)
    headed = model.startswith("hsfm")
    step = 0.9 * DT

    def walk(w, i, pos, yaw):
        S[w, i, 0:2] = pos; S[w, i, 2] = yaw
        S[w, i, 3:5] = 0.9 * np.array([np.cos(yaw), np.sin(yaw)])
        S[w, i, 5:8] = (0.9, 0.0, 0.0) if headed else (0.0, 0.0, 0.0)

    # traffic world 1: in the zone after substep 1 (1.5 steps away from it) / after substep 2 (2.5 steps); the two with the most room
    # at the edge of the zone, a metre apart in y
    edge = np.stack([np.full(N, goals[1, 0, 0, 0] + 3.0), S[1, :, 1]], -1)
    room = np.linalg.norm(edge[:, None] - S[1, None, :, 0:2], axis=-1)
    room[np.arange(N), np.arange(N)] = np.inf
    order = np.argsort(-room.min(axis=1))
    ta = int(order[0])
    tb = int(next(i for i in order[1:] if abs(S[1, i, 1] - S[1, ta, 1]) > 1.0))
    assert room[ta].min() > 0.75 and room[tb].min() > 0.75, (room[ta].min(), room[tb].min())
    for i, k in ((ta, 1.5), (tb, 2.5)):
        walk(1, i, (goals[1, i, 0, 0] + 3.0 + k * step, S[1, i, 1]), -np.pi)
    # circle world 0: the goal reached after substep 0 (0.5 steps outside r) / after substep 1 (1.5 steps)
    (ca, cb), gap = _lonely(S, goals, 0, 2, "goal")
    assert gap > 1.0, gap
    for i, k in ((ca, 0.5), (cb, 1.5)):
        u = goals[0, i, 0] / np.linalg.norm(goals[0, i, 0])               # (the goal is the point opposite: walk outwards along it)
        walk(0, i, goals[0, i, 0] - (S[0, i, 8] + k * step) * u, np.arctan2(u[1], u[0]))
    S32, g32 = f32(S), f32(goals)
    cw = _worlds(S32, g32, P, rb, rw, model)
    assert VARIANT_25 in cw.step_variant(), cw.step_variant()
    nsub = 5
    res = fused_substeps_vs_oracle(cw, SFMS.index(model), S32, g32, P, None, None, DT, nsub, True, respawn=rw, respawn_bounds=rb,
                                   group="substep loop in one exec region, per substep", what=f"events on consecutive substeps {model}")
    assert res["within"] >= res["substeps"] - res["ill_conditioned"] and res["goal_flips"] == 0, res
    # the events happened where they were staged (the traced launch is cs_step's: a second batch replays it for the records)
    trace = _worlds(S32, g32, P, rb, rw, model).step_trace(DT, nsub)
    x = np.concatenate([S32[None, :, :, 0], trace[..., 0]])               # [nsub + 1, W, rows]: x before substep k / after substep k - 1
    jumped = np.abs(np.diff(x, axis=0)) > 1.0                             # [nsub, W, rows]: respawned in substep k
    assert np.flatnonzero(jumped[:, 1, ta]).tolist() == [1] and np.flatnonzero(jumped[:, 1, tb]).tolist() == [2], (jumped[:, 1, ta], jumped[:, 1, tb])
    assert not jumped[:, 0].any()
    head = np.concatenate([g32[None, :, :, 0], trace[..., 10:12]])        # head of the goal list before substep k / after it
    switched = np.any(head[1:] != head[:-1], axis=-1)
    assert np.flatnonzero(switched[:, 0, ca]).tolist() == [1] and np.flatnonzero(switched[:, 0, cb]).tolist() == [2], (switched[:, 0, ca], switched[:, 0, cb])
    # the goal lists as committed
    got_goals = cw.get_goals()
    for w in range(2):
        _, ref_goals, _ = orc.step_block(SFMS.index(model), S32[w].astype(np.float64), g32[w].astype(np.float64), None, P.astype(np.float64), DT, nsub,
                                         np.zeros(N), True, respawn=bool(rw[w]), respawn_par=(rb[0], rb[1], 0.0))
        ref_goals = np.asarray(ref_goals).reshape(got_goals[w].shape)
        if w == 0:
            np.testing.assert_array_equal(got_goals[w], f32(ref_goals))
            np.testing.assert_array_equal(got_goals[w][ca], g32[w][ca][::-1])
        else:
            np.testing.assert_array_equal(got_goals[w][..., 0], f32(ref_goals)[..., 0])
            np.testing.assert_array_equal(np.isnan(got_goals[w]), np.isnan(ref_goals))
            assert np.nanmax(np.abs(got_goals[w][..., 1] - ref_goals[..., 1])) < 1e-5


@pytest.mark.parametrize("model", ["hsfm_farina", "hsfm_guo"])
def test_first_substep_refreshes_the_incoming_velocity(model):
    """Incoming rows whose stored (vx, vy) is not R(theta) bv (what a caller may hand in; the reference refreshes it in place,
    forces_parallel.py:254-256): substep 0 moves the position with the STORED velocity and forms the forces from the REFRESHED one.  The
    stored columns are off by ~0.05 m/s: taking the wrong one is 6e-4 m on the position or 1e-3 m/s on the velocity, against the 1e-5 bar."""
    W = 3
    S, goals, P, rb, rw = _walking(W, N, model, seed0=749)
    rng = np.random.default_rng(5)
    S = S.copy()
    S[:, :, 3:5] += rng.normal(0.0, 0.05, S[:, :, 3:5].shape).astype(np.float32)
    c, s = np.cos(S[..., 2].astype(np.float64)), np.sin(S[..., 2].astype(np.float64))
    assert np.abs(S[..., 3] - (c * S[..., 5] - s * S[..., 6])).min() > 1e-4
    _per_substep(S, goals, P, rb, rw, model, 3, VARIANT_25, f"stored velocity off R(theta) bv, {model}")


# the other builds inside the region (select_variant's choice at three worlds): rows, what step_variant() must name, CROWDSTEP_ROW16
OTHER_BUILDS = [(30, "MAXT=64,OCC=1,ROWS_CT=30,LEAN=1", None), (20, "MAXT=64,OCC=1,ROWS_CT=20,LEAN=1", None),
                (50, "MAXT=64,OCC=3,ROWS_CT=50,LEAN=1", None), (10, "MAXT=64,OCC=4,ROWS_CT=10,LEAN=1", "0")]


@pytest.mark.parametrize("n,variant,row16", OTHER_BUILDS)
def test_other_builds_in_the_region(n, variant, row16):
    """W = 3 through every other compile-time-row plain build (even row counts: the antipodal partner; 50 rows: one world per wavefront;
    10 rows: six worlds per wavefront, on the LDS kernel instead of the DPP-row one)."""
    if row16 is not None:
        os.environ["CROWDSTEP_ROW16"] = row16
    try:
        for model in ("hsfm_farina", "sfm_guo"):
            S, goals, P, rb, rw = _walking(3, n, model, seed0=853 + n)
            _per_substep(S, goals, P, rb, rw, model, 8, variant, f"{n} rows W=3 {model}")
    finally:
        if row16 is not None:
            os.environ.pop("CROWDSTEP_ROW16", None)
