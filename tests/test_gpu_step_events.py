"""The two rare events of a substep in the plain one-wavefront builds (MAXT = 64, LEAN = 1, compile-time row count: sfmstep_kernel.h
EARLY_VOTES): the goal switch and the respawn rule sit behind wave votes that the tail of a substep takes on the row it stores -- before
the respawn rule it gates, and a substep ahead of the goal switch it gates.  What a vote taken on the wrong row, against the wrong goal,
handed on wrongly or not replaced behind a respawn would break, at the smallest shapes that can break it:

  * a hit on the very first row of a launch (nobody voted on it), at the heads of substeps 1 and 2 in two worlds of one wavefront, and one
    that falls on the tail of the last substep (the list rotates in the NEXT launch; k substeps = k launches of one = 2 + 3, bitwise);
  * goal lists of length 0 (NaN), 1 (an agent parked inside r: the vote is taken in every substep) and 2;
  * a respawn in one world and a hit in the other world of the wavefront one substep later; two humans respawning in one substep;
  * rows that would flag with the rule off (for the launch, and for their world only);
  * 25 rows at W = 1 / 2 / 3 / 5, the other row counts at W = 3, Guo SFM and Moussaid HSFM, and the OCC = 4 twin at W = 4200.

Every parity check is per substep against the f64 oracle from the same f32 inputs at the 1e-5 bar of tests/parity_util.py; the staged
events are read back from the per-substep trace.  No row of these inputs may be one whose heading float32 has lost (row_errors).
"""
import os

import numpy as np
import pytest

from parity_util import f32, fused_substeps_vs_oracle

pytestmark = pytest.mark.gpu

DT = 0.0125
N = 25
NSUB = 5
SPEED = 0.9
STEP = SPEED * DT   # what a staged human walks per substep
GROUP = "goal switch and respawn rule behind early wave votes, per substep"
# select_variant's choice for a handful of worlds: rows -> (what step_variant() must name, CROWDSTEP_ROW16 for the launch)
BUILDS = {25: ("MAXT=64,OCC=1,ROWS_CT=25,LEAN=1", None), 30: ("MAXT=64,OCC=1,ROWS_CT=30,LEAN=1", None), 20: ("MAXT=64,OCC=1,ROWS_CT=20,LEAN=1", None),
          50: ("MAXT=64,OCC=3,ROWS_CT=50,LEAN=1", None), 10: ("MAXT=64,OCC=4,ROWS_CT=10,LEAN=1", "0")}


def _worlds(S, goals, P, rb, rw, model):
    from social_navigation_pyenvs_amd.batched import CrowdWorlds

    return CrowdWorlds(S, goals, P, None, None, type=model, all_params_equal=True, respawn_bounds=rb, respawn_worlds=rw)


class _row16:
    """The 10-row worlds on the LDS kernel instead of the DPP-row one for the launches inside; the variable is left as it was found."""

    def __init__(self, n):
        self.value = BUILDS[n][1]

    def __enter__(self):
        self.before = os.environ.get("CROWDSTEP_ROW16")
        if self.value is not None:
            os.environ["CROWDSTEP_ROW16"] = self.value

    def __exit__(self, *exc):
        if self.value is None:
            return
        if self.before is None:
            os.environ.pop("CROWDSTEP_ROW16", None)
        else:
            os.environ["CROWDSTEP_ROW16"] = self.before


_WALKING = {}


def _walking(W, n, model, seed0, pick=None):
    """Hybrid worlds two Gym steps in (distinct velocities, headings that turn), as float64 copies of the float32 rows: (states, goals, P,
    rb, rw); made once per shape.  `pick`: keep these worlds only (e.g. two circle worlds for one wavefront)."""
    from social_navigation_pyenvs_amd import scenarios as sc

    key = (W, n, model, seed0)
    if key not in _WALKING:
        S, goals, P, rb = sc.hybrid_worlds(W, n, model, seed0=seed0)
        rw = (np.arange(W) % 2 == 1).astype(np.int32)
        with _row16(n):
            cw = _worlds(f32(S), f32(goals), f32(P), rb, rw, model)
            for _ in range(2):
                cw.step(DT, 20)
        _WALKING[key] = (cw.get_states(), cw.get_goals(), f32(P), rb, rw)
    S, goals, P, rb, rw = _WALKING[key]
    sel = np.arange(W) if pick is None else np.asarray(pick)
    return S[sel].astype(np.float64), goals[sel].astype(np.float64), P, rb, rw[sel].copy()


def _walk(S, w, i, pos, yaw, headed):
    S[w, i, 0:2] = pos; S[w, i, 2] = yaw
    S[w, i, 3:5] = SPEED * np.array([np.cos(yaw), np.sin(yaw)])
    S[w, i, 5:8] = (SPEED, 0.0, 0.0) if headed else (0.0, 0.0, 0.0)


def _lonely_goals(S, goals, w, taken=()):
    """Humans of circle world w, the one whose goals[0] is farthest from every other body first"""
    n = S.shape[1]
    dg = np.linalg.norm(goals[w, :, 0][:, None] - S[w, None, :, 0:2], axis=-1)
    dg[np.arange(n), np.arange(n)] = np.inf
    order = [int(i) for i in np.argsort(-dg.min(axis=1)) if i not in taken]
    assert dg[order[0]].min() > 1.0, dg[order[0]].min()
    return order


def _stage_hit(S, goals, w, i, k, headed, off_goal=True):
    """Human i of circle world w walks at its goals[0] and stands within r of it first on the row that substep k reads (k = 0: the incoming
    row; k = the launch's substep count: the row its last tail stores).  It arrives half a radian off the radial direction: behind the
    switch the new goal lies 2.6 rad off its heading, not the 3.14 at which the sign of the heading torque is a coin flip of the last bit.
    `off_goal`: the row's goal columns name another point than the head of the list, so the switch has to rewrite them whatever the
    list's length."""
    g = goals[w, i, 0]
    yaw = np.arctan2(g[1], g[0]) + 0.5
    yaw -= 2.0 * np.pi * (yaw > np.pi)   # (the reference keeps every heading in [-pi, pi])
    u = np.array([np.cos(yaw), np.sin(yaw)])
    _walk(S, w, i, g - (S[w, i, 8] + (k - 0.5) * STEP) * u, yaw, headed)
    if off_goal:
        S[w, i, 10:12] = g + 2.0 * u + np.array([-u[1], u[0]])


def _roomy_at_zone_edge(S, goals, w, count, apart=1.0):
    """`count` humans of traffic world w with the most room where they would enter the respawn zone (|p - goals[0]| < 3), `apart` in y"""
    n = S.shape[1]
    edge = np.stack([goals[w, :, 0, 0] + 3.0, S[w, :, 1]], -1)
    room = np.linalg.norm(edge[:, None] - S[w, None, :, 0:2], axis=-1)
    room[np.arange(n), np.arange(n)] = np.inf
    out = []
    for i in np.argsort(-room.min(axis=1)):
        if all(abs(S[w, i, 1] - S[w, j, 1]) > apart for j in out):
            out.append(int(i))
        if len(out) == count:
            break
    assert len(out) == count and all(room[i].min() > 0.7 for i in out), [room[i].min() for i in out]
    return out


def _stage_respawn(S, goals, w, i, k, headed):
    """Human i of traffic world w walks left into the zone |p - goals[0]| < 3 with the move of substep k: the rule respawns it in substep k"""
    _walk(S, w, i, (goals[w, i, 0, 0] + 3.0 + (k + 0.5) * STEP, S[w, i, 1]), -np.pi, headed)


def _run(S, goals, P, rb, rw, model, nsub, what, worlds=None, variant=None):
    """Every substep of a launch of `nsub` against the oracle; returns (figures, trace events): switched [nsub, W, n] (the head of the goal
    list changed in substep k), jumped [nsub, W, n] (x moved by more than a metre in substep k), the trace itself."""
    from social_navigation_pyenvs_amd.batched import SFMS

    n = S.shape[1]
    S32, g32 = f32(S), f32(goals)
    with _row16(n):
        cw = _worlds(S32, g32, P, rb, rw, model)
        assert (variant or BUILDS[n][0]) in cw.step_variant(), cw.step_variant()
        res = fused_substeps_vs_oracle(cw, SFMS.index(model), S32, g32, P, None, None, DT, nsub, True, respawn=None if rb is None else rw,
                                       respawn_bounds=rb, worlds=worlds, group=GROUP, what=what)
        trace = _worlds(S32, g32, P, rb, rw, model).step_trace(DT, nsub)
    print(f"{what}: worst {res['worst']:.3e} (float32 oracle {res['worst_f32_oracle']:.3e}), {res['within']} of {res['substeps']} world-substeps "
          f"within 1e-5, {res['ill_conditioned']} ill conditioned, {res['goal_flips']} goal flips, {res['lost_heading_rows']} lost headings")
    assert res["lost_heading_rows"] == 0, res
    assert res["within"] >= res["substeps"] - res["ill_conditioned"] and res["goal_flips"] == 0, (what, res)
    head = np.nan_to_num(np.concatenate([g32[None, :, :, 0], trace[..., 10:12]]))
    switched = np.any(head[1:] != head[:-1], axis=-1)
    x = np.concatenate([S32[None, :, :, 0], trace[..., 0]])
    jumped = np.abs(np.diff(x, axis=0)) > 1.0
    return res, switched, jumped, trace


def _when(events, w, i):
    return np.flatnonzero(events[:, w, i]).tolist()


def test_hit_on_the_first_row_of_a_launch():
    """The incoming row stands within r of goals[0]: no earlier substep voted on it, substep 0 runs the switch unasked.  The row's goal
    columns name a third point, so they must become the NEW head of the rotated two-goal list in substep 0."""
    model = "hsfm_farina"
    S, goals, P, rb, rw = _walking(2, N, model, seed0=2011)
    ca = _lonely_goals(S, goals, 0)[0]
    _stage_hit(S, goals, 0, ca, 0, True)
    res, switched, jumped, trace = _run(S, goals, P, rb, rw, model, NSUB, "hit on the incoming row")
    assert _when(switched, 0, ca) == [0], switched[:, 0, ca]
    np.testing.assert_array_equal(trace[0, 0, ca, 8:10], f32(goals)[0, ca, 1])     # the row's goal columns: the old second goal
    np.testing.assert_array_equal(trace[0, 0, ca, 10:12], f32(goals)[0, ca, 1])
    assert switched.sum() == 1 and jumped.sum() == 0


def test_hits_at_the_heads_of_substeps_1_and_2_in_two_worlds_of_one_wavefront():
    """Two circle worlds in ONE wavefront (worlds 0 and 2 of a hybrid batch): a hit at the head of substep 1 in the first, at the head of
    substep 2 in the second -- the vote of substep 0's head gates substep 1's switch, and the wavefront votes again while it switches."""
    model = "hsfm_farina"
    S, goals, P, rb, rw = _walking(3, N, model, seed0=2027, pick=[0, 2])
    ca, cb = _lonely_goals(S, goals, 0)[0], _lonely_goals(S, goals, 1)[0]
    _stage_hit(S, goals, 0, ca, 1, True)
    _stage_hit(S, goals, 1, cb, 2, True)
    res, switched, jumped, trace = _run(S, goals, P, rb, rw, model, NSUB, "hits at the heads of substeps 1 and 2")
    assert _when(switched, 0, ca) == [1] and _when(switched, 1, cb) == [2], (switched[:, 0, ca], switched[:, 1, cb])
    assert switched.sum() == 2 and jumped.sum() == 0
    np.testing.assert_array_equal(trace[1, 0, ca, 8:10], f32(goals)[0, ca, 1])
    np.testing.assert_array_equal(trace[2, 1, cb, 8:10], f32(goals)[1, cb, 1])


@pytest.mark.parametrize("model", ["hsfm_farina", "sfm_guo"])
def test_hit_on_the_tail_of_the_last_substep_rotates_in_the_next_launch(model):
    """The row that the LAST tail of a launch of five stores stands within r: the vote taken at the head of substep 4 is non-zero, but the
    switch belongs to the head of the next launch's substep 0 (forces_parallel.py:226 tests the incoming position).  The list does not
    rotate in this launch, and a launch of five = five launches of one = a launch of two and one of three, states and goal lists, bit for
    bit (the build before the early votes satisfies the same); the launch behind them rotates the list in all three."""
    headed = model.startswith("hsfm")
    S, goals, P, rb, rw = _walking(2, N, model, seed0=2039)
    ca = _lonely_goals(S, goals, 0)[0]
    _stage_hit(S, goals, 0, ca, NSUB, headed, off_goal=False)
    res, switched, jumped, trace = _run(S, goals, P, rb, rw, model, NSUB, f"hit on the last tail {model}")
    assert switched.sum() == 0, np.argwhere(switched)
    S32, g32 = f32(S), f32(goals)
    whole, ones, split = (_worlds(S32, g32, P, rb, rw, model) for _ in range(3))
    whole.step(DT, NSUB)
    for _ in range(NSUB):
        ones.step(DT, 1)
    split.step(DT, 2); split.step(DT, 3)
    last = whole.get_states()[0, ca]
    assert np.linalg.norm(g32[0, ca, 0].astype(np.float64) - last[0:2]) < last[8], "the staged human did not arrive with the last tail"
    for other in (ones, split):
        np.testing.assert_array_equal(whole.get_states(), other.get_states())
        np.testing.assert_array_equal(whole.get_goals(), other.get_goals())
    np.testing.assert_array_equal(whole.get_goals(), g32)
    for cw in (whole, ones, split):
        cw.step(DT, 1)
    for other in (ones, split):
        np.testing.assert_array_equal(whole.get_states(), other.get_states())
        np.testing.assert_array_equal(whole.get_goals(), other.get_goals())
    np.testing.assert_array_equal(whole.get_goals()[0, ca], g32[0, ca, ::-1])
    np.testing.assert_array_equal(whole.get_states()[0, ca, 10:12], g32[0, ca, 1])


def test_goal_lists_of_length_zero_one_and_two():
    """Three humans of one circle world.  A list of length 1 (NaN second slot), its owner parked at rest inside r: some lane hits in every
    substep, so the vote is non-zero throughout, the list has nothing to rotate, and the row's goal columns (a third point before) are
    the goal from substep 0 on.  A list of length 0 (NaN head): never a hit, the row keeps its goal columns.  A list of length 2 whose
    owner arrives at the head of substep 1, as everywhere else."""
    model = "hsfm_farina"
    S, goals, P, rb, rw = _walking(2, N, model, seed0=2053)
    one, two, zero = _lonely_goals(S, goals, 0)[:3]
    _stage_hit(S, goals, 0, one, 0, True)
    S[0, one, 0:2] = goals[0, one, 0] * (1.0 - 0.1 / np.linalg.norm(goals[0, one, 0]))   # 0.1 m inside the goal's circle, at rest
    S[0, one, 3:8] = 0.0
    goals[0, one, 1] = np.nan
    _stage_hit(S, goals, 0, two, 1, True)
    goals[0, zero] = np.nan
    res, switched, jumped, trace = _run(S, goals, P, rb, rw, model, NSUB, "goal lists of length 0, 1, 2")
    g32 = f32(goals)
    assert _when(switched, 0, two) == [1] and switched.sum() == 1, np.argwhere(switched)
    for k in range(NSUB):
        np.testing.assert_array_equal(trace[k, 0, one, 8:10], g32[0, one, 0])
        np.testing.assert_array_equal(trace[k, 0, zero, 8:10], f32(S)[0, zero, 10:12])
        assert np.linalg.norm(trace[k, 0, one, 0:2].astype(np.float64) - g32[0, one, 0]) < 0.3
    cw = _worlds(f32(S), g32, P, rb, rw, model)
    cw.step(DT, NSUB)
    want = g32.copy()
    want[0, two] = g32[0, two, ::-1]
    np.testing.assert_array_equal(cw.get_goals(), want)


@pytest.mark.parametrize("s", [0, 2])
def test_respawn_in_one_world_and_hit_in_the_other_a_substep_later(s):
    """A circle world and a traffic world in one wavefront: a traffic human respawns in substep s, a circle human stands within r at the head
    of substep s + 1.  The wavefront that respawns re-runs the next goal switch without a vote: the respawned lane is tested there on its new
    position against its new goals[0] (whose y is the clamped position's), the circle lane on the row the tail stored."""
    model = "hsfm_farina"
    S, goals, P, rb, rw = _walking(2, N, model, seed0=2069)
    ca = _lonely_goals(S, goals, 0)[0]
    (t,) = _roomy_at_zone_edge(S, goals, 1, 1)
    _stage_hit(S, goals, 0, ca, s + 1, True)
    _stage_respawn(S, goals, 1, t, s, True)
    res, switched, jumped, trace = _run(S, goals, P, rb, rw, model, NSUB, f"respawn in substep {s}, hit at the head of substep {s + 1}")
    assert _when(jumped, 1, t) == [s] and jumped.sum() == 1, np.argwhere(jumped)
    assert _when(switched, 0, ca) == [s + 1], switched[:, 0, ca]
    # the respawned human: goals[0] = (old x, its y), written to the row's columns 6:8 as the reference does
    np.testing.assert_array_equal(trace[s, 1, t, 10:12], np.array([f32(goals)[1, t, 0, 0], trace[s, 1, t, 1]], np.float32))
    np.testing.assert_array_equal(trace[s, 1, t, 6:8], trace[s, 1, t, 10:12])


@pytest.mark.parametrize("model", ["hsfm_farina", "sfm_guo"])
def test_two_humans_respawn_in_one_substep(model):
    """Two humans of the traffic world walk into the zone with the move of substep 1: the lower index lands at max_x + 2 max_r (c = 0), the
    other 2 max_r behind it (c = 1), inside the one branch the wavefront takes on its vote."""
    headed = model.startswith("hsfm")
    S, goals, P, rb, rw = _walking(2, N, model, seed0=2081)
    ta, tb = _roomy_at_zone_edge(S, goals, 1, 2)
    for i in (ta, tb):
        _stage_respawn(S, goals, 1, i, 1, headed)
    res, switched, jumped, trace = _run(S, goals, P, rb, rw, model, NSUB, f"two respawns in substep 1 {model}")
    assert _when(jumped, 1, ta) == [1] and _when(jumped, 1, tb) == [1] and jumped.sum() == 2, np.argwhere(jumped)
    first, second = min(ta, tb), max(ta, tb)
    others = [i for i in range(N) if i not in (ta, tb)]
    max_x, max_r = float(trace[1, 1, others, 0].max()), float(S[1, :, 8].max())
    assert abs(float(trace[1, 1, first, 0]) - max(max_x + 2.0 * max_r, rb[0])) < 1e-5
    assert abs(float(trace[1, 1, second, 0]) - float(trace[1, 1, first, 0]) - 2.0 * max_r) < 1e-5


@pytest.mark.parametrize("off", ["launch", "world"])
def test_rows_that_would_flag_with_the_rule_off(off):
    """A traffic human walks into the zone with the rule off -- for the whole launch (no respawn bounds: CS_RESPAWN clear) or for its world
    (world flag 0 in a launch with the rule on): nobody jumps, every substep as the oracle without the rule."""
    model = "hsfm_farina"
    S, goals, P, rb, rw = _walking(2, N, model, seed0=2083)
    (t,) = _roomy_at_zone_edge(S, goals, 1, 1)
    _stage_respawn(S, goals, 1, t, 1, True)
    rw = np.zeros(2, np.int32)
    res, switched, jumped, trace = _run(S, goals, P, None if off == "launch" else rb, rw, model, NSUB, f"rule off for the {off}")
    assert jumped.sum() == 0, np.argwhere(jumped)
    assert np.linalg.norm(trace[-1, 1, t, 0:2].astype(np.float64) - goals[1, t, 0]) < 3.0, "the staged human did not enter the zone"


def _hit_and_respawn(S, goals, rw, headed, w_hit, w_resp):
    """A hit at the head of substep 1 in circle world w_hit and, where the batch has a traffic world, a respawn in substep 2 in w_resp"""
    ca = _lonely_goals(S, goals, w_hit)[0]
    _stage_hit(S, goals, w_hit, ca, 1, headed)
    t = None
    if w_resp is not None:
        (t,) = _roomy_at_zone_edge(S, goals, w_resp, 1)
        _stage_respawn(S, goals, w_resp, t, 2, headed)
    return ca, t


def _check_hit_and_respawn(switched, jumped, w_hit, ca, w_resp, t, worlds=None):
    ws = np.arange(switched.shape[1]) if worlds is None else np.asarray(worlds)
    assert _when(switched, w_hit, ca) == [1], switched[:, w_hit, ca]
    if t is not None:
        assert _when(jumped, w_resp, t) == [2], jumped[:, w_resp, t]
    assert jumped[:, ws].sum() == int(t is not None), np.argwhere(jumped)


@pytest.mark.parametrize("W", [1, 2, 3, 5])
def test_events_in_the_last_worlds_at_25_rows(W):
    """25 rows, two worlds per wavefront: W = 1 half a wavefront, W = 2 a full one, W = 3 and 5 a ragged last wavefront whose only world
    holds the hit (its idle half votes nothing); the respawn in the last traffic world."""
    model = "hsfm_farina"
    S, goals, P, rb, rw = _walking(W, N, model, seed0=2087)
    w_hit, w_resp = (W - 1) & ~1, (((W - 2) | 1) if W >= 2 else None)
    ca, t = _hit_and_respawn(S, goals, rw, True, w_hit, w_resp)
    res, switched, jumped, trace = _run(S, goals, P, rb, rw, model, NSUB, f"25 rows W={W}")
    _check_hit_and_respawn(switched, jumped, w_hit, ca, w_resp, t)


@pytest.mark.parametrize("n", [10, 20, 30, 50])
def test_events_at_the_other_row_counts(n):
    """10 / 20 / 30 / 50 rows at W = 3 (six, three, two and one world per wavefront; 50 rows: the OCC = 3 build's respawn walk)."""
    model = "hsfm_farina"
    S, goals, P, rb, rw = _walking(3, n, model, seed0=2099 + n)
    ca, t = _hit_and_respawn(S, goals, rw, True, 2, 1)
    res, switched, jumped, trace = _run(S, goals, P, rb, rw, model, NSUB, f"{n} rows W=3")
    _check_hit_and_respawn(switched, jumped, 2, ca, 1, t)


@pytest.mark.parametrize("model", ["sfm_guo", "hsfm_moussaid"])
def test_events_under_guo_sfm_and_moussaid_hsfm(model):
    """The builds without a heading (no carried velocity behind the respawn) and with partner velocities in LDS, 25 rows at W = 3."""
    S, goals, P, rb, rw = _walking(3, N, model, seed0=2111)
    ca, t = _hit_and_respawn(S, goals, rw, model.startswith("hsfm"), 2, 1)
    res, switched, jumped, trace = _run(S, goals, P, rb, rw, model, NSUB, f"25 rows W=3 {model}")
    _check_hit_and_respawn(switched, jumped, 2, ca, 1, t)


def test_events_in_the_last_wavefront_of_a_crowded_grid():
    """W = 4200: more than two wavefronts per SIMD, so the OCC = 4 twin runs (cs_step_variant says so).  The hit and the respawn in the two
    worlds of the last wavefront; those and the first wavefront's checked per substep."""
    model, W = "hsfm_farina", 4200
    S, goals, P, rb, rw = _walking(W, N, model, seed0=2113)
    ca, t = _hit_and_respawn(S, goals, rw, True, W - 2, W - 1)
    worlds = [0, 1, W - 2, W - 1]
    res, switched, jumped, trace = _run(S, goals, P, rb, rw, model, NSUB, f"25 rows W={W}", worlds=worlds, variant="MAXT=64,OCC=4,ROWS_CT=25,LEAN=1")
    assert res["substeps"] == NSUB * len(worlds)
    _check_hit_and_respawn(switched, jumped, W - 2, ca, W - 1, t, worlds=worlds)
