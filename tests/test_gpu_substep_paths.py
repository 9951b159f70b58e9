"""The rare-event blocks of the substep loop (sfmstep_substep.inc and its fragments) sit behind weighted wave-uniform branches, outside
the fall-through path of a quiet substep, and the priority turn of the younger wavefront of a SIMD is a scalar test (sfmstep_kernel.h
CS_RARE, wave_in_wg).  Every block that moved is driven here at the smallest shapes that reach it -- the inputs and the events they
produce are tests/substep_path_cases.py, asserted on the oracle alone in tests/test_substep_paths_cpu.py:

  * the contact pass: two bodies overlapping by 2 cm in substep 0, apart behind it (Helbing's pass and Moussaid's);
  * the goal switch behind the carried vote: a human inside r of goals[0] on the incoming row, one that arrives there in substep 2;
  * the respawn rule behind the tail's vote: a human of a traffic world that comes within 3 m of its goal in substep 1;
  * the recorders: every launch against the oracle is a cs_step_trace launch, and the trace's records are the rows single launches leave;
  * the priority turn: a grid of exactly two wavefronts per SIMD, the three events planted in worlds of the younger half.

W = 2 and 3 at 25 rows (a full wavefront; one with idle lanes) and at 50 rows (a world per wavefront), 25 humans + a robot row;
sfm_helbing, hsfm_farina, hsfm_new_moussaid.  Every case: each of the 3 substeps of one launch against the f64 oracle through
parity_util.fused_substeps_vs_oracle at its 1e-5 bar, and one launch of 3 substeps = three launches of 1, bit for bit."""
import numpy as np
import pytest

import substep_path_cases as spc
from parity_util import fused_substeps_vs_oracle

gpu = pytest.mark.gpu

GROUP = "substep paths: contact pass, voted goal switch, respawn rule, recorders, priority turn, per substep"
BUILDS = {(25, False): "MAXT=64,OCC=1,ROWS_CT=25,LEAN=1", (50, False): "MAXT=64,OCC=3,ROWS_CT=50,LEAN=1", (25, True): "MAXT=64,OCC=1,ROWS_CT=26,LEAN=3"}


def _check(model, S, goals, P, rb, rw, R, A, what, *, variant, worlds=None, layout="aos"):
    """One launch of NSUB substeps, every substep against the oracle; then NSUB = 1 + ... + 1 bit for bit, and the trace's records are
    the rows the single launches leave.  Returns the figures of the oracle comparison."""
    from social_navigation_pyenvs_amd.batched import CrowdWorlds, SFMS

    robot_row = R is not None

    def make():
        return CrowdWorlds(S, goals, P, None, None, type=model, all_params_equal=True, respawn_bounds=rb, respawn_worlds=rw, robot_row=robot_row,
                           robot=R, layout=layout)

    cw = make()
    assert variant in cw.step_variant(), cw.step_variant()
    res = fused_substeps_vs_oracle(cw, SFMS.index(model), S, goals, P, None, None, spc.DT, spc.NSUB, True, respawn=rw, respawn_bounds=rb,
                                   robot_row=robot_row, robot=R, action=A, worlds=worlds, group=GROUP, what=what)
    print(f"{what}: worst {res['worst']:.3e} (float32 oracle {res['worst_f32_oracle']:.3e}), {res['within']} of {res['substeps']} world-substeps "
          f"within 1e-5, {res['ill_conditioned']} ill conditioned")
    assert res["within"] >= res["substeps"] - res["ill_conditioned"], (what, res)
    whole, ones, traced = make(), make(), make()
    whole.step(spc.DT, spc.NSUB, A)
    trace = traced.step_trace(spc.DT, spc.NSUB, A) if A is not None else traced.step_trace(spc.DT, spc.NSUB)
    n = goals.shape[1]
    for k in range(spc.NSUB):
        ones.step(spc.DT, 1, A)
        np.testing.assert_array_equal(trace[k][:, :n, 0:8], ones.get_states()[:, :n, 0:8], err_msg=f"{what}: record {k} of the trace")
        np.testing.assert_array_equal(trace[k][:, :n, 8:10], ones.get_states()[:, :n, 10:12], err_msg=f"{what}: goal columns of record {k}")
    for other in (ones, traced):
        np.testing.assert_array_equal(whole.get_states(), other.get_states(), err_msg=what)
        np.testing.assert_array_equal(whole.get_goals(), other.get_goals(), err_msg=what)
        if robot_row:
            np.testing.assert_array_equal(whole.get_robot(), other.get_robot(), err_msg=what)
    return whole


@gpu
@pytest.mark.parametrize("W,n,robot_row", spc.SHAPES)
@pytest.mark.parametrize("model", spc.MODELS)
@pytest.mark.parametrize("kind", spc.KINDS)
def test_rare_event_blocks(kind, model, W, n, robot_row):
    S, goals, P, rb, rw, R, A, w, who = spc.case(kind, model, W, n, robot_row)
    whole = _check(model, S, goals, P, rb, rw, R, A, f"{kind} {model} W={W} {n} humans{' + robot' if robot_row else ''}", variant=BUILDS[(n, robot_row)])
    # the event left its mark on the GPU's rows too
    got, gl = whole.get_states(), whole.get_goals()
    if kind == "goals":
        for i in who:
            np.testing.assert_array_equal(gl[w, i, 0], goals[w, i, 1])
            np.testing.assert_array_equal(gl[w, i, 1], goals[w, i, 0])
    elif kind == "respawn":
        assert got[w, who[0], 0] > 0.0 and S[w, who[0], 0] < 0.0   # (from the goal line to the other end of the lane)


def _variant_of_shape(W, n, model=3):
    """cs_step_variant for a plain crowd batch of this shape (a function of the shape and the device: nothing is dereferenced)"""
    import ctypes as C

    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    d = _lib.cs_worlds()
    d.W, d.n, d.G, d.O, d.Smax = W, n, 2, 0, 0
    d.type = model
    d.flags = _lib.CS_ALL_PARAMS_EQUAL | _lib.CS_PARAMS_SHARED
    d.layout = _lib.CS_LAYOUT_SOA
    for field in ("d_state", "d_goals", "d_params", "d_safety"):
        setattr(d, field, C.c_void_p(0x1000))
    buf = C.create_string_buffer(256)
    assert lib.cs_step_variant(C.byref(d), 0, buf, 256) == _lib.CS_OK
    return buf.value.decode()


def _largest_uncrowded_batch(n):
    """The launcher calls a grid crowded, and picks the four-wave build, beyond two one-wavefront blocks per SIMD (crowdstep.hip
    select_variant): the largest W that still names the OCC = 1 build fills the device with exactly two -- the grid whose second half
    takes the priority turn.  Found from cs_step_variant, which asks the device for its SIMDs (4096 worlds of 25 rows on a whole MI355X)."""
    roomy = lambda W: f"OCC=1,ROWS_CT={n},LEAN=1" in _variant_of_shape(W, n)
    lo, hi = 2, 4
    while roomy(hi):
        lo, hi = hi, 2 * hi
        assert hi < 1 << 24
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if roomy(mid) else (lo, mid)
    return lo


@gpu
def test_priority_turn_of_the_younger_wavefronts():
    """A grid of exactly two wavefronts per SIMD (two 25-row worlds a wavefront): the second half of the grid takes the priority turn in
    every substep.  The three events sit in the last wavefronts' worlds; first and last 32 worlds against the oracle, all worlds 3 = 1 + 1 + 1."""
    n, model = 25, "hsfm_farina"
    W = _largest_uncrowded_batch(n)          # two worlds a wavefront: W / 2 wavefronts = 2 x SIMDs
    simds = W // 4
    assert W % 4 == 0 and W >= 64, W
    S, goals, P, rb, rw = spc.walking_worlds(W, n, model, 4211)
    for kind, we in (("contact", W - 2), ("goals", W - 4), ("respawn", W - 1)):
        spc.plant(kind, S, goals, w_even=we, w_odd=we)
    S, goals, P = S.astype(np.float32), goals.astype(np.float32), P.astype(np.float32)
    from social_navigation_pyenvs_amd.batched import CrowdWorlds

    cw = CrowdWorlds(S, goals, P, None, None, type=model, all_params_equal=True, respawn_bounds=rb, respawn_worlds=rw, layout="soa")
    assert f"grid={2 * simds} " in cw.step_variant(), cw.step_variant()   # (one-wavefront blocks: the launcher's condition for the turn)
    worlds = list(range(32)) + list(range(W - 32, W))
    whole = _check(model, S, goals, P, rb, rw, None, None, f"two wavefronts per SIMD, W={W}", variant="MAXT=64,OCC=1,ROWS_CT=25,LEAN=1", worlds=worlds, layout="soa")
    assert whole.get_states()[W - 1, :, 0].max() > rb[0] - 0.1
