"""What a wavefront of the plain one-wavefront builds does AROUND its substeps (sfmstep_kernel.h LAUNCH_TRIM: MAXT = 64, LEAN = 1, compile-time
row count): the load phase addresses every array as a kernel-argument base + a 32-bit lane offset and issues the action's and the invisible
robot's loads only in a launch that has them, the prologue keeps no default for a value only a lane with a human reads, the epilogue stores
off scalar bases.  A wrong offset, a load left out of a launch that needs it, or a lane without a world touching memory shows at the
smallest shapes:

  * 25 rows at W = 1 / 2 / 3 / 5 (half a wavefront; a full one; a last wavefront with one world; a workgroup with idle wavefronts), both
    state layouts; 10 / 30 / 50 rows at W = 3;
  * a visible robot with a constant action, an invisible robot with an action (its five columns and the action loaded), and both without
    an action (neither loaded);
  * goal lists of length 1 and 2 in a two-slot array, and a one-slot array (the second slot's load reads the first);
  * one parameter table for all worlds (CS_PARAMS_SHARED) and a table per world with equal rows: the same bits;
  * Guo SFM and Moussaid HSFM; W = 4200, where cs_step_variant names the OCC = 4 twin.

Every case: launches of 1 and of 3 substeps, every substep against the f64 oracle from the same f32 inputs at the 1e-5 bar of
tests/parity_util.py, and one launch of three substeps = three launches of one, bit for bit (states, goal lists, robot rows).
The launcher keeps shapes whose byte offsets do not fit 32 bits off these builds (crowdstep.hip offsets_fit_32): the last test, which needs
no GPU -- cs_step_variant reports the choice from the shape alone.
"""
import ctypes as C
import os

import numpy as np
import pytest

from parity_util import f32, fused_substeps_vs_oracle

gpu = pytest.mark.gpu

DT = 0.0125
GROUP = "launch trim: load phase, prologue and epilogue of the plain one-wavefront builds, per substep"
# select_variant's choice for a handful of worlds: rows -> (what step_variant() must name, CROWDSTEP_ROW16 for the launch)
BUILDS = {25: ("MAXT=64,OCC=1,ROWS_CT=25,LEAN=1", None), 30: ("MAXT=64,OCC=1,ROWS_CT=30,LEAN=1", None), 50: ("MAXT=64,OCC=3,ROWS_CT=50,LEAN=1", None),
          10: ("MAXT=64,OCC=4,ROWS_CT=10,LEAN=1", "0"), 26: ("MAXT=64,OCC=1,ROWS_CT=26,LEAN=3", None)}


class _row16:
    """The 10-row worlds on the LDS kernel instead of the DPP-row one for the launches inside; the variable is left as it was found."""

    def __init__(self, rows):
        self.value = BUILDS[rows][1] if rows in BUILDS else None

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


def _walking(W, n, model, seed0):
    """Hybrid worlds two Gym steps in (distinct velocities, headings that turn; circle worlds hold two-goal lists, traffic worlds one-goal
    lists and the respawn rule): float32 (states, goals, P, respawn bounds, respawn worlds); made once per shape and never written to."""
    from social_navigation_pyenvs_amd import scenarios as sc
    from social_navigation_pyenvs_amd.batched import CrowdWorlds

    key = (W, n, model, seed0)
    if key not in _WALKING:
        S, goals, P, rb = sc.hybrid_worlds(W, n, model, seed0=seed0)
        rw = (np.arange(W) % 2 == 1).astype(np.int32)
        with _row16(n):
            cw = CrowdWorlds(f32(S), f32(goals), f32(P), None, None, type=model, all_params_equal=True, respawn_bounds=rb, respawn_worlds=rw)
            for _ in range(2):
                cw.step(DT, 20)
            _WALKING[key] = (cw.get_states(), cw.get_goals(), f32(P), rb, rw)
    S, goals, P, rb, rw = _WALKING[key]
    return S.copy(), goals.copy(), P.copy(), rb, rw.copy()


def _robots(W, seed):
    rng = np.random.default_rng(seed)
    R = np.zeros((W, 13), np.float32)
    R[:, 0:2] = rng.uniform(-3, 3, (W, 2)); R[:, 8] = 0.3; R[:, 9] = 80; R[:, 10:12] = -R[:, 0:2]; R[:, 12] = 1.0
    return R, rng.uniform(-0.8, 0.8, (W, 2)).astype(np.float32)


def _check(S, goals, P, rb, rw, model, what, *, layout="aos", robot_row=False, R=None, A=None, worlds=None, variant=None):
    """Launches of 1 and of 3 substeps from (S, goals), every substep against the oracle; then 3 = 1 + 1 + 1 bit for bit.  Returns the
    worlds after the launch of three (for comparisons between cases)."""
    from social_navigation_pyenvs_amd.batched import CrowdWorlds, SFMS

    rows = S.shape[1]

    def make():
        return CrowdWorlds(S, goals, P, None, None, type=model, all_params_equal=True, respawn_bounds=rb, respawn_worlds=rw, robot_row=robot_row,
                           robot=R, layout=layout)

    with _row16(rows):
        for nsub in (1, 3):
            cw = make()
            assert (variant or BUILDS[rows][0]) in cw.step_variant(), cw.step_variant()
            res = fused_substeps_vs_oracle(cw, SFMS.index(model), S, goals, P, None, None, DT, nsub, True, respawn=rw, respawn_bounds=rb, robot_row=robot_row,
                                           robot=R if robot_row else None, action=A, worlds=worlds, group=GROUP, what=f"{what}, {nsub} substeps")
            print(f"{what}, {nsub} substeps: worst {res['worst']:.3e} (float32 oracle {res['worst_f32_oracle']:.3e}), {res['within']} of {res['substeps']} "
                  f"world-substeps within 1e-5, {res['ill_conditioned']} ill conditioned")
            assert res["within"] >= res["substeps"] - res["ill_conditioned"], (what, nsub, res)
        whole, ones = make(), make()
        whole.step(DT, 3, A)
        for _ in range(3):
            ones.step(DT, 1, A)
        np.testing.assert_array_equal(whole.get_states(), ones.get_states())
        np.testing.assert_array_equal(whole.get_goals(), ones.get_goals())
        if R is not None:
            np.testing.assert_array_equal(whole.get_robot(), ones.get_robot())
    return whole


@gpu
@pytest.mark.parametrize("layout", ["soa", "aos"])
@pytest.mark.parametrize("W", [1, 2, 3, 5])
def test_25_rows_at_the_edges_of_a_wavefront_and_a_workgroup(W, layout):
    model = "hsfm_farina"
    S, goals, P, rb, rw = _walking(W, 25, model, seed0=3001)
    _check(S, goals, P, rb, rw, model, f"25 rows W={W} {layout}", layout=layout)


@gpu
@pytest.mark.parametrize("n", [10, 30, 50])
def test_the_other_row_counts(n):
    model = "hsfm_farina"
    S, goals, P, rb, rw = _walking(3, n, model, seed0=3011 + n)
    _check(S, goals, P, rb, rw, model, f"{n} rows W=3")


@gpu
@pytest.mark.parametrize("action", [True, False])
def test_visible_robot(action):
    """The robot as the 26th row (LEAN = 3: outside the trimmed family, the same load phase), moved by a constant action or standing"""
    model = "hsfm_farina"
    S, goals, P, rb, rw = _walking(3, 25, model, seed0=3023)
    R, A = _robots(3, 7)
    S = np.concatenate([S, R[:, None, :]], axis=1)
    whole = _check(S, goals, P, rb, rw, model, f"visible robot, action {action}", robot_row=True, R=R, A=A if action else None)
    if action:
        np.testing.assert_allclose(whole.get_robot()[:, 0:2], R[:, 0:2] + 3 * DT * A, atol=2e-6)
        np.testing.assert_array_equal(whole.get_robot()[:, 3:5], A)
    else:
        np.testing.assert_array_equal(whole.get_robot(), R)


@gpu
@pytest.mark.parametrize("W", [2, 3])
@pytest.mark.parametrize("action", [True, False])
def test_invisible_robot(action, W):
    """d_robot without a robot row: the lane of row 0 advances it from the five columns the load phase brings -- in a launch with an
    action; without one neither the action nor the columns are loaded and the rows stay as they are.  The crowd never sees the robot:
    its rows are the rows of the worlds without one, bit for bit."""
    model = "hsfm_farina"
    S, goals, P, rb, rw = _walking(W, 25, model, seed0=3037)
    R, A = _robots(W, 11)
    plain = _check(S, goals, P, rb, rw, model, f"no robot W={W}", layout="soa")
    whole = _check(S, goals, P, rb, rw, model, f"invisible robot W={W}, action {action}", layout="soa", R=R, A=A if action else None)
    np.testing.assert_array_equal(whole.get_states(), plain.get_states())
    np.testing.assert_array_equal(whole.get_goals(), plain.get_goals())
    got = whole.get_robot()
    if action:
        want = R.astype(np.float64)
        want[:, 0:2] += 3 * float(np.float32(DT)) * A.astype(np.float64)
        np.testing.assert_allclose(got[:, 0:2], want[:, 0:2], atol=2e-6)   # three float32 fused multiply-adds on |x| < 4: 3 x half an ulp of 4 = 7e-7
        np.testing.assert_array_equal(got[:, 3:5], A)
        np.testing.assert_array_equal(got[:, 5:], R[:, 5:])
        np.testing.assert_array_equal(got[:, 2], R[:, 2])
    else:
        np.testing.assert_array_equal(got, R)


@gpu
def test_goal_lists_of_length_one_and_two_and_a_one_slot_array():
    """Hybrid worlds hold both lengths in a two-slot array (circle worlds two goals, traffic worlds one and a NaN slot).  The same worlds
    with a ONE-slot array (G = 1: the load of the second slot reads the first again): every human owns one goal."""
    model = "hsfm_farina"
    S, goals, P, rb, rw = _walking(3, 25, model, seed0=3041)
    assert np.isnan(goals[1, :, 1]).all() and not np.isnan(goals[0]).any() and not np.isnan(goals[:, :, 0]).any()
    _check(S, goals, P, rb, rw, model, "goal lists of length 1 and 2")
    _check(S, np.ascontiguousarray(goals[:, :, 0:1]), P, rb, rw, model, "one-slot goal array")


@gpu
def test_shared_and_per_world_parameter_tables_with_equal_rows():
    model = "hsfm_farina"
    S, goals, P, rb, rw = _walking(3, 25, model, seed0=3049)
    assert P.ndim == 2
    shared = _check(S, goals, P, rb, rw, model, "one parameter table (CS_PARAMS_SHARED)")
    assert shared.params_shared
    per_world = _check(S, goals, np.ascontiguousarray(np.broadcast_to(P, (3,) + P.shape)), rb, rw, model, "a parameter table per world")
    assert not per_world.params_shared
    np.testing.assert_array_equal(shared.get_states(), per_world.get_states())
    np.testing.assert_array_equal(shared.get_goals(), per_world.get_goals())


@gpu
@pytest.mark.parametrize("model", ["sfm_guo", "hsfm_moussaid"])
def test_guo_sfm_and_moussaid_hsfm(model):
    S, goals, P, rb, rw = _walking(3, 25, model, seed0=3061)
    _check(S, goals, P, rb, rw, model, f"25 rows W=3 {model}")


@gpu
def test_the_last_wavefront_of_a_crowded_grid():
    """W = 4200: more than two wavefronts per SIMD, the OCC = 4 twin (cs_step_variant says so); the first and the last wavefront's worlds
    against the oracle, all of them 3 = 1 + 1 + 1."""
    model, W = "hsfm_farina", 4200
    S, goals, P, rb, rw = _walking(W, 25, model, seed0=3067)
    _check(S, goals, P, rb, rw, model, f"25 rows W={W}", layout="soa", worlds=[0, 1, W - 2, W - 1], variant="MAXT=64,OCC=4,ROWS_CT=25,LEAN=1")


# ---- no GPU: the launcher's choice for shapes whose byte offsets do not fit 32 bits --------------------------------------------------
ROWS_PER_4GIB = 2 ** 32 // 80   # the largest offset these builds form is a row's into the parameter array: 80 bytes per row


def _variant_of_shape(W, n, model=3):
    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    d = _lib.cs_worlds()
    d.W, d.n, d.G, d.O, d.Smax = W, n, 2, 0, 0
    d.type = model
    d.flags = _lib.CS_ALL_PARAMS_EQUAL | _lib.CS_PARAMS_SHARED
    d.layout = _lib.CS_LAYOUT_SOA
    for field in ("d_state", "d_goals", "d_params", "d_safety"):
        setattr(d, field, C.c_void_p(0x1000))   # (never dereferenced: the plan is a function of the shape)
    buf = C.create_string_buffer(256)
    assert lib.cs_step_variant(C.byref(d), 0, buf, 256) == _lib.CS_OK
    return buf.value.decode()


@pytest.mark.parametrize("n", [25, 30, 50])
def test_shapes_beyond_32_bit_offsets_run_the_generic_build(n):
    """W x rows x 80 <= 2^32 keeps the compile-time build; one world more and the launch runs the generic build (64-bit addresses)"""
    fits, beyond = ROWS_PER_4GIB // n, ROWS_PER_4GIB // n + 1
    assert fits * n * 80 <= 2 ** 32 < beyond * n * 80
    assert f"ROWS_CT={n},LEAN=1" in _variant_of_shape(fits, n), _variant_of_shape(fits, n)
    assert "ROWS_CT=0,LEAN=0" in _variant_of_shape(beyond, n), _variant_of_shape(beyond, n)
    assert "ROWS_CT=25,LEAN=1" in _variant_of_shape(4096, 25), _variant_of_shape(4096, 25)
