"""GPU suite of the fused decision kernels at their tile and selection edges: cs_lookahead (csrc/lookahead.hip), k_value_net and
k_value_pick (csrc/value_net.hip) called directly on the synthetic arrays of tests/decision_edges.py.  The properties of those inputs --
finite references, mixed masks, margins to the reward branches, torch's own +-inf / NaN results -- and the mutants that each test would
catch are shown without a device in tests/test_decision_edges_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import decision_edges as de
import parity_util

pytestmark = pytest.mark.gpu

REL_BAR = de.REL_BAR


def _ready(pol):
    import torch

    pol.set_phase("test")
    pol.set_device(torch.device("cuda"))
    return pol


def _decide(net, rot, rew, acts, rob, gamma=de.GAMMA, dt=de.DT, override=None, want_choice=True):
    """cs_value_net_decide on host arrays: (values [W, A], choice [W] or None, action rows [W, 2]).  The outputs start as NaN / -7."""
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    W, A, n, _ = rot.shape
    dev = lambda a, dtype=torch.float32: torch.as_tensor(np.array(a), dtype=dtype, device="cuda")
    d_rot, d_rew, d_acts, d_rob = dev(rot), dev(rew), dev(acts), dev(rob)
    vals = torch.full((W, A), float("nan"), device="cuda")
    pick = torch.full((W,), -7, dtype=torch.int32, device="cuda")
    act = torch.full((W, 2), float("nan"), device="cuda")
    ovr = None if override is None else dev(override, torch.int32)
    value_net.decide(net, W, A, n, d_rot.data_ptr(), d_rew.data_ptr(), d_acts.data_ptr(), d_rob.data_ptr(), rob.shape[1], gamma, dt,
                     None if ovr is None else ovr.data_ptr(), vals.data_ptr(), pick.data_ptr() if want_choice else None, act.data_ptr(),
                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return vals.cpu().numpy(), pick.cpu().numpy() if want_choice else None, act.cpu().numpy()


def _acts(A):
    return de.pick_actions(A)


@pytest.mark.parametrize("n", de.N_SWEEP)
def test_identity_network_gives_reward_plus_minimum_px_to_the_bit(n):
    """k_value_net's group bookkeeping: with the "2, 1" CADRL whose output is px exactly and gamma = 1 (powf returns 1), every value is
    float32(rew + min_j px_j) as a raw word, for whole groups per tile, one group and zero rows, a full tile, and 2 - 4 chunks, with NG one
    short of a job, exact and one over, and A != 81 (the g / A index of v_pref).  Every minimum is unique; it is positive in every other
    group, where a zero row leaking in from the padding would win, and a neighbouring group's or a stale tile's row changes the answer
    either way (CPU file: the boundary one row off gives other values on every case)."""
    pol = _ready(de.identity_cadrl())
    net = pol.device_net()
    for W, A in de.WA_SWEEP:
        rot, rew, rob = de.identity_case(n, W, A)
        vals, pick, act = _decide(net, rot, rew, _acts(A), rob, gamma=1.0)
        want = de.identity_expected(rot, rew)
        assert de.same_words(vals, want), (n, W, A, np.argwhere(vals.view(np.uint32) != want.view(np.uint32))[:4])
        np.testing.assert_array_equal(pick, de.expected_pick(vals))
        np.testing.assert_array_equal(act, _acts(A)[pick])


@pytest.mark.parametrize("name", ["cadrl", "sarl"])
@pytest.mark.parametrize("n", [3, 16, 31, 40])
def test_a_group_gives_the_same_bits_wherever_its_rows_fall(name, n):
    """The header's claim: the W * A = 33 groups of the seeded default CADRL / calm SARL and the same groups (rows and rewards) shuffled
    along the flattened group axis give the same values, shuffled, bit for bit.  Every world has one v_pref, so the shuffle is legal."""
    pol = _ready(de.sweep_policy(name))
    net = pol.device_net()
    W, A = 3, 11
    c = de.sweep_case(name, n, W, A)
    rob = c["rob"].copy()
    rob[:, 7] = 1.25
    perm = np.random.default_rng(n).permutation(W * A)
    assert (perm != np.arange(W * A)).sum() > 25
    v1, _, _ = _decide(net, c["rot"], c["rew"], _acts(A), rob)
    rot2 = c["rot"].reshape(W * A, n, 13)[perm].reshape(W, A, n, 13)
    rew2 = c["rew"].reshape(W * A)[perm].reshape(W, A)
    v2, _, _ = _decide(net, rot2, rew2, _acts(A), rob)
    assert np.isfinite(v1).all()
    assert de.same_words(v2.reshape(-1), v1.reshape(-1)[perm])


@pytest.mark.parametrize("name", ["cadrl", "sarl"])
def test_sweep_against_the_float64_reference(name):
    """The seeded default CADRL / calm SARL on torch.randn rows over the tile edges (decision_edges.SWEEP_F64) against
    test_policy_seam.VALUE in float64 on the same float32 inputs.  Hard bar: REL_BAR = 1e-4 on test_gpu_value_policy._compare's scale in
    every case.  Tighter bar: the kernel's worst error over the sweep is at most parity_util.F32_SLACK (3: one float32 realisation against
    another) times the worst error of the torch float32 CPU forward against the same reference over the same sweep.

    The torch figure is CADRL 3.5e-6, SARL 6.4e-7; the kernel's had not been measured when this was written (HISTORY.md): both are printed
    and recorded in the parity report before the assertions."""
    pol = _ready(de.sweep_policy(name))
    net = pol.device_net()
    worst = worst_torch = 0.0
    for n, W, A in de.SWEEP_F64:
        c = de.sweep_case(name, n, W, A)
        vals, pick, _ = _decide(net, c["rot"], c["rew"], _acts(A), c["rob"])
        assert np.isfinite(vals).all(), (name, n, W, A)
        err = de.rel_error(vals, c["ref"])
        print(f"{name} n={n} W={W} A={A}: kernel {err:.3e}, torch float32 on the CPU {c['torch32_err']:.3e}")
        assert err < REL_BAR, (name, n, W, A, err)
        np.testing.assert_array_equal(pick, de.expected_pick(vals))
        worst, worst_torch = max(worst, err), max(worst_torch, c["torch32_err"])
    print(f"{name}: worst relative action-value error against float64 over the sweep: kernel {worst:.3e}, torch float32 on the CPU {worst_torch:.3e}")
    parity_util.record(f"decision edges: kernel against float64, {name} (relative action value)", worst, bar=REL_BAR)
    parity_util.record(f"decision edges: torch float32 CPU forward against float64, {name} (relative action value)", worst_torch, bar=REL_BAR)
    assert worst <= parity_util.F32_SLACK * worst_torch, (name, worst, worst_torch)


@pytest.mark.parametrize("with_global", [True, False])
@pytest.mark.parametrize("n", [5, 40])
def test_a_score_of_exactly_zero_is_masked(n, with_global):
    """sarl.py:48-52: a human whose attention score is exactly 0 gets weight exactly 0.  The attention reads relu(px) alone, |px| >= 0.1, so
    the mask is the set px < 0 in any precision: groups with no, some and only masked humans, whole groups per tile (n = 5) and two chunks
    (n = 40: phases 1 and 2).  Reference: the float64 restatement with np.exp(s) * (s != 0); REL_BAR on the finite groups, NaN (0 / 0)
    exactly where every human is masked.  A kernel without the mask is more than 100 * REL_BAR off on these inputs (CPU file)."""
    pol = _ready(de.masked_sarl(with_global))
    rot, rew, rob, masked = de.masked_case(n)
    ref, _ = de.masked_reference(pol, rot, rew, rob)
    vals, pick, _ = _decide(pol.device_net(), rot, rew, _acts(rot.shape[1]), rob)
    np.testing.assert_array_equal(~np.isfinite(vals), ~np.isfinite(ref))
    np.testing.assert_array_equal(np.isnan(vals), masked.all(axis=-1))
    err = de.rel_error(vals, ref)
    print(f"masked softmax n={n} global={with_global}: worst relative error on the finite groups {err:.3e}")
    parity_util.record("decision edges: masked softmax against float64 (relative action value, finite groups)", err, bar=REL_BAR)
    assert err < REL_BAR
    np.testing.assert_array_equal(pick, de.expected_pick(vals))             # a NaN value counts as the maximum


@pytest.mark.parametrize("n", [5, 40])
def test_nan_and_infinities_through_the_layers_and_the_minimum(n):
    """What torch gives for the identity module (CPU file): a NaN px makes the group's value NaN whether it comes before or after the finite
    minimum -- in the other chunk at n = 40 -- or a -inf; a +inf human leaves the finite minimum, +inf everywhere gives +inf, a -inf human
    -inf.  The +inf rows are the ones a layer's padded output columns used to turn into NaN (0 * inf in the columns beyond the layer's
    width, handed on by the next layer's zero weights): layer_fwd stores those columns as 0."""
    pol = _ready(de.identity_cadrl())
    rot, rew, rob = de.nonfinite_case(n)
    want = de.identity_expected(rot, rew)
    vals, pick, _ = _decide(pol.device_net(), rot, rew, _acts(rot.shape[1]), rob, gamma=1.0)
    assert de.same_words(vals, want), dict(zip(de.NONFINITE_GROUPS, zip(vals[0], want[0])))
    assert pick[0] == int(np.argmax(want[0])) == 0                         # the first NaN


PICK_CASES = [(A, (8, 9, 13)[k % 3]) for k, A in enumerate(de.A_PICK)] + [(81, 8), (81, 9)]


@pytest.mark.parametrize("A,stride", PICK_CASES)
def test_value_pick_follows_argmax_order_on_ties_nans_and_infinities(A, stride):
    """k_value_pick against np.argmax of the downloaded values: the zero CADRL hands the rewards through (checked as raw words, the sign of
    zero skipped), one world per pattern of decision_edges.pick_patterns plus 256 worlds of four values; 1, 2 and 3 - 4 trips of the
    lane-strided scan.  The robot rows carry NaN in every column the kernels have no business reading (they may read 0, 1, 4, 5, 6, 7), at
    strides 8, 9 and 13.  Then the override column (only -1 < o < A changes the pick), d_choice = NULL, and the strict < of the goal test:
    |p - g| equal to the radius in float32 moves, the next float32 radius stands still.  A tie rule preferring the later index fails the
    tie patterns (CPU file)."""
    pol = _ready(de.zero_cadrl())
    net = pol.device_net()
    names, values = de.pick_patterns(A)
    Wp = len(names)
    rng = np.random.default_rng(A)
    rot = rng.normal(size=(Wp, A, 2, 13)).astype(np.float32)
    rob = de.robot_rows(Wp, stride, rng)
    acts = _acts(A)
    vals, pick, act = _decide(net, rot, values, acts, rob)
    assert de.same_words(np.where(vals == 0, np.float32(0), vals), np.where(values == 0, np.float32(0), values))
    want = de.expected_pick(vals)
    bad = np.nonzero(pick != want)[0]
    assert bad.size == 0, [(names[w], int(pick[w]), int(want[w])) for w in bad[:8]]
    assert de.same_words(act, acts[want])
    # d_choice = NULL still writes the action rows
    _, none, act2 = _decide(net, rot, values, acts, rob, want_choice=False)
    assert none is None and de.same_words(act2, act)
    # the override column on the first seven patterns
    ov = de.OVERRIDES(A)
    _, pick3, act3 = _decide(net, rot[:7], values[:7], acts, rob[:7], override=ov)
    want3 = de.expected_pick(vals[:7], ov)
    np.testing.assert_array_equal(pick3, want3)
    assert pick3[1] == 0 and pick3[2] == A - 1 and de.same_words(act3, acts[want3])
    # the goal test
    on_edge = de.robot_rows(2, stride, rng, p=0.0, g=np.array([0.5, 0.0]), radius=np.array([0.5, np.nextafter(np.float32(0.5), np.float32(1.0))]))
    _, pick4, act4 = _decide(net, rot[1:3], values[1:3], acts, on_edge)
    np.testing.assert_array_equal(pick4, want[1:3])                          # the choice is reported either way
    assert de.same_words(act4[0], acts[want[1]]) and not act4[1].any() and not np.signbit(act4[1]).any()


def _lookahead(c):
    """cs_lookahead on the host arrays of a decision_edges.lookahead_case: (rotated [3, A, n, 13|15], rewards [3, A]), NaN-filled before"""
    import torch

    from social_navigation_pyenvs_amd import _lib

    W, A, n = 3, c["A"], c["n"]
    dev = lambda a: torch.as_tensor(np.array(a), dtype=torch.float32, device="cuda")
    acts, nxt, cur, rob = dev(c["actions"]), dev(c["nxt"]), dev(c["cur"]), dev(c["rob"])
    rot = torch.full((W, A, n, 15 if c["headed"] else 13), float("nan"), device="cuda")
    rew = torch.full((W, A), float("nan"), device="cuda")
    P = C.c_void_p
    _lib.check(_lib.load().cs_lookahead(C.c_int(W), C.c_int(n), C.c_int(A), C.c_int(int(c["headed"])), P(acts.data_ptr()), P(nxt.data_ptr()),
                                        P(cur.data_ptr()), P(rob.data_ptr()), C.c_int(c["stride"]), C.c_float(c["dt"]), P(rot.data_ptr()),
                                        P(rew.data_ptr()), P(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return rot.cpu().numpy(), rew.cpu().numpy()


@pytest.mark.parametrize("A,n,headed,stride", de.LOOK_CASES)
def test_lookahead_beyond_g8(A, n, headed, stride):
    """cs_lookahead with 1 - 3 trips of phase 1's a += 256, up to 70 humans, headed rows, three different robots in one launch and robot
    strides 8, 9, 13 (NaN in the unread columns), against tests/test_lookahead.py's own bars: the rotated rows within 5e-6 of the float64
    oracle on the float32-rounded inputs, the rewards within 1e-6 of the oracle's float32 instantiation -- on every (world, action) whose
    float64 margin to a branch edge (swept distance against 0, dmin against 0.2, dg against the radius) is at least 1e-5; the CPU file caps
    what that leaves out at 1 % per case."""
    c = de.lookahead_reference(A, n, headed, stride)
    rot, rew = _lookahead(c)
    assert rot.shape == c["rot64"].shape and np.isfinite(rot).all() and np.isfinite(rew).all()
    e_rot = float(np.max(np.abs(rot.astype(np.float64) - c["rot64"])))
    keep = c["keep"]
    e_rew = float(np.max(np.abs(rew.astype(np.float64)[keep] - c["rew32"].astype(np.float64)[keep])))
    print(f"lookahead A={A} n={n} headed={headed} stride={stride}: rotated {e_rot:.3e}, rewards {e_rew:.3e} on {int(keep.sum())} of {keep.size} entries")
    parity_util.record("decision edges: cs_lookahead rotated rows against the float64 oracle", e_rot, bar=5e-6)
    assert e_rot < 5e-6
    assert e_rew < 1e-6
