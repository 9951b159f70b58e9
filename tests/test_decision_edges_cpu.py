"""CPU side of tests/test_gpu_decision_edges.py: the inputs of tests/decision_edges.py have the properties the GPU tests rely on, shown
with torch on the CPU, numpy and the oracle alone -- and the mutants (softmax mask dropped, tie rule preferring the later index, group
boundary one row off) give another answer on these very inputs, so the GPU tests can fail."""
import numpy as np
import pytest
import torch

import decision_edges as de
import parity_util
from test_value_policy_cpu import model_values

REL_BAR = de.REL_BAR


@pytest.mark.parametrize("n", de.N_SWEEP)
def test_identity_network_is_px_and_every_group_minimum_is_unique(n):
    """torch's float32 forward of the "2, 1" CADRL returns px as raw words; every group's minimum is unique, positive in some groups and
    negative in others; a group boundary one row off changes the expected values."""
    pol = de.identity_cadrl()
    for W, A in de.WA_SWEEP:
        rot, rew, rob = de.identity_case(n, W, A)
        with torch.no_grad():
            out = pol.model(torch.as_tensor(rot))[..., 0].numpy()
        assert de.same_words(out, rot[..., de.PX])
        px = np.sort(rot[..., de.PX].reshape(W * A, n), axis=1)
        assert n == 1 or np.all(px[:, 0] < px[:, 1])
        if W * A >= 31:
            assert (px[:, 0] < 0).any() and (px[:, 0] > 0).any()
            assert (px[1::2, 0] > 0).all()                              # the lifted groups: a zero row from the padding would be their minimum
        want = de.identity_expected(rot, rew)
        assert np.isfinite(want).all()
        if W * A > 1:
            assert not de.same_words(want, de.identity_expected(rot, rew, shift=1))


@pytest.mark.parametrize("name", ["cadrl", "sarl"])
def test_float64_reference_is_finite_and_torch_float32_error_over_the_sweep(name):
    """The float64 reference of the whole sweep is finite in every group (SARL's unmasked softmax overflows nowhere with the calm attention
    layer); the worst error of the torch float32 CPU forward against it is what F32_SLACK times bounds the kernel with on the GPU.

    Measured: CADRL 3.5e-6, SARL 6.4e-7 (relative to each world's largest |value|, floor 1)."""
    worst = 0.0
    for n, W, A in de.SWEEP_F64:
        c = de.sweep_case(name, n, W, A)
        assert np.isfinite(c["ref"]).all(), (name, n, W, A)
        assert c["torch32_err"] < REL_BAR, (name, n, W, A, c["torch32_err"])
        worst = max(worst, c["torch32_err"])
    print(f"{name}: torch float32 CPU forward against the float64 reference over the sweep: worst relative error {worst:.3e}")
    parity_util.record(f"decision edges: torch float32 CPU forward against float64, {name} (relative action value)", worst, bar=REL_BAR)
    assert 0.0 < worst < REL_BAR


@pytest.mark.parametrize("with_global", [True, False])
@pytest.mark.parametrize("n", [5, 40])
def test_masked_scores_are_exactly_zero_and_the_mask_matters(n, with_global):
    """The expected mask is mixed, groups without and with only masked humans exist, the torch module scores the masked humans exactly 0
    and agrees with the float64 restatement (NaN where every human is masked); a restatement WITHOUT the mask is farther than
    100 * REL_BAR from it on the groups with some masked humans."""
    pol = de.masked_sarl(with_global)
    rot, rew, rob, masked = de.masked_case(n)
    per_group = masked.sum(axis=-1)
    assert (per_group == 0).any() and (per_group == n).any() and ((per_group > 0) & (per_group < n)).any()
    assert np.abs(rot[..., de.PX]).min() >= np.float32(0.1)
    ref, scores = de.masked_reference(pol, rot, rew, rob)
    np.testing.assert_array_equal(scores == 0, masked)
    np.testing.assert_array_equal(scores[~masked], rot[..., de.PX][~masked].astype(np.float64))
    np.testing.assert_array_equal(np.isnan(ref), per_group == n)
    assert np.isfinite(ref[per_group < n]).all()
    net = model_values(pol, rot).astype(np.float64)                                        # the shipped torch module in float32
    got = rew.astype(np.float64) + de.discount(rob)[:, None] * net
    np.testing.assert_array_equal(np.isnan(got), np.isnan(ref))
    assert de.rel_error(got, ref) < REL_BAR
    mutant, _ = de.masked_reference(pol, rot, rew, rob, mask=False)
    some = (per_group > 0) & (per_group < n)
    scale = max(1.0, float(np.nanmax(np.abs(ref))))
    assert np.max(np.abs(mutant[some] - ref[some])) / scale > 100 * REL_BAR
    assert np.isfinite(mutant).all()                                                       # (without the mask no group divides 0 by 0)


@pytest.mark.parametrize("n", [5, 40])
def test_torch_min_keeps_a_nan_and_the_layers_keep_an_infinity(n):
    """torch's forward of the identity module on NaN / +-inf rows and torch.min over the humans: NaN wherever a human's px is NaN (before or
    after the finite minimum, or a -inf), the finite minimum beside a +inf human, +inf where every human is +inf, -inf beside a -inf."""
    pol = de.identity_cadrl()
    rot, rew, rob = de.nonfinite_case(n)
    with torch.no_grad():
        out = pol.model(torch.as_tensor(rot))[..., 0].min(dim=-1).values.numpy()
    want = rot[..., de.PX].min(axis=-1)
    assert de.same_words(out, want)
    kinds = dict(zip(de.NONFINITE_GROUPS, out[0]))
    assert all(np.isnan(kinds[k]) for k in ("nan early", "nan late", "nan then -inf", "-inf then nan"))
    assert kinds["+inf early"] == kinds["+inf late"] == np.float32(-5.0)
    assert kinds["all +inf"] == np.inf and kinds["-inf early"] == kinds["-inf late"] == -np.inf
    if n == 40:                                                           # the two positions lie in different chunks of 32 humans
        assert 1 < 32 <= n - 2
    exp = de.identity_expected(rot, rew)
    np.testing.assert_array_equal(np.isnan(exp[0]), np.isnan(out[0]))
    np.testing.assert_array_equal(np.isinf(exp[0]), np.isinf(out[0]))


@pytest.mark.parametrize("A", de.A_PICK)
def test_pick_patterns_tell_the_tie_rules_apart(A):
    """The zero network's torch forward leaves values == rewards; the lane-by-lane model of k_value_pick equals np.argmax on every pattern;
    the mutant that prefers the later index does not (from A = 2 on)."""
    names, values = de.pick_patterns(A)
    assert len(set(names)) == 14 and values.shape == (len(names), A)
    pol = de.zero_cadrl()
    with torch.no_grad():
        out = pol.model(torch.randn(3, 5, 13))
    assert not out.numpy().any()                                                           # rewards + disc * 0 keeps a reward's bits (but a zero's sign)
    want = de.expected_pick(values)
    rows = list(range(13)) + list(range(13, len(names), 8))
    assert [de.pick_model(values[r]) for r in rows] == [int(want[r]) for r in rows]
    if A > 1:
        later = [de.pick_model(values[r], prefer_later=True) for r in rows]
        differ = {names[r] for r, p in zip(rows, later) if p != want[r]}
        assert {"all equal", "two NaNs", "all NaN", "all -inf", "two +inf", "four values", "-0.0 before +0.0"} <= differ, differ
        if A > 2:
            assert {"tie inside one lane's trips", "tie, the lower index in the higher lane"} <= differ, differ
    ov = de.OVERRIDES(A)
    forced = de.expected_pick(values[:7], ov)
    assert forced[1] == 0 and forced[2] == A - 1 and all(forced[k] == want[k] for k in (0, 3, 4, 5, 6))


def test_goal_radius_edge_in_float32():
    """|p - g| = 0.5 exactly: not inside a radius of 0.5 (strict <), inside the next float32"""
    d = np.sqrt(np.float32(0.0) * np.float32(0.0) + np.float32(-0.5) * np.float32(-0.5), dtype=np.float32)
    assert d == np.float32(0.5) and not d < np.float32(0.5) and d < np.nextafter(np.float32(0.5), np.float32(1.0))


def test_lookahead_cases_cover_the_branches_and_stay_clear_of_their_edges():
    """With the oracle alone: every case leaves out at most 1 % of its (world, action) entries (float64 margin to a branch edge below 1e-5),
    every goal is at least 1 m from every next robot position, the float32 oracle agrees with the float64 one on the kept entries, and the
    sweep holds every reward branch -- world 0 collides, world 2 reaches its goal with some actions and not with others."""
    seen = set()
    left_out = total = 0
    for A, n, headed, stride in de.LOOK_CASES:
        c = de.lookahead_reference(A, n, headed, stride)
        keep, rew = c["keep"], c["rew64"]
        assert (~keep).sum() <= 0.01 * keep.size, (A, n, headed, int((~keep).sum()))
        left_out, total = left_out + int((~keep).sum()), total + keep.size
        assert c["dg"].min() >= 1.0
        assert np.max(np.abs(c["rew32"][keep] - rew[keep])) < 1e-6
        assert np.isnan(c["rob"][:, 2:4]).all() and np.isnan(c["rob"][:, 8:]).all() and np.isfinite(c["rot64"]).all()
        seen |= {"collision"} if (rew[0] == -0.25).any() else set()
        seen |= {"discomfort"} if ((rew < 0) & (rew > -0.25)).any() else set()
        seen |= {"nothing"} if (rew[1] == 0).any() else set()
        if A >= 81:
            assert (rew[2] == 1).any() and (rew[2] != 1).any(), (A, n)
            seen.add("goal")
    print(f"look-ahead sweep: {left_out} of {total} (world, action) entries within 1e-5 of a branch edge")
    assert seen == {"collision", "discomfort", "nothing", "goal"}
    assert {h for _, _, h, _ in de.LOOK_CASES} == {True, False} and {s for *_, s in de.LOOK_CASES} == {8, 9, 13}
