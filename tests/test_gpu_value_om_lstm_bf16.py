"""GPU suite of the opt-in bf16 arithmetic of OM-LSTM-RL's decision (cs_value_net_decide_lstm_om_bf16, csrc/value_net_lstm_om_bf16.hip;
DESIGN.md 4.5): the kernel against tests/om_lstm_bf16_emulation.py's float64 emulation of the contract on the cases of
tests/test_value_om_lstm_bf16_cpu.py (which shows what the arithmetic alone does on them), bit equality between launches, the order and the
pairing against the float32 kernel's rule, isolation, the training step, the batched Gym and golden G22 under bf16.

The two tiers of tests/test_gpu_value_lstm_bf16.py, with its bars:
  tight   at most 1/4 of a case's sequences farther than 4 x E_ref from the float64 emulation;
  loose   EVERY sequence within parity_util.F32_SLACK x the case's worst |float64 emulation - full-precision float64|.
Every comparison between two launches of this library is bitwise."""
import functools

import numpy as np
import pytest

import bf16_emulation as em
import decision_edges as de
import lstm_cases as lc
import om_lstm_bf16_emulation as oem
import om_lstm_cases as olc
import parity_util
import test_gpu_value_om_lstm as f32om
import test_value_om_lstm_bf16_cpu as cpu
from test_gpu_value_om_lstm import random_case, seeded_policy
from value_calls import _stream, _up, same_bits

pytestmark = pytest.mark.gpu

F32 = np.float32
DT, GAMMA = cpu.DT, cpu.GAMMA
WIDE_MLP1 = f32om.WIDE_MLP1


def bf16_net(pol, pairing="reference"):
    from social_navigation_pyenvs_amd.crowd_nav.policy.value_net import DeviceNet

    net = DeviceNet(pol.model, pol.joint_state_dim, pol.map_columns(), pol.om_grid(), pairing)
    net.refresh_mapped("bf16")
    return net


def decide_bf16(net, rot, maps, rew, acts, rob, in_order=1, gamma=GAMMA, dt=DT, override=None):
    """value_net.decide_lstm_om_bf16 on host arrays or device tensors, as test_gpu_value_om_lstm.om_call: (values [W, A], choice [W], action
    [W, 2]) numpy; the outputs are NaN- / -5-filled before: every element must be written."""
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    W, A, n, _ = rot.shape
    vals = torch.full((W, A), np.nan, device="cuda")
    pick = torch.full((W,), -5, dtype=torch.int32, device="cuda")
    act = torch.full((W, 2), np.nan, device="cuda")
    d_rot, d_maps, d_rew, d_acts, d_rob = (_up(x, torch.float32).contiguous() for x in (rot, maps, rew, acts, rob))
    assert tuple(d_maps.shape) == (W, n, net.om_cols)
    d_ovr = None if override is None else _up(override, torch.int32)
    value_net.decide_lstm_om_bf16(net, W, A, n, in_order, d_rot.data_ptr(), d_maps.data_ptr(), d_rew.data_ptr(), d_acts.data_ptr(), d_rob.data_ptr(),
                                  d_rob.shape[1], gamma, dt, None if d_ovr is None else d_ovr.data_ptr(), vals.data_ptr(), pick.data_ptr(),
                                  act.data_ptr(), _stream())
    torch.cuda.synchronize()
    return vals.cpu().numpy(), pick.cpu().numpy(), act.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _kernel(idx):
    case = cpu.CASES[idx]
    d = cpu.case_data(case)
    return decide_bf16(bf16_net(d["pol"], case[7]), *(np.array(d[k]) for k in ("rot", "maps", "rew", "acts", "rob")), in_order=case[8])     # (copies: read-only inputs)


def kernel_on(case):
    """The kernel's (values, choice, action) on a case of the CPU file, one launch shared by the two tiers"""
    return _kernel(cpu.CASES.index(case))


# ---------------------------------------------------------------------------------------------------------------- the two tiers
@pytest.mark.parametrize("case", cpu.TIGHT, ids=cpu.case_id)
def test_short_sequences_agree_with_the_emulation(case):
    """Measured on the MI355X: HISTORY.md lists the share and the median of every case."""
    d = cpu.case_data(case)
    vals, pick, act = kernel_on(case)
    share, median = cpu.share_beyond(vals, d)
    print(f"{cpu.case_id(case)}: E_ref {d['e_ref']:.3e}; kernel: share beyond {cpu.MARGIN:g} x E_ref {share:.3f}, median {median:.3e}")
    parity_util.record("om_lstm_bf16_tight_share", share, bar=cpu.TIGHT_CAP)
    parity_util.record("om_lstm_bf16_tight_median", median, bar=cpu.MARGIN * d["e_ref"])
    assert np.all(np.isfinite(vals))
    assert np.array_equal(pick, np.argmax(vals, axis=1)) and same_bits(act, d["acts"][pick])
    assert share <= cpu.TIGHT_CAP, (share, d["e_ref"])


@pytest.mark.parametrize("case", cpu.CASES, ids=cpu.case_id)
def test_every_sequence_stays_within_the_arithmetics_own_error(case):
    d = cpu.case_data(case)
    vals, pick, act = kernel_on(case)
    worst = float(np.max(np.abs(vals.astype(np.float64) - d["emu64"])))
    print(f"{cpu.case_id(case)}: the arithmetic's own error {d['own_error']:.3e}; kernel against the float64 emulation {worst:.3e} "
          f"(ratio {worst / d['own_error']:.3f})")
    parity_util.record("om_lstm_bf16_loose_ratio", worst / d["own_error"], bar=parity_util.F32_SLACK)
    assert np.all(np.isfinite(vals)) and np.array_equal(pick, np.argmax(vals, axis=1)) and same_bits(act, d["acts"][pick])
    assert worst <= parity_util.F32_SLACK * d["own_error"], (worst, d["own_error"])


# ---------------------------------------------------------------------------------------------------------------- bit equality
@pytest.fixture(scope="module")
def default_case():
    pol = seeded_policy(1, 13, 77)
    rot, maps, rew, acts, rob = random_case(3, 3, 81, 5, 13, 48)
    return pol, rot, maps, rew, acts, rob


@pytest.mark.parametrize("pairing", olc.PAIRINGS)
def test_a_world_alone_gives_the_bits_of_the_batch(default_case, pairing):
    pol, rot, maps, rew, acts, rob = default_case
    net = bf16_net(pol, pairing)
    batch = decide_bf16(net, rot, maps, rew, acts, rob)
    assert np.all(np.isfinite(batch[0]))
    for w in (1, 2):                    # worlds that start inside a tile: their action 0 lies in the tile before most of their actions'
        alone = decide_bf16(net, rot[w:w + 1], maps[w:w + 1], rew[w:w + 1], acts, rob[w:w + 1])
        assert all(same_bits(a, b[w:w + 1]) for a, b in zip(alone, batch))


@pytest.mark.parametrize("network,H,overrides", [(1, 50, {}), (2, 64, WIDE_MLP1)])
def test_a_pair_alone_gives_the_bits_of_the_batch(network, H, overrides):
    """A (world, action) alone, W = A = 1, and the same rows and maps at two positions of a 3 x 27 batch, one of them in the third tile."""
    pol = seeded_policy(network, 13, 78, lstm_rl__global_state_dim=H, **overrides)
    net = bf16_net(pol, "own")
    rot, maps, rew, acts, rob = random_case(4, 3, 27, 5, 13, 48)
    rot[2, 20], rew[2, 20], rob[2], maps[2] = rot[0, 4], rew[0, 4], rob[0], maps[0]          # the pair again, 70 sequences on: the third tile
    batch = decide_bf16(net, rot, maps, rew, acts, rob)[0]
    alone = decide_bf16(net, rot[:1, 4:5], maps[:1], rew[:1, 4:5], acts[4:5], rob[:1])[0]
    assert np.all(np.isfinite(batch)) and same_bits(alone[0, :1], batch[0, 4:5]) and same_bits(alone[0, :1], batch[2, 20:21])


@pytest.mark.parametrize("network,pairing", [(1, "reference"), (2, "own")])
def test_the_tile_edges_give_the_bits_of_the_batch(network, pairing):
    """W * A of 1, 31, 32 and 33 cut from one batch of 33 sequences (action 0 stays in: the pairing may need it): a tile not full, full, and
    one sequence into the next."""
    net = bf16_net(seeded_policy(network, 13, 79), pairing)
    rot, maps, rew, acts, rob = random_case(4, 1, 33, 5, 13, 48)
    whole = decide_bf16(net, rot, maps, rew, acts, rob)[0]
    assert np.all(np.isfinite(whole))
    for count in (1, 31, 32, 33):
        part = decide_bf16(net, rot[:, :count], maps, rew[:, :count], acts[:count], rob)[0]
        assert same_bits(part, whole[:, :count]), count


def test_the_first_action_of_an_earlier_tile_orders_the_maps():
    """First-action pairing with pair 0 in an earlier tile than the sequence: W = 1, A = 40, action 35 lies in the second tile; it gives the
    bits it gives right behind action 0 in a launch of the two (the same pair-0 rows, another tile, another lane), and its order differs
    from action 0's, so the pairing shows."""
    pol = seeded_policy(1, 13, 80)
    rot, maps, rew, acts, rob = random_case(8, 1, 40, 5, 13, 48)
    rot[0, 0, :, 11] = np.array([0.5, 0.6, 0.7, 0.8, 0.9], F32)
    rot[0, 35, :, 11] = np.array([0.9, 0.8, 0.7, 0.6, 0.5], F32)
    ref, own = bf16_net(pol, "reference"), bf16_net(pol, "own")
    whole = decide_bf16(ref, rot, maps, rew, acts, rob)[0]
    two = decide_bf16(ref, rot[:, [0, 35]], maps, rew[:, [0, 35]], acts[[0, 35]], rob)[0]
    assert np.all(np.isfinite(whole)) and same_bits(two[0], whole[0, [0, 35]])
    own_whole = decide_bf16(own, rot, maps, rew, acts, rob)[0]
    assert same_bits(own_whole[0, :1], whole[0, :1]) and not same_bits(own_whole[0, 35:36], whole[0, 35:36])


def test_rows_sorted_on_the_host_give_the_bits_of_the_kernels_sort(default_case):
    pol, rot, maps, rew, acts, rob = default_case
    perm = lc.decision_order(rot[..., 11])
    assert np.any(perm != perm[:, :1])
    sorted_rot = lc.sort_rows(rot)
    ref, own = bf16_net(pol, "reference"), bf16_net(pol, "own")
    maps0 = np.take_along_axis(maps, perm[:, 0][..., None], axis=1)       # the world's maps permuted by action 0's order
    got = decide_bf16(ref, rot, maps, rew, acts, rob, 1)
    lying = decide_bf16(ref, sorted_rot, maps0, rew, acts, rob, 0)
    assert all(same_bits(a, b) for a, b in zip(got, lying))
    assert all(same_bits(a, b) for a, b in zip(lying, decide_bf16(own, sorted_rot, maps0, rew, acts, rob, 0)))      # as they lie: one order
    for a in (0, 40):                   # the own pairing: one action a world, so that a world's maps can follow that action's order
        one = (rot[:, a:a + 1], maps, rew[:, a:a + 1], acts[a:a + 1], rob)
        maps_a = np.take_along_axis(maps, perm[:, a][..., None], axis=1)
        assert same_bits(decide_bf16(own, *one, 1)[0], decide_bf16(own, sorted_rot[:, a:a + 1], maps_a, *one[2:], 0)[0])


def test_identical_map_rows_give_the_same_bits_under_both_pairings(default_case):
    pol, rot, maps, rew, acts, rob = default_case
    same = np.ascontiguousarray(np.broadcast_to(maps[:, :1], maps.shape))
    a = decide_bf16(bf16_net(pol, "reference"), rot, same, rew, acts, rob)
    b = decide_bf16(bf16_net(pol, "own"), rot, same, rew, acts, rob)
    assert all(same_bits(x, y) for x, y in zip(a, b))
    c = decide_bf16(bf16_net(pol, "reference"), rot, maps, rew, acts, rob)
    assert not same_bits(a[0], c[0])


@pytest.mark.parametrize("network,H,n,overrides", [(1, 50, 5, {}), (1, 96, 5, dict(lstm_rl__mlp2_dims="40, 1")), (2, 50, 5, {}), (2, 64, 2, WIDE_MLP1),
                                                   (2, 17, 7, dict(lstm_rl__mlp1_dims="20"))])
def test_zero_map_weights_give_the_values_of_the_narrow_bf16_kernel(network, H, n, overrides):
    """Property (c): the map columns' weights zero -- the values are == those of cs_value_net_decide_lstm_bf16 on the narrow network and the
    same rotated rows (the map k-steps add exact zeros for finite maps), under both pairings; gates in registers and from the blob, mlp1
    of several layers and of one."""
    import torch

    from test_gpu_value_lstm_bf16 import bf16_net as narrow_net
    from test_gpu_value_lstm_bf16 import decide_bf16 as narrow_decide

    pol = seeded_policy(network, 13, 61, lstm_rl__global_state_dim=H, **overrides)
    narrow = lc.lstm_policy(network, 13, lstm_rl__global_state_dim=H, **overrides)
    wide_key = "mlp1.0.weight" if network == 2 else "lstm.weight_ih_l0"
    sd = {k: v.clone() for k, v in pol.model.state_dict().items()}
    with torch.no_grad():
        pol.model.state_dict()[wide_key][:, 13:] = 0.0
    sd[wide_key] = sd[wide_key][:, :13].clone()
    narrow.model.load_state_dict(sd, strict=True)
    rot, maps, rew, acts, rob = random_case(11 + n, 2, 40, n, 13, 48)
    want = narrow_decide(narrow_net(narrow), rot, rew, acts, rob)
    assert np.all(np.isfinite(want[0]))
    for pairing in olc.PAIRINGS:
        got = decide_bf16(bf16_net(pol, pairing), rot, maps, rew, acts, rob)
        assert all(same_bits(a, b) for a, b in zip(got, want)), pairing


# ---------------------------------------------------------------------------------------------------------------- the order
def test_ties_and_a_nan_distance_follow_the_float32_kernels_rule():
    """Inputs where the order alone decides: every action of a world holds the SAME five rows (two of them tied in distance, one with a NaN
    distance in world 1), lying in another permutation, beside identical maps and equal rewards.  Two actions get the same value exactly when
    the rule evaluates their rows in the same order; that pattern is the host rule's (lstm_cases.decision_order) and the float32 OM kernel's,
    under both pairings.  And the kernel's own sort equals the kernel on rows permuted on the host by the rule, bitwise."""
    import itertools

    pol = seeded_policy(1, 13, 32)
    perms = [list(p) for p in itertools.permutations(range(5))][::7][:12]
    W, A = 2, len(perms)
    rot, maps, rew, acts, rob = random_case(6, W, A, 5, 13, 48)
    base = rot[:, 0].copy()
    base[0, [1, 3], 11] = F32(1.25)                                 # world 0: two humans tied
    base[1, [0, 4], 11] = F32(0.75)                                 # world 1: two tied, and a NaN distance, which sorts first
    base[1, 2, 11] = np.nan
    for a, p in enumerate(perms):
        rot[:, a] = base[:, p]
    rew[:] = rew[:, :1]
    maps = np.ascontiguousarray(np.broadcast_to(maps[:, :1], maps.shape))
    order = lc.decision_order(rot[..., 11])
    evaluated = np.take_along_axis(np.broadcast_to(np.array(perms)[None], order.shape), order, axis=2)       # which base row each step reads
    want_equal = np.all(evaluated[:, :, None] == evaluated[:, None, :], axis=3)
    assert 0 < want_equal[0].sum() - A and not want_equal[0].all()  # some actions collapse to one order, not all
    for pairing in olc.PAIRINGS:
        got = decide_bf16(bf16_net(pol, pairing), rot, maps, rew, acts, rob)
        f32 = f32om.om_call(f32om.device_net(pol, pairing), rot, maps, rew, acts, rob, 1)
        # world 0 shows the order in its values; world 1's NaN is a distance, which the network reads too: all NaN in both kernels, its
        # order is held by the bitwise comparison with the rows permuted on the host alone
        words, f32_words = got[0][0].view(np.int32), f32[0][0].view(np.int32)
        assert np.all(np.isfinite(got[0][0])) and np.all(np.isfinite(f32[0][0])) and np.all(np.isnan(got[0][1])) and np.all(np.isnan(f32[0][1]))
        assert np.array_equal(words[:, None] == words[None, :], want_equal[0]), pairing
        assert np.array_equal(f32_words[:, None] == f32_words[None, :], want_equal[0]), pairing
        assert np.array_equal(got[1], f32[1])                       # the picks: world 0 by the same equalities, world 1 by the NaN rule
        lying = decide_bf16(bf16_net(pol, pairing), lc.sort_rows(rot), maps, rew, acts, rob, 0)
        assert same_bits(got[0], lying[0]) and np.array_equal(got[1], lying[1])


# ---------------------------------------------------------------------------------------------------------------- isolation
@pytest.mark.parametrize("network", [1, 2])
def test_a_nan_and_an_infinity_stay_in_their_sequence(network):
    """A NaN and a +-inf in one sequence's rotated rows: its value is NaN, every other sequence keeps its bits, the pick follows
    decision_edges.expected_pick (a NaN counts as the maximum)."""
    net = bf16_net(seeded_policy(network, 13, 57), "own")
    rot, maps, rew, acts, rob = random_case(13, 3, 27, 5, 13, 48)
    clean = decide_bf16(net, rot, maps, rew, acts, rob)[0]
    bad = rot.copy()
    bad[1, 5, 2, 3], bad[1, 5, 4, 6], bad[1, 5, 0, 8] = np.nan, np.inf, -np.inf
    vals, pick, act = decide_bf16(net, bad, maps, rew, acts, rob)
    assert np.isnan(vals[1, 5]) and np.all(np.isfinite(clean))
    keep = np.ones(vals.shape, bool)
    keep[1, 5] = False
    assert same_bits(vals[keep], clean[keep])
    assert np.array_equal(pick, de.expected_pick(vals)) and pick[1] == 5 and same_bits(act, acts[pick])


@pytest.mark.parametrize("network", [1, 2])
@pytest.mark.parametrize("pairing", olc.PAIRINGS)
def test_a_nan_in_a_map_row_reaches_the_sequences_that_read_it(network, pairing):
    """Every sequence of a world reads every map row of that world once, under either pairing: a NaN in one map row of world 1 makes all of
    world 1's values NaN and leaves every other world's bits."""
    net = bf16_net(seeded_policy(network, 13, 58), pairing)
    rot, maps, rew, acts, rob = random_case(14, 3, 27, 5, 13, 48)
    clean = decide_bf16(net, rot, maps, rew, acts, rob)[0]
    bad = maps.copy()
    bad[1, 3, 17] = np.nan
    vals = decide_bf16(net, rot, bad, rew, acts, rob)[0]
    assert np.all(np.isfinite(clean)) and np.all(np.isnan(vals[1])) and same_bits(vals[[0, 2]], clean[[0, 2]])


def test_forced_actions_and_the_goal_behave_as_in_cs_value_net_decide():
    net = bf16_net(seeded_policy(1, 13, 55))
    rot, maps, rew, acts, rob = random_case(9, 4, 7, 5, 13, 48)
    rob[3, 5:7] = rob[3, 0:2] + F32(0.1)                                # within its radius (0.3) of the goal
    free = decide_bf16(net, rot, maps, rew, acts, rob)
    forced = decide_bf16(net, rot, maps, rew, acts, rob, override=np.array([5, -1, 99, 2], np.int32))
    assert same_bits(free[0], forced[0])
    greedy = np.argmax(free[0], axis=1)
    assert np.array_equal(free[1], greedy) and np.array_equal(forced[1], [5, greedy[1], greedy[2], 2])      # an index outside 0..A-1 is greedy
    assert same_bits(forced[2][:3], acts[forced[1][:3]]) and np.array_equal(forced[2][3], [0, 0]) and np.array_equal(free[2][3], [0, 0])


def test_refusals_with_real_buffers_leave_the_outputs_untouched():
    """n = 129, sorted_by_distance = 2, map_order = 2, om_cols of another network, a blob of another size, a null pointer: CS_ERR_ARG and a
    message before any launch."""
    import torch

    from social_navigation_pyenvs_amd import _lib
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    pol = seeded_policy(1, 13, 55)
    net = bf16_net(pol)
    blob = net.blobs[value_net.MAPPED_RECURRENT_BF16]
    lib = _lib.load()
    rot, maps, rew, acts, rob = random_case(9, 2, 3, 129, 13, 48)
    d = {k: _up(a, torch.float32) for k, a in dict(rot=rot, maps=maps, rew=rew, acts=acts, rob=rob).items()}
    vals = torch.full((2, 3), np.nan, device="cuda")
    pick = torch.full((2,), -5, dtype=torch.int32, device="cuda")
    act = torch.full((2, 2), np.nan, device="cuda")

    def call(n=5, C_=48, in_order=1, map_order=1, n_bytes=blob.numel(), rewards=d["rew"].data_ptr(), weights=blob.data_ptr(), d_maps=d["maps"].data_ptr()):
        rc = lib.cs_value_net_decide_lstm_om_bf16(net.dims.ctypes.data, len(net.dims), weights, n_bytes, 2, 3, n, 13, C_, in_order, map_order,
                                                  d["rot"].data_ptr(), d_maps, rewards, d["acts"].data_ptr(), d["rob"].data_ptr(), 9, GAMMA, DT, None,
                                                  vals.data_ptr(), pick.data_ptr(), act.data_ptr(), _stream())
        return rc, lib.cs_last_error().decode()

    f32_bytes = 4 * f32om.device_net(pol).blob.numel()
    for kw, fragment in [(dict(n=129), "at most 128 humans a world (CS_VN_LSTM_MAX_N)"), (dict(in_order=2), "sorted_by_distance is 0 or 1"),
                         (dict(map_order=2), "map_order is CS_VN_MAPS_OWN or CS_VN_MAPS_FIRST_ACTION"), (dict(C_=0), "om_cols must be at least 1"),
                         (dict(C_=32), "the weight blob does not have the size of this network"),
                         (dict(n_bytes=blob.numel() - 4), "the weight blob does not have the size of this network"),
                         (dict(n_bytes=f32_bytes), "the weight blob does not have the size of this network"),
                         (dict(rewards=None), "null argument"), (dict(weights=None), "null argument"), (dict(d_maps=None), "null argument")]:
        rc, msg = call(**kw)
        assert (rc, fragment in msg) == (_lib.CS_ERR_ARG, True), (kw, msg)
    torch.cuda.synchronize()
    assert torch.isnan(vals).all() and torch.isnan(act).all() and (pick == -5).all()
    assert call()[0] == 0                                               # (and the same buffers are good for a decision)
    torch.cuda.synchronize()
    assert torch.isfinite(vals).all() and (pick >= 0).all()


def test_the_float32_decision_is_untouched_by_a_bf16_one():
    """After a bf16 decision a float32 decision of the same policy gives the bits a fresh float32 DeviceNet gives, and the two blobs are two
    tensors."""
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    pol = f32om._ready(seeded_policy(1, 13, 55))
    rot, maps, rew, acts, rob = random_case(9, 2, 27, 5, 13, 48)
    pol.set_mapped_precision("bf16")
    net = pol.device_net()
    half = decide_bf16(net, rot, maps, rew, acts, rob)
    pol.set_mapped_precision("f32")
    key = value_net.MAPPED_RECURRENT_BF16
    assert pol.device_net() is net and net.blobs[key] is not None and net.blobs["bf16"] is None and net.blobs[value_net.RECURRENT_BF16] is None
    assert net.blob.data_ptr() != net.blobs[key].data_ptr() and net.blob.dtype.is_floating_point
    after = f32om.om_call(net, rot, maps, rew, acts, rob, 1)
    fresh = f32om.om_call(f32om.device_net(pol), rot, maps, rew, acts, rob, 1)
    assert all(same_bits(a, b) for a, b in zip(after, fresh)) and not same_bits(half[0], after[0])


# ---------------------------------------------------------------------------------------------------------------- training, the Gym
def test_a_fused_training_step_reaches_the_bf16_decision():
    """8 device-reset worlds of 3 humans, the policy in bf16: two fused steps (set_gradient("device_lstm_om"), set_update("device")) move no
    version counter and drop the bf16 blob's key; ``act_device`` afterwards repacks it and decides with the updated weights -- the action
    values of a fresh policy loaded with the trained state_dict, bit for bit, and not those from before the steps."""
    import torch

    from test_gpu_value_policy import _batched, _ready

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net
    from social_navigation_pyenvs_amd.crowd_nav.utils.memory import ReplayMemory
    from social_navigation_pyenvs_amd.crowd_nav.utils.trainer import Trainer

    def policy():
        torch.manual_seed(2347)
        pol = olc.om_lstm_policy(1, 13)
        pol.set_mapped_precision("bf16")
        return pol

    env = _batched(3, W=8)
    pol = _ready(policy(), env)
    memory = ReplayMemory(64)
    for k in range(3):
        memory.push_batch(env.joint_state_device(pol), env.value_device(pol) + 0.5 + 0.1 * k)
        env.step_device(env.act_device("sfm_helbing"))
    env.act_device(pol)
    untrained = env.last_values_device()[0].clone()
    net = pol.device_net()
    key = value_net.MAPPED_RECURRENT_BF16
    stale = net.blobs[key].clone()
    trainer = Trainer(pol.model, memory, torch.device("cuda"), 16)
    trainer.set_learning_rate(0.01)
    trainer.set_gradient("device_lstm_om", net=net)
    trainer.set_update("device")
    assert np.isfinite(trainer.optimize_batch(2))
    assert net._keys[key] is None and net._keys["f32"] == net._versions()
    env.act_device(pol)
    values = env.last_values_device()[0].clone()
    torch.cuda.synchronize()
    assert pol.device_net() is net and net._keys[key] == net._versions() and not torch.equal(net.blobs[key], stale)
    fresh = _ready(policy(), env)
    fresh.model.load_state_dict({k: v.detach().clone() for k, v in pol.model.state_dict().items()})
    env.act_device(fresh)
    want = env.last_values_device()[0].clone()
    torch.cuda.synchronize()
    assert fresh.device_net().flat is None and torch.equal(fresh.device_net().blobs[key], net.blobs[key])
    values, want, untrained = values.cpu().numpy(), want.cpu().numpy(), untrained.cpu().numpy()
    assert np.all(np.isfinite(values)) and same_bits(values, want) and not same_bits(values, untrained)
    env.close()


def test_predict_and_the_batched_gym_decide_in_bf16():
    """W = 4 device-reset worlds x 5 humans after set_mapped_precision("bf16"): act_device is lookahead + the maps of the next humans +
    decide_lstm_om_bf16 by hand and four predict calls, bitwise; value_device returns the bits it returned before the setter."""
    import torch

    from test_gpu_value_policy import _PeekedEnv, _batched

    from social_navigation_pyenvs_amd.crowd_nav.utils.state import FullState, JointState, ObservableState

    env = _batched(5, W=4)
    for _ in range(3):
        env.step_device(env.act_device("sfm_helbing"))
    pol = f32om._ready(seeded_policy(1, 13, 91))
    pol.time_step = env.robot_time_step
    v32 = env.value_device(pol).clone()
    pol.set_mapped_precision("bf16")
    act = env.act_device(pol).clone()
    values, choice = (t.clone() for t in env.last_values_device())
    torch.cuda.synchronize()
    rot, rew = env.lookahead_device(pol.action_space_ndarray)
    maps = env.occupancy_maps_device(4, 1.0, 3, which="next")
    _, _, rob = env._worlds_on_side_stream(env._device_loop_state(), peek=False)
    torch.cuda.synchronize()
    net = pol.device_net()
    assert net.map_order == "reference" and same_bits(net.last_maps.cpu().numpy(), maps.cpu().numpy())
    acts = np.asarray(pol.action_space_ndarray, F32)
    want = decide_bf16(bf16_net(pol), rot, maps, rew, acts, rob, gamma=pol.gamma, dt=env.robot_time_step)
    assert same_bits(values.cpu().numpy(), want[0]) and np.array_equal(choice.cpu().numpy(), want[1]) and same_bits(act.cpu().numpy(), want[2])
    f32 = f32om.om_call(f32om.device_net(pol), rot, maps, rew, acts, rob, 1, gamma=pol.gamma, dt=env.robot_time_step)
    assert not same_bits(want[0], f32[0])                                                    # (it is the other arithmetic)
    assert same_bits(env.value_device(pol).cpu().numpy(), v32.cpu().numpy())                 # V(s) stays float32
    robot, obs, peek = env.cw.d_robot.download(), env.observe_device().cpu().numpy(), env.cw.peek(env.robot_time_step)
    for w in range(4):
        r = robot[w]
        state = JointState(FullState(*[float(x) for x in (r[0], r[1], r[3], r[4], r[8], r[10], r[11], r[12], r[2])]),
                           [ObservableState(*[float(x) for x in h]) for h in obs[w]])
        pol.set_env(_PeekedEnv(peek[w][:, :6]))
        a = pol.predict(state)
        assert (F32(a.vx), F32(a.vy)) == (act[w, 0].item(), act[w, 1].item()) and same_bits(np.asarray(pol.action_values, F32), values[w].cpu().numpy())
    pol.set_map_order("own")                                                                  # keeps its meaning beside the precision
    env.act_device(pol)
    own_values = env.last_values_device()[0].clone()
    torch.cuda.synchronize()
    assert same_bits(own_values.cpu().numpy(), decide_bf16(bf16_net(pol, "own"), rot, maps, rew, acts, rob, gamma=pol.gamma, dt=env.robot_time_step)[0])
    env.close()


# ---------------------------------------------------------------------------------------------------------------- golden G22
@pytest.mark.parametrize("wkey", ["omlstm1_13", "omlstm2_13"])
def test_g22_decisions_under_bf16(wkey):
    """Every recorded decision of the reference as one batch through decide_for_worlds(mapped_precision="bf16"): pick == argmax, and every
    pick that differs from the reference's recorded one is explained by bf16_emulation.classify_flip (gap <= 2 e against the float64
    restatement).  The float64 emulation's own count is pinned in the CPU file; HISTORY.md lists both."""
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    cs = [c for c in olc.g22()["decision"] if c["wkey"] == wkey]
    pol = f32om._ready(olc.g22_policy(wkey))
    pol.set_mapped_precision("bf16")
    acts = cs[0]["action_space"].astype(F32)
    nxt, cur, rob = (np.stack([c[k] for c in cs]).astype(F32) for k in ("next_humans", "obs", "robot"))
    W, A = len(cs), len(acts)
    vals = torch.full((W, A), np.nan, device="cuda")
    pick = torch.full((W,), -5, dtype=torch.int32, device="cuda")
    act = torch.full((W, 2), np.nan, device="cuda")
    gamma, dt = float(cs[0]["gamma"]), float(cs[0]["dt"])
    net = pol.device_net()
    rot, rew = value_net.decide_for_worlds(net, pol.decision_input, pol.decision_precision, _up(acts), _up(nxt), _up(cur), _up(rob), gamma, dt, None,
                                           vals, pick, act, _stream(), mapped_precision=pol.mapped_precision)
    torch.cuda.synchronize()
    vals, pick, act, maps = vals.cpu().numpy(), pick.cpu().numpy(), act.cpu().numpy(), net.last_maps.cpu().numpy()
    rot, rew = rot.cpu().numpy(), rew.cpu().numpy()
    full, _ = f32om.restated(pol.model, rot, maps, rew, rob[:, 7], "reference", gamma, dt)
    emu64 = oem.action_values(lc.weights64(pol.model), rot, maps, rew, np.power(gamma, dt * rob[:, 7].astype(np.float64)), "reference")
    assert W >= 20 and np.all(np.isfinite(vals)) and np.array_equal(pick, np.argmax(vals, axis=1)) and same_bits(act, acts[pick])
    flips = 0
    for k, c in enumerate(cs):
        if pick[k] != int(c["chosen"]):
            flips += 1
            ok, gap, e = em.classify_flip(int(c["chosen"]), int(pick[k]), full[k], emu64[k])
            print(f"G22 {wkey} decision {k}: the kernel picks {pick[k]}, the reference {c['chosen']}: gap {gap:.3e}, e {e:.3e}")
            assert ok, (k, gap, e)
    worst = float(np.max(np.abs(vals - emu64)))
    print(f"G22 {wkey} under bf16: {flips} of {W} decisions flipped, all explained (the float64 emulation: {cpu.G22_EMULATION_FLIPS[wkey]}); "
          f"kernel against the float64 emulation {worst:.3e}")
    parity_util.record(f"om_lstm_bf16_g22_flips_{wkey}", flips, bar=W)
