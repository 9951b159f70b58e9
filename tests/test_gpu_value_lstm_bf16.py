"""GPU suite of the opt-in bf16 arithmetic of LSTM-RL's decision (cs_value_net_decide_lstm_bf16, csrc/value_net_lstm_bf16.hip; DESIGN.md
4.5): the kernel against tests/lstm_bf16_emulation.py's float64 emulation of the contract on the cases of tests/test_value_lstm_bf16_cpu.py
(which shows what the arithmetic alone does on them), bit equality between launches, golden G21 under bf16, and the edges.

Two tiers, because a bf16 rounding sits between two float32 realisations of one contract: where one lands on the other side of a rounding
boundary that element moves by 2^-9 relative, and the recurrence carries it on.
  tight   at most 1/4 of a case's sequences farther than 4 x E_ref from the float64 emulation (E_ref: torch's CPU float32 module against
          lstm_cases.forward64 on the case's rows).  The float32 emulation alone stays at or below 1/8 (the CPU file), every excluded
          arithmetic is beyond 1/2 (the CPU file's mutants).
  loose   EVERY sequence within parity_util.F32_SLACK x the case's worst |float64 emulation - full-precision float64|.
Every comparison between two launches of this library is bitwise."""
import functools

import numpy as np
import pytest

import bf16_emulation as em
import decision_edges as de
import lstm_bf16_emulation as lem
import lstm_cases as lc
import parity_util
import test_value_lstm_bf16_cpu as cpu
from value_calls import _stream, _up, decide_call, same_bits

pytestmark = pytest.mark.gpu

F32 = np.float32
DT, GAMMA = cpu.DT, cpu.GAMMA


def bf16_net(pol):
    from social_navigation_pyenvs_amd.crowd_nav.policy.value_net import DeviceNet

    net = DeviceNet(pol.model, pol.joint_state_dim)
    net.refresh_recurrent("bf16")
    return net


def decide_bf16(net, rot, rew, acts, rob, in_order=1, gamma=GAMMA, dt=DT, override=None):
    """value_net.decide_lstm_bf16 on host arrays, as value_calls.decide_call: (values [W, A], choice [W], action [W, 2]) numpy; the outputs
    are NaN- / -5-filled before: every element must be written."""
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    W, A, n, _ = rot.shape
    vals = torch.full((W, A), np.nan, device="cuda")
    pick = torch.full((W,), -5, dtype=torch.int32, device="cuda")
    act = torch.full((W, 2), np.nan, device="cuda")
    d_rot, d_rew, d_acts, d_rob = _up(rot, torch.float32), _up(rew, torch.float32), _up(acts, torch.float32), _up(rob, torch.float32)
    d_ovr = None if override is None else _up(override, torch.int32)
    value_net.decide_lstm_bf16(net, W, A, n, in_order, d_rot.data_ptr(), d_rew.data_ptr(), d_acts.data_ptr(), d_rob.data_ptr(), d_rob.shape[1], gamma, dt,
                               None if d_ovr is None else d_ovr.data_ptr(), vals.data_ptr(), pick.data_ptr(), act.data_ptr(), _stream())
    torch.cuda.synchronize()
    return vals.cpu().numpy(), pick.cpu().numpy(), act.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _kernel(idx):
    d = cpu.case_data((cpu.TIGHT + cpu.LOOSE_ONLY)[idx])
    return decide_bf16(bf16_net(d["pol"]), *(np.array(d[k]) for k in ("rot", "rew", "acts", "rob")))        # (copies: the shared inputs are read-only)


def kernel_on(case):
    """The kernel's (values, choice, action) on a case of the CPU file, one launch shared by the two tiers"""
    return _kernel((cpu.TIGHT + cpu.LOOSE_ONLY).index(case))


# ---------------------------------------------------------------------------------------------------------------- the two tiers
@pytest.mark.parametrize("case", cpu.TIGHT, ids=cpu.case_id)
def test_short_and_feedforward_sequences_agree(case):
    """Measured on the MI355X: HISTORY.md lists the share and the median of every case."""
    d = cpu.case_data(case)
    vals, pick, act = kernel_on(case)
    share, median = cpu.share_beyond(vals, d)
    print(f"{cpu.case_id(case)}: E_ref {d['e_ref']:.3e}; kernel: share beyond {cpu.MARGIN:g} x E_ref {share:.3f}, median {median:.3e}")
    parity_util.record("lstm_bf16_tight_share", share, bar=cpu.TIGHT_CAP)
    parity_util.record("lstm_bf16_tight_median", median, bar=cpu.MARGIN * d["e_ref"])
    assert np.all(np.isfinite(vals))
    assert np.array_equal(pick, np.argmax(vals, axis=1)) and same_bits(act, d["acts"][pick])
    assert share <= cpu.TIGHT_CAP, (share, d["e_ref"])


@pytest.mark.parametrize("case", cpu.TIGHT + cpu.LOOSE_ONLY, ids=cpu.case_id)
def test_every_sequence_stays_within_the_arithmetics_own_error(case):
    d = cpu.case_data(case)
    vals, pick, _ = kernel_on(case)
    worst = float(np.max(np.abs(vals.astype(np.float64) - d["emu64"])))
    print(f"{cpu.case_id(case)}: the arithmetic's own error {d['own_error']:.3e}; kernel against the float64 emulation {worst:.3e} "
          f"(ratio {worst / d['own_error']:.3f})")
    parity_util.record("lstm_bf16_loose_ratio", worst / d["own_error"], bar=parity_util.F32_SLACK)
    assert np.all(np.isfinite(vals)) and np.array_equal(pick, np.argmax(vals, axis=1))
    assert worst <= parity_util.F32_SLACK * d["own_error"], (worst, d["own_error"])


# ---------------------------------------------------------------------------------------------------------------- bit equality
@pytest.mark.parametrize("network,H,overrides", [(1, 50, {}), (2, 64, dict(lstm_rl__mlp1_dims="60, 50"))])
def test_a_pair_alone_gives_the_bits_of_the_batch(network, H, overrides):
    """A (world, action) alone, W = A = 1, and the same rows at two positions of a 3 x 27 batch (another tile, another lane)."""
    from test_gpu_value_lstm import random_case, seeded_policy

    net = bf16_net(seeded_policy(network, 13, 77, lstm_rl__global_state_dim=H, **overrides))
    rot, rew, acts, rob = random_case(3, 3, 27, 5, 13)
    rot[2, 20], rew[2, 20], rob[2] = rot[0, 4], rew[0, 4], rob[0]       # the pair again, 70 sequences on: the third tile
    batch = decide_bf16(net, rot, rew, acts, rob)[0]
    alone = decide_bf16(net, rot[:1, 4:5], rew[:1, 4:5], acts[4:5], rob[:1])[0]
    assert np.all(np.isfinite(batch)) and same_bits(alone[0, :1], batch[0, 4:5]) and same_bits(alone[0, :1], batch[2, 20:21])


@pytest.mark.parametrize("network", [1, 2])
def test_the_tile_edges_give_the_bits_of_the_batch(network):
    """W * A of 1, 31, 32 and 33 cut from one batch of 33 sequences: a tile not full, full, and one sequence into the next."""
    from test_gpu_value_lstm import random_case, seeded_policy

    net = bf16_net(seeded_policy(network, 13, 78))
    rot, rew, acts, rob = random_case(4, 1, 33, 5, 13)
    whole = decide_bf16(net, rot, rew, acts, rob)[0]
    assert np.all(np.isfinite(whole))
    for count in (1, 31, 32, 33):
        part = decide_bf16(net, rot[:, :count], rew[:, :count], acts[:count], rob)[0]
        assert same_bits(part, whole[:, :count]), count
    last = decide_bf16(net, rot[:, 32:], rew[:, 32:], acts[32:], rob)[0]                    # the second tile's only sequence, alone
    assert same_bits(last, whole[:, 32:])


def test_ties_and_sorted_sequences_follow_the_order_rule():
    """test_gpu_value_lstm's tied distances: sorted_by_distance = 1 equals sorted_by_distance = 0 on the rows permuted by the rule."""
    from test_gpu_value_lstm import random_case, seeded_policy

    net = bf16_net(seeded_policy(1, 13, 31))
    rot, rew, acts, rob = random_case(5, 1, 6, 5, 13)
    d = F32(1.25)
    rot[0, 0, [1, 3], 11] = d                                   # two humans tied, (px, py) on opposite sides
    rot[0, 0, 1, 6:8], rot[0, 0, 3, 6:8] = (d, 0), (-d, 0)
    rot[0, 1, [0, 2, 4], 11] = d                                # three tied
    rot[0, 1, 0, 6:8], rot[0, 1, 2, 6:8], rot[0, 1, 4, 6:8] = (d, 0), (0, d), (-d, 0)
    rot[0, 2, :, 11] = F32(0.5)                                 # all tied: the humans in reverse
    rot[0, 3] = rot[0, 3][np.argsort(-rot[0, 3, :, 11], kind="stable")]        # already in order
    rot[0, 4] = rot[0, 4][np.argsort(rot[0, 4, :, 11], kind="stable")]         # reversed
    got = decide_bf16(net, rot, rew, acts, rob, 1)
    permuted = lc.sort_rows(rot)
    lying = decide_bf16(net, permuted, rew, acts, rob, 0)
    assert np.all(np.isfinite(got[0])) and all(same_bits(a, b) for a, b in zip(got, lying))
    assert not same_bits(decide_bf16(net, rot, rew, acts, rob, 0)[0], got[0])               # (the order matters to this network)


def test_the_float32_decision_is_untouched_by_a_bf16_one():
    """After a bf16 decision a float32 decision of the same policy gives the bits a fresh float32 DeviceNet gives, and the two blobs are
    two tensors."""
    from test_gpu_value_lstm import _ready, device_net, random_case, seeded_policy

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    pol = _ready(seeded_policy(1, 13, 55))
    rot, rew, acts, rob = random_case(9, 2, 27, 5, 13)
    pol.set_recurrent_precision("bf16")
    net = pol.device_net()
    half = decide_bf16(net, rot, rew, acts, rob)
    pol.set_recurrent_precision("f32")
    assert pol.device_net() is net and net.blobs[value_net.RECURRENT_BF16] is not None and net.blobs["bf16"] is None
    assert net.blob.data_ptr() != net.blobs[value_net.RECURRENT_BF16].data_ptr() and net.blob.dtype.is_floating_point
    after = decide_call(net, rot, rew, acts, rob, 1)
    fresh = decide_call(device_net(pol), rot, rew, acts, rob, 1)
    assert all(same_bits(a, b) for a, b in zip(after, fresh)) and not same_bits(half[0], after[0])


def test_a_fused_training_step_reaches_the_bf16_decision():
    """One Trainer.set_update("device") step in mode "device_lstm" (B = 33, n = 2) moves no version counter; the bf16 blob packed before it
    is dropped, and the bf16 decision afterwards is that of a fresh DeviceNet built from the updated parameters."""
    import torch

    import value_grad_cases as vg
    import value_step_cases as vs
    from test_gpu_value_lstm import random_case

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    trainer = vs.trainer_for(vs.model_of("lstm1_13")[0], "device_lstm", "device")
    net = trainer.net
    x, v = vs.batch_of("lstm1_13", 33, 2)
    trainer.data_loader = vg.in_order_loader([(x.cuda(), v.cuda())] * 2)
    rot, rew, acts, rob = random_case(11, 2, 27, 5, 13)
    stale_blob = net.refresh_recurrent("bf16").clone()
    stale = decide_bf16(net, rot, rew, acts, rob)
    trainer.optimize_batch(1)
    torch.cuda.synchronize()
    assert net._keys[value_net.RECURRENT_BF16] is None and net._keys["f32"] == net._versions()
    blob = net.refresh_recurrent("bf16")
    got = decide_bf16(net, rot, rew, acts, rob)
    fresh_net = value_net.DeviceNet(trainer.model, 13)
    want = decide_bf16(bf16_net_of(fresh_net), rot, rew, acts, rob)
    assert not torch.equal(blob, stale_blob) and torch.equal(blob, fresh_net.blobs[value_net.RECURRENT_BF16])
    assert all(same_bits(a, b) for a, b in zip(got, want)) and not same_bits(got[0], stale[0])


def bf16_net_of(net):
    net.refresh_recurrent("bf16")
    return net


def test_predict_and_the_batched_gym_decide_in_bf16():
    """W = 4 device-reset worlds x 5 humans after set_recurrent_precision("bf16"): act_device is lookahead + decide_lstm_bf16 by hand and
    four predict calls, bitwise; value_device stays float32."""
    import torch

    from test_gpu_value_lstm import _ready, device_net, seeded_policy
    from test_gpu_value_policy import _PeekedEnv, _batched

    from social_navigation_pyenvs_amd.crowd_nav.utils.state import FullState, JointState, ObservableState

    env = _batched(5, W=4)
    for _ in range(3):
        env.step_device(env.act_device("sfm_helbing"))
    pol = _ready(seeded_policy(1, 13, 91))
    pol.time_step = env.robot_time_step
    v32 = env.value_device(pol).clone()
    pol.set_recurrent_precision("bf16")
    act = env.act_device(pol).clone()
    values, choice = (t.clone() for t in env.last_values_device())
    torch.cuda.synchronize()
    rot, rew = env.lookahead_device(pol.action_space_ndarray)
    _, _, rob = env._worlds_on_side_stream(env._device_loop_state(), peek=False)
    torch.cuda.synchronize()
    acts = np.asarray(pol.action_space_ndarray, F32)
    hand = rot.cpu().numpy(), rew.cpu().numpy(), acts, rob.cpu().numpy()
    want = decide_bf16(bf16_net(pol), *hand, gamma=pol.gamma, dt=env.robot_time_step)
    assert same_bits(values.cpu().numpy(), want[0]) and np.array_equal(choice.cpu().numpy(), want[1]) and same_bits(act.cpu().numpy(), want[2])
    f32 = decide_call(device_net(pol), *hand, 1, gamma=pol.gamma, dt=env.robot_time_step)
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
    env.close()


# ---------------------------------------------------------------------------------------------------------------- golden G21
@pytest.mark.parametrize("wkey", ["lstm1_13", "lstm2_13"])
def test_g21_decisions_under_bf16(wkey):
    """Every recorded decision of the reference as one batch through decide_for_worlds(recurrent_precision="bf16"): pick == argmax, and every
    pick that differs from the reference's recorded one is explained by bf16_emulation.classify_flip (gap <= 2 e against forward64).  The
    float64 emulation's own count is pinned in the CPU file; HISTORY.md lists both."""
    import torch

    from test_gpu_value_lstm import _ready, restated

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    cs = [c for c in lc.g21()["decision"] if c["wkey"] == wkey]
    pol = _ready(lc.g21_policy(wkey))
    pol.set_recurrent_precision("bf16")
    acts = cs[0]["action_space"].astype(F32)
    nxt, cur, rob = (np.stack([c[k] for c in cs]).astype(F32) for k in ("next_humans", "obs", "robot"))
    W, A = len(cs), len(acts)
    vals = torch.full((W, A), np.nan, device="cuda")
    pick = torch.full((W,), -5, dtype=torch.int32, device="cuda")
    act = torch.full((W, 2), np.nan, device="cuda")
    gamma, dt = float(cs[0]["gamma"]), float(cs[0]["dt"])
    rot, rew = value_net.decide_for_worlds(pol.device_net(), pol.decision_input, pol.decision_precision, _up(acts), _up(nxt), _up(cur), _up(rob), gamma, dt,
                                           None, vals, pick, act, _stream(), recurrent_precision=pol.recurrent_precision)
    torch.cuda.synchronize()
    vals, pick, act = vals.cpu().numpy(), pick.cpu().numpy(), act.cpu().numpy()
    rot, rew = rot.cpu().numpy(), rew.cpu().numpy()
    full, _ = restated(pol.model, rot, rew, rob[:, 7], gamma, dt)
    emu64 = lem.action_values(lc.weights64(pol.model), rot, rew, np.power(gamma, dt * rob[:, 7].astype(np.float64)))
    assert W >= 20 and np.all(np.isfinite(vals)) and np.array_equal(pick, np.argmax(vals, axis=1)) and same_bits(act, acts[pick])
    flips = 0
    for k, c in enumerate(cs):
        if pick[k] != int(c["chosen"]):
            flips += 1
            ok, gap, e = em.classify_flip(int(c["chosen"]), int(pick[k]), full[k], emu64[k])
            print(f"G21 {wkey} decision {k}: the kernel picks {pick[k]}, the reference {c['chosen']}: gap {gap:.3e}, e {e:.3e}")
            assert ok, (k, gap, e)
    worst = float(np.max(np.abs(vals - emu64)))
    print(f"G21 {wkey} under bf16: {flips} of {W} decisions flipped, all explained (the float64 emulation: {cpu.G21_EMULATION_FLIPS[wkey]}); "
          f"kernel against the float64 emulation {worst:.3e}")
    parity_util.record(f"lstm_bf16_g21_flips_{wkey}", flips, bar=W)


# ---------------------------------------------------------------------------------------------------------------- edges
@pytest.mark.parametrize("network", [1, 2])
def test_a_nan_and_an_infinity_stay_in_their_sequence(network):
    """A NaN and a +-inf in one sequence's rows: its value is NaN, every other sequence keeps its bits, the pick follows
    decision_edges.expected_pick (a NaN counts as the maximum)."""
    from test_gpu_value_lstm import random_case, seeded_policy

    net = bf16_net(seeded_policy(network, 13, 57))
    rot, rew, acts, rob = random_case(13, 3, 27, 5, 13)
    clean = decide_bf16(net, rot, rew, acts, rob)[0]
    bad = rot.copy()
    bad[1, 5, 2, 3], bad[1, 5, 4, 6], bad[1, 5, 0, 8] = np.nan, np.inf, -np.inf
    vals, pick, act = decide_bf16(net, bad, rew, acts, rob)
    assert np.isnan(vals[1, 5]) and np.all(np.isfinite(clean))
    keep = np.ones(vals.shape, bool)
    keep[1, 5] = False
    assert same_bits(vals[keep], clean[keep])
    assert np.array_equal(pick, de.expected_pick(vals)) and pick[1] == 5 and same_bits(act, acts[pick])


def test_forced_actions_and_the_goal_behave_as_in_cs_value_net_decide():
    from test_gpu_value_lstm import random_case, seeded_policy

    net = bf16_net(seeded_policy(1, 13, 55))
    rot, rew, acts, rob = random_case(9, 4, 7, 5, 13)
    rob[3, 5:7] = rob[3, 0:2] + F32(0.1)                                # within its radius (0.3) of the goal
    free = decide_bf16(net, rot, rew, acts, rob)
    forced = decide_bf16(net, rot, rew, acts, rob, override=np.array([5, -1, 99, 2], np.int32))
    assert same_bits(free[0], forced[0])
    greedy = np.argmax(free[0], axis=1)
    assert np.array_equal(free[1], greedy) and np.array_equal(forced[1], [5, greedy[1], greedy[2], 2])      # an index outside 0..A-1 is greedy
    assert same_bits(forced[2][:3], acts[forced[1][:3]]) and np.array_equal(forced[2][3], [0, 0]) and np.array_equal(free[2][3], [0, 0])


def test_refusals_with_real_buffers_leave_the_outputs_untouched():
    """n = 129, sorted_by_distance = 2, a blob of another size, a null pointer: CS_ERR_ARG and a message before any launch."""
    import torch

    from test_gpu_value_lstm import random_case, seeded_policy

    from social_navigation_pyenvs_amd import _lib

    pol = seeded_policy(1, 13, 55)
    net = bf16_net(pol)
    blob = net.blobs["recurrent_bf16"]
    lib = _lib.load()
    rot, rew, acts, rob = random_case(9, 2, 3, 129, 13)
    d = {k: _up(a, torch.float32) for k, a in dict(rot=rot, rew=rew, acts=acts, rob=rob).items()}
    vals = torch.full((2, 3), np.nan, device="cuda")
    pick = torch.full((2,), -5, dtype=torch.int32, device="cuda")
    act = torch.full((2, 2), np.nan, device="cuda")

    def call(n=5, in_order=1, n_bytes=blob.numel(), rewards=d["rew"].data_ptr(), weights=blob.data_ptr()):
        rc = lib.cs_value_net_decide_lstm_bf16(net.dims.ctypes.data, len(net.dims), weights, n_bytes, 2, 3, n, 13, in_order, d["rot"].data_ptr(), rewards,
                                               d["acts"].data_ptr(), d["rob"].data_ptr(), 9, GAMMA, DT, None, vals.data_ptr(), pick.data_ptr(),
                                               act.data_ptr(), _stream())
        return rc, lib.cs_last_error().decode()

    for kw, fragment in [(dict(n=129), "at most 128 humans a world (CS_VN_LSTM_MAX_N)"), (dict(in_order=2), "sorted_by_distance is 0 or 1"),
                         (dict(n_bytes=blob.numel() - 4), "the weight blob does not have the size of this network"),
                         (dict(n_bytes=4 * pol.device_net().blob.numel()), "the weight blob does not have the size of this network"),
                         (dict(rewards=None), "null argument"), (dict(weights=None), "null argument")]:
        rc, msg = call(**kw)
        assert (rc, fragment in msg) == (_lib.CS_ERR_ARG, True), (kw, msg)
    torch.cuda.synchronize()
    assert torch.isnan(vals).all() and torch.isnan(act).all() and (pick == -5).all()
    assert call()[0] == 0                                               # (and the same buffers are good for a decision)
    torch.cuda.synchronize()
    assert torch.isfinite(vals).all() and (pick >= 0).all()
