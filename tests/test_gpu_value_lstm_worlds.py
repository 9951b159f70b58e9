"""GPU suite of LSTM-RL's decision from the resident worlds (cs_value_net_decide_lstm_worlds, cs_value_net_decide_lstm_worlds_bf16;
csrc/value_net_lstm_worlds.hip, value_net_lstm_worlds_bf16.hip): the recurrent kernels that generate their rows in LDS against cs_lookahead ->
cs_value_net_decide_lstm[_bf16] on the same buffers, bit for bit, in both arithmetics; tied distances; a world alone against the batch; the
override column and the goal; rows as they lie; the batched Gym and ``predict`` with ``set_recurrent_input("fused")`` against ``"tensor"``; and
the reference's recorded decisions (golden G21).

Every comparison between the two paths is bitwise (np.array_equal on the float32 / int32 views) and every compared value is finite."""
import numpy as np
import pytest

import lstm_cases as lc
from test_gpu_value_lstm import SHAPES, WIDE_MLP1, _RecordedEnv, device_net, seeded_policy
from test_gpu_value_policy import _batched, _ready
from test_gpu_value_worlds import DT, GAMMA, _outputs, assert_same_bits, reward_branches, worlds
from value_calls import _stream, _up, same_bits

pytestmark = pytest.mark.gpu

F32 = np.float32
PRECISIONS = ("f32", "bf16")
# (network, H, overrides): the networks of test_gpu_value_lstm.SHAPES that choose the float32 kernel's four (WREG, MLP1) builds, and one more,
# "2-h96": in the bf16 arithmetic "2-h64-wide" keeps its gates in registers (4 + 4 slots of 16 bytes), so network 2 with the gates from the
# blob needs more than 8 blocks there.  builds() states which build each runs in each arithmetic; the coverage test asserts all four occur
NETS = {
    "1-h50": (1, 50, {}),                        # register-resident gates
    "1-h64": (1, 64, {}),                        # the widest register-resident LSTM
    "1-h96": (1, 96, dict(lstm_rl__mlp2_dims="40, 1")),      # 12 blocks: the gates from the blob
    "2-h50": (2, 50, {}),                        # network 2's default: register-resident gates behind mlp1
    "2-h64-wide": (2, 64, WIDE_MLP1),            # network 2 with the gates from the blob in float32 (8 + 7 k-groups), in registers in bf16
    "2-h96": (2, 96, {}),                        # network 2 with the gates from the blob in both arithmetics: 12 blocks
}


def builds(name, precision):
    """(WREG, MLP1) of the build the worlds entry of `precision` launches for NETS[name], by the entries' own rule (value_net_lstm_worlds.hip:
    at most 8 blocks of 8 hidden units and 14 k-groups of 8, h's and the input's; value_net_lstm_worlds_bf16.hip: at most 8 blocks, 4 slots of
    W_hh in k-steps of 16 and 4 of the x part -- k-steps of 16 of mlp1's last width, or the two float32 k-groups of the 13 | 15 columns)"""
    network, H, overrides = NETS[name]
    up = lambda x, m: -(-x // m)
    mlp1 = network == 2
    xin = int(overrides.get("lstm_rl__mlp1_dims", lc.LSTM_SECTION["mlp1_dims"]).split(",")[-1]) if mlp1 else 13
    if precision == "f32":
        return up(H, 8) <= 8 and up(H, 8) + up(xin, 8) <= 14, mlp1
    return up(H, 8) <= 8 and up(H, 16) <= 4 and (up(xin, 16) if mlp1 else up(xin, 8)) <= 4, mlp1


@pytest.fixture(scope="module")
def nets():
    """(net name, cols) -> (policy, DeviceNet with both blobs current), built once"""
    made = {}

    def get(name, cols=13):
        if (name, cols) not in made:
            network, H, overrides = NETS[name]
            pol = seeded_policy(network, cols, 3100 + 7 * sorted(NETS).index(name) + cols, lstm_rl__global_state_dim=H, **overrides)
            net = device_net(pol)
            net.refresh_recurrent("bf16")
            made[name, cols] = (pol, net)
        return made[name, cols]

    return get


def decide_fused(net, case, precision, sorted_by_distance=1, override=None, rewards=True):
    """cs_value_net_decide_lstm_worlds[_bf16] on a case of worlds(): (rewards [W, A] or None, values [W, A], choice [W], action [W, 2]) numpy"""
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    acts, nxt, cur, rob = (_up(x) for x in case)
    W, n, A, headed = cur.shape[0], cur.shape[1], acts.shape[0], cur.shape[2] == 7
    vals, pick, act = _outputs(W, A)
    rew = torch.full((W, A), np.nan, device="cuda") if rewards else None
    ovr = None if override is None else _up(override, torch.int32)
    entry = value_net.decide_lstm_worlds if precision == "f32" else value_net.decide_lstm_worlds_bf16
    entry(net, W, A, n, headed, sorted_by_distance, acts.data_ptr(), nxt.data_ptr(), cur.data_ptr(), rob.data_ptr(), rob.shape[1], GAMMA, DT,
          None if ovr is None else ovr.data_ptr(), None if rew is None else rew.data_ptr(), vals.data_ptr(), pick.data_ptr(), act.data_ptr(), _stream())
    torch.cuda.synchronize()
    return (None if rew is None else rew.cpu().numpy(), vals.cpu().numpy(), pick.cpu().numpy(), act.cpu().numpy())


def decide_rows(net, rot, rew, case, precision, sorted_by_distance=1, override=None):
    """cs_value_net_decide_lstm[_bf16] on rows rot [W, A, n, cols] and rewards: (values, choice, action) numpy"""
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    acts, rob = _up(case[0]), _up(case[3])
    rot, rew = _up(rot), _up(rew)
    W, A, n, _ = rot.shape
    vals, pick, act = _outputs(W, A)
    ovr = None if override is None else _up(override, torch.int32)
    entry = value_net.decide_lstm if precision == "f32" else value_net.decide_lstm_bf16
    entry(net, W, A, n, sorted_by_distance, rot.data_ptr(), rew.data_ptr(), acts.data_ptr(), rob.data_ptr(), rob.shape[1], GAMMA, DT,
          None if ovr is None else ovr.data_ptr(), vals.data_ptr(), pick.data_ptr(), act.data_ptr(), _stream())
    torch.cuda.synchronize()
    return vals.cpu().numpy(), pick.cpu().numpy(), act.cpu().numpy()


def decide_tensor(net, case, precision, sorted_by_distance=1, override=None, want_rows=False):
    """cs_lookahead -> cs_value_net_decide_lstm[_bf16] on the same case: (rewards, values, choice, action) numpy [, the rows [W, A, n, cols]]"""
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    acts, nxt, cur, rob = (_up(x) for x in case)
    rot, rew = value_net.lookahead(acts, nxt, cur, rob, DT, _stream())
    out = (rew.cpu().numpy(),) + decide_rows(net, rot, rew, case, precision, sorted_by_distance, override)
    torch.cuda.synchronize()
    return out + (rot.cpu().numpy(),) if want_rows else out


# ---------------------------------------------------------------------------------------------------------------- bit equality
# net, cols, n, W, A: every n of {1, 2, 5, 33, 64, 128}; W * A of {1, 31, 32, 33, 243} around one job and eight jobs, the last of 19 sequences;
# W = 5, A = 7: every job crosses a world; both column counts; every net of NETS (the kernel's four builds) in both
CASES = [
    ("1-h50", 13, 5, 3, 81), ("1-h50", 15, 1, 1, 1), ("1-h50", 13, 2, 31, 1), ("1-h50", 15, 5, 5, 7), ("1-h50", 13, 128, 1, 32),
    ("1-h64", 13, 33, 1, 32), ("1-h64", 15, 5, 3, 81),
    ("1-h96", 15, 64, 3, 11), ("1-h96", 13, 5, 5, 7), ("1-h96", 13, 2, 1, 1),
    ("2-h50", 13, 5, 33, 1), ("2-h50", 15, 33, 3, 81), ("2-h50", 13, 5, 5, 7), ("2-h50", 13, 64, 1, 1),
    ("2-h64-wide", 13, 2, 31, 1), ("2-h64-wide", 15, 128, 3, 11), ("2-h64-wide", 13, 1, 1, 32),
    ("2-h96", 13, 5, 3, 81), ("2-h96", 15, 33, 5, 7), ("2-h96", 13, 2, 1, 33),
]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("net,cols,n,W,A", CASES)
def test_fused_equals_lookahead_then_decide(nets, net, cols, n, W, A, precision):
    """rewards_out, values, choice and action_out of the worlds entry are those of cs_lookahead -> the tensor entry, bit for bit; the same
    decision without d_rewards_out.  With three or more worlds the inputs hold all four reward branches (asserted)."""
    _, dnet = nets(net, cols)
    case = worlds(W, n, A, cols == 15, seed=2000 * n + 10 * W + A)
    want = decide_tensor(dnet, case, precision)
    label = f"{net} {precision} cols={cols} W={W} A={A} n={n}"
    assert_same_bits(decide_fused(dnet, case, precision), want, label)
    if W >= 3:
        assert all(reward_branches(want[0]).values()), (label, reward_branches(want[0]))
    assert_same_bits(decide_fused(dnet, case, precision, rewards=False)[1:], want[1:], label + " (no rewards_out)")


def test_the_cases_cover_the_issues_edges():
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    assert set(PRECISIONS) == set(value_net.RECURRENT.worlds) == set(value_net.RECURRENT_PRECISIONS)      # an entry per arithmetic, each tested
    assert {c[2] for c in CASES} >= {1, 2, 5, 33, 64, 128} and {c[3] * c[4] for c in CASES} >= {1, 31, 32, 33, 243} and (5, 7) in {c[3:] for c in CASES}
    assert {c[0] for c in CASES} == set(NETS) and {(c[0], c[1]) for c in CASES} >= {(name, cols) for name in ("1-h50", "2-h50") for cols in (13, 15)}
    # NETS hold the networks of test_gpu_value_lstm.SHAPES that reach the float32 builds: H 50 and 64 in registers, 96 from the blob, both mlp1's
    shapes = {(s[0], s[2], tuple(sorted(s[6].items()))) for s in SHAPES}
    assert all((network, H, tuple(sorted(o.items()))) in shapes for name, (network, H, o) in NETS.items() if name != "2-h96")
    # every one of the eight new builds is launched: in each arithmetic the nets of CASES run all four (WREG, MLP1) pairs, by the entries' rule
    every = {(wreg, mlp1) for wreg in (True, False) for mlp1 in (True, False)}
    for precision in PRECISIONS:
        assert {builds(c[0], precision) for c in CASES} == every, precision
    assert builds("2-h64-wide", "f32") == (False, True) and builds("2-h64-wide", "bf16") == (True, True) and builds("2-h96", "bf16") == (False, True)
    assert all(c[3] < 3 or c[4] >= 7 or c[3] >= 4 for c in CASES)          # (what worlds() needs for the four reward branches)


# ---------------------------------------------------------------------------------------------------------------- ties
def tied_worlds(n=5):
    """Three worlds whose robot stands at (1.0, 0.5) and whose action 0 is (0, 0): next humans at bit-equal distance 1.25 from the robot's
    next position on different sides -- two of them (world 0), three (world 1), all n = 5 (world 2); every difference, square and sum is
    exact in float32 (1.25^2 = 0.75^2 + 1^2 = 1.5625).  The other humans stand at distinct distances."""
    acts, nxt, cur, rob = worlds(3, n, 6, False, seed=41)
    rob[:, 0:2] = (1.0, 0.5)
    rob[:, 5:7] = (5.0, 4.0)
    ring = np.array([(2.25, 0.5), (-0.25, 0.5), (1.0, 1.75), (1.0, -0.75), (1.75, 1.5)], F32)
    far = np.array([(1.0 + 2.0 + 0.5 * j, 0.5 + 0.25 * j) for j in range(n)], F32)
    for w, tied in enumerate(([1, 3], [0, 2, 4], list(range(n)))):
        nxt[w, :, 0:2] = far
        nxt[w, tied, 0:2] = ring[:len(tied)]
    cur[..., 0:2], cur[..., 2:4], nxt[..., 2:4] = nxt[..., 0:2], 0.0, 0.0
    return (acts, nxt, cur, rob), ([1, 3], [0, 2, 4], list(range(n)))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("net", ["1-h50", "2-h50"])
def test_tied_distances_fall_as_in_the_tensor(nets, net, precision):
    _, dnet = nets(net)
    case, tied = tied_worlds()
    want = decide_tensor(dnet, case, precision, want_rows=True)
    rot = want[4]
    for w, rows in enumerate(tied):
        da = rot[w, 0, :, 11]
        assert np.all(da[rows].view(np.int32) == F32(1.25).view(np.int32)) and np.sum(da == F32(1.25)) == len(rows), (w, da)
        order = lc.decision_order(da)
        assert [j for j in order if j in rows] == sorted(rows, reverse=True), (w, order)          # equal keys by decreasing row
    assert np.array_equal(lc.decision_order(rot[2, 0, :, 11]), [4, 3, 2, 1, 0])
    # the tensor path's order is that rule: the sort equals the kernel on the rows permuted by it, as they lie
    lying = decide_rows(dnet, lc.sort_rows(rot), want[0], case, precision, 0)
    assert all(same_bits(a, b) for a, b in zip(want[1:4], lying))
    assert not same_bits(decide_rows(dnet, rot, want[0], case, precision, 0)[0][:, 0], want[1][:, 0])      # (the order matters to these networks)
    assert_same_bits(decide_fused(dnet, case, precision), want[:4], f"ties {net} {precision}")


# ---------------------------------------------------------------------------------------------------------------- a pair alone
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("net,n", [("1-h50", 5), ("2-h64-wide", 33)])
def test_a_world_alone_equals_the_batch(nets, net, n, precision):
    """Worlds 0, 1 and W - 1 of a W = 64 call equal three W = 1 calls: no atomics, the same bits wherever a pair falls in a job."""
    _, dnet = nets(net)
    W = 64
    case = worlds(W, n, 81, False, seed=600 + n)
    batch = decide_fused(dnet, case, precision)
    assert all(np.all(np.isfinite(x)) for x in batch) and all(reward_branches(batch[0]).values())
    acts, nxt, cur, rob = case
    for w in (0, 1, W - 1):
        alone = decide_fused(dnet, (acts, nxt[w:w + 1], cur[w:w + 1], rob[w:w + 1]), precision)
        assert_same_bits(alone, tuple(x[w:w + 1] for x in batch), f"{net} {precision} n={n} world {w}")


# ---------------------------------------------------------------------------------------------------------------- override, goal, rows as they lie
@pytest.mark.parametrize("precision", PRECISIONS)
def test_fused_with_an_override_column_and_robots_on_their_goal(nets, precision):
    """As test_gpu_value_worlds': a forced action per world, -1 and an index outside the action set (greedy), robots on their goal."""
    _, dnet = nets("1-h50")
    W, A, n = 6, 81, 5
    override = np.array([5, -1, 80, 81, 0, 17], np.int32)
    for on_goal in (False, True):
        case = worlds(W, n, A, False, seed=77, on_goal=on_goal)
        want = decide_tensor(dnet, case, precision, override=override)
        got = decide_fused(dnet, case, precision, override=override)
        assert_same_bits(got, want, f"override on_goal={on_goal}")
        assert got[2][[0, 2, 4, 5]].tolist() == [5, 80, 0, 17]
        assert np.array_equal(got[2][[1, 3]], np.argmax(got[1], axis=1)[[1, 3]])
        if on_goal:
            assert not got[3].any() and np.all((got[0] == 1.0) | (got[0] == F32(-0.25)))
        else:
            rob = case[3]
            there = np.hypot(rob[:, 0] - rob[:, 5], rob[:, 1] - rob[:, 6]) < rob[:, 4]
            assert there.tolist() == [False, False, True, False, False, False]
            np.testing.assert_array_equal(got[3], np.where(there[:, None], F32(0), case[0][got[2]]))
            assert all(reward_branches(got[0]).values())


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("net", ["1-h50", "2-h50"])
def test_rows_as_they_lie(nets, net, precision):
    """sorted_by_distance = 0 equals the tensor entry with 0, and differs from the sorted decision."""
    _, dnet = nets(net)
    case = worlds(5, 7, 7, False, seed=91)
    want = decide_tensor(dnet, case, precision, 0)
    got = decide_fused(dnet, case, precision, 0)
    assert_same_bits(got, want, f"unsorted {net} {precision}")
    assert not same_bits(got[1], decide_fused(dnet, case, precision, 1)[1])


# ---------------------------------------------------------------------------------------------------------------- the Gym, predict
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("network", [1, 2])
@pytest.mark.parametrize("query_env", [True, False])
def test_the_env_decides_the_same_with_either_input(network, query_env, precision):
    """64 resident worlds x 5 humans, five act -> step rounds: act_device with ``set_recurrent_input("fused")`` leaves the actions, values and
    choices of ``"tensor"``.  A fused decision allocates less than one look-ahead tensor (W * 81 * n * 13 * 4 bytes: derived, the tensor's
    own size) and the tensor path, measured the same way, at least that (it allocates the tensor)."""
    import torch

    env = _batched(5, W=64)
    pol = _ready(seeded_policy(network, 13, 3300 + network, action_space__query_env=str(query_env).lower()), env)
    pol.set_recurrent_precision(precision)
    assert pol.recurrent_input == "tensor"
    rot_bytes = env.W * 81 * env.n * 13 * 4

    def decide(how):
        pol.set_recurrent_input(how)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        act = env.act_device(pol)
        assert act is env.action_buffer()
        torch.cuda.synchronize()
        grown = torch.cuda.max_memory_allocated() - before
        values, choice = env.last_values_device()
        return act.cpu().numpy().copy(), values.cpu().numpy().copy(), choice.cpu().numpy().copy(), grown

    for k in range(5):
        a_t, v_t, c_t, grown_t = decide("tensor")
        a_f, v_f, c_f, grown_f = decide("fused")
        assert np.all(np.isfinite(v_t)) and np.all(np.isfinite(v_f)) and np.all(np.isfinite(a_f))
        assert np.array_equal(v_f.view(np.int32), v_t.view(np.int32)), (k, int(np.sum(v_f != v_t)))
        assert np.array_equal(c_f, c_t) and np.array_equal(a_f.view(np.int32), a_t.view(np.int32)), k
        print(f"network {network} {precision} query_env={query_env} round {k}: a decision allocates {grown_t} bytes (tensor), {grown_f} bytes (fused); "
              f"rot is {rot_bytes}")
        if k > 0:                       # (the first round also allocates what stays: the values and choices of last_values_device)
            assert grown_f < rot_bytes <= grown_t, (k, grown_f, grown_t, rot_bytes)
        env.step_device(env.action_buffer())
    assert (pol.decision_input, pol.decision_precision, pol.recurrent_precision) == ("tensor", "f32", precision)
    env.close()


def _state(rob, cur):
    from social_navigation_pyenvs_amd.crowd_nav.utils.state import FullState, JointState, ObservableState

    return JointState(FullState(*[float(x) for x in rob]), [ObservableState(*[float(x) for x in h]) for h in cur])


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("network", [1, 2])
def test_predict_with_either_input(network, precision):
    """The W = 1 ``predict`` on one synthetic world, test and train phase: the action and the 81 action values of "fused" are those of
    "tensor", bit for bit; the training phase's ``last_state`` (``transform``: it never read the decision's rows) is the same tensor."""
    import torch

    pol = _ready(seeded_policy(network, 13, 3400 + network))
    pol.set_recurrent_precision(precision)
    pol.time_step, pol.query_env = DT, True
    pol.build_action_space(1.0)
    _, nxt, cur, rob = worlds(2, 7, 81, False, seed=9)
    state = _state(rob[1], cur[1])
    pol.set_env(_RecordedEnv(nxt[1]))
    got = {}
    for how in ("tensor", "fused"):
        pol.set_recurrent_input(how)
        pol.set_phase("test")
        a = pol.predict(state)
        got[how] = [np.array([a.vx, a.vy], F32), np.asarray(pol.action_values, F32)]
        pol.set_phase("train")
        pol.set_epsilon(0.0)
        b = pol.predict(state)
        got[how] += [np.array([b.vx, b.vy], F32), pol.last_state.cpu().numpy().astype(F32)]
        assert all(np.all(np.isfinite(x)) for x in got[how]) and got[how][1].shape == (81,) and got[how][3].shape == (7, 13)
    for t, f in zip(got["tensor"], got["fused"]):
        assert same_bits(t, f)
    assert same_bits(got["fused"][0], got["fused"][2])
    torch.cuda.synchronize()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("wkey", ["lstm1_13", "lstm2_13"])
def test_g21_through_predict_with_the_fused_input(wkey, precision):
    """Every recorded decision of the reference (golden G21) through the W = 1 ``predict`` with either input: the fused path gives the
    tensor path's action and action values, bit for bit -- the tensor path, which test_gpu_value_lstm[_bf16] hold against the reference, is
    the yardstick."""
    cs = [c for c in lc.g21()["decision"] if c["wkey"] == wkey]
    assert len(cs) >= 20
    pol = _ready(lc.g21_policy(wkey))
    pol.set_recurrent_precision(precision)
    pol.time_step = float(cs[0]["dt"])
    pol.build_action_space(float(cs[0]["robot"][7]))
    same = 0
    for k, c in enumerate(cs):
        state = _state(c["robot"], c["obs"])
        pol.set_env(_RecordedEnv(c["next_humans"]))
        seen = {}
        for how in ("tensor", "fused"):
            pol.set_recurrent_input(how)
            a = pol.predict(state)
            seen[how] = (np.array([a.vx, a.vy], F32), np.asarray(pol.action_values, F32))
            assert np.all(np.isfinite(seen[how][1]))
        assert same_bits(seen["fused"][0], seen["tensor"][0]) and same_bits(seen["fused"][1], seen["tensor"][1]), k
        same += int(np.argmax(seen["fused"][1])) == int(c["chosen"])
    print(f"G21 {wkey} {precision}: {len(cs)} decisions, fused = tensor bit for bit; {same} with the reference's action")
