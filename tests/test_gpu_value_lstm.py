"""GPU suite of LSTM-RL: the recurrent decision kernel (cs_value_net_decide_lstm, csrc/value_net_lstm.hip) against the
reference's recorded decisions (golden G21) and lstm_cases' float64 restatement of both networks, its order rule, its shapes and edges, and
the policy and the batched Gym on top of it.

The tolerance of every comparison with the restatement is 4 x E_ref, E_ref being what the test measures on its own inputs: the largest
difference between torch's CPU float32 module and the restatement (neither is the code under test).  Every comparison between two launches
of this library is bitwise (np.array_equal on the int32 views)."""
import copy

import numpy as np
import pytest

import lstm_cases as lc
from value_calls import _stream, _up, decide_call, same_bits

pytestmark = pytest.mark.gpu

F32 = np.float32
DT, GAMMA = 0.25, 0.9
MARGIN = 4.0


def _ready(pol):
    import torch

    pol.set_phase("test")
    pol.set_device(torch.device("cuda"))
    pol.time_step = DT
    return pol


def device_net(pol):
    from social_navigation_pyenvs_amd.crowd_nav.policy.value_net import DeviceNet

    net = DeviceNet(pol.model, pol.joint_state_dim)
    net.refresh()
    return net


def restated(model, rot, rew, vpref, gamma=GAMMA, dt=DT, sort=True):
    """(action values [W, A] of the float64 restatement, E_ref) on rot [W, A, n, cols] (float32 values): the rows in the decision's order
    when `sort`, the network by both the restatement and torch's CPU float32 module, reward + gamma^(dt v_pref) V"""
    rows = np.asarray(rot, F32).astype(np.float64)
    rows = lc.sort_rows(rows) if sort else rows
    v64 = lc.forward64(lc.weights64(model), rows)
    e_ref = float(np.max(np.abs(lc.torch_values(copy.deepcopy(model).cpu(), rows) - v64)))
    disc = np.power(float(gamma), dt * np.asarray(vpref, np.float64))
    return np.asarray(rew, np.float64) + disc[:, None] * v64, e_ref


def random_case(seed, W, A, n, cols):
    """rows with distinct positive distances, rewards, an action table and robot rows far from their goals"""
    rng = np.random.default_rng(seed)
    rot = rng.uniform(-2.0, 2.0, (W, A, n, cols)).astype(F32)
    da = (0.4 + 0.05 * rng.permuted(np.tile(np.arange(n), (W, A, 1)), axis=2) + rng.uniform(0, 0.02, (W, A, n))).astype(F32)
    rot[..., 11] = da
    rew = rng.uniform(-0.25, 1.0, (W, A)).astype(F32)
    acts = rng.uniform(-1.0, 1.0, (A, 2)).astype(F32)
    rob = np.tile(np.array([0, 0, 0, 0, 0.3, 5, 5, 1.0, 0], F32), (W, 1))
    rob[:, 7] = rng.uniform(0.5, 1.5, W).astype(F32)
    return rot, rew, acts, rob


def seeded_policy(network, cols, seed, **overrides):
    pol = lc.lstm_policy(network, cols, **overrides)
    lc.draw_weights(pol.model, seed, calm_last=True)
    return pol


# ---------------------------------------------------------------------------------------------------------------- golden G21
class _RecordedEnv:
    """What predict() asks its env for: the next human states the reference's env handed to its policy"""

    def __init__(self, nxt):
        self.motion_model_manager = self
        self._nxt = np.asarray(nxt, np.float64)

    def get_next_human_observable_states(self, dt, theta_and_omega_visible=False):
        return self._nxt


@pytest.mark.parametrize("wkey", ["lstm1_13", "lstm2_13"])
def test_g21_decisions_are_the_references(wkey):
    """Every recorded decision of the reference, W = 1 through predict and all of them stacked as one batch through decide_for_worlds: the
    reference's choice for ALL decisions, the 81 action values within 4 x E_ref of the float64 restatement.
    Measured on the MI355X: network 1 kernel 1.69e-5 against E_ref 1.81e-5 (ratio 0.93), network 2 4.93e-5 against 7.84e-5
    (0.63)."""
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net
    from social_navigation_pyenvs_amd.crowd_nav.utils.state import FullState, JointState, ObservableState

    cs = [c for c in lc.g21()["decision"] if c["wkey"] == wkey]
    assert len(cs) >= 20
    pol = _ready(lc.g21_policy(wkey))
    acts = cs[0]["action_space"].astype(F32)
    assert all(np.array_equal(c["action_space"], cs[0]["action_space"]) for c in cs)
    pol.action_space_ndarray = cs[0]["action_space"]
    nxt, cur, rob = (np.stack([c[k] for c in cs]).astype(F32) for k in ("next_humans", "obs", "robot"))
    W, A = len(cs), len(acts)
    vals = torch.full((W, A), np.nan, device="cuda")
    pick = torch.full((W,), -5, dtype=torch.int32, device="cuda")
    act = torch.full((W, 2), np.nan, device="cuda")
    net = pol.device_net()
    rot, rew = value_net.decide_for_worlds(net, pol.decision_input, pol.decision_precision, _up(acts), _up(nxt), _up(cur), _up(rob), float(cs[0]["gamma"]),
                                           float(cs[0]["dt"]), None, vals, pick, act, _stream())
    torch.cuda.synchronize()
    vals, pick, act = vals.cpu().numpy(), pick.cpu().numpy(), act.cpu().numpy()
    want, e_ref = restated(pol.model, rot.cpu().numpy(), rew.cpu().numpy(), rob[:, 7], float(cs[0]["gamma"]), float(cs[0]["dt"]))
    err = float(np.max(np.abs(vals.astype(np.float64) - want)))
    ref_err = float(np.max(np.abs(np.stack([c["action_values"] for c in cs]) - want)))
    print(f"{wkey}: {W} decisions, E_ref {e_ref:.3e}, kernel against the restatement {err:.3e} (ratio {err / e_ref:.2f}), the reference's recorded values "
          f"against it {ref_err:.3e}")
    assert np.array_equal(pick, np.array([c["chosen"] for c in cs]))
    assert np.array_equal(act, np.stack([c["action"] for c in cs]).astype(F32))
    assert err <= MARGIN * e_ref, (err, e_ref)
    # W = 1 through predict: the bits of the batch
    pol.time_step = float(cs[0]["dt"])
    pol.build_action_space(float(cs[0]["robot"][7]))
    assert np.array_equal(np.asarray(pol.action_space_ndarray, F32), acts)
    for k, c in enumerate(cs):
        state = JointState(FullState(*[float(x) for x in c["robot"]]), [ObservableState(*[float(x) for x in h]) for h in c["obs"]])
        pol.set_env(_RecordedEnv(c["next_humans"]))
        a = pol.predict(state)
        assert (F32(a.vx), F32(a.vy)) == (act[k, 0], act[k, 1]) and same_bits(np.asarray(pol.action_values, F32), vals[k]), k


# ---------------------------------------------------------------------------------------------------------------- the order
def test_ties_and_sorted_sequences_follow_the_order_rule():
    """Two and three humans at bit-equal distances on different sides of the robot, a sequence already in order and one reversed: the
    kernel's sort equals the kernel on the rows permuted by the rule (bitwise), and the restatement on them (4 x E_ref)."""
    pol = seeded_policy(1, 13, 31)
    net = device_net(pol)
    rot, rew, acts, rob = random_case(5, 1, 6, 5, 13)
    d = F32(1.25)
    rot[0, 0, [1, 3], 11] = d                                   # two humans tied, (px, py) on opposite sides
    rot[0, 0, 1, 6:8], rot[0, 0, 3, 6:8] = (d, 0), (-d, 0)
    rot[0, 1, [0, 2, 4], 11] = d                                # three tied
    rot[0, 1, 0, 6:8], rot[0, 1, 2, 6:8], rot[0, 1, 4, 6:8] = (d, 0), (0, d), (-d, 0)
    rot[0, 2, :, 11] = F32(0.5)                                 # all tied: the humans in reverse
    rot[0, 3] = rot[0, 3][np.argsort(-rot[0, 3, :, 11], kind="stable")]        # already in order
    rot[0, 4] = rot[0, 4][np.argsort(rot[0, 4, :, 11], kind="stable")]         # reversed
    assert np.array_equal(lc.decision_order(rot[0, 0, :, 11])[[k for k in range(5) if rot[0, 0, lc.decision_order(rot[0, 0, :, 11])[k], 11] == d]], [3, 1])
    assert np.array_equal(lc.decision_order(rot[0, 2, :, 11]), [4, 3, 2, 1, 0])
    assert np.array_equal(lc.decision_order(rot[0, 3, :, 11]), np.arange(5)) and np.array_equal(lc.decision_order(rot[0, 4, :, 11]), np.arange(5)[::-1])
    got = decide_call(net, rot, rew, acts, rob, 1)
    permuted = lc.sort_rows(rot)
    lying = decide_call(net, permuted, rew, acts, rob, 0)
    assert all(same_bits(a, b) for a, b in zip(got, lying))
    # rows already in order, no two distances equal: the sort changes nothing (tied rows would swap again, by the rule)
    assert same_bits(decide_call(net, permuted, rew, acts, rob, 1)[0][:, 3:], lying[0][:, 3:])
    want, e_ref = restated(pol.model, rot, rew, rob[:, 7])
    assert float(np.max(np.abs(got[0] - want))) <= MARGIN * e_ref
    unsorted, _ = restated(pol.model, rot, rew, rob[:, 7], sort=False)
    assert float(np.max(np.abs(unsorted - want))) > 100 * e_ref                                            # (the order matters to this network)


# ---------------------------------------------------------------------------------------------------------------- shapes
WIDE_MLP1 = dict(lstm_rl__mlp1_dims="60, 50")
SHAPES = [
    # network, cols, H, n, W, A, overrides: every n of {1, 2, 5, 33, 64}, W * A of {1, 31, 32, 33, 243}, H of {8, 33, 50, 64}, both column
    # counts and networks, mlp widths that are no multiple of 32, and each of the kernel's four builds
    (1, 13, 50, 5, 3, 81, {}),                                                       # the default: register-resident weights, 243 sequences
    (1, 15, 8, 1, 1, 1, dict(lstm_rl__mlp2_dims="1")),                               # one human, one sequence, one block, one layer
    (1, 13, 33, 2, 31, 1, dict(lstm_rl__mlp2_dims="70, 33, 1")),                     # H and widths off the tile
    (1, 13, 64, 33, 1, 32, {}),                                                      # 8 blocks x 10 k-groups: the widest register-resident LSTM
    (1, 15, 96, 64, 3, 11, dict(lstm_rl__mlp2_dims="40, 1")),                        # 12 blocks: weights from the blob; the one-block world size
    (2, 13, 50, 5, 33, 1, {}),                                                       # network 2's default: 14 k-groups in registers
    (2, 15, 33, 5, 3, 81, dict(lstm_rl__mlp1_dims="40, 20", lstm_rl__mlp2_dims="70, 1")),
    (2, 13, 64, 2, 31, 1, WIDE_MLP1),                                                # 8 + 7 k-groups: network 2 with weights from the blob
]


@pytest.mark.parametrize("network,cols,H,n,W,A,overrides", SHAPES)
def test_shapes_against_the_restatement(network, cols, H, n, W, A, overrides):
    pol = seeded_policy(network, cols, 100 + H + n, lstm_rl__global_state_dim=H, **overrides)
    net = device_net(pol)
    rot, rew, acts, rob = random_case(7 * n + W, W, A, n, cols)
    vals, pick, act = decide_call(net, rot, rew, acts, rob, 1)
    want, e_ref = restated(pol.model, rot, rew, rob[:, 7])
    if W * A < 64:                      # E_ref of a handful of sequences is a draw, not a bound: 64 more rows of the same shape and distribution
        more = random_case(7 * n + W + 1000, 1, 64, n, cols)
        e_ref = max(e_ref, restated(pol.model, more[0], more[1], more[3][:, 7])[1])
    err = float(np.max(np.abs(vals - want)))
    print(f"network {network}, {cols} columns, H {H}, n {n}, {W} x {A}: E_ref {e_ref:.3e}, kernel {err:.3e} (ratio {err / e_ref:.2f})")
    assert np.all(np.isfinite(vals)) and err <= MARGIN * e_ref, (err, e_ref)
    assert np.array_equal(pick, np.argmax(vals, axis=1)) and same_bits(act, acts[pick])


def test_the_shapes_cover_the_issues_edges():
    assert {s[3] for s in SHAPES} >= {1, 2, 5, 33, 64} and {s[4] * s[5] for s in SHAPES} >= {1, 31, 32, 33, 243}
    assert {s[2] for s in SHAPES} >= {8, 33, 50, 64} and {s[1] for s in SHAPES} == {13, 15} and {s[0] for s in SHAPES} == {1, 2}


# ---------------------------------------------------------------------------------------------------------------- bit equality
@pytest.mark.parametrize("network,H,overrides", [(1, 50, {}), (2, 64, WIDE_MLP1)])
def test_a_pair_alone_gives_the_bits_of_the_batch(network, H, overrides):
    """A (world, action) alone, W = A = 1, and the same rows at two positions of a larger batch (another tile, another lane)."""
    pol = seeded_policy(network, 13, 77, lstm_rl__global_state_dim=H, **overrides)
    net = device_net(pol)
    rot, rew, acts, rob = random_case(3, 3, 27, 5, 13)
    rot[2, 20], rew[2, 20], rob[2] = rot[0, 4], rew[0, 4], rob[0]       # the pair again, 70 sequences on: the third tile
    batch = decide_call(net, rot, rew, acts, rob, 1)[0]
    alone = decide_call(net, rot[:1, 4:5], rew[:1, 4:5], acts[4:5], rob[:1], 1)[0]
    assert same_bits(alone[0, :1], batch[0, 4:5]) and same_bits(alone[0, :1], batch[2, 20:21])


# ---------------------------------------------------------------------------------------------------------------- override, goal
def test_forced_actions_and_the_goal_behave_as_in_cs_value_net_decide():
    pol = seeded_policy(1, 13, 55)
    net = device_net(pol)
    rot, rew, acts, rob = random_case(9, 4, 7, 5, 13)
    rob[3, 5:7] = rob[3, 0:2] + F32(0.1)                                # within its radius (0.3) of the goal
    free = decide_call(net, rot, rew, acts, rob, 1)
    forced = decide_call(net, rot, rew, acts, rob, 1, override=np.array([5, -1, 99, 2], np.int32))
    assert same_bits(free[0], forced[0])
    greedy = np.argmax(free[0], axis=1)
    assert np.array_equal(free[1], greedy) and np.array_equal(forced[1], [5, greedy[1], greedy[2], 2])      # an index outside 0..A-1 is greedy
    assert same_bits(forced[2][:3], acts[forced[1][:3]]) and np.array_equal(forced[2][3], [0, 0]) and np.array_equal(free[2][3], [0, 0])


# ---------------------------------------------------------------------------------------------------------------- the Gym
def test_the_batched_gym_decides_and_evaluates_with_lstm_rl():
    """W = 4 device-reset worlds x 5 humans: act_device is lookahead + decide_lstm by hand and four predict calls, bitwise; value_device,
    joint_state_device and state_value are the module on transform's unsorted rows, also with a deep-copied model=; explore= forces."""
    import torch

    from test_gpu_value_policy import _PeekedEnv, _batched

    from social_navigation_pyenvs_amd.crowd_nav.utils.state import FullState, JointState, ObservableState

    env = _batched(5, W=4)
    for _ in range(3):
        env.step_device(env.act_device("sfm_helbing"))
    pol = _ready(seeded_policy(1, 13, 91))
    pol.time_step = env.robot_time_step
    act = env.act_device(pol).clone()
    values, choice = (t.clone() for t in env.last_values_device())
    torch.cuda.synchronize()
    rot, rew = env.lookahead_device(pol.action_space_ndarray)
    _, _, rob = env._worlds_on_side_stream(env._device_loop_state(), peek=False)
    torch.cuda.synchronize()
    acts = np.asarray(pol.action_space_ndarray, F32)
    want = decide_call(pol.device_net(), rot.cpu().numpy(), rew.cpu().numpy(), acts, rob.cpu().numpy(), 1, gamma=pol.gamma, dt=env.robot_time_step)
    assert same_bits(values.cpu().numpy(), want[0]) and np.array_equal(choice.cpu().numpy(), want[1]) and same_bits(act.cpu().numpy(), want[2])
    ref, e_ref = restated(pol.model, rot.cpu().numpy(), rew.cpu().numpy(), rob[:, 7].cpu().numpy(), pol.gamma, env.robot_time_step)
    assert float(np.max(np.abs(want[0] - ref))) <= MARGIN * e_ref

    robot, obs, peek = env.cw.d_robot.download(), env.observe_device().cpu().numpy(), env.cw.peek(env.robot_time_step)
    target = copy.deepcopy(pol.model)
    with torch.no_grad():
        for prm in target.parameters():
            prm.mul_(0.5)
    rows = env.joint_state_device(pol)
    v, rows2 = env.value_device(pol, with_state=True)
    vt = env.value_device(pol, model=target)
    torch.cuda.synchronize()
    assert tuple(rows.shape) == (4, 5, 13) and same_bits(rows.cpu().numpy(), rows2.cpu().numpy())
    for mod, got in ((pol.model, v), (target, vt)):
        v64 = lc.forward64(lc.weights64(mod), rows.cpu().numpy().astype(np.float64))
        e = float(np.max(np.abs(lc.torch_values(copy.deepcopy(mod).cpu(), rows.cpu().numpy()) - v64)))
        assert float(np.max(np.abs(got.cpu().numpy() - v64))) <= MARGIN * e
    for w in range(4):
        r = robot[w]
        state = JointState(FullState(*[float(x) for x in (r[0], r[1], r[3], r[4], r[8], r[10], r[11], r[12], r[2])]),
                           [ObservableState(*[float(x) for x in h]) for h in obs[w]])
        pol.set_env(_PeekedEnv(peek[w][:, :6]))
        a = pol.predict(state)
        assert (F32(a.vx), F32(a.vy)) == (act[w, 0].item(), act[w, 1].item()) and same_bits(np.asarray(pol.action_values, F32), values[w].cpu().numpy())
        assert same_bits(pol.transform(state).cpu().numpy(), rows[w].cpu().numpy()) or \
            float((pol.transform(state).cpu() - rows[w].cpu()).abs().max()) <= 1e-5          # (torch's rotate against the kernel's: rounding)
        assert F32(pol.state_value(state)) == v[w].item() and F32(pol.state_value(state, model=target)) == vt[w].item()
    forced = torch.tensor([3, -1, 80, -1], dtype=torch.int32, device="cuda")
    env.act_device(pol, explore=forced)
    torch.cuda.synchronize()
    _, picked = env.last_values_device()
    assert np.array_equal(picked.cpu().numpy(), [3, want[1][1], 80, want[1][3]])
    with pytest.raises(TypeError, match="no-train policy"):
        env.act_step_device(pol)
    env.close()
