"""GPU suite of the value-based robot policies (crowd_nav.policy CADRL / SARL on csrc/value_net.hip): the batched decision pinned on the
reference's recorded decisions (golden G16), the kernel against the torch float32 forward of the same module on the same device, the
W = 1 ``predict`` against the batch bit for bit, and the edges (goal reached, forced actions, 1 and 70 humans, the act -> step loop).

The bars are the ones tests/test_policy_seam.py holds the project to: the chosen action equal in >= 99 % of the decisions, any other pick
within 1e-4 of the best value relative to the decision's largest |value| (floor 1), every action value within 1e-4 on that scale."""
import configparser

import numpy as np
import pytest

import parity_util
from test_policy_seam import _groups
from test_value_policy_cpu import fixture_state_dict, make_policy, seeded_weights

pytestmark = pytest.mark.gpu

REL_BAR = 1e-4


def _batched(n, W=4096, headed=False, model="sfm_guo"):
    from test_gpu_generators import _config

    from social_navigation_pyenvs_amd.social_gym.social_nav_gym import BatchedSocialNavGym

    env = BatchedSocialNavGym(_config("hybrid_scenario", human_num=n, policy=model), W, headed_obs=headed)
    env.reset(phase="test", first_case=11, device=True)
    return env


def _ready(pol, env=None):
    import torch

    pol.set_phase("test")
    pol.set_device(torch.device("cuda"))
    if env is not None:
        pol.time_step = env.robot_time_step
    return pol


def _calm(pol):
    """Scale the attention's last layer by 0.1: scores stay far below 88, so the published softmax (no maximum subtraction) overflows nowhere."""
    import torch

    last = [m for m in pol.model.attention if isinstance(m, torch.nn.Linear)][-1]
    with torch.no_grad():
        last.weight.mul_(0.1)
        last.bias.mul_(0.1)


def _torch_values(pol, rot, rew, robot_vpref, gamma, dt, chunk=256):
    """The baseline forward: policy.model in float32 under no_grad on the look-ahead rows [W, A, n, cols] -> action values [W, A]."""
    import torch

    W, A, n, cols = rot.shape
    out = torch.empty((W, A), dtype=torch.float32, device=rot.device)
    with torch.no_grad():
        for w0 in range(0, W, chunk):
            x = rot[w0:w0 + chunk].reshape(-1, n, cols)
            v = pol.model(x)[..., 0].min(dim=-1).values if pol.name == "CADRL" else pol.model(x)[:, 0]
            out[w0:w0 + chunk] = v.view(-1, A)
    disc = torch.pow(torch.as_tensor(gamma, dtype=torch.float64, device=rot.device), dt * robot_vpref.double()).float()
    return rew + disc[:, None] * out


def _compare(values, choice, ref, label, need_all=False):
    """Kernel values / choices [W, A], [W] against reference values: (worst relative value error, same picks, total).  The published
    masked softmax has no maximum subtraction: where the reference forward itself overflows (exp of a score beyond 88 with untrained
    weights) the kernel must be non-finite in the same places, and those worlds are compared no further."""
    bad = ~np.isfinite(ref)
    np.testing.assert_array_equal(~np.isfinite(values), bad)
    ok = ~bad.any(axis=1)
    # (untrained SARL weights at G16's scale overflow in about half of the 25-human worlds; the `calm` cases -- the attention's last layer
    #  scaled by 0.1 -- overflow nowhere, and there every world is compared)
    assert ok.all() if need_all else ok.sum() >= min(1000, len(ref) // 4), (label, int(ok.sum()), len(ref))
    parity_util.REPORT.setdefault("value policy: worlds compared / worlds where the reference forward overflows", {})[label] = [int(ok.sum()), int((~ok).sum())]
    values, choice, ref = values[ok], choice[ok], ref[ok]
    scale = np.maximum(1.0, np.max(np.abs(ref), axis=1))
    worst = float(np.max(np.max(np.abs(values - ref), axis=1) / scale))
    best = np.argmax(ref, axis=1)
    same = int(np.sum(best == choice))
    rows = np.arange(len(ref))
    gap = np.abs(ref[rows, choice] - ref[rows, best]) / scale
    print(f"{label}: {len(ref)} worlds compared ({int((~ok).sum())} more where the reference forward overflows), worst relative action-value "
          f"error {worst:.3e}, same pick {same}/{len(ref)}, worst gap of another pick {float(gap.max()):.3e}")
    assert np.all(gap <= REL_BAR), (label, float(gap.max()))
    return worst, same, len(ref)


def test_g16_batched_decisions_are_the_references():
    """Each recorded decision of the reference's CADRL / SARL is one world of a batch (set up as test_policy_seam does); the policy carries
    the fixture's weights and act_device decides.

    Measured on the MI355X: 135 / 135 decisions with the reference's action; worst relative action-value error 3.1e-5 (SARL, 5 humans;
    CADRL 6.7e-6, SARL with 10 humans 4.8e-6) against the bar of 1e-4 -- the torch float32 forward on the CPU sits at 2.9e-5 itself."""
    from social_navigation_pyenvs_amd.social_gym.social_nav_gym import BatchedSocialNavGym

    groups, w = _groups()
    total = same = 0
    worst = 0.0
    for key, cs in groups.items():
        c0 = cs[0]
        W, n = len(cs), int(c0["mm_states"].shape[0])
        scen = {"circular_crossing": "circle_crossing"}.get(str(c0["scenario"]), str(c0["scenario"]))
        cfg = configparser.RawConfigParser()
        cfg.read_dict({
            "env": {"time_limit": 50, "time_step": float(c0["substep"]), "robot_time_step": float(c0["dt"]), "val_size": 100, "test_size": 500, "randomize_attributes": "false"},
            "reward": {"success_reward": 1, "collision_penalty": -0.25, "discomfort_dist": 0.2, "discomfort_penalty_factor": 0.5},
            "sim": {"train_val_sim": scen, "test_sim": scen, "square_width": 10, "circle_radius": 7, "human_num": n, "traffic_length": 14, "traffic_height": 3},
            "humans": {"visible": "true", "policy": str(c0["model"]), "radius": 0.3, "v_pref": 1, "sensor": "coordinates"},
            "robot": {"visible": "false", "policy": "none", "radius": 0.3, "v_pref": 1, "sensor": "coordinates"},
        })
        env = BatchedSocialNavGym(cfg, W)
        env.reset(phase="test", first_case=0, device=True)
        cw = env.cw
        S = np.stack([c["mm_states"][:n] for c in cs]).astype(np.float32)
        G = np.full((W, n, cw.G, 2), np.nan, np.float32)
        for k, c in enumerate(cs):
            g = np.asarray(c["mm_goals"], np.float32)[:n]
            G[k, :, :min(cw.G, g.shape[1])] = g[:, :cw.G]
        R = np.zeros((W, 13), np.float32)
        for k, c in enumerate(cs):
            R[k, [0, 1, 3, 4, 8, 10, 11, 12, 2]] = c["robot"]
            R[k, 9] = 80.0
        cw.set_states(S); cw.set_goals(G); cw.set_robot(R)
        pol = _ready(make_policy(str(c0["policy"])), env)
        pol.model.load_state_dict(fixture_state_dict(w[key]), strict=True)
        pol.gamma = float(c0["gamma"])
        pol.build_action_space(float(c0["robot"][7]))
        np.testing.assert_allclose(pol.action_space_ndarray, c0["action_space"], atol=1e-12)
        act = env.act_device(pol).cpu().numpy()
        values, choice = (t.cpu().numpy() for t in env.last_values_device())
        ref = np.stack([np.asarray(c["action_values"], np.float64) for c in cs])
        np.testing.assert_array_equal(choice, np.argmax(values, axis=1))                  # the kernel's pick is the first maximum of its own values
        np.testing.assert_array_equal(act, pol.action_space_ndarray.astype(np.float32)[choice])
        wv, s, t = _compare(values.astype(np.float64), choice, ref, f"G16 {key}")
        assert [int(np.argmax(r)) for r in ref] == [int(c["chosen"]) for c in cs]
        worst, same, total = max(worst, wv), same + s, total + t
        env.close()
    parity_util.record("g16 value policy: act_device(CADRL / SARL) against the reference's recorded action values (relative)", worst, bar=REL_BAR)
    print(f"G16: {same}/{total} decisions with the reference's action, worst relative action-value error {worst:.3e}")
    assert total >= 100 and same >= 0.99 * total, (same, total)
    assert worst < REL_BAR, worst


VARIANTS = [
    ("cadrl", {}, 5, False, False),
    ("cadrl", {}, 25, False, False),
    ("sarl", {}, 5, False, False),
    ("sarl", {}, 25, False, False),
    ("sarl", {}, 25, False, True),           # calm attention: all 4096 worlds finite, all compared
    ("sarl", {}, 5, False, True),
    ("cadrl", dict(cadrl__mlp_dims="64, 37, 1"), 5, False, False),
    ("sarl", dict(sarl__with_global_state="false"), 5, False, False),
    ("sarl", dict(sarl__mlp1_dims="40, 72", sarl__mlp2_dims="33", sarl__attention_dims="20, 1", sarl__mlp3_dims="90, 1"), 25, False, False),
    ("sarl", dict(sarl__with_theta_and_omega_visible="true"), 5, True, False),
    ("cadrl", dict(sarl__with_theta_and_omega_visible="true", cadrl__mlp_dims="256, 200, 1"), 5, True, False),
]


@pytest.mark.parametrize("name,overrides,n,headed,calm", VARIANTS)
def test_kernel_against_the_torch_forward_on_4096_worlds(name, overrides, n, headed, calm):
    """act_device's [W, 81] values against the torch float32 forward of policy.model on lookahead_device's output (same device, same rows)."""
    import torch

    env = _batched(n, headed=headed, model="hsfm_farina" if headed else "sfm_guo")
    for _ in range(3):
        env.step_device(env.act_device("sfm_helbing"))
    pol = _ready(make_policy(name, **overrides), env)
    seeded_weights(pol.model, 1700 + n)
    if calm:
        _calm(pol)
    act = env.act_device(pol).clone()
    values, choice = (t.clone() for t in env.last_values_device())
    rot, rew = env.lookahead_device(pol.action_space_ndarray)
    assert rot.shape == (env.W, 81, n, 15 if headed else 13)
    vpref = env.cw.d_robot.torch().view(env.W, 13)[:, 12]
    ref = _torch_values(pol, rot, rew, vpref, pol.gamma, env.robot_time_step)
    label = f"{name} {overrides or 'default'} n={n}{' headed' if headed else ''}{' calm' if calm else ''}"
    worst, same, total = _compare(values.cpu().numpy().astype(np.float64), choice.cpu().numpy(), ref.cpu().numpy().astype(np.float64), label,
                                  need_all=calm or name == "cadrl")
    parity_util.record("value policy kernel against the torch float32 forward, 4096 worlds (relative action value)", worst, bar=REL_BAR)
    assert worst < REL_BAR and same >= 0.99 * total, (worst, same, total)
    np.testing.assert_array_equal(choice.cpu().numpy(), torch.argmax(values, dim=1).cpu().numpy())
    acts32 = pol.action_space_ndarray.astype(np.float32)
    np.testing.assert_array_equal(act.cpu().numpy(), acts32[choice.cpu().numpy()])         # (no robot is at its goal after three steps)
    env.close()


class _PeekedEnv:
    """What predict() asks its env for: the crowd's own one-step look-ahead of ONE world, as the batch's cs_peek computed it."""

    def __init__(self, nxt):
        self.motion_model_manager = self
        self._nxt = nxt

    def get_next_human_observable_states(self, dt, theta_and_omega_visible=False):
        return self._nxt.astype(np.float64) if theta_and_omega_visible else self._nxt[:, [0, 1, 3, 4]].astype(np.float64)


@pytest.mark.parametrize("name,n,headed", [("cadrl", 5, False), ("sarl", 5, False), ("cadrl", 25, False), ("sarl", 25, False), ("sarl", 5, True)])
def test_w1_predict_equals_the_batch_bit_for_bit(name, n, headed):
    from social_navigation_pyenvs_amd.crowd_nav.utils.state import FullState, JointState, ObservableState, ObservableStateHeaded

    env = _batched(n, headed=headed, model="hsfm_farina" if headed else "sfm_guo")
    W = env.W
    for _ in range(3):
        env.step_device(env.act_device("sfm_helbing"))
    pol = _ready(make_policy(name, **(dict(sarl__with_theta_and_omega_visible="true") if headed else {})), env)
    seeded_weights(pol.model, 1800 + n)
    act = env.act_device(pol).cpu().numpy().copy()
    values, choice = (t.cpu().numpy().copy() for t in env.last_values_device())
    robot = env.cw.d_robot.download()
    obs = env.observe_device().cpu().numpy()
    peek = env.cw.peek(env.robot_time_step)
    rows = np.unique(np.r_[0, W - 1, np.random.default_rng(n).choice(W, 398, replace=False)])
    for w in rows:
        r = robot[w]
        humans = [ObservableStateHeaded(*[float(x) for x in h]) if headed else ObservableState(*[float(x) for x in h]) for h in obs[w]]
        state = JointState(FullState(*[float(x) for x in (r[0], r[1], r[3], r[4], r[8], r[10], r[11], r[12], r[2])]), humans)
        pol.set_env(_PeekedEnv(peek[w][:, :6]))
        a = pol.predict(state)
        assert np.float32(a.vx) == act[w, 0] and np.float32(a.vy) == act[w, 1], (w, a, act[w])
        assert len(pol.action_values) == 81
        np.testing.assert_array_equal(np.asarray(pol.action_values, np.float32), values[w])
    if name == "sarl":
        aw = pol.get_attention_weights()
        assert aw.shape == (n,) and abs(float(aw.sum()) - 1.0) < 1e-5
    env.close()


WIDE = dict(sarl__mlp1_dims="256, 256", sarl__mlp2_dims="256, 256", sarl__attention_dims="256, 256, 1", sarl__mlp3_dims="256, 256, 1")


@pytest.mark.parametrize("name,n,overrides", [("cadrl", 1, {}), ("sarl", 1, {}), ("cadrl", 70, {}), ("sarl", 70, {}), ("sarl", 64, {}), ("sarl", 65, {}),
                                              ("cadrl", 33, {}), ("sarl", 7, {}), ("sarl", 1, WIDE), ("sarl", 2, WIDE), ("sarl", 40, WIDE),
                                              ("cadrl", 3, dict(cadrl__mlp_dims="256, 256, 256, 1"))])
def test_any_number_of_humans_on_synthetic_rows(name, n, overrides):
    """The kernel alone on random look-ahead rows: n = 1, n beyond one 32-row tile (chunks of a group), group sizes that leave a tile partly
    empty, and the widest networks the entry point takes (every width 256: the largest LDS maps, at 1 and 2 humans).  Reference: the torch
    float32 forward, SARL with the calm attention layer so that every world is compared.  And a world alone (W = 1) equals the same world inside
    the batch, bit for bit.  (1 and 70 humans run here through value_net.decide on synthetic rows, not through act_device: the device
    generators place 5 - 50 humans.)"""
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    W, A = 37, 81
    pol = _ready(make_policy(name, **overrides))
    seeded_weights(pol.model, 1900 + n)
    if overrides:                       # 256-wide layers at N(0, 0.25) blow the activations up: the default init's scale instead
        with torch.no_grad():
            for prm in pol.model.parameters():
                prm.mul_(0.25)
    if name == "sarl":
        _calm(pol)
    pol.build_action_space(1.0)
    g = torch.Generator(device="cuda").manual_seed(n)
    rot = torch.randn((W, A, n, 13), generator=g, device="cuda")
    rot[..., :6] = rot[:, :, :1, :6]                      # the self state is the same in every human's row of a (world, action)
    rew = torch.randn((W, A), generator=g, device="cuda") * 0.1
    rob = torch.rand((W, 9), generator=g, device="cuda") + 1.0      # far from the goal: |p - g| vs radius is tested elsewhere
    rob[:, 4] = 0.01
    acts = torch.as_tensor(pol.action_space_ndarray.astype(np.float32), device="cuda")
    net = pol.device_net()

    def run(lo, hi):
        k = hi - lo
        vals = torch.zeros((k, A), device="cuda")
        pick = torch.zeros(k, dtype=torch.int32, device="cuda")
        act = torch.zeros((k, 2), device="cuda")
        value_net.decide(net, k, A, n, rot[lo:hi].contiguous().data_ptr(), rew[lo:hi].contiguous().data_ptr(), acts.data_ptr(),
                         rob[lo:hi].contiguous().data_ptr(), 9, 0.9, 0.25, None, vals.data_ptr(), pick.data_ptr(), act.data_ptr(),
                         torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return vals.cpu().numpy(), pick.cpu().numpy(), act.cpu().numpy()

    vals, pick, act = run(0, W)
    ref = _torch_values(pol, rot, rew, rob[:, 7], 0.9, 0.25).cpu().numpy().astype(np.float64)
    worst, same, total = _compare(vals.astype(np.float64), pick, ref, f"synthetic {name} n={n}{' wide' if overrides else ''}", need_all=True)
    assert worst < REL_BAR and same >= 0.99 * total
    np.testing.assert_array_equal(act, pol.action_space_ndarray.astype(np.float32)[pick])
    for w in (0, 17, W - 1):
        v1, p1, a1 = run(w, w + 1)
        np.testing.assert_array_equal(v1[0], vals[w])
        assert p1[0] == pick[w] and np.array_equal(a1[0], act[w])


def test_goal_reached_and_forced_actions():
    import torch

    env = _batched(5, W=256)
    pol = _ready(make_policy("sarl"), env)
    seeded_weights(pol.model, 2000)
    R = env.cw.d_robot.download()
    at_goal = np.arange(0, 256, 7)
    R[at_goal, 0] = R[at_goal, 10] + 0.5 * R[at_goal, 8]          # inside the goal radius
    R[at_goal, 1] = R[at_goal, 11]
    env.cw.set_robot(R)
    greedy = env.act_device(pol).cpu().numpy().copy()
    values, choice = (t.cpu().numpy().copy() for t in env.last_values_device())
    acts32 = pol.action_space_ndarray.astype(np.float32)
    others = np.setdiff1d(np.arange(256), at_goal)
    assert not greedy[at_goal].any()                                 # reach_destination: ActionXY(0, 0)
    np.testing.assert_array_equal(greedy[others], acts32[choice[others]])
    explore = torch.full((256,), -1, dtype=torch.int32, device="cuda")
    forced = np.arange(1, 256, 5)
    explore[torch.as_tensor(forced, device="cuda")] = torch.as_tensor((forced % 81).astype(np.int32), device="cuda")
    act = env.act_device(pol, explore=explore).cpu().numpy().copy()
    values2, choice2 = (t.cpu().numpy().copy() for t in env.last_values_device())
    np.testing.assert_array_equal(values2, values)                   # the same observation: the same values, whatever is forced
    np.testing.assert_array_equal(choice2[forced], forced % 81)
    free = np.setdiff1d(np.arange(256), forced)
    np.testing.assert_array_equal(choice2[free], choice[free])
    moving = np.setdiff1d(np.arange(256), at_goal)
    np.testing.assert_array_equal(act[moving], acts32[choice2[moving]])
    assert not act[at_goal].any()
    with pytest.raises(ValueError, match="explore"):
        env.act_device(pol, explore=torch.zeros(256, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="explore"):
        env.act_device("bp", explore=explore)
    env.close()


@pytest.mark.parametrize("name,query_env", [("cadrl", True), ("sarl", False)])
def test_act_step_loop_reads_the_current_observation(name, query_env):
    """64 worlds, 50 Gym steps of act_device -> step_device with auto-reset: at every step the action is what a standalone launch of the
    kernel gives on that step's look-ahead rows, and a robot that was not reset carries the previous action as its velocity."""
    import ctypes as C

    import torch

    from social_navigation_pyenvs_amd import _lib
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    env = _batched(5, W=64)
    pol = _ready(make_policy(name, action_space__query_env=str(query_env).lower()), env)
    seeded_weights(pol.model, 2100)
    ended, act_prev, distinct = 0, None, set()
    for k in range(50):
        act = env.act_device(pol)
        assert act is env.action_buffer()
        values, choice = (t.clone() for t in env.last_values_device())
        rob = env.cw.d_robot.torch().view(env.W, 13).clone()
        if query_env:                                  # the same cs_peek + cs_lookahead, called from outside
            rot, rew = env.lookahead_device(pol.action_space_ndarray)
            net, acts = pol.device_net(), torch.as_tensor(pol.action_space_ndarray.astype(np.float32), device="cuda")
            rob9 = rob[:, [0, 1, 3, 4, 8, 10, 11, 12, 2]].contiguous()
            v = torch.zeros_like(values); p = torch.zeros_like(choice); a = torch.zeros_like(act)
            value_net.decide(net, env.W, 81, env.n, rot.data_ptr(), rew.data_ptr(), acts.data_ptr(), rob9.data_ptr(), 9, pol.gamma,
                             env.robot_time_step, None, v.data_ptr(), p.data_ptr(), a.data_ptr(), torch.cuda.current_stream().cuda_stream)
            np.testing.assert_array_equal(v.cpu().numpy(), values.cpu().numpy())
            np.testing.assert_array_equal(a.cpu().numpy(), act.cpu().numpy())
        else:      # constant-velocity look-ahead built HERE from a clone of the current observation, then cs_lookahead + the kernel standalone
            obs = env.observe_device().clone()
            T = env.robot_time_step
            nxt = torch.stack([obs[..., 0] + obs[..., 2] * T, obs[..., 1] + obs[..., 3] * T, obs[..., 2], obs[..., 3]], -1).contiguous()
            acts = torch.as_tensor(pol.action_space_ndarray.astype(np.float32), device="cuda")
            rob9 = rob[:, [0, 1, 3, 4, 8, 10, 11, 12, 2]].contiguous()
            rot = torch.empty((env.W, 81, env.n, 13), device="cuda"); rew = torch.empty((env.W, 81), device="cuda")
            stream = torch.cuda.current_stream().cuda_stream
            P = C.c_void_p
            _lib.check(_lib.load().cs_lookahead(C.c_int(env.W), C.c_int(env.n), C.c_int(81), C.c_int(0), P(acts.data_ptr()), P(nxt.data_ptr()),
                                                P(obs.data_ptr()), P(rob9.data_ptr()), C.c_int(9), C.c_float(T), P(rot.data_ptr()), P(rew.data_ptr()), P(stream)))
            v = torch.zeros_like(values); p = torch.zeros_like(choice); a = torch.zeros_like(act)
            value_net.decide(pol.device_net(), env.W, 81, env.n, rot.data_ptr(), rew.data_ptr(), acts.data_ptr(), rob9.data_ptr(), 9, pol.gamma, T,
                             None, v.data_ptr(), p.data_ptr(), a.data_ptr(), stream)
            np.testing.assert_array_equal(v.cpu().numpy(), values.cpu().numpy())
            np.testing.assert_array_equal(a.cpu().numpy(), act.cpu().numpy())
        if act_prev is not None:
            kept = (env._dl.counter != 0).cpu().numpy()
            np.testing.assert_array_equal(rob.cpu().numpy()[kept][:, 3:5], act_prev[kept])
        act_prev = act.cpu().numpy().copy()
        distinct.update(int(c) for c in choice.cpu().numpy())
        _, _, term, trunc, _ = env.step_device(env.action_buffer())
        ended += int((term | trunc).sum().item())
    print(f"{name}: {ended} episodes ended in 50 steps of 64 worlds, {len(distinct)} distinct actions chosen")
    assert len(distinct) > 3
    env.close()


def test_weight_blob_follows_the_parameters():
    """The packed blob is rebuilt when a parameter changes (an optimiser step, load_state_dict) and only then."""
    import torch

    env = _batched(5, W=64)
    pol = _ready(make_policy("cadrl"), env)
    seeded_weights(pol.model, 2200)
    env.act_device(pol)
    v0 = env.last_values_device()[0].clone()
    blob0 = pol.device_net().blob
    env.act_device(pol)
    assert pol.device_net().blob is blob0
    with torch.no_grad():
        pol.model.value_network[6].bias.add_(1.0)          # the last layer's bias: every network output moves by exactly that much
    env.act_device(pol)
    assert pol.device_net().blob is not blob0
    v1 = env.last_values_device()[0]
    disc = 0.9 ** (0.25 * 1.0)
    np.testing.assert_allclose((v1 - v0).cpu().numpy(), disc, rtol=0, atol=1e-4 * max(1.0, float(v0.abs().max())))
    env.close()
