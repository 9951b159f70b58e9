"""GPU suite of the opt-in bf16 arithmetic of the value-network decision (cs_value_net_decide_bf16, csrc/value_net_bf16.hip; Python:
``set_decision_precision("bf16")``).  The reference is tests/bf16_emulation.py, the float64 restatement of the arithmetic's contract
(DESIGN.md 4.5); the inputs are the synthetic arrays of tests/decision_edges.py and golden G16.

The bar of the comparison is the project's rule for one float32 realisation against another (parity_util.F32_SLACK): the kernel's worst
relative action-value error against the float64 emulation is at most F32_SLACK times the error of the emulation's own
float32-accumulation mode against its float64 mode, over the same sweep.  No case is excluded."""
import configparser
import functools

import numpy as np
import pytest

import bf16_emulation as em
import decision_edges as de
import parity_util
from test_policy_seam import _groups
from test_value_policy_cpu import fixture_state_dict, make_policy, numpy_weights, seeded_weights

pytestmark = pytest.mark.gpu

# the issue's sweep: n = 1, 16, 17, 31, 32, 33, 97 with W * A of 1, 31, 32, 33 (decision_edges.WA_SWEEP[:4]: A of 1, 1, 32, 11)
N_BF16 = [1, 16, 17, 31, 32, 33, 97]
SWEEP = [(n, W, A) for n in N_BF16 for W, A in de.WA_SWEEP[:4]]
WIDTHS = dict(sarl__mlp1_dims="40, 256", sarl__mlp2_dims="72, 33", sarl__attention_dims="20, 1", sarl__mlp3_dims="90, 1")   # 40, 72, 33, 20, 90: no multiples of 16


def _ready(pol, precision="bf16"):
    import torch

    pol.set_phase("test")
    pol.set_device(torch.device("cuda"))
    pol.set_decision_precision(precision)
    return pol


def _decide(pol, rot, rew, acts, rob, gamma=de.GAMMA, dt=de.DT):
    """The policy's decision entry on host arrays: (values [W, A], choice [W]); the outputs start as NaN / -7."""
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    net = pol.device_net()
    W, A, n, _ = rot.shape
    dev = lambda a, dtype=torch.float32: torch.as_tensor(np.array(a, order="C"), dtype=dtype, device="cuda")     # (C order: an index array leaves another layout)
    d_rot, d_rew, d_acts, d_rob = dev(rot), dev(rew), dev(acts), dev(rob)
    vals = torch.full((W, A), float("nan"), device="cuda")
    pick = torch.full((W,), -7, dtype=torch.int32, device="cuda")
    act = torch.full((W, 2), float("nan"), device="cuda")
    value_net.decide(net, W, A, n, d_rot.data_ptr(), d_rew.data_ptr(), d_acts.data_ptr(), d_rob.data_ptr(), rob.shape[1], gamma, dt, None,
                     vals.data_ptr(), pick.data_ptr(), act.data_ptr(), torch.cuda.current_stream().cuda_stream, precision=pol.decision_precision)
    torch.cuda.synchronize()
    return vals.cpu().numpy(), pick.cpu().numpy()


def _variant_policy(variant):
    """(name, policy on the CPU, with_global, cols) of a network variant; seeded weights at G16's scale, SARL with the calm attention layer"""
    if variant in ("cadrl", "sarl"):
        return variant, de.sweep_policy(variant), True, 13
    if variant == "sarl no global":
        pol = make_policy("sarl", sarl__with_global_state="false")
    elif variant == "sarl 15 columns":
        pol = make_policy("sarl", sarl__with_theta_and_omega_visible="true")
    elif variant == "cadrl 15 columns":
        pol = make_policy("cadrl", sarl__with_theta_and_omega_visible="true")
    else:
        pol = make_policy("sarl", **WIDTHS)
    seeded_weights(pol.model, 4400)
    if variant == "sarl widths":       # a 256-wide layer at N(0, 0.25) blows the activations up: the default init's scale (test_gpu_value_policy)
        import torch

        with torch.no_grad():
            for prm in pol.model.parameters():
                prm.mul_(0.25)
    name = "cadrl" if variant.startswith("cadrl") else "sarl"
    if name == "sarl":
        de._calm(pol)
    return name, pol, variant != "sarl no global", pol.joint_state_dim


@functools.lru_cache(maxsize=None)
def _rows(n, W, A, cols):
    """decision_edges.sweep_case's rows for 13 columns; torch.randn rows of the same kind for 15.  Read-only."""
    import torch

    if cols == 13:
        c = de.sweep_case("cadrl", n, W, A)
        return c["rot"], c["rew"], c["rob"]
    g = torch.Generator().manual_seed(100000 * n + 100 * A + W + 7)
    rot = torch.randn((W, A, n, cols), generator=g)
    rot[..., :6] = rot[:, :, :1, :6]
    rew = torch.randn((W, A), generator=g) * 0.1
    out = rot.numpy(), rew.numpy(), de.robot_rows(W, 9, np.random.default_rng([n, W, A, 47]))
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("variant,sweep", [
    ("cadrl", SWEEP + [(5, 2, 81), (32, 1, 65)]),
    ("sarl", SWEEP + [(5, 2, 81), (32, 1, 65)]),
    ("sarl no global", [(n, 3, 11) for n in N_BF16]),
    ("sarl 15 columns", [(n, 3, 11) for n in (1, 17, 33)]),
    ("cadrl 15 columns", [(n, 3, 11) for n in (1, 17, 33)]),
    ("sarl widths", [(n, 3, 11) for n in N_BF16]),
])
def test_kernel_against_the_float64_emulation(variant, sweep):
    """Worst relative action-value error of the kernel against the float64 emulation over the sweep (decision_edges.rel_error's scale), held
    to F32_SLACK times the float32-accumulation emulation's error against the same reference over the same sweep.

    Measured on the MI355X: see HISTORY.md ("bf16 decision arithmetic") for the two figures of every network."""
    name, host, with_global, cols = _variant_policy(variant)
    w = numpy_weights(host.model)
    pol = _ready(_variant_policy(variant)[1])
    worst = worst32 = 0.0
    for n, W, A in sweep:
        rot, rew, rob = _rows(n, W, A, cols)
        disc = de.discount(rob)
        e64 = em.action_values(name, rot, rew, disc, w, with_global)
        e32 = em.action_values(name, rot, rew, disc, w, with_global, acc="f32")
        vals, pick = _decide(pol, rot, rew, de.pick_actions(A), rob)
        assert np.isfinite(e64).all() and np.isfinite(vals).all(), (variant, n, W, A)
        err, err32 = de.rel_error(vals, e64), de.rel_error(e32, e64)
        print(f"{variant} n={n} W={W} A={A}: kernel {err:.3e}, float32-accumulation emulation {err32:.3e}")
        np.testing.assert_array_equal(pick, de.expected_pick(vals))
        worst, worst32 = max(worst, err), max(worst32, err32)
    print(f"bf16 {variant}: worst relative action-value error against the float64 emulation: kernel {worst:.3e}, float32-accumulation emulation {worst32:.3e}")
    parity_util.record(f"bf16 decision: kernel against the float64 emulation, {variant} (relative action value)", worst, bar=de.REL_BAR)
    parity_util.record(f"bf16 decision: float32-accumulation emulation against the float64 emulation, {variant} (relative action value)", worst32, bar=de.REL_BAR)
    assert worst <= parity_util.F32_SLACK * worst32, (variant, worst, worst32)


@pytest.mark.parametrize("name", ["cadrl", "sarl"])
def test_one_world_alone_and_inside_batches_of_33_and_4096(name):
    """W = 1 against the same world inside batches of 33 and 4096 (n = 5, A = 11: 45056 groups in 1408 workgroups)"""
    pol = _ready(de.sweep_policy(name))
    A, n = 11, 5
    rng = np.random.default_rng(48)
    rot = rng.normal(size=(4096, A, n, 13)).astype(np.float32)
    rot[..., :6] = rot[:, :, :1, :6]
    rew = (rng.normal(size=(4096, A)) * 0.1).astype(np.float32)
    rob = de.robot_rows(4096, 9, rng)
    big, _ = _decide(pol, rot, rew, de.pick_actions(A), rob)
    assert np.isfinite(big).all()
    mid, _ = _decide(pol, rot[100:133], rew[100:133], de.pick_actions(A), rob[100:133])
    np.testing.assert_array_equal(mid, big[100:133])
    for w in (0, 100, 117, 132, 4095):
        one, _ = _decide(pol, rot[w:w + 1], rew[w:w + 1], de.pick_actions(A), rob[w:w + 1])
        np.testing.assert_array_equal(one[0], big[w])


@pytest.mark.parametrize("n", [3, 16, 40])
def test_shuffled_humans_keep_the_cadrl_minimum(n):
    """The humans of every group in another order: each row's value is the same fixed chain wherever the row sits, the minimum picks the same word"""
    pol = _ready(de.sweep_policy("cadrl"))
    c = de.sweep_case("cadrl", n, 3, 11)
    v1, _ = _decide(pol, c["rot"], c["rew"], de.pick_actions(11), c["rob"])
    perm = np.random.default_rng(n).permutation(n)
    assert (perm != np.arange(n)).any()
    v2, _ = _decide(pol, c["rot"][:, :, perm], c["rew"], de.pick_actions(11), c["rob"])
    assert np.isfinite(v1).all() and de.same_words(v1, v2)


def _g16_env(cs):
    from social_navigation_pyenvs_amd.social_gym.social_nav_gym import BatchedSocialNavGym

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
    return env


def test_g16_every_flipped_decision_is_explained():
    """The reference's 135 recorded decisions as worlds of a batch (test_gpu_value_policy's set-up), decided with the bf16 arithmetic.  A
    decision whose pick differs from the reference's `chosen` is a flip; it is explained when gap <= 2 e (bf16_emulation.classify_flip), with
    e from the float64 EMULATION on the batch's own look-ahead rows, never from the kernel.  Zero unexplained flips; the count is recorded."""
    groups, w = _groups()
    total = flips = 0
    for key, cs in groups.items():
        c0 = cs[0]
        name = str(c0["policy"])
        env = _g16_env(cs)
        pol = _ready(make_policy(name))
        pol.time_step = env.robot_time_step
        pol.model.load_state_dict(fixture_state_dict(w[key]), strict=True)
        pol.gamma = float(c0["gamma"])
        pol.build_action_space(float(c0["robot"][7]))
        env.act_device(pol)
        values, choice = (t.cpu().numpy() for t in env.last_values_device())
        np.testing.assert_array_equal(choice, np.argmax(values, axis=1))
        rot, rew = (t.cpu().numpy() for t in env.lookahead_device(pol.action_space_ndarray))
        disc = np.array([float(c["gamma"]) ** (float(c["dt"]) * float(c["robot"][7])) for c in cs])
        full = rew.astype(np.float64) + disc[:, None] * em.full_precision(name, rot, w[key])
        e64 = em.action_values(name, rot, rew, disc, w[key])
        for k, c in enumerate(cs):
            total += 1
            if int(choice[k]) != int(c["chosen"]):
                flips += 1
                ok, gap, e = em.classify_flip(int(c["chosen"]), int(choice[k]), full[k], e64[k])
                print(f"G16 {key} decision {k}: bf16 picks {int(choice[k])}, the reference {int(c['chosen'])}: gap {gap:.3e}, emulation error e {e:.3e}")
                assert ok, (key, k, gap, e)
        env.close()
    print(f"G16 bf16: {flips} of {total} decisions flipped, all explained")
    parity_util.REPORT["bf16 decision: G16 decisions flipped against the reference's choice (all explained by gap <= 2 e)"] = {"decisions": total, "flips": flips}
    assert total == 135


def test_nan_and_infinities_follow_the_emulation():
    """decision_edges.nonfinite_case through the identity network: layer 0 is float32, its output is rounded to bf16 as layer 1's operand, so
    a finite value is bf16(px) exactly (one product per sum) and NaN / +-inf arrive where the emulation puts them -- raw words equal."""
    pol = _ready(de.identity_cadrl())
    w = numpy_weights(de.identity_cadrl().model)
    for n in (5, 40):
        rot, rew, rob = de.nonfinite_case(n)
        want = em.action_values("cadrl", rot, rew, np.ones(1), w).astype(np.float32)
        vals, pick = _decide(pol, rot, rew, de.pick_actions(rot.shape[1]), rob, gamma=1.0)
        np.testing.assert_array_equal(np.isnan(vals), np.isnan(want))
        assert np.isnan(want[0, [0, 1, 7, 8]]).all() and want[0, 4] == np.inf and want[0, 5] == -np.inf
        assert de.same_words(vals, want), dict(zip(de.NONFINITE_GROUPS, zip(vals[0], want[0])))
        assert pick[0] == 0


@pytest.mark.parametrize("with_global", [True, False])
@pytest.mark.parametrize("n", [5, 40])
def test_zero_scores_and_all_masked_groups_follow_the_emulation(n, with_global):
    """decision_edges.masked_case: the attention reads relu(px) alone, so a score is exactly 0 where px < 0 in this arithmetic too (bf16 of a
    positive float32 is positive).  NaN exactly where every human is masked; the finite groups under the sweep's rule."""
    host = de.masked_sarl(with_global)
    w = numpy_weights(host.model)
    pol = _ready(de.masked_sarl(with_global))
    rot, rew, rob, masked = de.masked_case(n)
    disc = de.discount(rob)
    e64 = em.action_values("sarl", rot, rew, disc, w, with_global)
    e32 = em.action_values("sarl", rot, rew, disc, w, with_global, acc="f32")
    vals, pick = _decide(pol, rot, rew, de.pick_actions(rot.shape[1]), rob)
    np.testing.assert_array_equal(np.isnan(e64), masked.all(axis=-1))
    np.testing.assert_array_equal(np.isnan(vals), np.isnan(e64))
    np.testing.assert_array_equal(~np.isfinite(vals), ~np.isfinite(e64))
    err, err32 = de.rel_error(vals, e64), de.rel_error(e32, e64)
    print(f"bf16 masked softmax n={n} global={with_global}: kernel {err:.3e}, float32-accumulation emulation {err32:.3e}")
    parity_util.record("bf16 decision: masked softmax against the float64 emulation (relative action value, finite groups)", err, bar=de.REL_BAR)
    assert err <= parity_util.F32_SLACK * err32, (err, err32)
    np.testing.assert_array_equal(pick, de.expected_pick(vals))


@pytest.mark.parametrize("name", ["cadrl", "sarl"])
def test_act_device_and_predict_agree_and_the_two_blobs_do_not_alias(name):
    """96 device-generated worlds, 5 humans, 3 steps: the bf16 actions of act_device equal the W = 1 predict of sampled worlds; switching
    back to "f32" reproduces, bit for bit, the f32 decision taken on the same observation before the switch."""
    from test_gpu_value_policy import _PeekedEnv, _batched

    from social_navigation_pyenvs_amd.crowd_nav.utils.state import FullState, JointState, ObservableState

    env = _batched(5, W=96)
    pol = _ready(make_policy(name), "f32")
    pol.time_step = env.robot_time_step
    seeded_weights(pol.model, 2300)
    differ = 0
    for step in range(3):
        f32_act = env.act_device(pol).cpu().numpy().copy()
        f32_values = env.last_values_device()[0].cpu().numpy().copy()
        pol.set_decision_precision("bf16")
        act = env.act_device(pol).cpu().numpy().copy()
        values, choice = (t.cpu().numpy().copy() for t in env.last_values_device())
        differ += int((values != f32_values).sum())
        robot, obs, peek = env.cw.d_robot.download(), env.observe_device().cpu().numpy(), env.cw.peek(env.robot_time_step)
        for wi in np.unique(np.r_[0, 95, np.random.default_rng(step).choice(96, 10, replace=False)]):
            r = robot[wi]
            state = JointState(FullState(*[float(x) for x in (r[0], r[1], r[3], r[4], r[8], r[10], r[11], r[12], r[2])]),
                               [ObservableState(*[float(x) for x in h]) for h in obs[wi]])
            pol.set_env(_PeekedEnv(peek[wi][:, :6]))
            a = pol.predict(state)
            assert np.float32(a.vx) == act[wi, 0] and np.float32(a.vy) == act[wi, 1], (step, wi)
            np.testing.assert_array_equal(np.asarray(pol.action_values, np.float32), values[wi])
        pol.set_decision_precision("f32")
        np.testing.assert_array_equal(env.act_device(pol).cpu().numpy(), f32_act)
        np.testing.assert_array_equal(env.last_values_device()[0].cpu().numpy(), f32_values)
        env.step_device(env.action_buffer())
    assert differ > 0                       # the two arithmetics are two: the bf16 values are not the f32 ones
    env.close()
