"""GPU suite of the ORCA robot policy (csrc/policy_orca.hip, cs_policy_orca): every decision against the C restatement of RVO2
(oracle/orca_oracle.c, agent 0 of one doStep) bit for bit -- the bar the ORCA crowd kernel holds against the same restatement --, a batch
against the W = 1 ``predict``, the resident worlds of the batched Gym, the device-resident act -> step loop and the fused call."""
import numpy as np
import pytest

import orca_policy_cases as oc
import parity_util

pytestmark = pytest.mark.gpu


def _states(robot13, obs):
    from social_navigation_pyenvs_amd.crowd_nav.utils.state import FullState, JointState, ObservableState

    r = [float(x) for x in robot13]
    return JointState(FullState(r[0], r[1], r[3], r[4], r[8], r[10], r[11], r[12], r[2]), [ObservableState(*[float(x) for x in h[:5]]) for h in obs])


def _policy(time_step=oc.TIME_STEP, safety_space=0):
    from social_navigation_pyenvs_amd.crowd_nav.policy_no_train.orca import ORCA

    p = ORCA()
    p.time_step = time_step
    p.safety_space = safety_space
    return p


def _predict(case):
    pol = _policy(case["time_step"], case["safety_space"])
    st = _states(case["robot"], case["obs"])
    a = pol.predict(st)
    assert pol.last_state is st
    return np.array([a.vx, a.vy], np.float32)


@pytest.fixture(scope="module")
def cases():
    """Every random and edge case with the oracle's answer and the W = 1 predict, computed once and left unchanged."""
    from social_navigation_pyenvs_amd import _lib

    _lib.require_gpu()
    out = []
    for c in oc.random_cases() + oc.edge_cases():
        out.append(dict(c, ref=oc.reference_action(c["robot"], c["obs"], c["time_step"], c["safety_space"]), predicted=_predict(c)))
    return out


def test_predict_equals_the_oracle_bit_for_bit(cases):
    assert len(cases) == len(oc.SIZES) * oc.WORLDS_PER_SIZE + len(oc.edge_cases())
    wrong = []
    for c in cases:
        got, ref = c["predicted"], c["ref"].action
        assert got.dtype == ref.dtype == np.float32
        same = np.array_equal(got, ref)
        parity_util.record("policy_orca_predict_vs_restatement", 0.0 if same else float(np.max(np.abs(got.astype(np.float64) - ref))))
        if not same:
            wrong.append((c["name"], c["ref"].kind, c["ref"].colliding, got, ref))
    print(f"ORCA predict: {len(cases)} decisions compared with the restatement, {len(wrong)} differ")
    assert not wrong, (len(wrong), wrong[:8])
    # the tie case's two orders have different answers (CPU suite), so both being right means the lower row index took the tenth slot
    tie = {c["name"]: c for c in cases if c["name"].startswith("tie")}
    assert not np.array_equal(tie["tie"]["predicted"], tie["tie-swapped"]["predicted"])


def _launch(torch, robot, obs, time_step=oc.TIME_STEP, safety_space=0):
    """One cs_policy_orca launch on [W, 13] / [W, n, cols] numpy arrays; returns the [W, 2] actions."""
    from social_navigation_pyenvs_amd.crowd_nav.policy_no_train import orca

    W, n, cols = obs.shape
    d_robot = torch.from_numpy(np.ascontiguousarray(robot, np.float32)).cuda()
    d_obs = torch.from_numpy(np.ascontiguousarray(obs if n else np.zeros((W, 1, cols)), np.float32)).cuda()
    d_act = torch.full((W, 2), float("nan"), dtype=torch.float32, device="cuda")
    orca.launch(W, n, d_robot.data_ptr(), d_obs.data_ptr(), cols, time_step, oc.NEIGHBOR_DIST, oc.MAX_NEIGHBORS, oc.TIME_HORIZON, safety_space,
                d_act.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    return d_act.cpu().numpy()


@pytest.mark.parametrize("n", oc.SIZES)
def test_a_batch_equals_the_single_predicts(cases, n):
    torch = pytest.importorskip("torch")
    mine = oc.cases_of_size(cases, n)
    assert len(mine) == oc.WORLDS_PER_SIZE
    for W in (48, 5):            # 12 full blocks; one full block and a last block with one live wavefront
        sub = mine[:W]
        act = _launch(torch, np.stack([c["robot"] for c in sub]), np.stack([c["obs"] for c in sub]).reshape(W, n, 5))
        np.testing.assert_array_equal(act, np.stack([c["predicted"] for c in sub]), err_msg=f"n={n} W={W}")


@pytest.mark.parametrize("n", [25, 70])
def test_a_batch_of_different_robots_with_seven_column_rows(cases, n):
    """Every world its own radius and v_pref, rows with theta and omega behind the five columns that are read."""
    torch = pytest.importorskip("torch")
    mine = oc.cases_of_size(cases, n)
    W = len(mine)
    rng = np.random.default_rng(n)
    robot = np.stack([c["robot"] for c in mine]).copy()
    robot[:, 8] = np.float32(0.2) + np.float32(0.004) * np.arange(W, dtype=np.float32)
    robot[:, 12] = np.float32(0.6) + np.float32(0.02) * np.arange(W, dtype=np.float32)
    assert len(set(robot[:, 8])) == W and len(set(robot[:, 12])) == W
    obs = np.concatenate([np.stack([c["obs"] for c in mine]), rng.uniform(-3, 3, (W, n, 2)).astype(np.float32)], axis=2)
    act = _launch(torch, robot, obs)
    for w in range(W):
        np.testing.assert_array_equal(act[w], oc.reference_action(robot[w], obs[w], oc.TIME_STEP).action, err_msg=f"world {w}")
        np.testing.assert_array_equal(act[w], _launch(torch, robot[w:w + 1], obs[w:w + 1])[0], err_msg=f"world {w} alone")


def _batched(n, W=4096):
    from test_gpu_generators import _config

    from social_navigation_pyenvs_amd.social_gym.social_nav_gym import BatchedSocialNavGym

    env = BatchedSocialNavGym(_config("hybrid_scenario", human_num=n, policy="sfm_guo"), W)
    env.reset(phase="test", first_case=11, device=True)
    return env


@pytest.mark.parametrize("n", [5, 25])
def test_act_device_on_the_resident_worlds(n):
    pytest.importorskip("torch")
    env = _batched(n)
    W = env.W
    pol = _policy(None)                 # time_step None: the robot time step
    for _ in range(3):                  # robots and humans in motion
        env.step_device(env.act_device(pol))
    act = env.act_device(pol)
    assert act is env.action_buffer()
    act = act.cpu().numpy().copy()
    assert np.all(np.isfinite(act))
    robot = env.cw.d_robot.download().reshape(W, 13)
    obs = env._dl.obs.cpu().numpy()
    single = _policy(env.robot_time_step)
    rows = np.unique(np.r_[0, W - 1, np.random.default_rng(n).choice(W, 382, replace=False)])
    for w in rows:
        a = single.predict(_states(robot[w], obs[w]))
        assert np.float32(a.vx) == act[w, 0] and np.float32(a.vy) == act[w, 1], (w, a, act[w])
        np.testing.assert_array_equal(act[w], oc.reference_action(robot[w], obs[w], env.robot_time_step).action, err_msg=f"world {w}")
    env.action_buffer().fill_(float("nan"))
    np.testing.assert_array_equal(env.act_device("orca_device").cpu().numpy(), act)


def test_act_step_loop_reads_the_current_observation():
    """64 worlds, 100 Gym steps of act_device -> step_device with auto-reset: at every step the actions are the kernel's answer on that
    step's observation and robot rows, and a robot that was not reset carries the previous action as its velocity."""
    torch = pytest.importorskip("torch")
    from social_navigation_pyenvs_amd.crowd_nav.policy_no_train import orca

    env = _batched(5, W=64)
    pol = _policy(None)
    ended = 0
    act_prev = None
    for k in range(100):
        act = env.act_device(pol)
        assert act is env.action_buffer()
        obs = env._dl.obs.clone()
        rob = env.cw.d_robot.torch().view(env.W, 13).clone()
        np.testing.assert_array_equal(obs.cpu().numpy(), env.observe_device().cpu().numpy())     # the observation of the resident rows
        check = torch.full_like(act, float("nan"))
        orca.launch(env.W, env.n, rob.data_ptr(), obs.data_ptr(), obs.shape[2], env.robot_time_step, pol.neighbor_dist, pol.max_neighbors,
                    pol.time_horizon, pol.safety_space, check.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        np.testing.assert_array_equal(act.cpu().numpy(), check.cpu().numpy())
        if act_prev is not None:
            kept = (env._dl.counter != 0).cpu().numpy()       # worlds that were not reset by the previous step
            np.testing.assert_array_equal(rob.cpu().numpy()[kept][:, 3:5], act_prev[kept])
        act_prev = act.cpu().numpy().copy()
        _, _, term, trunc, _ = env.step_device(env.action_buffer())
        ended += int((term | trunc).sum().item())
    assert ended > 0         # episodes ended and were reset on the way
    print(f"ORCA: {ended} episodes ended in 100 steps of 64 worlds")


def test_act_step_device_equals_the_two_calls():
    pytest.importorskip("torch")
    two, one = _batched(5, W=64), _batched(5, W=64)
    pol = _policy(None)
    for k in range(20):
        a2 = two.act_device(pol).cpu().numpy().copy()
        r2 = [t.cpu().numpy().copy() for t in two.step_device(two.action_buffer())]
        r1 = [t.cpu().numpy().copy() for t in one.act_step_device(pol if k % 2 else "orca_device")]
        np.testing.assert_array_equal(one.action_buffer().cpu().numpy(), a2, err_msg=f"step {k}: actions")
        for i, (x, y) in enumerate(zip(r1, r2)):
            np.testing.assert_array_equal(x, y, err_msg=f"step {k}: result {i}")


def test_refusals():
    pytest.importorskip("torch")
    env = _batched(5, W=8)
    with pytest.raises(ValueError, match="explore"):
        env.act_device(_policy(None), explore=object())
    with pytest.raises(NotImplementedError, match="rvo2"):        # the no-train factory's key keeps raising
        env.act_device("orca")
    env.cw.unicycle = True
    try:
        for call in (env.act_device, env.act_step_device):
            for policy in (_policy(None), "orca_device"):
                with pytest.raises(ValueError, match="holonomic"):
                    call(policy)
    finally:
        env.cw.unicycle = False
    assert np.all(np.isfinite(env.act_device("orca_device").cpu().numpy()))
