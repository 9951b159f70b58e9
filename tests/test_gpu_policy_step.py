"""GPU suite of the policy-driven Gym step: ``act_step_device(p)`` (cs_gym_step_policy / cs_gym_step_staged_policy: the robot's no-train
policy decided in the step launch's head) against the two calls it replaces, ``act_device(p)`` -> ``step_device(action_buffer())``.

The yardstick is the two-launch path, which golden G18 pins on the reference (tests/test_gpu_policy_no_train.py).  Both paths evaluate
the same float32 expressions on the same inputs and sum the humans' terms in the same butterfly, so the comparison has NO tolerance:
every buffer is compared as raw 32-bit words after every step (stricter than array_equal: -0 != +0, a NaN equals itself only bit for
bit), and a single differing bit fails.

Grid at 96 worlds: five policies x {5, 25} humans x {sfm_guo, hsfm_farina} crowd x {robot invisible, visible} x {same-step, NEXT_STEP}.
At 4096 worlds (the benchmark's batch: two wavefronts per SIMD, the builds with the one-wave register budget) a subset, BIG below: every
policy, both crowds, both robots, both reset modes and both human counts appear in it at least once.
One shape of the grid has no step build that decides: 5 humans with an invisible robot step on the DPP-row kernel, whose Gym step is
already several launches; there act_step_device runs the decision kernel in front of them inside the same library call (asserted, with
ORCA, in test_worlds_without_a_deciding_build_take_the_launches_inside_one_call)."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POLICIES = ["bp", "ssp", "sfm_helbing", "sfm_guo", "sfm_moussaid"]
STEPS = 60
BIG = [("sfm_moussaid", 25, "sfm_guo", False, True), ("bp", 25, "hsfm_farina", True, "next_step"), ("ssp", 5, "sfm_guo", True, True),
       ("sfm_helbing", 5, "hsfm_farina", False, "next_step"), ("sfm_guo", 25, "hsfm_farina", False, True),
       ("sfm_moussaid", 25, "sfm_guo", True, "next_step")]


def _env(n, W, crowd, visible, first_case=11):
    from test_gpu_generators import _config

    from social_navigation_pyenvs_amd.social_gym.social_nav_gym import BatchedSocialNavGym

    env = BatchedSocialNavGym(_config("hybrid_scenario", human_num=n, policy=crowd), W, robot_visible=visible)
    env.reset(phase="test", first_case=first_case, device=True)
    return env


def _buffers(env, ret):
    """Everything a Gym step leaves on the device, by name."""
    dl = env._dl
    obs, reward, term, trunc, info = ret
    return dict(crowd_rows=env.cw.d_state.torch(), goals=env.cw.d_goals.torch(), robot_rows=env.cw.d_robot.torch(), observation=obs,
                reward=reward, terminated=term, truncated=trunc, info=info, reward_row=dl.out, reset_failed_mask=env.reset_failed_mask(),
                action_buffer=env.action_buffer(), counter=dl.counter, seeds=dl.seeds, global_time=dl.gtime, epoch=dl.epoch,
                pending=dl.pending)


def _words(t):
    import torch

    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _assert_same_bits(a, b, what):
    import torch

    for name in a:
        x, y = _words(a[name]), _words(b[name])
        if not torch.equal(x, y):
            np.testing.assert_array_equal(x.cpu().numpy(), y.cpu().numpy(), err_msg=f"{what}: {name}")
            raise AssertionError(f"{what}: {name} differs")


def _run_pair(two, one, pol_two, pol_one, auto_reset, what, steps=STEPS):
    """`two` decides and steps in two calls, `one` in one; compared after every step.  Returns the number of episodes that ended."""
    import torch

    ended = 0
    for k in range(steps):
        act = two.act_device(pol_two)
        assert act is two.action_buffer()
        ret_two = two.step_device(two.action_buffer(), auto_reset=auto_reset)
        ret_one = one.act_step_device(pol_one, auto_reset=auto_reset)
        torch.cuda.synchronize()
        _assert_same_bits(_buffers(two, ret_two), _buffers(one, ret_one), f"{what} step {k}")
        ended += int((ret_one[2] | ret_one[3]).sum().item())
    return ended


def _fused_expected(n, visible):
    return not (n == 5 and not visible)      # (the DPP-row kernel's small worlds: module docstring)


def _assert_variant(env, n, crowd, visible, W):
    """Which build ran: the step build that decides in its head (the twin of the plain step's build: same budget and row count,
    LEAN = 8 + the twin's) or the decision kernel in front of the plain step's."""
    v, plain = env.act_step_variant(), env.cw.step_variant()
    if not _fused_expected(n, visible):
        assert v == "k_policy_no_train + " + plain and "row16" in plain, (v, plain)
        return
    soc, headed = {"sfm_guo": (1, 0), "hsfm_farina": (0, 1)}[crowd]
    lean = 3 if visible else 1
    m = re.search(r"OCC=(\d+),ROWS_CT=(\d+),LEAN=(\d+)", plain)
    assert m and int(m.group(3)) == lean, plain
    assert v.startswith(f"k_sfm_step<SOC={soc},HEADED={headed},PEQ=1,MAXT=64,OCC={m.group(1)},ROWS_CT={m.group(2)},LEAN=8+{lean}>"), (v, plain)
    assert "policy decided in the head" in v and int(m.group(2)) == n + (1 if visible else 0), (v, plain)


_PAIRS = {}
_STEPS_RUN = {}


def _pair96(n, crowd, visible, mode):
    """The two environments of one (shape, crowd, robot, reset mode) at 96 worlds, shared by the five policies' cases (each continues
    where the previous one stopped: the two stay bit-identical or the case that broke them fails)."""
    key = (n, crowd, visible, mode)
    if key not in _PAIRS:
        _PAIRS[key] = (_env(n, 96, crowd, visible), _env(n, 96, crowd, visible))
    return _PAIRS[key]


@pytest.mark.parametrize("mode", [True, "next_step"], ids=["same_step", "next_step"])
@pytest.mark.parametrize("visible", [False, True], ids=["invisible", "visible"])
@pytest.mark.parametrize("crowd", ["sfm_guo", "hsfm_farina"])
@pytest.mark.parametrize("n", [5, 25])
@pytest.mark.parametrize("policy", POLICIES)
def test_one_call_equals_act_then_step_bit_for_bit_96_worlds(policy, n, crowd, visible, mode):
    torch = pytest.importorskip("torch")
    two, one = _pair96(n, crowd, visible, mode)
    _assert_variant(one, n, crowd, visible, 96)
    ended = _run_pair(two, one, policy, policy, mode, f"{policy} n={n} {crowd} visible={visible} {mode}")
    _STEPS_RUN[(n, crowd, visible, mode)] = _STEPS_RUN.get((n, crowd, visible, mode), 0) + STEPS
    if _STEPS_RUN[(n, crowd, visible, mode)] == STEPS * len(POLICIES):
        # the pair has been through the five policies: episodes ended on the way and staged episodes were taken over -- part of what was compared
        assert int(one._dl.epoch.sum().item()) > 0 and torch.equal(one._dl.epoch, two._dl.epoch)
        two.close()
        one.close()
        del _PAIRS[(n, crowd, visible, mode)]
    print(f"{policy} n={n} {crowd} visible={visible} {mode}: {ended} episodes ended in {STEPS} steps of 96 worlds, variant {one.act_step_variant()}")


@pytest.mark.parametrize("policy,n,crowd,visible,mode", BIG, ids=[f"{b[0]}-{b[1]}-{b[2]}-{'vis' if b[3] else 'inv'}-{b[4]}" for b in BIG])
def test_one_call_equals_act_then_step_bit_for_bit_4096_worlds(policy, n, crowd, visible, mode):
    pytest.importorskip("torch")
    two, one = _env(n, 4096, crowd, visible), _env(n, 4096, crowd, visible)
    try:
        _assert_variant(one, n, crowd, visible, 4096)
        if n == 25:
            assert "OCC=1" in one.act_step_variant(), one.act_step_variant()     # two wavefronts per SIMD: the one-wave register budget
        ended = _run_pair(two, one, policy, policy, mode, f"4096 worlds {policy} n={n} {crowd} visible={visible} {mode}")
        assert ended > 0 and int(one._dl.epoch.sum().item()) > 0
        print(f"4096 worlds {policy} n={n} {crowd} visible={visible} {mode}: {ended} episodes ended, variant {one.act_step_variant()}")
    finally:
        two.close()
        one.close()


@pytest.mark.parametrize("n,crowd,visible", [(10, "orca", False), (5, "sfm_guo", False)], ids=["orca-10", "row16-5"])
def test_worlds_without_a_deciding_build_take_the_launches_inside_one_call(n, crowd, visible):
    """ORCA (10 humans) and the DPP-row kernel's small worlds: one call, the decision kernel and the step's launches behind each other,
    the same bits."""
    pytest.importorskip("torch")
    two, one = _env(n, 96, crowd, visible), _env(n, 96, crowd, visible)
    try:
        v = one.act_step_variant()
        assert v == "k_policy_no_train + " + one.cw.step_variant(), v
        assert ("k_orca_step" in v) == (crowd == "orca"), v
        for policy in ("sfm_guo", "ssp"):
            _run_pair(two, one, policy, policy, True, f"{crowd} {policy}")
    finally:
        two.close()
        one.close()


def test_time_step_and_parameters_key_the_bound_arguments():
    """A policy with its own time_step and one with its own parameters, alternating with the default policy of the same name on one
    environment: each call must run with ITS arguments (the bound ctypes arguments are cached per (policy id, time step, parameters))."""
    pytest.importorskip("torch")
    from social_navigation_pyenvs_amd.crowd_nav.policy_no_train.policy_factory import policy_factory

    def variants():
        slow = policy_factory["sfm_helbing"]()
        slow.time_step = 0.1
        heavy = policy_factory["sfm_helbing"]()
        heavy.params = dict(heavy.params, mass=60.0, Ai=1500.0, relaxation_time=0.4)
        return ["sfm_helbing", slow, heavy, "sfm_helbing", heavy, slow]

    probe = variants()[2].packed_params()
    assert probe[20] == 60.0 and probe[1] == 1500.0 and probe[0] == np.float32(0.4)      # the changed parameters reach the packed row
    two, one = _env(25, 96, "sfm_guo", False), _env(25, 96, "sfm_guo", False)
    try:
        seen = []
        for k, (p2, p1) in enumerate(zip(variants() * 4, variants() * 4)):
            _run_pair(two, one, p2, p1, True, f"variant {k}", steps=3)
            seen.append(one.action_buffer().clone())
        # ... and the three are three different decisions (a cache that ignored the key would still pass the equality above)
        import torch

        two.act_device("sfm_helbing")
        base = two.action_buffer().clone()
        for p in variants()[1:3]:
            assert not torch.equal(two.act_device(p), base)
    finally:
        two.close()
        one.close()


@pytest.mark.parametrize("visible", [False, True], ids=["invisible", "visible"])
@pytest.mark.parametrize("policy", ["sfm_moussaid", "ssp"])
def test_a_world_decides_the_same_bits_alone_second_of_its_wavefront_and_in_4096(policy, visible):
    """World 1235 of a batch of 4096 x 25 from first_case 11 (the SECOND world of its wavefront) is the episode of seed case 1246.  The
    same episode as the only world of W = 1 (first of its wavefront) and as world 1 of W = 2 (second of its wavefront): the same
    actions, robot rows, observation and rewards, bit for bit, over 12 steps without resets."""
    torch = pytest.importorskip("torch")
    big, alone, second = _env(25, 4096, "sfm_guo", visible), _env(25, 1, "sfm_guo", visible, first_case=1246), _env(25, 2, "sfm_guo", visible, first_case=1245)
    try:
        assert "policy decided in the head" in alone.act_step_variant() and "policy decided in the head" in big.act_step_variant()
        k = 1235
        for step in range(12):
            rets = [e.act_step_device(policy, auto_reset=False) for e in (big, alone, second)]
            torch.cuda.synchronize()
            for env, ret, w, name in ((alone, rets[1], 0, "W=1"), (second, rets[2], 1, "second of W=2")):
                a, b = _buffers(big, rets[0]), _buffers(env, ret)
                for key in ("action_buffer", "robot_rows", "observation", "reward", "reward_row", "terminated", "truncated", "info"):
                    x = _words(a[key]).reshape(4096, -1)[k]
                    y = _words(b[key]).reshape(env.W, -1)[w]
                    assert torch.equal(x, y), (policy, visible, step, name, key, x, y)
    finally:
        for e in (big, alone, second):
            e.close()


def test_sharded_gym_reaches_act_step_device_through_the_local_env():
    pytest.importorskip("torch")
    from social_navigation_pyenvs_amd.social_gym.sharded_gym import ShardedBatchedSocialNavGym

    assert "act_step_device" not in vars(ShardedBatchedSocialNavGym)
    env = _env(5, 8, "sfm_guo", True)
    try:
        sh = ShardedBatchedSocialNavGym.__new__(ShardedBatchedSocialNavGym)
        sh.env = env
        assert sh.act_step_device == env.act_step_device
    finally:
        env.close()
