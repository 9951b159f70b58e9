"""CPU side of social_gym/device_loop.py: the clock table the step kernel indexes, the depth of the staging batch, the declared fields of
``DeviceLoop``, and the one statement of the value-based policies' refusals in ``BatchedSocialNavGym`` -- each text and type as recorded
from the two statements it replaces.  No GPU: the loop itself is tests/test_gpu_device_loop.py."""
from types import SimpleNamespace

import numpy as np
import pytest

from test_value_policy_cpu import make_policy

from social_navigation_pyenvs_amd.social_gym.device_loop import DeviceLoop, StepPieces, clock_table, stage_depth

F32 = np.float32


@pytest.mark.parametrize("time_step,factor,time_limit", [(0.25, 1, 5), (0.0125, 20, 50), (1 / 60, 15, 25)])
def test_clock_table_is_the_float32_accumulation_of_the_gym(time_step, factor, time_limit):
    """Entry k is ``global_time`` after k Gym steps: k * factor float32 additions of float32(time_step), one at a time."""
    expected, t = [F32(0)], F32(0)
    for _ in range(int(time_limit / (time_step * factor)) + 8 - 1):
        for _ in range(factor):
            t = F32(t + F32(time_step))
        expected.append(t)
    got = clock_table(time_limit, time_step, factor)
    assert got.dtype == F32 and got.shape == (int(time_limit / (time_step * factor)) + 8,)
    assert np.array_equal(got, np.array(expected, F32))
    assert got[0] == 0 and np.all(np.diff(got) > 0) and got[-8] >= time_limit - time_step * factor    # the limit is reached inside the table


def test_stage_depth_is_a_power_of_two_under_the_cap():
    GiB = 1 << 30
    assert stage_depth(5.4e6, 64, GiB) == 64                # 4096 x 25 worlds: the class default is kept
    assert stage_depth(64 << 20, 64, GiB) == 16
    assert stage_depth(5.4e6, 3, GiB) == 2 and stage_depth(5.4e6, 1, GiB) == 1
    for level in (1, 4096, 5.4e6, 64 << 20, GiB, 3 * GiB):
        for depth in (-1, 0, 1, 2, 3, 5, 8, 63, 64, 65, 1000):
            d = stage_depth(level, depth, GiB)
            assert d >= 1 and d & (d - 1) == 0 and d <= max(1, depth)
            assert d <= 2 or d * level <= GiB


def test_an_undeclared_field_is_an_attribute_error():
    loop = DeviceLoop.__new__(DeviceLoop)                  # (no __init__: nothing touches a device)
    fields = DeviceLoop.__slots__
    assert len(set(fields)) == len(fields) and not hasattr(loop, "__dict__")
    for name in ("counter", "seeds", "gtime", "clock", "mask", "epoch", "base_seed", "staged_seed", "staged_status", "failed", "pending", "act",
                 "obs", "out", "state", "cols", "results", "staging", "stage_book", "staging_desc", "gen", "refill_args", "refill_ev", "stream",
                 "stream_b", "depth", "stride", "ns_masks", "mode", "obs_fresh", "vn_values", "vn_choice", "la_cols", "la_robot_cols", "la_robot",
                 "pieces", "pnt_named", "pnt_args", "parity", "since_refill", "cw", "released"):
        assert name in fields, name
    loop.parity = 1
    assert loop.parity == 1
    for name in ("paritty", "obs_fresh_", "stream_c"):
        with pytest.raises(AttributeError):
            setattr(loop, name, 0)
        with pytest.raises(AttributeError):
            getattr(loop, name)
    with pytest.raises(AttributeError):
        loop.counter                                       # declared, not yet assigned
    pieces = StepPieces(1, 2, 3, 4, 5)
    assert (pieces.step, pieces.tail, pieces.fold, pieces.keep, pieces.results) == (1, 2, 3, 4, 5)
    with pytest.raises(AttributeError):
        pieces.folded = None
    # the dictionary's way of reading stays, for callers outside the package: the same fields, the same refusal of an unknown name
    loop.pieces = {(0, "same_step"): pieces}
    assert loop["parity"] == 1 and loop["pieces", 0, "same_step"] is pieces and loop[("pieces", 0, "same_step")]["fold"] == 3
    for read in (lambda: loop["paritty"], lambda: pieces["folded"], lambda: loop["counter"]):
        with pytest.raises(AttributeError):
            read()
    with pytest.raises(KeyError):
        loop["pieces", 1, "same_step"]
    with pytest.raises(TypeError):
        loop["parity"] = 0


def _env(headed=False, human_num=5):
    from test_gpu_generators import _config

    from social_navigation_pyenvs_amd.social_gym.social_nav_gym import BatchedSocialNavGym

    return BatchedSocialNavGym(_config("hybrid_scenario", human_num=human_num, policy="sfm_guo"), 8, headed_obs=headed)


# who asks, and what the policy was about to do: act_device's statement and value_device's / joint_state_device's, as they stood
CALLERS = [("act_device", "decides", True), ("value_device", "evaluates a state", False), ("joint_state_device", "evaluates a state", False)]


@pytest.mark.parametrize("who,before,kinematics_first", CALLERS)
def test_the_refusals_of_a_value_based_policy_keep_their_texts(who, before, kinematics_first):
    from social_navigation_pyenvs_amd.crowd_nav.policy.policy_factory import policy_factory

    def refusal(env, pol):
        with pytest.raises(Exception) as e:
            env._refuse_value_policy(who, pol, before, kinematics_first=kinematics_first)
        return type(e.value), str(e.value)

    assert refusal(_env(), "bp") == (TypeError, f"{who} takes a value-based policy (CADRL, SARL), not 'bp'")
    bare = policy_factory["sarl"]()
    bare.kinematics = "holonomic"
    assert refusal(_env(), bare) == (AttributeError, f"SARL: configure() the policy before it {before}")
    unicycle = make_policy("sarl")
    unicycle.kinematics = "unicycle"
    holonomic = (ValueError, f"{who}: the value-based policies act in ActionXY and need a holonomic robot")
    assert refusal(_env(), unicycle) == holonomic
    env = _env()
    env.cw = SimpleNamespace(unicycle=True, d_robot=object())
    assert refusal(env, make_policy("cadrl")) == holonomic
    differ = (ValueError, f"{who}: the policy's with_theta_and_omega_visible and the batch's headed_obs differ")
    assert refusal(_env(headed=True), make_policy("cadrl")) == differ
    assert refusal(_env(), make_policy("sarl", sarl__with_theta_and_omega_visible="true")) == differ
    env = _env()
    env.cw = SimpleNamespace(unicycle=False, d_robot=None)
    assert refusal(env, make_policy("sarl")) == (ValueError, f"{who} needs the robot rows")
    om = make_policy("om_sarl", sarl__with_om="true")
    assert refusal(_env(human_num=1), om) == (ValueError, f"{who}: OM-SARL's occupancy maps need at least two humans a world")
    # a policy that is neither configured nor holonomic: act_device names the kinematics, the state's readers the configuration
    assert refusal(_env(), policy_factory["sarl"]()) == (holonomic if kinematics_first else (AttributeError, f"SARL: configure() the policy before it {before}"))
    for good, humans in ((make_policy("sarl"), 1), (om, 2)):                      # nothing to refuse
        assert _env(human_num=humans)._refuse_value_policy(who, good, before, kinematics_first=kinematics_first) is None


def test_the_public_calls_refuse_before_anything_touches_the_device():
    """No world has been generated and no GPU is asked for: the refusal comes first on both paths, and a good policy gets as far as the
    missing device-generated batch."""
    from social_navigation_pyenvs_amd.crowd_nav.policy.policy_factory import policy_factory

    bare = policy_factory["cadrl"]()
    bare.kinematics = "holonomic"
    with pytest.raises(AttributeError, match=r"^CADRL: configure\(\) the policy before it decides$"):
        _env().act_device(bare)
    with pytest.raises(AttributeError, match=r"^CADRL: configure\(\) the policy before it evaluates a state$"):
        _env().value_device(bare)
    with pytest.raises(ValueError, match="^act_device: the policy's with_theta_and_omega_visible and the batch's headed_obs differ$"):
        _env(headed=True).act_device(make_policy("sarl"))
    om = make_policy("om_sarl", sarl__with_om="true")
    for call in (lambda env: env.act_device(om), lambda env: env.joint_state_device(om)):
        with pytest.raises(ValueError, match="OM-SARL's occupancy maps need at least two humans a world$"):
            call(_env(human_num=1))
        with pytest.raises(RuntimeError, match=r"reset\(\.\.\., device=True\)"):
            call(_env())
