"""CPU suite of the policy-driven Gym step (cs_gym_step_policy / cs_gym_step_staged_policy, BatchedSocialNavGym.act_step_device): the
new entry points are exported and declared, refuse what they cannot run before any device call, and the Python call refuses the
policies it does not take.  No device is needed: every call below fails its argument checks first."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["cs_gym_step_policy", "cs_gym_step_staged_policy", "cs_gym_step_policy_variant"]


def _lib():
    import __graft_entry__ as g

    g.build()
    from social_navigation_pyenvs_amd import _lib

    return _lib, _lib.load()


def test_new_entry_points_are_exported_and_declared_and_the_abi_version_stays():
    _l, lib = _lib()
    header = open(os.path.join(ROOT, "include", "crowdstep.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name), name
        assert name in _l.ABI_SYMBOLS
        assert re.search(r"^int " + name + r"\(", header, re.M), name
    assert lib.cs_abi_version() == 4 == _l.ABI_VERSION
    assert "#define CS_ABI_VERSION 4" in header


_BOOK_PTRS = ("d_counter", "d_seeds", "d_mask", "d_clock", "d_reward", "d_terminated", "d_truncated", "d_info")

# (what is changed from a well-formed call, a fragment of the message)
REFUSALS = [
    (dict(policy=5), "unknown no-train policy id"),
    (dict(policy=-1), "unknown no-train policy id"),
    (dict(time_step=0.0), "time_step must be positive"),
    (dict(time_step=-0.25), "time_step must be positive"),
    (dict(time_step=float("nan")), "time_step must be positive"),
    (dict(unicycle=True), "unicycle"),
    (dict(robot=False), "robot rows"),
    (dict(action=None), "null action buffer"),
    (dict(params=None), "need their parameters"),
    (dict(mass=0.0), "mass and relaxation_time must be non-zero"),
    (dict(book="null"), "null buffer in cs_gym_book"),
    (dict(n_substeps=0), "n_substeps must be positive"),
    (dict(obs=None), "null argument"),
]


@pytest.mark.parametrize("staged", [False, True], ids=["cs_gym_step_policy", "cs_gym_step_staged_policy"])
@pytest.mark.parametrize("change,fragment", REFUSALS, ids=[f"{i}-{list(r[0])[0]}" for i, r in enumerate(REFUSALS)])
def test_policy_step_entries_check_their_arguments_before_touching_a_device(staged, change, fragment):
    """Every pointer below is a dummy that is never dereferenced: each call is refused with CS_ERR_ARG and its message by the argument
    checks, which run before the first device call."""
    _l, lib = _lib()
    from social_navigation_pyenvs_amd.generators import cs_generator

    a = dict(policy=2, time_step=0.25, unicycle=False, robot=True, action=0x1000, params="ok", mass=80.0, book="ok", n_substeps=1, obs=0x1000)
    a.update(change)
    desc = _l.cs_worlds(W=4, n=5, G=2, type=1, layout=_l.CS_LAYOUT_AOS, flags=_l.CS_ROBOT_UNICYCLE if a["unicycle"] else 0)
    desc.d_state = desc.d_goals = desc.d_params = desc.d_safety = 0x1000
    if a["robot"]:
        desc.d_robot = 0x1000
    book = _l.cs_gym_book(**({k: 0x1000 for k in _BOOK_PTRS} if a["book"] == "ok" else {}), clock_len=4, auto_reset=1)
    prm = None if a["params"] is None else (C.c_float * 21)(*([0.5] + [1.0] * 19 + [a["mass"]]))
    cfg = (C.c_float * 5)(25.0, 1.0, -0.25, 0.2, 0.5)
    dev = C.c_void_p(0x1000)
    head = (C.byref(desc), C.c_float(0.01), C.c_int(a["n_substeps"]), C.c_void_p(a["action"]), C.c_float(0.25), dev, cfg, dev, C.byref(book),
            C.c_int(0), C.c_void_p(a["obs"]))
    tail = (C.c_int(a["policy"]), C.c_float(a["time_step"]), prm, None)
    if staged:
        gen = cs_generator(scenario=0, n=5, insert_robot=0, randomize_attributes=0, randomize_positions=1, max_tries=100, circle_radius=7.0,
                           traffic_length=14.0, traffic_height=3.0, robot_radius=0.3, human_mass=75.0, robot_mass=80.0, robot_desired_speed=1.0)
        sb = _l.cs_stage_book(d_seeds=0x1000, d_base_seed=0x1000, d_epoch=0x1000, d_staged_seed=0x1000, d_staged_status=0x1000,
                              d_failed=0x1000, seed_stride=0, depth=1, d_pending=0x1000)
        rc = lib.cs_gym_step_staged_policy(*head, C.byref(gen), C.byref(desc), C.byref(sb), *tail)
    else:
        rc = lib.cs_gym_step_policy(*head, *tail)
    assert rc == _l.CS_ERR_ARG, (change, rc)
    assert fragment in lib.cs_last_error().decode(), lib.cs_last_error()
    with pytest.raises(ValueError, match=re.escape(fragment)):
        _l.check(rc)


def test_null_descriptor_and_variant_query_are_refused():
    _l, lib = _lib()
    buf = C.create_string_buffer(64)
    assert lib.cs_gym_step_policy_variant(None, buf, C.c_size_t(64)) == _l.CS_ERR_ARG
    cfg = (C.c_float * 5)()
    dev = C.c_void_p(0x1000)
    book = _l.cs_gym_book(clock_len=4)
    assert lib.cs_gym_step_policy(None, C.c_float(0.01), C.c_int(1), dev, C.c_float(0.25), dev, cfg, dev, C.byref(book), C.c_int(0), dev,
                                  C.c_int(0), C.c_float(0.25), None, None) == _l.CS_ERR_ARG


def _env():
    from test_gpu_generators import _config

    from social_navigation_pyenvs_amd.social_gym.social_nav_gym import BatchedSocialNavGym

    return BatchedSocialNavGym(_config("hybrid_scenario", human_num=5, policy="sfm_guo"), 4)


def test_act_step_device_exists_and_refuses_the_policies_it_does_not_take():
    from social_navigation_pyenvs_amd.crowd_nav.policy.cadrl import CADRL
    from social_navigation_pyenvs_amd.social_gym.sharded_gym import ShardedBatchedSocialNavGym
    from social_navigation_pyenvs_amd.social_gym.social_nav_gym import BatchedSocialNavGym

    assert callable(getattr(BatchedSocialNavGym, "act_step_device"))
    assert "act_step_device" not in vars(ShardedBatchedSocialNavGym)     # reached through its __getattr__, not implemented twice
    env = _env()
    with pytest.raises(TypeError, match="act_device"):                    # a value-based policy: the message names the call that takes it
        env.act_step_device(CADRL())
    with pytest.raises(TypeError):
        env.act_step_device(object())
    with pytest.raises(TypeError):                                        # explore= belongs to act_device's value-based policies
        env.act_step_device("bp", explore=None)
    with pytest.raises(RuntimeError, match="device=True"):                # a well-formed call needs worlds generated on the device
        env.act_step_device("bp")
    # the existing calls keep their signatures
    import inspect

    assert list(inspect.signature(BatchedSocialNavGym.step_device).parameters) == ["self", "actions", "auto_reset"]
    assert list(inspect.signature(BatchedSocialNavGym.act_device).parameters) == ["self", "policy", "explore"]
    assert list(inspect.signature(BatchedSocialNavGym.act_step_device).parameters) == ["self", "policy", "auto_reset"]
