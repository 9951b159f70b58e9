"""CPU side of the value network on the worlds' current state (cs_value_net_state, csrc/value_net_state.hip): the exported
symbol, its argument checks without a device, golden G19 (the reference's ``MultiHumanRL.transform`` and value networks on 24 joint
states) against its own float64 restatement, and the refusals of ``BatchedSocialNavGym.joint_state_device`` / ``value_device`` that need
no GPU.  The kernel itself is tests/test_gpu_value_state.py, which takes ``g19`` and ``g19_policy`` from here."""
import ctypes as C
import functools
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
from golden_io import load_cases  # noqa: E402

from test_value_policy_cpu import make_policy  # noqa: E402

F32 = np.float32
ROW_SLACK = 5e-6        # the kernel-vs-float64 bar of tests/test_lookahead.py, added to the reference's own float32 error
_CADRL = [4, 150, 100, 100, 1]
_SARL = [1, 2, 150, 100, 2, 100, 50, 3, 100, 100, 1, 4, 150, 100, 100, 1]
_POINTERS = ("d_weights", "d_current", "d_robot", "d_values")


@functools.lru_cache(maxsize=None)
def g19():
    """golden G19: ({wkey: weights case}, {cols: states case})"""
    cases = load_cases("g19_transform")
    return ({c["wkey"]: c for c in cases if c["kind"] == "weights"}, {int(c["cols"]): c for c in cases if c["kind"] == "states"})


def g19_weights(model, case):
    """tests/golden/make_golden_g19.py draw_weights, restated: the weights of a G19 network from its recorded seed -- numpy's frozen
    RandomState stream in the sorted order of the state_dict keys, N(0, 0.25) matrices, N(0, 0.1) biases, SARL's attention output layer
    times 0.1 -- checked against the recorded SHA-256 of their float32 bytes."""
    import torch

    sd = model.state_dict()
    assert sorted(sd) == list(case["weights_keys"]) and [list(sd[k].shape) for k in sorted(sd)] == case["weights_shapes"]
    rs = np.random.RandomState(int(case["seed"]))
    last = max((k for k in sd if k.startswith("attention.") and k.endswith(".weight")), key=lambda k: int(k.split(".")[1]), default=None)
    h = hashlib.sha256()
    with torch.no_grad():
        for key in sorted(sd):
            w = (rs.standard_normal(tuple(sd[key].shape)) * (0.25 if sd[key].dim() > 1 else 0.1)).astype(F32)
            if case["calm"] and last and key.rsplit(".", 1)[0] == last.rsplit(".", 1)[0]:
                w = w * F32(0.1)
            sd[key].copy_(torch.from_numpy(w))
            h.update(key.encode() + b"\0" + np.ascontiguousarray(w).tobytes())
    assert h.hexdigest() == case["sha256"], "the seeded weights are not the ones the fixture's values were recorded with"


def g19_policy(name, cols):
    """A configured policy of this project with the weights of G19's network `name`_`cols`"""
    pol = make_policy(name, **(dict(sarl__with_theta_and_omega_visible="true") if cols == 15 else {}))
    g19_weights(pol.model, g19()[0][f"{name}_{cols}"])
    return pol


def g19_reference_row_error():
    """The reference's own float32 error on G19's rows: max |transform - float64 restatement| over the whole fixture"""
    return max(float(np.max(np.abs(c["rows"].astype(np.float64) - c["rows64"]))) for c in g19()[1].values())


def test_the_symbol_is_declared_listed_and_exported():
    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(_lib._PKG), "include", "crowdstep.h")).read()
    sym = "cs_value_net_state"
    assert sym in _lib.ABI_SYMBOLS and hasattr(lib, sym) and f"int {sym}(" in header
    assert _lib.ABI_VERSION == 4 and lib.cs_abi_version() == 4 and "#define CS_ABI_VERSION 4" in header


def _call(**change):
    """cs_value_net_state on fake pointers (never followed: every call here fails a check)"""
    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    a = dict(kind=0, dims=_CADRL, W=4, n=5, headed=0, robot_stride=9, n_weight_floats=None, null=(), rewards=True, rotated_out=True)
    a.update(change)
    dims = np.array(a["dims"], np.int32)
    nf = C.c_size_t(0)
    if a["n_weight_floats"] is None:
        lib.cs_value_net_pack(C.c_int(0), np.array(_CADRL, np.int32).ctypes.data_as(C.c_void_p), C.c_int(len(_CADRL)), C.c_int(15 if a["headed"] else 13),
                              None, None, C.byref(nf))
        assert nf.value > 0
    else:
        nf = C.c_size_t(a["n_weight_floats"])
    fake = lambda name: None if name in a["null"] else C.c_void_p(0x1000)
    rc = lib.cs_value_net_state(
        C.c_int(a["kind"]), None if "dims" in a["null"] else dims.ctypes.data_as(C.c_void_p), C.c_int(len(dims)), fake("d_weights"), nf,
        C.c_int(a["W"]), C.c_int(a["n"]), C.c_int(a["headed"]), fake("d_current"), fake("d_robot"), C.c_int(a["robot_stride"]),
        C.c_void_p(0x1000) if a["rewards"] else None, C.c_float(0.9), C.c_float(0.25), C.c_void_p(0x1000) if a["rotated_out"] else None,
        fake("d_values"), None)
    return rc, lib.cs_last_error().decode()


@pytest.mark.parametrize("change,fragment", [
    (dict(kind=2), "unknown value network kind"),
    (dict(kind=-1), "unknown value network kind"),
    (dict(null=("dims",)), "null or empty layer description"),
    (dict(kind=1, dims=_SARL[:-5]), "layer description ends early"),
    (dict(W=0), "W must be positive"),
    (dict(W=-3), "W must be positive"),
    (dict(n=0), "n must be at least 1"),
    *[(dict(null=(name,)), "null argument") for name in _POINTERS],
    (dict(n_weight_floats=5), "does not have the size"),
    (dict(robot_stride=7), "robot rows need at least 8 columns"),
])
def test_the_entry_point_checks_its_arguments_before_touching_a_device(change, fragment):
    """CS_ERR_ARG with cs_value_net_decide's messages where the checks overlap, no device present."""
    from social_navigation_pyenvs_amd import _lib

    rc, message = _call(**change)
    assert rc == _lib.CS_ERR_ARG
    assert fragment in message
    with pytest.raises(ValueError, match="crowdstep"):
        _lib.check(rc)


def test_the_checks_come_in_the_order_of_the_decision():
    """check_decide_args' order: W, n, the pointers, the blob's size, the robot stride."""
    order = [dict(W=0), dict(n=0), dict(null=("d_current",)), dict(n_weight_floats=5), dict(robot_stride=7)]
    fragments = ["W must be positive", "n must be at least 1", "null argument", "does not have the size", "robot rows need"]
    for i, fragment in enumerate(fragments):
        merged = {}
        for later in order[i:]:
            merged.update(later)
        assert fragment in _call(**merged)[1], (i, merged)


@pytest.mark.parametrize("missing", [dict(rewards=False), dict(rotated_out=False), dict(rewards=False, rotated_out=False)])
def test_null_rewards_and_null_rotated_out_pass_the_checks(missing):
    """Both are optional: with them NULL the checks hold exactly as with them given -- the same later check fails with the same message,
    and no check names them.  (Past the checks the call needs a device.)"""
    from social_navigation_pyenvs_amd import _lib

    for later in (dict(robot_stride=7), dict(n_weight_floats=5)):
        with_both, without = _call(**later), _call(**missing, **later)
        assert with_both == without and without[0] == _lib.CS_ERR_ARG and "null argument" not in without[1]


def test_g19_loads_and_its_float64_restatement_agrees_with_the_reference_rows():
    """24 states, n in {1, 5}, 13 and 15 columns, the goal at least 1 m away; the recorded transform against the fixture's own float64
    restatement of rotate: within float32 rounding of the rows' magnitude (a few ulp of values below 16: sums of two products and the
    float32 cos / sin), which is the reference's own error the GPU suite's row bar starts from."""
    weights, states = g19()
    assert sorted(weights) == ["cadrl_13", "cadrl_15", "sarl_13", "sarl_15"] and sorted(states) == [13, 15]
    total = 0
    for cols, c in states.items():
        n, off = c["n"], c["offset"]
        total += len(n)
        assert sorted(set(n.tolist())) == [1, 5] and c["humans"].shape == (int(n.sum()), cols - 8)
        assert c["rows"].dtype == F32 and c["rows"].shape == c["rows64"].shape == (int(n.sum()), cols)
        assert c["cadrl"].shape == (int(n.sum()),) and c["sarl"].shape == (len(n),) and off.tolist() == np.concatenate([[0], np.cumsum(n)[:-1]]).tolist()
        assert np.all(np.hypot(c["robot"][:, 5] - c["robot"][:, 0], c["robot"][:, 6] - c["robot"][:, 1]) >= 1.0)
        assert np.all(np.isfinite(c["cadrl"])) and np.all(np.isfinite(c["sarl"]))
        assert np.array_equal(c["robot"], c["robot"].astype(F32).astype(np.float64)) and np.array_equal(c["humans"], c["humans"].astype(F32).astype(np.float64))
    assert total == 24
    err = g19_reference_row_error()
    print(f"G19: the reference's float32 transform against the float64 restatement: max |difference| {err:.3e}")
    assert 0.0 < err < 16 * 8 * float(np.finfo(F32).eps)       # 8 ulp at magnitude 16: 1.5e-5


@pytest.mark.parametrize("name,cols", [("cadrl", 13), ("sarl", 13), ("cadrl", 15), ("sarl", 15)])
def test_the_shipped_modules_reproduce_g19_on_the_host(name, cols):
    """The weights rebuilt from the recorded seed are the recorded ones (SHA-256), and the shipped torch module on the shipped ``rotate``
    gives the reference's rows (within the row bar) and values (1e-4 relative to max(1, max |V|)) on the host."""
    import torch

    pol = g19_policy(name, cols)
    c = g19()[1][cols]
    bar = g19_reference_row_error() + ROW_SLACK
    for i, (n, off) in enumerate(zip(c["n"], c["offset"])):
        joint = np.concatenate([np.repeat(c["robot"][i][None], n, 0), c["humans"][off:off + n]], 1).astype(F32)
        rows = pol.rotate(torch.from_numpy(joint), theta_and_omega_visible=cols == 15)
        assert float(np.max(np.abs(rows.numpy().astype(np.float64) - c["rows64"][off:off + n]))) <= bar
        with torch.no_grad():
            out = pol.model(torch.from_numpy(c["rows"][off:off + n])[None])
        ref = c["cadrl"][off:off + n] if name == "cadrl" else c["sarl"][i:i + 1]
        scale = max(1.0, float(np.max(np.abs(ref))))
        assert float(np.max(np.abs(out.numpy().reshape(-1).astype(np.float64) - ref))) / scale < 1e-4


def _env(headed=False):
    from test_gpu_generators import _config

    from social_navigation_pyenvs_amd.social_gym.social_nav_gym import BatchedSocialNavGym

    return BatchedSocialNavGym(_config("hybrid_scenario", human_num=5, policy="sfm_guo"), 8, headed_obs=headed)


@pytest.mark.parametrize("method", ["joint_state_device", "value_device"])
def test_the_gym_refuses_without_a_gpu(method):
    """A unicycle policy, a headed mismatch (either way), an unconfigured policy, something that is no value-based policy, rewards
    without bootstrap: raised before anything touches the device (no world has been generated, no GPU is asked for)."""
    from social_navigation_pyenvs_amd.crowd_nav.policy.policy_factory import policy_factory

    call = lambda env, pol, **kw: getattr(env, method)(pol, **kw)
    pol = make_policy("sarl")
    pol.kinematics = "unicycle"
    with pytest.raises(ValueError, match="holonomic robot"):
        call(_env(), pol)
    with pytest.raises(ValueError, match="with_theta_and_omega_visible and the batch's headed_obs differ"):
        call(_env(headed=True), make_policy("cadrl"))
    with pytest.raises(ValueError, match="with_theta_and_omega_visible and the batch's headed_obs differ"):
        call(_env(), make_policy("sarl", sarl__with_theta_and_omega_visible="true"))
    with pytest.raises(AttributeError, match="configure"):
        call(_env(), policy_factory["sarl"]())
    with pytest.raises(TypeError, match="value-based policy"):
        call(_env(), "bp")
    if method == "value_device":
        with pytest.raises(ValueError, match="bootstrap=True"):
            call(_env(), make_policy("sarl"), rewards=object())
    # a good policy gets as far as the missing device-generated batch
    with pytest.raises(RuntimeError, match=r"reset\(\.\.\., device=True\)"):
        call(_env(), make_policy("sarl"))


def test_state_net_refuses_another_architecture():
    """``model=`` must have the policy's architecture: refused by the description, before any packing."""
    pol = make_policy("sarl")
    other = make_policy("sarl", sarl__mlp2_dims="33").model
    with pytest.raises(ValueError, match="another architecture"):
        pol.state_net(other)
    with pytest.raises(ValueError, match="another architecture"):
        pol.state_net(make_policy("cadrl").model)
