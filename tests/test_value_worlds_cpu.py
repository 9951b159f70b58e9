"""CPU side of the value-network decision from the resident worlds (cs_value_net_decide_worlds, csrc/value_net_worlds.hip):
the exported symbol, its argument checks without a device, and the policies' ``set_decision_input``.  The kernel against cs_lookahead +
cs_value_net_decide is tests/test_gpu_value_worlds.py."""
import ctypes as C

import numpy as np
import pytest

from test_value_policy_cpu import make_policy

_CADRL = [4, 150, 100, 100, 1]
_SARL = [1, 2, 150, 100, 2, 100, 50, 3, 100, 100, 1, 4, 150, 100, 100, 1]
_POINTERS = ("d_weights", "d_actions", "d_next", "d_current", "d_robot", "d_values", "d_action_out")


def test_the_symbol_is_declared_listed_and_exported():
    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    header = open(_lib.os.path.join(_lib.os.path.dirname(_lib._PKG), "include", "crowdstep.h")).read()
    sym = "cs_value_net_decide_worlds"
    assert sym in _lib.ABI_SYMBOLS and hasattr(lib, sym) and f"int {sym}(" in header
    assert _lib.ABI_VERSION == 4 and lib.cs_abi_version() == 4 and "#define CS_ABI_VERSION 4" in header


def _call(**change):
    """cs_value_net_decide_worlds on fake pointers (never followed: every row here fails a check, or stops at the one that needs a device)"""
    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    a = dict(kind=0, dims=_CADRL, W=4, A=81, n=5, headed=0, robot_stride=9, n_weight_floats=None, null=(), rewards_out=True)
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
    rc = lib.cs_value_net_decide_worlds(
        C.c_int(a["kind"]), None if "dims" in a["null"] else dims.ctypes.data_as(C.c_void_p), C.c_int(len(dims)), fake("d_weights"), nf,
        C.c_int(a["W"]), C.c_int(a["A"]), C.c_int(a["n"]), C.c_int(a["headed"]), fake("d_actions"), fake("d_next"), fake("d_current"), fake("d_robot"),
        C.c_int(a["robot_stride"]), C.c_float(0.9), C.c_float(0.25), None, C.c_void_p(0x1000) if a["rewards_out"] else None, fake("d_values"), None,
        fake("d_action_out"), None)
    return rc, lib.cs_last_error().decode()


@pytest.mark.parametrize("change,fragment", [
    (dict(kind=2), "unknown value network kind"),
    (dict(kind=-1), "unknown value network kind"),
    (dict(dims=[4, 150, 300, 100, 1]), "layer widths must be between 1 and 256"),
    (dict(dims=[4, 150, 100, 100, 2]), "end in one output"),
    (dict(dims=[5, 150, 100, 100, 1]), "a chain needs at least one layer and its widths"),
    (dict(kind=1, dims=_SARL[:-5]), "layer description ends early"),
    (dict(kind=1, dims=_SARL + [3]), "trailing entries"),
    (dict(null=("dims",)), "null or empty layer description"),
    (dict(n=0), "n must be at least 1"),
    (dict(W=0), "W and A must be positive"),
    (dict(A=0), "W and A must be positive"),
    *[(dict(null=(name,)), "null argument") for name in _POINTERS],
    (dict(n_weight_floats=5), "does not have the size"),
    (dict(robot_stride=7), "robot rows need at least 8 columns"),
])
def test_the_entry_point_checks_its_arguments_before_touching_a_device(change, fragment):
    """The union of cs_value_net_decide's and cs_lookahead's checks with their messages: CS_ERR_ARG, no device present."""
    from social_navigation_pyenvs_amd import _lib

    rc, message = _call(**change)
    assert rc == _lib.CS_ERR_ARG
    assert fragment in message
    with pytest.raises(ValueError, match="crowdstep"):
        _lib.check(rc)


def test_a_null_rewards_out_passes_the_checks():
    """d_rewards_out is optional: with it NULL the checks hold exactly as with it given -- the same later check fails with the same message,
    and no check names it.  (Past the checks the call needs a device.)"""
    from social_navigation_pyenvs_amd import _lib

    for later in (dict(robot_stride=7), dict(n_weight_floats=5)):
        with_out, without = _call(**later), _call(rewards_out=False, **later)
        assert with_out == without and without[0] == _lib.CS_ERR_ARG and "null argument" not in without[1]


def test_decision_input_setter():
    for name in ("cadrl", "sarl"):
        pol = make_policy(name)
        assert pol.decision_input == "tensor" and pol.decision_precision == "f32"
        pol.set_decision_input("fused")
        assert pol.decision_input == "fused"
        for bad in ("Fused", "worlds", None, 1, ""):
            with pytest.raises(ValueError, match="decision input"):
                pol.set_decision_input(bad)
        assert pol.decision_input == "fused"
        # "fused" + "bf16" is refused by whichever setter would complete the pair, and nothing changes
        with pytest.raises(ValueError, match="bf16 kernel has its own tile loader"):
            pol.set_decision_precision("bf16")
        assert (pol.decision_input, pol.decision_precision) == ("fused", "f32")
        pol.set_decision_input("tensor")
        pol.set_decision_precision("bf16")
        with pytest.raises(ValueError, match="bf16 kernel has its own tile loader"):
            pol.set_decision_input("fused")
        assert (pol.decision_input, pol.decision_precision) == ("tensor", "bf16")
        pol.set_decision_precision("f32")
        pol.set_decision_input("fused")
        assert (pol.decision_input, pol.decision_precision) == ("fused", "f32")
