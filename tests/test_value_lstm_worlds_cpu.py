"""CPU suite of LSTM-RL's decision from the resident worlds (cs_value_net_decide_lstm_worlds[_bf16], ``set_recurrent_input``): the symbols,
every refusal of the two entries and of the setter that needs no device, and ``decide_for_worlds``' routing on a stubbed library."""
import ctypes as C
import os

import numpy as np
import pytest

import lstm_cases as lc
from om_lstm_cases import om_lstm_policy
from test_value_om_cpu import om_policy
from test_value_policy_cpu import make_policy

ENTRIES = ("cs_value_net_decide_lstm_worlds", "cs_value_net_decide_lstm_worlds_bf16")
DIMS = [50, 0, 4, 150, 100, 100, 1]
WIDE = [256, 2, 256, 256, 3, 256, 256, 1]


def test_the_symbols_are_declared_listed_and_exported():
    from social_navigation_pyenvs_amd import _lib
    from social_navigation_pyenvs_amd.csrc import build

    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(_lib._PKG), "include", "crowdstep.h")).read()
    for sym in ENTRIES:
        assert sym in _lib.ABI_SYMBOLS and sym in _lib.ABI and hasattr(lib, sym) and f"int {sym}(" in header, sym
    assert _lib.ABI[ENTRIES[0]] == _lib.ABI[ENTRIES[1]] and len(_lib.ABI[ENTRIES[0]][1]) == 22
    assert {"value_net_lstm_worlds.hip", "value_net_lstm_worlds_bf16.hip"} <= set(build.SOURCES)
    assert _lib.ABI_VERSION == 4 and "#define CS_ABI_VERSION 4" in header          # additive entries: the version stays


def _blob_units(entry, dims, cols=13):
    """the length the entry expects of its blob: floats of cs_value_net_pack_lstm, bytes of cs_value_net_pack_lstm_bf16"""
    from social_navigation_pyenvs_amd import _lib

    d = np.ascontiguousarray(dims, np.int32)
    size = C.c_size_t(0)
    pack = "cs_value_net_pack_lstm_bf16" if entry.endswith("bf16") else "cs_value_net_pack_lstm"
    assert getattr(_lib.load(), pack)(d.ctypes.data, len(d), cols, None, None, C.byref(size)) == _lib.CS_OK
    return size.value


def _decide(entry, dims, n_units, W=2, A=3, n=5, headed=0, sorted_by_distance=1, stride=9, null=None):
    """The entry with dummy device addresses: only calls whose checks refuse them before any device call"""
    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    d = np.ascontiguousarray(dims, np.int32)
    dev = {k: 0x1000 for k in ("weights", "actions", "next", "current", "robot", "values", "action_out")}
    if null:
        dev[null] = None
    rc = getattr(lib, entry)(d.ctypes.data, len(d), dev["weights"], n_units, W, A, n, headed, sorted_by_distance, dev["actions"], dev["next"],
                             dev["current"], dev["robot"], stride, 0.9, 0.25, None, None, dev["values"], None, dev["action_out"], None)
    return rc, lib.cs_last_error().decode()


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_entries_check_their_arguments_without_a_device(entry):
    """The return codes and message fragments of cs_value_net_decide_lstm[_bf16] and of cs_value_net_decide_worlds, in this entry's name
    where the sibling gives its own."""
    from social_navigation_pyenvs_amd import _lib

    size, wide_size = _blob_units(entry, DIMS), _blob_units(entry, WIDE)
    for kw, fragment in [
        (dict(W=0), "W and A must be positive"),
        (dict(A=0), "W and A must be positive"),
        (dict(n=0), "n must be at least 1"),
        *[(dict(null=name), "null argument") for name in ("weights", "actions", "next", "current", "robot", "values", "action_out")],
        (dict(n_units=size - 4), "the weight blob does not have the size of this network"),
        (dict(stride=7), "robot rows need at least 8 columns"),
        (dict(sorted_by_distance=2), "sorted_by_distance is 0 or 1"),
        (dict(sorted_by_distance=-1), "sorted_by_distance is 0 or 1"),
        (dict(n=129), f"{entry} takes at most 128 humans a world (CS_VN_LSTM_MAX_N)"),
        # (the widest float32 network at 128 humans: 160 KiB with or without the frame table; the bf16 rows of the same network fit)
        *([] if entry.endswith("bf16") else [(dict(dims=WIDE, n_units=wide_size, n=128), "do not fit the 160 KiB of LDS")]),
    ]:
        kw = dict(kw)
        rc, msg = _decide(entry, kw.pop("dims", DIMS), kw.pop("n_units", size), **kw)
        assert (rc, fragment in msg) == (_lib.CS_ERR_ARG, True), (kw, msg)
    for bad in ([50, 0, 2, 10, 2], [0, 0, 1, 1], [50, 0]):          # the description's errors come through the decision too
        assert _decide(entry, bad, 1)[0] == _lib.CS_ERR_ARG
    # the column count follows from theta_and_omega_visible, and the plan is built for it: a network 2 whose mlp1 reads 15 columns has
    # the blob of 13 (both round up to two k-groups), so the count is checked where it is known, on the DeviceNet (below)
    assert _blob_units(entry, DIMS, 15) == size
    if entry.endswith("bf16"):
        assert _decide(entry, DIMS, size - 1)[1].count("the weight blob does not have the size") == 1        # (no whole number of floats)


def _no_device(monkeypatch):
    from social_navigation_pyenvs_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the device was touched before the refusal")

    monkeypatch.setattr(_lib, "require_gpu", boom)
    monkeypatch.setattr(_lib.DeviceBuffer, "__init__", boom)


@pytest.mark.parametrize("public", ["decide_lstm_worlds", "decide_lstm_worlds_bf16"])
def test_the_python_entries_refuse_other_families_and_a_contradicting_column_count(monkeypatch, public):
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    _no_device(monkeypatch)
    monkeypatch.setattr(value_net, "_head", lambda *a: pytest.fail("the library was reached"))
    call = lambda net, headed: getattr(value_net, public)(net, 1, 3, 5, headed, 1, *([0x1000] * 4), 9, 0.9, 0.25, None, None, 0x1000, None, 0x1000, 0)
    for pol, cols, om in ((make_policy("cadrl"), 13, 0), (make_policy("sarl"), 13, 0), (om_policy(13), 13, om_policy(13).map_columns()),
                          (om_lstm_policy(1), 13, om_lstm_policy(1).map_columns())):
        with pytest.raises(ValueError, match=f"{public}: the network is not an LSTM-RL one without map columns"):
            call(value_net.DeviceNet(pol.model, cols, om), False)
    for cols, headed in ((13, True), (15, False)):
        net = value_net.DeviceNet(lc.lstm_policy(1, cols).model, cols)
        with pytest.raises(ValueError, match=f"{public}: a network of {cols} input columns and headed={headed} differ"):
            call(net, headed)
    net = value_net.DeviceNet(lc.lstm_policy(2).model, 13)
    with pytest.raises(ValueError, match="no recurrent bf16 blob yet" if public.endswith("bf16") else "no f32 blob yet"):
        call(net, False)


def test_the_setter_accepts_and_refuses_per_policy_class(monkeypatch):
    """All six policy classes hold ``recurrent_input`` "tensor"; "fused" is LSTM-RL's alone; every refusal is a ValueError with its reason and
    comes before anything touches the device."""
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net
    from social_navigation_pyenvs_amd.crowd_nav.policy.multi_human_rl import MultiHumanRL

    _no_device(monkeypatch)
    assert value_net.RECURRENT_INPUTS == ("tensor", "fused")
    assert value_net.RECURRENT.worlds == {"f32": ENTRIES[0], "bf16": ENTRIES[1]}
    assert all(f.worlds is None for f in (value_net.FEED_FORWARD, value_net.MAPPED, value_net.RECURRENT_MAPPED))
    for network in (1, 2):
        pol = lc.lstm_policy(network)
        assert pol.recurrent_input == "tensor"
        pol.set_recurrent_input("fused")
        assert (pol.recurrent_input, pol.recurrent_precision, pol.decision_input, pol.decision_precision) == ("fused", "f32", "tensor", "f32")
        pol.set_recurrent_precision("bf16")             # the two combine freely, in either order
        assert (pol.recurrent_input, pol.recurrent_precision) == ("fused", "bf16")
        pol.set_recurrent_input("tensor")
        pol.set_recurrent_input("fused")
        for bad in ("lookahead", "FUSED", None, 1, ""):
            with pytest.raises(ValueError, match="recurrent input .*: one of 'tensor', 'fused'"):
                pol.set_recurrent_input(bad)
        assert pol.recurrent_input == "fused"
        with pytest.raises(ValueError, match="recurrent network: LSTM-RL has the one kernel"):       # the sentence existing tests pin
            pol.set_decision_input("fused")
        assert pol.decision_input == "tensor"
    om = om_lstm_policy(1)
    with pytest.raises(ValueError, match="pairs every row with a map and has no loader that generates the rows"):
        om.set_recurrent_input("fused")
    for pol in (make_policy("cadrl"), make_policy("sarl"), om_policy(13), MultiHumanRL()):
        with pytest.raises(ValueError, match="not an LSTM-RL one .*set_decision_input"):
            pol.set_recurrent_input("fused")
    for pol in (om, make_policy("cadrl"), make_policy("sarl"), om_policy(13), MultiHumanRL()):
        assert pol.recurrent_input == "tensor"
        with pytest.raises(ValueError, match="one of 'tensor', 'fused'"):
            pol.set_recurrent_input("rows")
        pol.set_recurrent_input("tensor")
        assert pol.recurrent_input == "tensor"
    # the check itself, for who holds a family and for who holds none
    assert value_net.check_recurrent_input("fused") == "fused" and value_net.check_recurrent_input("fused", value_net.RECURRENT) == "fused"
    for family in (value_net.FEED_FORWARD, value_net.MAPPED, value_net.RECURRENT_MAPPED):
        assert value_net.check_recurrent_input("tensor", family) == "tensor"
        with pytest.raises(ValueError, match='recurrent input "fused"'):
            value_net.check_recurrent_input("fused", family)


class _StubLibrary:
    """Records the entries called; every one answers CS_OK"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0

        return entry


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_decide_for_worlds_routes_a_fused_recurrent_decision_to_one_call(monkeypatch, precision):
    import torch

    from social_navigation_pyenvs_amd import _lib
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    stub = _StubLibrary()
    monkeypatch.setattr(_lib, "load", lambda: stub)
    monkeypatch.setattr(value_net, "lookahead", lambda *a, **k: pytest.fail("a fused decision ran the look-ahead"))
    net = value_net.DeviceNet(lc.lstm_policy(1).model, 13)
    net.blobs["f32"], net.blobs[value_net.RECURRENT_BF16] = torch.zeros(12), torch.zeros(40, dtype=torch.uint8)
    W, A, n = 3, 81, 5
    acts, nxt, cur, rob = torch.zeros(A, 2), torch.zeros(W, n, 4), torch.zeros(W, n, 5), torch.zeros(W, 9)
    vals, pick, act = torch.zeros(W, A), torch.zeros(W, dtype=torch.int32), torch.zeros(W, 2)
    out = value_net.decide_for_worlds(net, "tensor", "f32", acts, nxt, cur, rob, 0.9, 0.25, None, vals, pick, act, 0, recurrent_precision=precision,
                                      recurrent_input="fused")
    assert out == (None, None)
    (name, args), = stub.calls
    blob = net.blobs["f32" if precision == "f32" else value_net.RECURRENT_BF16]
    assert name == value_net.RECURRENT.worlds[precision] and len(args) == len(_lib.ABI[name][1])
    assert args[2:9] == (blob.data_ptr(), blob.numel(), W, A, n, False, 1) and args[9:14] == (acts.data_ptr(), nxt.data_ptr(), cur.data_ptr(), rob.data_ptr(), 9)
    assert args[16:] == (None, None, vals.data_ptr(), pick.data_ptr(), act.data_ptr(), 0)
    # the pinned sentence of the feed-forward input, a bad name and another family: refused before the library is reached
    stub.calls.clear()
    with pytest.raises(ValueError, match="recurrent network: LSTM-RL has the one kernel"):
        value_net.decide_for_worlds(net, "fused", "f32", acts, nxt, cur, rob, 0.9, 0.25, None, vals, pick, act, 0, recurrent_input="fused")
    with pytest.raises(ValueError, match="one of 'tensor', 'fused'"):
        value_net.decide_for_worlds(net, "tensor", "f32", acts, nxt, cur, rob, 0.9, 0.25, None, vals, pick, act, 0, recurrent_input="worlds")
    # ... and what the tensor path refuses of the other families' arguments, with its sentences
    for kw, sentence in ((dict(mapped_precision="bf16"), "kernel of OM-LSTM-RL"), (dict(wide_precision="bf16"), "kernel of OM-SARL"),
                         (dict(mapped_precision="half"), "mapped precision 'half': one of"), (dict(wide_precision="fp8"), "wide precision 'fp8': one of")):
        with pytest.raises(ValueError, match=sentence):
            value_net.decide_for_worlds(net, "tensor", "f32", acts, nxt, cur, rob, 0.9, 0.25, None, vals, pick, act, 0, recurrent_input="fused", **kw)
    sarl = value_net.DeviceNet(make_policy("sarl").model, 13)
    with pytest.raises(ValueError, match="not an LSTM-RL one"):
        value_net.decide_for_worlds(sarl, "tensor", "f32", acts, nxt, cur, rob, 0.9, 0.25, None, vals, pick, act, 0, recurrent_input="fused")
    assert stub.calls == []
