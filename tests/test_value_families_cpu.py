"""The network families of the value-based policies (value_net.Family: feed-forward CADRL / SARL, map-widened OM-SARL, recurrent LSTM-RL),
from outside: which (decision input, precision) pairs each family accepts and the words it refuses the others with, through
``check_decision_input`` and through the policies' setters; and ``value_net.pack`` against direct calls of the four pack entries.

The expectations were recorded from the code before the family table existed (flags tested in five places); the table must answer the same."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import lstm_cases as lc
from test_value_om_cpu import om_policy
from test_value_policy_cpu import make_policy, seeded_weights

INPUTS = ("tensor", "fused", "lookahead")        # DECISION_INPUTS and a name that is none
PRECISIONS = ("f32", "bf16", "fp8")              # PRECISIONS and a name that is none

BAD_INPUT = "decision input {0!r}: one of 'tensor', 'fused'"
BAD_PRECISION = "decision precision {1!r}: one of 'f32', 'bf16'"
# family -> (check_decision_input's flags, a policy of the family, the sentence it refuses a pair with)
FAMILIES = {
    "feed-forward": (dict(), lambda: make_policy("sarl"),
                     'decision input "fused" with decision precision "bf16": the bf16 kernel has its own tile loader and reads the look-ahead '
                     'tensor; choose "tensor" or "f32"'),
    "mapped": (dict(om_cols=48), lambda: om_policy(),
               'decision input {0!r} with decision precision {1!r} for a network with occupancy-map columns: no kernel pairs the map columns '
               'with the "fused" or the "bf16" tile loader; OM-SARL decides with "tensor" and "f32"'),
    "recurrent": (dict(recurrent=True), lambda: lc.lstm_policy(1),
                  'decision input {0!r} with decision precision {1!r} for a recurrent network: LSTM-RL has the one kernel, float32 on the '
                  'look-ahead tensor; it decides with "tensor" and "f32"'),
}
# what check_decision_input answered for (family, input, precision): None = accepted, else the message's template.  A feed-forward
# network's "tensor" runs in every precision and the function does not look at the precision's name then (the setters do).
REFUSED = "the family's sentence"
RECORDED = {
    "feed-forward": {("tensor", "f32"): None, ("tensor", "bf16"): None, ("tensor", "fp8"): None,
                     ("fused", "f32"): None, ("fused", "bf16"): REFUSED, ("fused", "fp8"): BAD_PRECISION},
    "mapped": {("tensor", "f32"): None, ("tensor", "bf16"): REFUSED, ("tensor", "fp8"): BAD_PRECISION,
               ("fused", "f32"): REFUSED, ("fused", "bf16"): REFUSED, ("fused", "fp8"): REFUSED},
    "recurrent": {("tensor", "f32"): None, ("tensor", "bf16"): REFUSED, ("tensor", "fp8"): BAD_PRECISION,
                  ("fused", "f32"): REFUSED, ("fused", "bf16"): REFUSED, ("fused", "fp8"): REFUSED},
}
for _table in RECORDED.values():
    _table.update({("lookahead", p): BAD_INPUT for p in PRECISIONS})
CASES = [(family, di, p) for family in FAMILIES for di in INPUTS for p in PRECISIONS]


def outcome(call):
    """None when `call` returns, else (exception type, its message)"""
    try:
        call()
    except Exception as e:  # noqa: BLE001
        return type(e), str(e)
    return None


def expected(family, template, di, p):
    if template is None:
        return None
    return ValueError, (FAMILIES[family][2] if template is REFUSED else template).format(di, p)


@pytest.mark.parametrize("family,di,p", CASES)
def test_check_decision_input_answers_as_recorded(family, di, p):
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    flags = FAMILIES[family][0]
    got = outcome(lambda: value_net.check_decision_input(di, p, flags.get("om_cols", 0), flags.get("recurrent", False)))
    assert got == expected(family, RECORDED[family][di, p], di, p)
    if got is None:
        assert value_net.check_decision_input(di, p, **flags) == di


@pytest.mark.parametrize("family,di,p", CASES)
def test_the_setters_answer_as_recorded(family, di, p):
    """set_decision_input(di), then set_decision_precision(p), on a fresh policy ("tensor", "f32"): the first refusal, or both held.  The
    precision's setter looks at the precision's name before the pair."""
    pol = FAMILIES[family][1]()
    first = outcome(lambda: pol.set_decision_input(di))
    assert first == expected(family, RECORDED[family][di, "f32"], di, "f32")
    if first is not None:
        assert (pol.decision_input, pol.decision_precision) == ("tensor", "f32")
        return
    second = outcome(lambda: pol.set_decision_precision(p))
    assert second == expected(family, BAD_PRECISION if p == "fp8" else RECORDED[family][di, p], di, p)
    assert (pol.decision_input, pol.decision_precision) == (di, "f32" if second is not None else p)


def test_the_table_covers_every_declared_mode():
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    assert set(INPUTS[:2]) == set(value_net.DECISION_INPUTS) and set(PRECISIONS[:2]) == set(value_net.PRECISIONS)
    assert len(CASES) == 27 and all(len(t) == 9 for t in RECORDED.values())


# ---------------------------------------------------------------------------------------------------------------- the blobs
def direct_pack(entry, lead, arrays, unit):
    """The size query and the packing call of a pack entry, written out: `lead` are the entry's arguments before the arrays"""
    from social_navigation_pyenvs_amd import _lib

    arrays = [np.ascontiguousarray(a, np.float32) for a in arrays]
    ptrs = (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])
    count = C.c_size_t(0)
    _lib.check(entry(*lead, None, None, C.byref(count)))
    blob = np.zeros(count.value, unit)
    _lib.check(entry(*lead, ptrs, blob.ctypes.data, C.byref(count)))
    return blob


PACK_CASES = [(name, cols) for name in ("cadrl", "sarl", "om_sarl", "lstm_rl 1", "lstm_rl 2") for cols in (13, 15)]


@pytest.mark.parametrize("name,cols", PACK_CASES)
def test_pack_gives_the_bytes_of_the_entry_called_directly(name, cols):
    from social_navigation_pyenvs_amd import _lib
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    headed = dict(sarl__with_theta_and_omega_visible="true") if cols == 15 else {}
    pol = (om_policy(cols) if name == "om_sarl" else lc.lstm_policy(int(name[-1]), cols) if name.startswith("lstm_rl") else make_policy(name, **headed))
    assert pol.joint_state_dim == cols
    seeded_weights(pol.model, 3100 + 2 * PACK_CASES.index((name, cols)))
    kind, dims, layers = value_net.describe(pol.model)
    arrays = [p.detach().numpy() for layer in layers for p in value_net.layer_params(layer)]
    lib, d = _lib.load(), np.ascontiguousarray(dims, np.int32)
    sha = lambda blob: hashlib.sha256(blob.tobytes()).hexdigest()
    if name == "om_sarl":
        assert pol.map_columns() == 48
        want = {"f32": direct_pack(lib.cs_value_net_pack_om, (kind, d.ctypes.data, len(d), cols, 48), arrays, np.float32)}
    elif name.startswith("lstm_rl"):
        want = {"f32": direct_pack(lib.cs_value_net_pack_lstm, (d.ctypes.data, len(d), cols), arrays, np.float32)}
    else:
        want = {"f32": direct_pack(lib.cs_value_net_pack, (kind, d.ctypes.data, len(d), cols), arrays, np.float32),
                "bf16": direct_pack(lib.cs_value_net_pack_bf16, (kind, d.ctypes.data, len(d), cols), arrays, np.uint8)}
    for precision, blob in want.items():
        got = value_net.pack(kind, dims, cols, arrays, precision, pol.map_columns())
        assert got.dtype == blob.dtype and got.size == blob.size > 0 and np.any(blob != 0)
        assert sha(got) == sha(blob), (name, cols, precision)
