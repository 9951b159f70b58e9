"""CPU suite of LSTM-RL: the policy classes against the reference's recorded networks (golden G21), the float64 restatement the GPU suite
measures against, cs_value_net_pack_lstm's blob against the layout include/crowdstep.h documents, and every refusal that needs no device."""
import ctypes as C
import os

import numpy as np
import pytest

import lstm_cases as lc

F32 = np.float32


def test_the_symbols_are_declared_listed_and_exported():
    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(_lib._PKG), "include", "crowdstep.h")).read()
    for sym in ("cs_value_net_pack_lstm", "cs_value_net_decide_lstm"):
        assert sym in _lib.ABI_SYMBOLS and hasattr(lib, sym) and f"int {sym}(" in header, sym
    assert _lib.ABI_VERSION == 4 and lib.cs_abi_version() == 4 and "#define CS_ABI_VERSION 4" in header
    assert "#define CS_VN_LSTM_MAX_N 128" in header


def test_the_factory_key_configures_from_the_references_keys():
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.policy import lstm_rl
    from social_navigation_pyenvs_amd.crowd_nav.policy.policy_factory import policy_factory

    assert policy_factory["lstm_rl_device"] is lstm_rl.LstmRL
    pol = lc.lstm_policy(1)
    assert pol.name == "LSTM-RL" and pol.multiagent_training is True and pol.with_om is False and pol.with_interaction_module is False
    assert isinstance(pol.model, lstm_rl.ValueNetwork1) and isinstance(pol.model.lstm, torch.nn.LSTM) and pol.model.lstm.batch_first
    assert (pol.model.lstm.input_size, pol.model.lstm.hidden_size, pol.model.lstm_hidden_dim, pol.model.self_state_dim) == (13, 50, 50, 6)
    pol2 = lc.lstm_policy(2, 15, lstm_rl__global_state_dim=33, lstm_rl__mlp1_dims="40, 20", lstm_rl__mlp2_dims="70, 1")
    assert isinstance(pol2.model, lstm_rl.ValueNetwork2) and pol2.interaction_module_dims == [40, 20] and pol2.with_interaction_module is True
    assert (pol2.model.lstm.input_size, pol2.model.lstm.hidden_size) == (20, 33) and pol2.model.mlp1[0].in_features == 15
    assert not isinstance(pol2.model.mlp1[-1], torch.nn.ReLU)                   # lstm_rl.py: mlp() without last_relu, unlike SARL's mlp1
    assert pol2.model.mlp[0].in_features == 6 + 33 and [m.out_features for m in pol2.model.mlp if hasattr(m, "out_features")] == [70, 1]
    # the old key keeps raising, and names the new one
    with pytest.raises(NotImplementedError, match="recurrent") as e:
        policy_factory["lstm_rl"]()
    assert "lstm_rl_device" in str(e.value)


@pytest.mark.parametrize("wkey", ["lstm1_13", "lstm1_15", "lstm2_13"])
def test_state_dict_is_the_references_and_the_modules_reproduce_g21(wkey):
    """The state_dict keys and shapes are G21's recorded ones (a reference checkpoint loads with strict=True); with the recorded weights the
    torch modules reproduce the reference's forward and transform outputs, and the float64 restatement agrees to the recorded E_ref."""
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.utils.state import FullState, JointState, ObservableState, ObservableStateHeaded

    case = next(c for c in lc.g21()["weights"] if c["wkey"] == wkey)
    pol = lc.g21_policy(wkey)                                   # asserts the keys, the shapes and the SHA-256 of the rebuilt weights
    sd = pol.model.state_dict()
    assert {"lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0", "mlp.0.weight", "mlp.6.bias"} <= set(sd)
    H, cols = 50, int(case["cols"])
    assert tuple(sd["lstm.weight_ih_l0"].shape) == (4 * H, 50 if case["network"] == 2 else cols) and tuple(sd["lstm.weight_hh_l0"].shape) == (4 * H, H)
    other = lc.lstm_policy(int(case["network"]), cols)
    other.model.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    pol.set_device(torch.device("cpu"))
    w64 = lc.weights64(pol.model)
    conditions = next((c for c in lc.g21().get("conditions", []) if c["wkey"] == wkey), None)
    worst = 0.0
    for c in (c for c in lc.g21()["forward"] if c["wkey"] == wkey):
        got = lc.torch_values(pol.model, c["rows"])
        assert np.allclose(got, c["out"], rtol=1e-5, atol=1e-5), float(np.max(np.abs(got - c["out"])))
        worst = max(worst, float(np.max(np.abs(got - lc.forward64(w64, c["rows"])) / np.maximum(1.0, np.abs(got)))))
    for c in (c for c in lc.g21()["transform"] if c["wkey"] == wkey):
        headed = bool(c["headed"])
        for i, (n, off) in enumerate(zip(c["n"], c["offset"])):
            state = JointState(FullState(*[float(x) for x in c["robot"][i]]),
                               [(ObservableStateHeaded if headed else ObservableState)(*[float(x) for x in h]) for h in c["humans"][off:off + n]])
            rows = pol.transform(state).numpy()
            assert rows.shape == (n, cols) and np.allclose(rows, c["rows"][off:off + n], rtol=1e-5, atol=1e-5)     # the humans' own order
            got = float(lc.torch_values(pol.model, c["rows"][off:off + n][None])[0])
            assert abs(got - float(c["out"][i])) <= 1e-5 * max(1.0, abs(got))
    if conditions is not None:          # the restatement against torch's module: within the recorded E_ref's order on unit-scale values
        assert conditions["min_da"] > 1e-5 and conditions["flips"] == 0 and conditions["min_gap"] >= 8 * conditions["e_ref"]
        assert worst <= 4 * conditions["e_ref"], (worst, conditions["e_ref"])


def test_the_order_rule():
    assert np.array_equal(lc.decision_order([0.5, 2.0, 1.0]), [1, 2, 0])
    assert np.array_equal(lc.decision_order([1.0, 2.0, 1.0, 2.0]), [3, 1, 2, 0])            # ties by decreasing human index
    rot = np.zeros((2, 3, 13))
    rot[..., 11] = [[0.5, 2.0, 1.0], [3.0, 1.0, 2.0]]
    rot[..., 0] = [[0, 1, 2], [0, 1, 2]]
    assert np.array_equal(lc.sort_rows(rot)[..., 0], [[1, 2, 0], [0, 2, 1]])


# ---------------------------------------------------------------------------------------------------------------- the pack entry
@pytest.mark.parametrize("H", [8, 33, 50, 64])
@pytest.mark.parametrize("network", [1, 2])
def test_the_blob_is_the_documented_layout(H, network):
    kw = dict(lstm_rl__global_state_dim=H, lstm_rl__mlp2_dims="70, 33, 1")
    if network == 2:
        kw["lstm_rl__mlp1_dims"] = "40, 20"
    pol = lc.lstm_policy(network, 15 if H == 33 else 13, **kw)
    lc.draw_weights(pol.model, 40 + H)
    dims, arrays = lc.model_dims(pol.model), lc.model_arrays(pol.model)
    cols = pol.joint_state_dim
    rc, msg, size = lc.pack_call(dims, cols, None, size_only=True)
    want = lc.layout_blob(dims, arrays)
    assert (rc, size) == (0, want.size), msg
    rc, msg, blob = lc.pack_call(dims, cols, arrays)
    assert rc == 0, msg
    assert blob.tobytes() == want.tobytes()
    # the seam packs the same bytes, and describes the network with the same dims
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    kind, d, layers = value_net.describe(pol.model)
    assert kind == value_net.CS_VN_LSTM and d.tolist() == dims
    params = [p.detach().numpy() for l in layers for p in value_net.layer_params(l)]
    assert value_net.pack(kind, d, cols, params).tobytes() == want.tobytes()


PACK_ERRORS = [
    ([50, 0, 4, 150, 100, 100, 1], 14, "rotated rows have 13 or 15 columns"),
    ([], 13, "null or empty layer description"),
    ([50, 0, 1], 13, "null or empty layer description"),
    ([0, 0, 1, 1], 13, "the LSTM's hidden width must be between 1 and 256"),
    ([257, 0, 1, 1], 13, "the LSTM's hidden width must be between 1 and 256"),
    ([50, -1, 1, 1], 13, "mlp1 has zero or more layers, mlp at least one, each with its widths"),
    ([50, 0, 0, 1], 13, "mlp1 has zero or more layers, mlp at least one, each with its widths"),
    ([50, 3, 10, 10], 13, "mlp1 has zero or more layers, mlp at least one, each with its widths"),
    ([50, 1, 10, 2, 1], 13, "mlp1 has zero or more layers, mlp at least one, each with its widths"),
    ([50, 2, 10, 10], 13, "layer description ends early"),
    ([50, 0, 2, 0, 1], 13, "layer widths must be between 1 and 256"),
    ([50, 1, 300, 1, 1], 13, "layer widths must be between 1 and 256"),
    ([50, 9] + [8] * 9 + [8] + [8] * 7 + [1], 13, "at most 16 layers in all"),
    ([50, 0, 2, 10, 2], 13, "mlp ends in one output"),
    ([50, 0, 1, 1, 7], 13, "layer description has trailing entries"),
]


@pytest.mark.parametrize("dims,cols,fragment", PACK_ERRORS)
def test_the_pack_entry_refuses_bad_descriptions(dims, cols, fragment):
    from social_navigation_pyenvs_amd import _lib

    rc, msg, _ = lc.pack_call(dims, cols, None, size_only=True)
    assert (rc, fragment in msg) == (_lib.CS_ERR_ARG, True), msg


def test_the_pack_entry_refuses_null_pointers():
    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    dims = np.array([8, 0, 1, 1], np.int32)
    nf = C.c_size_t(0)
    assert lib.cs_value_net_pack_lstm(dims.ctypes.data, 4, 13, None, None, None) == _lib.CS_ERR_ARG and b"null argument" in lib.cs_last_error()
    assert lib.cs_value_net_pack_lstm(dims.ctypes.data, 4, 13, None, None, C.byref(nf)) == 0 and nf.value > 0
    blob = np.zeros(nf.value, F32)
    assert lib.cs_value_net_pack_lstm(dims.ctypes.data, 4, 13, None, blob.ctypes.data, C.byref(nf)) == _lib.CS_ERR_ARG and b"null argument" in lib.cs_last_error()
    ptrs = (C.c_void_p * 6)(*([blob.ctypes.data] * 5 + [None]))
    assert lib.cs_value_net_pack_lstm(dims.ctypes.data, 4, 13, ptrs, blob.ctypes.data, C.byref(nf)) == _lib.CS_ERR_ARG
    assert b"null weight or bias array" in lib.cs_last_error()


# ---------------------------------------------------------------------------------------------------------------- the decide entry
def _decide(dims, n_floats, W=2, A=3, n=5, cols=13, sorted_by_distance=1, stride=9, null=None):
    """cs_value_net_decide_lstm with dummy device addresses: only calls whose checks refuse them before any device call"""
    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    d = np.ascontiguousarray(dims, np.int32)
    dev = {k: 0x1000 for k in ("weights", "rotated", "rewards", "actions", "robot", "values", "action_out")}
    if null:
        dev[null] = None
    rc = lib.cs_value_net_decide_lstm(d.ctypes.data, len(d), dev["weights"], n_floats, W, A, n, cols, sorted_by_distance, dev["rotated"], dev["rewards"],
                                      dev["actions"], dev["robot"], stride, 0.9, 0.25, None, dev["values"], None, dev["action_out"], None)
    return rc, lib.cs_last_error().decode()


def test_the_decide_entry_checks_its_arguments_without_a_device():
    from social_navigation_pyenvs_amd import _lib

    dims = [50, 0, 4, 150, 100, 100, 1]
    _, _, size = lc.pack_call(dims, 13, None, size_only=True)
    wide = [256, 2, 256, 256, 3, 256, 256, 1]
    _, _, wide_size = lc.pack_call(wide, 13, None, size_only=True)
    for kw, fragment in [
        (dict(cols=12), "rotated rows have 13 or 15 columns"),
        (dict(W=0), "W and A must be positive"),
        (dict(A=0), "W and A must be positive"),
        (dict(n=0), "n must be at least 1"),
        (dict(null="rotated"), "null argument"),
        (dict(null="action_out"), "null argument"),
        (dict(n_floats=size - 1), "the weight blob does not have the size of this network"),
        (dict(stride=7), "robot rows need at least 8 columns"),
        (dict(sorted_by_distance=2), "sorted_by_distance is 0 or 1"),
        (dict(n=129), "at most 128 humans a world (CS_VN_LSTM_MAX_N)"),
        (dict(dims=wide, n_floats=wide_size, n=128), "do not fit the 160 KiB of LDS"),
    ]:
        kw = dict(kw)
        rc, msg = _decide(kw.pop("dims", dims), kw.pop("n_floats", size), **kw)
        assert (rc, fragment in msg) == (_lib.CS_ERR_ARG, True), (kw, msg)
    for bad in ([50, 0, 2, 10, 2], [0, 0, 1, 1]):                   # the description's errors come through the decision too
        assert _decide(bad, 1)[0] == _lib.CS_ERR_ARG


# ---------------------------------------------------------------------------------------------------------------- the policy's refusals
def test_the_policy_refuses_what_it_cannot_run():
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    with pytest.raises(NotImplementedError, match="OM-LSTM-RL"):
        lc.lstm_policy(1, lstm_rl__with_om="true")
    with pytest.raises(ValueError, match="holonomic"):
        lc.lstm_policy(1, action_space__kinematics="unicycle")
    pol = lc.lstm_policy(1)
    with pytest.raises(ValueError, match="recurrent"):
        pol.set_decision_precision("bf16")
    with pytest.raises(ValueError, match="recurrent"):
        pol.set_decision_input("fused")
    with pytest.raises(ValueError, match="one of"):
        pol.set_decision_precision("fp8")
    pol.set_decision_precision("f32")
    pol.set_decision_input("tensor")
    assert (pol.decision_precision, pol.decision_input) == ("f32", "tensor")
    # check_decision_input answers today's callers as before
    assert value_net.check_decision_input("fused", "f32") == "fused" and value_net.check_decision_input("tensor", "bf16") == "tensor"
    with pytest.raises(ValueError, match="own tile loader"):
        value_net.check_decision_input("fused", "bf16")
    with pytest.raises(ValueError, match="occupancy-map"):
        value_net.check_decision_input("fused", "f32", 48)
    kind, dims, layers = value_net.describe(pol.model)
    with pytest.raises(ValueError, match="recurrent"):
        value_net.pack(kind, dims, 13, [], precision="bf16")
    # a DeviceNet's version key covers the LSTM's four tensors
    net = value_net.DeviceNet(pol.model, 13)
    before = net._versions()
    assert len(before) == 2 * 4 + 4
    import torch

    with torch.no_grad():
        pol.model.lstm.bias_hh_l0.add_(1.0)
    assert net._versions() != before
