"""CPU suite of OM-LSTM-RL (lstm_rl.with_om = true): the two C entries' declarations and refusals, cs_value_net_pack_lstm_om's blob against
the layout include/crowdstep.h documents, the fourth network family, the policy class against the reference's recorded networks and serial
decisions (golden G22), and the float64 restatement with the two pairings of rows and maps."""
import ctypes as C
import os

import numpy as np
import pytest

import lstm_cases as lc
import om_lstm_cases as olc

F32 = np.float32
DEFAULT_DIMS = [50, 0, 4, 150, 100, 100, 1]


def test_the_symbols_are_declared_listed_and_exported():
    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(_lib._PKG), "include", "crowdstep.h")).read()
    for sym in ("cs_value_net_pack_lstm_om", "cs_value_net_decide_lstm_om"):
        assert sym in _lib.ABI_SYMBOLS and sym in _lib.ABI and hasattr(lib, sym) and f"int {sym}(" in header, sym
    assert _lib.ABI_VERSION == 4 and lib.cs_abi_version() == 4 and "#define CS_ABI_VERSION 4" in header
    assert "enum { CS_VN_MAPS_OWN = 0, CS_VN_MAPS_FIRST_ACTION = 1 };" in header
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    assert dict(value_net.MAP_ORDERS) == {"own": 0, "reference": 1}


# ---------------------------------------------------------------------------------------------------------------- the pack entry
@pytest.mark.parametrize("network,cols,grid,H", [(1, 13, (4, 1.0, 3), 50), (2, 13, (4, 1.0, 3), 50), (1, 15, (3, 0.7, 3), 33), (2, 15, (1, 2.0, 1), 8)])
def test_the_blob_is_the_documented_layout(network, cols, grid, H):
    """The default shapes (13 + 48 columns, both networks) and widths that are no multiple of 8 (15 + 27 = 42, 15 + 1 = 16 is one)."""
    kw = dict(lstm_rl__global_state_dim=H)
    if H != 50:
        kw.update(lstm_rl__mlp2_dims="70, 33, 1", lstm_rl__mlp1_dims="40, 20")
    pol = olc.om_lstm_policy(network, cols, grid, **kw)
    om_cols = grid[0] ** 2 * grid[2]
    assert pol.map_columns() == om_cols and pol.input_dim() == cols + om_cols
    lc.draw_weights(pol.model, 60 + H)
    dims, arrays = lc.model_dims(pol.model), lc.model_arrays(pol.model)
    assert arrays[0].shape[1] == cols + om_cols                  # the one wider K: weight_ih (network 1) or mlp1's first weight (network 2)
    want = lc.layout_blob(dims, arrays)
    rc, msg, size = olc.pack_call(dims, cols, om_cols, None, size_only=True)
    assert (rc, size) == (0, want.size), msg
    rc, msg, blob = olc.pack_call(dims, cols, om_cols, arrays)
    assert rc == 0, msg
    assert blob.tobytes() == want.tobytes()
    # value_net.pack through the family is the entry called directly
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    kind, d, layers = value_net.describe(pol.model)
    assert kind == value_net.CS_VN_LSTM and d.tolist() == dims and value_net.family_of(kind, om_cols) is value_net.RECURRENT_MAPPED
    params = [p.detach().numpy() for l in layers for p in value_net.layer_params(l)]
    assert value_net.pack(kind, d, cols, params, om_cols=om_cols).tobytes() == want.tobytes()
    if -(-(cols + om_cols) // 8) != -(-cols // 8):                # more k-groups than the narrow network's first product: a longer blob
        assert want.size > lc.pack_call(dims, cols, None, size_only=True)[2]


@pytest.mark.parametrize("dims,cols,om_cols,fragment", [
    (DEFAULT_DIMS, 13, 0, "om_cols must be at least 1"),
    (DEFAULT_DIMS, 13, -3, "om_cols must be at least 1"),
    (DEFAULT_DIMS, 13, 244, "rotated and map columns together exceed a layer's 256 inputs"),
    (DEFAULT_DIMS, 15, 242, "rotated and map columns together exceed a layer's 256 inputs"),
    (DEFAULT_DIMS, 14, 48, "rotated rows have 13 or 15 columns"),
    ([50, 0, 2, 10, 2], 13, 48, "mlp ends in one output"),
    ([], 13, 48, "null or empty layer description"),
])
def test_the_pack_entry_refuses_bad_descriptions(dims, cols, om_cols, fragment):
    from social_navigation_pyenvs_amd import _lib

    rc, msg, _ = olc.pack_call(dims, cols, om_cols, None, size_only=True)
    assert (rc, fragment in msg) == (_lib.CS_ERR_ARG, True), msg


def test_the_widest_rows_pack():
    assert olc.pack_call(DEFAULT_DIMS, 13, 243, None, size_only=True)[0] == 0 and olc.pack_call(DEFAULT_DIMS, 15, 241, None, size_only=True)[0] == 0


# ---------------------------------------------------------------------------------------------------------------- the decide entry
def _decide(dims, n_floats, W=2, A=3, n=5, cols=13, om_cols=48, sorted_by_distance=1, map_order=1, stride=9, null=None):
    """cs_value_net_decide_lstm_om with dummy device addresses: only calls whose checks refuse them before any device call"""
    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    d = np.ascontiguousarray(dims, np.int32)
    dev = {k: 0x1000 for k in ("weights", "rotated", "maps", "rewards", "actions", "robot", "values", "action_out")}
    if null:
        dev[null] = None
    rc = lib.cs_value_net_decide_lstm_om(d.ctypes.data, len(d), dev["weights"], n_floats, W, A, n, cols, om_cols, sorted_by_distance, map_order,
                                         dev["rotated"], dev["maps"], dev["rewards"], dev["actions"], dev["robot"], stride, 0.9, 0.25, None,
                                         dev["values"], None, dev["action_out"], None)
    return rc, lib.cs_last_error().decode()


def test_the_decide_entry_checks_its_arguments_without_a_device():
    from social_navigation_pyenvs_amd import _lib

    _, _, size = olc.pack_call(DEFAULT_DIMS, 13, 48, None, size_only=True)
    wide = [256, 2, 256, 256, 3, 256, 256, 1]
    _, _, wide_size = olc.pack_call(wide, 13, 48, None, size_only=True)
    wide1 = [256, 0, 1, 1]                                      # network 1: joint rows of 256 + 256 + 4 floats, twice 32 of them, beside the rest
    _, _, wide1_size = olc.pack_call(wide1, 13, 243, None, size_only=True)
    for kw, fragment in [
        (dict(om_cols=0), "om_cols must be at least 1"),
        (dict(om_cols=244), "rotated and map columns together exceed a layer's 256 inputs"),
        (dict(null="maps"), "null argument"),
        (dict(map_order=2), "map_order is CS_VN_MAPS_OWN or CS_VN_MAPS_FIRST_ACTION"),
        (dict(map_order=-1), "map_order is CS_VN_MAPS_OWN or CS_VN_MAPS_FIRST_ACTION"),
        (dict(cols=12), "rotated rows have 13 or 15 columns"),
        (dict(W=0), "W and A must be positive"),
        (dict(n=0), "n must be at least 1"),
        (dict(null="rotated"), "null argument"),
        (dict(n_floats=size - 1), "the weight blob does not have the size of this network"),
        (dict(stride=7), "robot rows need at least 8 columns"),
        (dict(sorted_by_distance=2), "sorted_by_distance is 0 or 1"),
        (dict(n=129), "at most 128 humans a world (CS_VN_LSTM_MAX_N)"),
        (dict(dims=wide, n_floats=wide_size, n=128), "do not fit the 160 KiB of LDS"),
        (dict(dims=wide1, n_floats=wide1_size, om_cols=243, n=128), "do not fit the 160 KiB of LDS"),
    ]:
        kw = dict(kw)
        rc, msg = _decide(kw.pop("dims", DEFAULT_DIMS), kw.pop("n_floats", size), **kw)
        assert (rc, fragment in msg) == (_lib.CS_ERR_ARG, True), (kw, msg)
    # the narrow blob is not this entry's blob
    _, _, narrow = lc.pack_call(DEFAULT_DIMS, 13, None, size_only=True)
    assert _decide(DEFAULT_DIMS, narrow)[0] == _lib.CS_ERR_ARG and narrow != size


# ---------------------------------------------------------------------------------------------------------------- the family
def test_the_family_accepts_one_mode_and_refuses_the_others_in_its_own_words():
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    fam = value_net.RECURRENT_MAPPED
    assert fam.modes == (("tensor", "f32"),) and fam.min_humans == 2 and fam.state_launch is False and fam.takes_maps and not fam.takes_kind
    assert dict(fam.pack) == {"f32": ("cs_value_net_pack_lstm_om", np.float32)} and dict(fam.decide) == {"f32": "cs_value_net_decide_lstm_om"}
    assert value_net.family_of(value_net.CS_VN_LSTM, 48) is fam and value_net.family_of(value_net.CS_VN_LSTM) is value_net.RECURRENT
    assert value_net.family_of(value_net.CS_VN_SARL, 48) is value_net.MAPPED
    assert value_net.check_decision_input("tensor", "f32", 48, recurrent=True) == "tensor"
    for di, p in (("tensor", "bf16"), ("fused", "f32"), ("fused", "bf16")):
        with pytest.raises(ValueError, match="recurrent network with occupancy-map columns: OM-LSTM-RL has the one") as e:
            value_net.check_decision_input(di, p, 48, recurrent=True)
        assert repr(di) in str(e.value) and repr(p) in str(e.value)
    pol = olc.om_lstm_policy(1)
    assert pol.family is fam
    with pytest.raises(ValueError, match="OM-LSTM-RL has the one"):
        pol.set_decision_precision("bf16")
    with pytest.raises(ValueError, match="OM-LSTM-RL has the one"):
        pol.set_decision_input("fused")
    with pytest.raises(ValueError, match="one of"):
        pol.set_decision_precision("fp8")
    assert (pol.decision_precision, pol.decision_input) == ("f32", "tensor")
    with pytest.raises(ValueError, match="OM-LSTM-RL has the one"):
        value_net.pack(*value_net.describe(pol.model)[:2], 13, [], precision="bf16", om_cols=48)
    net = value_net.DeviceNet(pol.model, 13, 48, pol.om_grid())
    assert net.family is fam and net.map_order == "reference" and net.lstm
    with pytest.raises(ValueError, match="map order"):
        value_net.DeviceNet(pol.model, 13, 48, pol.om_grid(), "first")
    narrow = value_net.DeviceNet(lc.lstm_policy(1).model, 13)
    with pytest.raises(ValueError, match="decide_lstm_om"):
        value_net.decide_lstm_om(narrow, 1, 1, 2, 0, 0, 0, 0, 0, 0, 9, 0.9, 0.25, None, 0, None, 0)
    with pytest.raises(ValueError, match="decide_lstm:"):
        value_net.decide_lstm(net, 1, 1, 2, 0, 0, 0, 0, 0, 9, 0.9, 0.25, None, 0, None, 0)


# ---------------------------------------------------------------------------------------------------------------- the policy
def test_the_factory_key_configures_from_the_references_keys():
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.policy import lstm_rl, om_lstm_rl
    from social_navigation_pyenvs_amd.crowd_nav.policy.policy_factory import policy_factory

    assert policy_factory["om_lstm_rl"] is om_lstm_rl.OMLstmRL and issubclass(om_lstm_rl.OMLstmRL, lstm_rl.LstmRL)
    pol = olc.om_lstm_policy(1)
    assert pol.name == "LSTM-RL" and pol.with_om is True and pol.with_interaction_module is False and pol.multiagent_training is True
    assert isinstance(pol.model, lstm_rl.ValueNetwork1) and (pol.model.lstm.input_size, pol.model.lstm.hidden_size) == (61, 50)
    assert pol.map_columns() == 48 and pol.input_dim() == 61 and pol.om_grid() == (4, 1.0, 3) and pol.map_order == "reference"
    pol2 = olc.om_lstm_policy(2, 15)
    assert isinstance(pol2.model, lstm_rl.ValueNetwork2) and pol2.model.mlp1[0].in_features == 63
    assert (pol2.model.lstm.input_size, pol2.model.lstm.hidden_size) == (50, 50) and not isinstance(pol2.model.mlp1[-1], torch.nn.ReLU)
    with pytest.raises(ValueError, match="lstm_rl_device"):
        olc.om_lstm_policy(1, lstm_rl__with_om="false")
    with pytest.raises(NotImplementedError, match="om_channel_size 4"):
        olc.om_lstm_policy(1, om__om_channel_size=4)
    with pytest.raises(ValueError, match="cell_num must be positive"):
        olc.om_lstm_policy(1, om__cell_num=0)
    with pytest.raises(ValueError, match="cell_num must be positive"):
        olc.om_lstm_policy(1, om__cell_size=0.0)
    # the narrow key keeps raising, and names the new one
    with pytest.raises(NotImplementedError, match="OM-LSTM-RL") as e:
        lc.lstm_policy(1, lstm_rl__with_om="true")
    assert "om_lstm_rl" in str(e.value)
    # the pairing: a name of the two, carried by the policy's DeviceNets
    pol.set_map_order("own")
    assert pol.map_order == "own" and pol._new_device_net(pol.model).map_order == "own"
    with pytest.raises(ValueError, match="map order 'positional': one of 'reference', 'own'"):
        pol.set_map_order("positional")
    assert pol.map_order == "own"
    with pytest.raises(ValueError, match="build_occupancy_maps needs at least two humans"):
        pol.build_occupancy_maps([object()])


@pytest.mark.parametrize("wkey", ["omlstm1_13", "omlstm1_15", "omlstm2_13"])
def test_state_dict_is_the_references_and_the_modules_reproduce_g22_forward(wkey):
    """The state_dict keys and shapes are G22's recorded ones (a reference OM-LSTM-RL checkpoint loads with strict=True); with the recorded
    weights the torch modules reproduce the reference's forward outputs and its outputs on its transform rows."""
    import torch

    case = next(c for c in olc.g22()["weights"] if c["wkey"] == wkey)
    assert case["name"] == "LSTM-RL" and case["om_cols"] == 48
    pol = olc.g22_policy(wkey)                                  # asserts the keys, the shapes and the SHA-256 of the rebuilt weights
    sd = pol.model.state_dict()
    cols = int(case["cols"])
    wide_key = "mlp1.0.weight" if case["network"] == 2 else "lstm.weight_ih_l0"
    assert sd[wide_key].shape[1] == cols + 48 and tuple(sd["lstm.weight_hh_l0"].shape) == (200, 50)
    other = olc.om_lstm_policy(int(case["network"]), cols)
    other.model.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    pol.set_device(torch.device("cpu"))
    forward = [c for c in olc.g22()["forward"] if c["wkey"] == wkey]
    assert sorted(c["n"] for c in forward) == [2, 5, 9]
    for c in forward:
        assert c["rows"].shape[2] == cols + 48
        got = lc.torch_values(pol.model, c["rows"])
        assert np.allclose(got, c["out"], rtol=1e-5, atol=1e-5), float(np.max(np.abs(got - c["out"])))
    for c in (c for c in olc.g22()["transform"] if c["wkey"] == wkey):
        for i, (n, off) in enumerate(zip(c["n"], c["offset"])):
            got = float(lc.torch_values(pol.model, c["rows"][off:off + n][None])[0])
            assert abs(got - float(c["out"][i])) <= 1e-5 * max(1.0, abs(got))
            # the reference's rows are the float64 rotated rows beside om_cases' maps, in the humans' own order, every human beside its own map
            robot, humans = c["robot"][i], c["humans"][off:off + n]
            rows64 = olc.rotated64(robot, [robot[2:4]], humans[:, :4], humans[:, 4], 0.0)[0]
            if c["headed"]:
                rows64 = np.concatenate([rows64, humans[:, 5:7]], 1)
            maps = olc.maps64_of(humans[None, :, :4], (4, 1.0, 3))[0]
            assert np.allclose(c["rows"][off:off + n], np.concatenate([rows64, maps], 1), rtol=1e-5, atol=2e-5)


def test_the_parallel_branch_of_the_reference_raises():
    (e,) = olc.g22()["exception"]
    assert (e["branch"], e["type"]) == ("parallel", "UnboundLocalError") and "next_human_states" in e["message"]


@pytest.mark.parametrize("wkey", ["omlstm1_13", "omlstm2_13"])
def test_the_restatement_with_the_first_action_pairing_is_the_references_decision(wkey):
    """Every recorded serial decision restated in float64 from the recorded states alone (rotate, sort, maps, pairing, network): with the
    reference's pairing the 81 action values are the recorded ones within the E_ref the generator measured and the arg-max is the
    reference's; with the own pairing they are not (condition c), so the pairing is observable in G22."""
    cs = [c for c in olc.g22()["decision"] if c["wkey"] == wkey]
    cond = next(c for c in olc.g22()["conditions"] if c["wkey"] == wkey)
    assert len(cs) >= 20 == min(20, cond["decisions"]) and cond["min_da"] > 1e-5 and cond["flips"] == 0
    assert cond["min_gap"] >= 8 * cond["e_ref"] and 2 * cond["reordered"] >= cond["decisions"] and cond["own_diff"] > 100 * cond["e_ref"]
    w64 = lc.weights64(olc.g22_policy(wkey).model)
    worst = own_worst = 0.0
    reordered = 0
    for c in cs:
        values, net, rot, maps = olc.restate_decision(w64, c, "reference")
        orders = lc.decision_order(rot[..., 11])
        assert np.array_equal(orders, c["orders"]) and np.array_equal(orders[0], c["order0"])
        assert np.allclose(c["maps"], maps[c["order0"]], atol=1e-5)            # what the reference built, once, on action 0's sorted humans
        worst = max(worst, float(np.max(np.abs(net - c["net_outputs"]))))
        assert float(np.max(np.abs(values - c["action_values"]))) <= cond["e_ref"] * (1 + 1e-9)
        assert int(np.argmax(values)) == c["chosen"] and np.array_equal(c["action_space"][c["chosen"]], c["action"])
        own_worst = max(own_worst, float(np.max(np.abs(olc.restate_decision(w64, c, "own")[0] - c["action_values"]))))
        reordered += int(np.any(orders != orders[:1]))
    assert worst <= cond["e_ref"] * (1 + 1e-9) and 2 * reordered >= len(cs)
    assert own_worst > 100 * cond["e_ref"], (own_worst, cond["e_ref"])


def test_the_pairing_rule_of_the_restatement():
    """wide_rows on a hand-made case: action 0 orders the humans 2, 0, 1; action 1 orders them 1, 0, 2"""
    rot = np.zeros((1, 2, 3, 13))
    rot[0, :, :, 0] = [[10, 11, 12], [10, 11, 12]]              # column 0 names the human
    rot[0, :, :, 11] = [[2.0, 1.0, 3.0], [2.0, 3.0, 1.0]]
    maps = np.array([[[100.0], [101.0], [102.0]]])
    ref = olc.wide_rows(rot, maps, "reference")
    own = olc.wide_rows(rot, maps, "own")
    assert ref.shape == (1, 2, 3, 14)
    assert np.array_equal(ref[0, :, :, 0], [[12, 10, 11], [11, 10, 12]]) and np.array_equal(own[0, :, :, 0], ref[0, :, :, 0])
    assert np.array_equal(own[0, :, :, 13], [[102, 100, 101], [101, 100, 102]])
    assert np.array_equal(ref[0, :, :, 13], [[102, 100, 101], [102, 100, 101]])       # by position: action 0's order for every action
    lying = olc.wide_rows(rot, maps, "reference", sort=False)
    assert np.array_equal(lying[0, 1, :, 0], [10, 11, 12]) and np.array_equal(lying[0, 1, :, 13], [100, 101, 102])
