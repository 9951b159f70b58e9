"""CPU suite of the optimisation step of the networks with occupancy-map columns (OM-SARL, OM-LSTM-RL): golden G25 against this project's
modules under CPU autograd and its Trainer, the host-only entries (cs_value_net_grad_sizes_om, cs_value_net_grad_sizes_lstm_om,
cs_value_net_blob_index_om, cs_value_net_blob_index_lstm_om), the flat layout, and the Python seams' and the trainer's refusals.  No GPU:
every library call here is refused or answered before a device call.  tests/test_abi_cpu.py holds the header against ``_lib.ABI``."""
import ctypes as C

import numpy as np
import pytest

import lstm_grad_cases as lg
import om_grad_cases as og
import value_grad_cases as vg
import value_step_cases as vs

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- golden G25
@pytest.mark.parametrize("net", og.G25_NETS)
def test_the_modules_under_cpu_autograd_reproduce_g25s_gradients_and_loss(net):
    """The reference's recorded .grad and loss against this project's module: the yardstick with G25's gradient in the candidate's place."""
    model = og.g25_module(net)
    case = og.g25()[net]
    x, v = og.g25_batches(net)[0]
    assert tuple(x.shape) == (7, 5, case["cols"] + case["om_cols"])
    (loss32, g32), (loss64, g64) = vg.references(model, x, v)
    vg.assert_within_yardstick(vg.split_like(case["grads"], vg.sorted_parameters(model)), g32, g64, f"{net} G25 gradients")
    lg.check_loss(case["loss"], loss32, loss64, f"{net} G25")


@pytest.mark.parametrize("net", og.G25_NETS)
def test_g25s_minibatches_are_sparse_away_from_the_kinks_and_leave_no_tensor_without_a_gradient(net):
    """What the fixture promises: map columns that are mostly 0 (some of the four-row minibatch 0 in every row), no ReLU input of the
    float64 module within 2^-16 of zero, and no parameter tensor whose whole gradient vanishes on the recorded minibatch -- the yardstick's
    fallback (a vanishing tensor is measured against the network's largest gradient) then applies to the one tensor that vanishes by
    construction, the attention's last bias (the softmax weights of a sample sum to one)."""
    model = og.g25_module(net)
    case = og.g25()[net]
    cols = case["cols"]
    batches = og.g25_batches(net)
    for x, _ in batches:
        maps = x[:, :, cols:].numpy()
        assert 0.6 < float(np.mean(maps == 0.0)) < 0.9 and np.all(x[:, :, :cols].numpy() != 0.0)
        assert vg.relu_margins(model, x).min() >= vg.KINK_MARGIN
    assert np.any(~np.any(batches[2][0][:, :, cols:].numpy() != 0.0, axis=(0, 1)))
    _, g64 = vg.autograd(model, *batches[0], double=True)
    names = sorted(dict(model.named_parameters()))
    top = max(float(np.max(np.abs(g))) for g in g64)
    last_bias = max((k for k in names if k.startswith("attention.") and k.endswith(".bias")), key=lambda k: int(k.split(".")[1]), default=None)
    for name, g in zip(names, g64):
        assert (float(np.max(np.abs(g))) > top * 2.0 ** -40) == (name != last_bias), name


@pytest.mark.parametrize("net", og.G25_NETS)
def test_the_trainer_in_autograd_mode_reproduces_g25s_training(net):
    model = og.g25_module(net)
    case = og.g25()[net]
    batches = og.g25_batches(net)
    losses32, snaps32 = vg.train_steps(model, batches)
    losses64, snaps64 = vg.train_steps(model, batches, double=True)
    recorded = vg.split_like(case["trained"].astype(np.float64), vg.sorted_parameters(model))
    start = [p.detach().double().numpy() for p in vg.sorted_parameters(model)]
    vg.assert_within_yardstick([r - s for r, s in zip(recorded, start)], vg.updates(snaps32[-1], model), vg.updates(snaps64[-1], model),
                               f"{net} G25 trained parameters")
    lg.check_loss(case["average"], sum(losses32) / 3, sum(losses64) / 3, f"{net} G25 average")


# ---------------------------------------------------------------------------------------------------------------- the host entries
def _nets():
    """one mapped DeviceNet per family and network, with the module's parameter count"""
    out = []
    for policy, which, cols, om_cols in (("sarl", 1, 13, 48), ("sarl", 0, 15, 18), ("lstm", 1, 13, 48), ("lstm", 2, 15, 18)):
        model = og.module(policy, which, cols, om_cols)
        out.append((og.device_net(model, cols, om_cols), sum(p.numel() for p in model.parameters())))
    return out


def test_grad_sizes_om_is_the_region_size_restated():
    """Feed-forward: gpt = 32 / n groups a tile (1 above 32 humans), jrows = min(up(ceil(B / 256), gpt), 32) groups a job, a region of
    up(P + 1, 4) floats per workgroup.  Recurrent: a workgroup per 32 samples, at most 256, and behind its region the tape [n][6][32][up(H, 8)].
    Neither depends on the row's width but through P."""
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    up = lambda x, m: (x + m - 1) // m * m
    for net, P in _nets():
        for B, n in ((1, 2), (7, 5), (33, 3), (100, 5), (1537, 5), (8193, 2), (2, 33)):
            if net.lstm:
                want = min((B + 31) // 32, 256) * (up(P + 1, 4) + n * 6 * 32 * up(lg.H_SMALL, 8))
            else:
                gpt = 32 // n if n <= 32 else 1
                jrows = min(up((B + 255) // 256, gpt), 32)
                want = min((B + jrows - 1) // jrows, 256) * up(P + 1, 4)
            assert value_net.grad_sizes_om(net, B, n) == (P, want), (net.family.decide["f32"], B, n)


@pytest.mark.parametrize("over,fragment", [(dict(om_cols=0), "om_cols must be at least 1"), (dict(om_cols=244), "exceed a layer's 256 inputs"),
                                           (dict(cols=14), "rotated rows have 13 or 15 columns"), (dict(null=True), "null argument"),
                                           (dict(B=0), "B must be positive")])
def test_the_size_entries_refuse_bad_arguments(over, fragment):
    """om_cols = 0, cols + om_cols = 257 (13 + 244), cols = 14, null outputs: CS_ERR_ARG from both families' entries"""
    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    for net, _ in _nets():
        lead = net.family.lead(net.kind) + (net.dims.ctypes.data, len(net.dims))
        entry = lib.cs_value_net_grad_sizes_lstm_om if net.lstm else lib.cs_value_net_grad_sizes_om
        a, b = C.c_size_t(0), C.c_size_t(0)
        out = (None, None) if over.get("null") else (C.byref(a), C.byref(b))
        rc = entry(*lead, over.get("cols", 13), over.get("om_cols", net.om_cols), over.get("B", 7), 5, *out)
        assert rc == _lib.CS_ERR_ARG and fragment in lib.cs_last_error().decode(), (rc, lib.cs_last_error().decode())


def test_the_feed_forward_entries_are_sarls_alone():
    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    dims = np.array([3, 37, 29, 1], np.int32)
    a, b = C.c_size_t(0), C.c_size_t(0)
    assert lib.cs_value_net_grad_sizes_om(0, dims.ctypes.data, len(dims), 13, 18, 7, 1, C.byref(a), C.byref(b)) == _lib.CS_ERR_ARG
    assert "occupancy maps belong to SARL's network" in lib.cs_last_error().decode()


def test_the_lds_refusal_names_the_widths():
    """A network whose tile does not fit the 160 KiB with its wide input tile is refused with the widths and the bytes in the sentence"""
    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    net = og.device_net(og.module("sarl", 1, 15, 241, full=True), 15, 241)
    a, b = C.c_size_t(0), C.c_size_t(0)
    rc = lib.cs_value_net_grad_sizes_om(net.kind, net.dims.ctypes.data, len(net.dims), 15, 241, 100, 5, C.byref(a), C.byref(b))
    msg = lib.cs_last_error().decode()
    assert rc == _lib.CS_ERR_ARG and "rows of 15 + 241 columns" in msg and "do not fit the 160 KiB of LDS" in msg, msg
    # the reference's widths with the reference's 48 map columns fit, for every family and network; so do 192 columns at the test widths
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    for policy, which in (("sarl", 1), ("sarl", 0), ("lstm", 1), ("lstm", 2)):
        for cols in (13, 15):
            assert value_net.grad_sizes_om(og.device_net(og.module(policy, which, cols, 48, full=True), cols, 48), 100, 5)[0] > 0
            assert value_net.grad_sizes_om(og.device_net(og.module(policy, which, cols, 192), cols, 192), 7, 5)[0] > 0
    assert value_net.grad_sizes_om(og.device_net(og.module("sarl", 1, 15, 48, full=True), 15, 48), 2, 33)[0] > 0


@pytest.mark.parametrize("policy,which", [("sarl", 1), ("sarl", 0), ("lstm", 1), ("lstm", 2)])
@pytest.mark.parametrize("cols,om_cols", [(13, 1), (15, 1), (13, 18), (15, 18), (13, 48), (15, 48)])
def test_param_offsets_and_the_blob_index_of_mapped_nets(policy, which, cols, om_cols):
    """``param_offsets`` is the cumulative sizes of ``describe``'s tensors -- the wide first layer and the LSTM's four included -- and every
    parameter is read by exactly one blob float of ``blob_index_om`` (tests/test_value_step_cpu.py's check): against the host pack of distinct
    integers, the float at index[i] is parameter i (the LSTM's bias pairs share a float that holds their sum), no other two parameters share
    a float, and every float no index names -- the k-group padding of the wide first layer among them -- is 0."""
    from social_navigation_pyenvs_amd import _lib
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    model = og.module(policy, which, cols, om_cols)
    net = og.device_net(model, cols, om_cols)
    tensors = [p for layer in net.layers for p in value_net.layer_params(layer)]
    offsets = value_net.param_offsets(net)
    assert offsets == tuple(np.concatenate([[0], np.cumsum([p.numel() for p in tensors])]).tolist())
    assert {id(p) for p in tensors} == {id(p) for p in model.parameters()} and len(tensors) == len(list(model.parameters()))
    assert tensors[0].shape[1] == cols + om_cols
    P = offsets[-1]
    assert P == sum(p.numel() for p in model.parameters()) and P < 2 ** 23
    flat = np.arange(1, P + 1, dtype=F32)
    pairs = {}
    if net.lstm:
        at = dict(zip((id(p) for p in tensors), offsets))
        ih, hh = at[id(model.lstm.bias_ih_l0)], at[id(model.lstm.bias_hh_l0)]
        pairs = {ih + r: hh + r for r in range(4 * model.lstm.hidden_size)}
    index = value_net.blob_index_om(net)
    blob = og.host_pack(net, flat)
    assert index.shape == (P,) and index.min() >= 0 and index.max() < blob.size
    want = flat.copy()
    for a, b in pairs.items():
        assert index[a] == index[b]
        want[a] = want[b] = flat[a] + flat[b]
    assert np.array_equal(blob[index], want)
    owners = np.delete(index, list(pairs.values()))
    assert np.unique(owners).size == owners.size == P - len(pairs)
    rest = np.ones(blob.size, bool)
    rest[index] = False
    assert rest.any() and np.all(blob[rest] == 0.0)
    lead = net.family.lead(net.kind) + (net.dims.ctypes.data, len(net.dims))
    entry = getattr(_lib.load(), "cs_value_net_blob_index_lstm_om" if net.lstm else "cs_value_net_blob_index_om")
    with pytest.raises(ValueError, match="the flat parameters do not have the size"):
        _lib.check(entry(*lead, cols, om_cols, index.ctypes.data, P - 1))
    with pytest.raises(ValueError, match="null argument"):
        _lib.check(entry(*lead, cols, om_cols, None, P))
    with pytest.raises(ValueError, match="om_cols must be at least 1"):
        _lib.check(entry(*lead, cols, 0, index.ctypes.data, P))


# ---------------------------------------------------------------------------------------------------------------- the Python refusals
def test_the_predicates_and_the_helpers_name_each_family_once():
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    assert value_net.has_mapped_gradient_kernel(value_net.MAPPED) and value_net.has_mapped_gradient_kernel(value_net.RECURRENT_MAPPED)
    assert not value_net.has_mapped_gradient_kernel(value_net.FEED_FORWARD) and not value_net.has_mapped_gradient_kernel(value_net.RECURRENT)
    for family in (value_net.MAPPED, value_net.RECURRENT_MAPPED):
        assert not value_net.has_gradient_kernel(family) and not value_net.has_recurrent_gradient_kernel(family)
    for text in (value_net.GRADIENT_REFUSAL, value_net.RECURRENT_GRADIENT_REFUSAL):
        assert "occupancy-map columns" in text and "device_om" in text and "device_lstm_om" in text and "keeps torch's autograd" not in text
    assert "covers the feed-forward networks" in value_net.GRADIENT_REFUSAL and "device_lstm" in value_net.GRADIENT_REFUSAL
    assert "covers LSTM-RL's two networks" in value_net.RECURRENT_GRADIENT_REFUSAL
    narrow = [value_net.DeviceNet(vg.sarl_module(13, True), 13), value_net.DeviceNet(lg.lstm_module(2, 13), 13)]
    for net in narrow:
        for call, names in ((lambda: value_net.grad_sizes_om(net, 7, 5), "grad_sizes / grad_sizes_lstm"),
                            (lambda: value_net.pack_om_on_device(net, None), "pack_on_device / pack_lstm_on_device"),
                            (lambda: value_net.loss_and_grad_om(net, None, None, None, None), "loss_and_grad / loss_and_grad_lstm"),
                            (lambda: value_net.train_step_om(net, None, None, None, None, None, 0.01, 0.9), "train_step / train_step_lstm"),
                            (lambda: value_net.blob_index_om(net), "cs_value_net_blob_index / cs_value_net_blob_index_lstm"),
                            (lambda: net.adopt_flat(object(), mapped=True), r"adopt_flat\(flat\)")):
            with pytest.raises(ValueError, match=f"a network without map columns has {names}"):
                call()
    # the names without _om go on refusing a mapped net, with their present sentences
    om_sarl, om_lstm = og.device_net(og.module("sarl", 1, 13, 48), 13, 48), og.device_net(og.module("lstm", 1, 13, 48), 13, 48)
    for net in (om_sarl, om_lstm):
        for call in (lambda: value_net.pack_on_device(net, None), lambda: value_net.grad_sizes(net, 7, 5),
                     lambda: value_net.loss_and_grad(net, None, None, None, None), lambda: net.adopt_flat(object())):
            with pytest.raises(ValueError, match="covers the feed-forward networks"):
                call()
        for call in (lambda: value_net.pack_lstm_on_device(net, None), lambda: value_net.grad_sizes_lstm(net, 7, 5),
                     lambda: value_net.loss_and_grad_lstm(net, None, None, None, None)):
            with pytest.raises(ValueError, match="covers LSTM-RL's two networks"):
                call()
    total = value_net.param_offsets(om_sarl)[-1]
    with pytest.raises(ValueError, match=f"one contiguous CUDA float32 tensor of {total} elements"):       # accepted as a family, refused as a tensor
        om_sarl.adopt_flat(torch.zeros(total), mapped=True)
    with pytest.raises(ValueError, match="adopted no flat parameters"):
        om_sarl.updated_on_device()


def test_the_map_modes_refuse_what_they_cannot_run():
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net
    from social_navigation_pyenvs_amd.crowd_nav.utils import trainer as tr
    from social_navigation_pyenvs_amd.crowd_nav.utils.memory import ReplayMemory

    assert tr.MAP_GRADIENTS == ("device_om", "device_lstm_om")
    assert tr.GRADIENTS == ("autograd", "device", "device_lstm") and tr.UPDATES == ("torch", "device")
    cpu = torch.device("cpu")
    om_sarl, om_lstm = og.module("sarl", 1, 13, 48), og.module("lstm", 2, 13, 48)
    trainer = tr.Trainer(om_sarl, ReplayMemory(8), cpu, 4)
    with pytest.raises(ValueError, match="one of 'autograd', 'device', 'device_lstm', or for a network with occupancy-map columns 'device_om', "
                                         "'device_lstm_om'"):
        trainer.set_gradient("fused")
    # without net=: a first layer of 61 inputs does not say how many of them are map columns
    for model, mode in ((om_sarl, "device_om"), (om_lstm, "device_lstm_om")):
        with pytest.raises(ValueError, match="a first layer of 61 inputs does not say how many of them are map columns"):
            tr.Trainer(model, ReplayMemory(8), cpu, 4).set_gradient(mode)
    # the other family's module
    with pytest.raises(ValueError, match="the module is not SARL's network"):
        tr.Trainer(om_lstm, ReplayMemory(8), cpu, 4).set_gradient("device_om", net=og.device_net(om_lstm, 13, 48))
    with pytest.raises(ValueError, match="the module is not SARL's network"):
        tr.Trainer(vg.cadrl_module(13), ReplayMemory(8), cpu, 4).set_gradient("device_om")
    with pytest.raises(ValueError, match="the module has no LSTM"):
        tr.Trainer(om_sarl, ReplayMemory(8), cpu, 4).set_gradient("device_lstm_om", net=og.device_net(om_sarl, 13, 48))
    # a net without map columns: the narrow mode is named
    sarl, lstm = vg.sarl_module(13, True), lg.lstm_module(1, 15)
    for model, cols, mode, narrow in ((sarl, 13, "device_om", "device"), (lstm, 15, "device_lstm_om", "device_lstm")):
        for net in (None, value_net.DeviceNet(model, cols)):
            with pytest.raises(ValueError, match=rf'no occupancy-map columns; it trains with set_gradient\("{narrow}"\)'):
                tr.Trainer(model, ReplayMemory(8), cpu, 4).set_gradient(mode, net=net)
    # another model's net, a net whose columns are not the first layer's
    with pytest.raises(ValueError, match="not this model's mapped one"):
        trainer.set_gradient("device_om", net=og.device_net(og.module("sarl", 1, 13, 48), 13, 48))
    with pytest.raises(ValueError, match=r"13 \+ 18 columns are not the first layer's 61 inputs"):
        trainer.set_gradient("device_om", net=og.device_net(om_sarl, 13, 18))
    # the existing refusals: a CPU model, a model that is not float32
    for model, mode in ((om_sarl, "device_om"), (om_lstm, "device_lstm_om")):
        with pytest.raises(ValueError, match="the model is on the CPU"):
            tr.Trainer(model, ReplayMemory(8), cpu, 4).set_gradient(mode, net=og.device_net(model, 13, 48))
    double = og.module("sarl", 1, 13, 48).double()
    with pytest.raises(ValueError, match="the gradient kernel is float32|the model is on the CPU"):
        tr.Trainer(double, ReplayMemory(8), cpu, 4).set_gradient("device_om", net=og.device_net(double, 13, 48))
    assert trainer.gradient == "autograd" and trainer.net is None and trainer.update == "torch"
    # the narrow modes go on refusing map-column modules
    with pytest.raises(ValueError, match="covers the feed-forward networks"):
        trainer.set_gradient("device")
    with pytest.raises(ValueError, match="occupancy-map columns"):
        tr.Trainer(om_lstm, ReplayMemory(8), cpu, 4).set_gradient("device_lstm")
    with pytest.raises(ValueError, match="device_om.*device_lstm_om"):
        trainer.set_update("device")


def test_the_memorys_rows_are_checked_against_the_wide_width():
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.utils.trainer import Trainer

    for shape, dtype in (((4, 5, 13), torch.float32), ((4, 5, 61), torch.float64), ((4, 61), torch.float32)):
        with pytest.raises(ValueError, match=r"the gradient kernel takes float32 \[n, 61\]"):
            Trainer._check_states(torch.zeros(shape, dtype=dtype), 61, 1, 'Trainer.set_gradient("device_om")')
    Trainer._check_states(torch.zeros((4, 5, 61)), 61, 1)


def test_the_symbols_are_exported_and_bound():
    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    for stem in ("grad_sizes", "loss_grad", "train_step", "blob_index"):
        for infix in ("", "_lstm"):
            narrow, wide = f"cs_value_net_{stem}{infix}", f"cs_value_net_{stem}{infix}_om"
            assert wide in _lib.ABI and hasattr(lib, wide)
            assert len(_lib.ABI[wide][1]) == len(_lib.ABI[narrow][1]) + 1           # `int om_cols` behind `cols`
    for narrow, wide in (("cs_value_net_pack_device", "cs_value_net_pack_om_device"), ("cs_value_net_pack_lstm_device", "cs_value_net_pack_lstm_om_device")):
        assert wide in _lib.ABI and hasattr(lib, wide) and len(_lib.ABI[wide][1]) == len(_lib.ABI[narrow][1]) + 1
    assert lib.cs_abi_version() == 4
