"""CPU suite of the recurrent loss-and-gradient kernel and of the trainer mode around it (csrc/value_net_lstm_grad.hip,
crowd_nav/utils/trainer.py "device_lstm"): the three entries are declared, listed and exported; their refusals come before
any device call; the sizes are the flat layout; the Python refusals; and a float32 numpy restatement of the kernel's backward (manual
backpropagation through time with the kernel's activation formulas, tests/lstm_grad_cases.py) meets the yardstick on golden G24's networks,
as G24's recorded gradients do.  The kernel itself is tests/test_gpu_value_lstm_grad.py."""
import ctypes as C
import os

import numpy as np
import pytest

import lstm_grad_cases as lg
import value_grad_cases as vg

NET1_DIMS = [19, 0, 3, 41, 27, 1]
NET2_DIMS = [19, 2, 40, 33, 3, 41, 27, 1]
SYMBOLS = ("cs_value_net_grad_sizes_lstm", "cs_value_net_loss_grad_lstm", "cs_value_net_pack_lstm_device")


def _sizes(dims, cols=13, B=7, n=5):
    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    d = np.ascontiguousarray(dims, np.int32)
    blob, params, scratch = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    assert lib.cs_value_net_pack_lstm(d.ctypes.data, len(d), cols, None, None, C.byref(blob)) == 0, lib.cs_last_error()
    rc = lib.cs_value_net_grad_sizes_lstm(d.ctypes.data, len(d), cols, B, n, C.byref(params), C.byref(scratch))
    return rc, lib.cs_last_error().decode(), blob.value, params.value, scratch.value


def _loss_grad(dims=NET2_DIMS, cols=13, B=7, n=5, null=None, blob_off=0, param_off=0, scratch_off=0):
    """cs_value_net_loss_grad_lstm with dummy device addresses: only calls whose checks refuse them before any device call"""
    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    _, _, blob, params, scratch = _sizes(dims, cols, max(B, 1), min(max(n, 1), 128))
    d = np.ascontiguousarray(dims, np.int32)
    dev = {k: 0x1000 for k in ("weights", "params", "rows", "targets", "grad", "loss", "values", "scratch")}
    if null:
        dev[null] = None
    rc = lib.cs_value_net_loss_grad_lstm(d.ctypes.data, len(d), dev["weights"], blob + blob_off, dev["params"], params + param_off, B, n, cols,
                                         dev["rows"], dev["targets"], dev["grad"], dev["loss"], dev["values"], dev["scratch"], scratch + scratch_off, None)
    return rc, lib.cs_last_error().decode()


def test_the_symbols_are_declared_listed_and_exported():
    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(_lib._PKG), "include", "crowdstep.h")).read()
    for sym in SYMBOLS:
        assert sym in _lib.ABI_SYMBOLS and sym in _lib.ABI and hasattr(lib, sym) and f"int {sym}(" in header, sym
    for cited in ("lstm_rl.py:9-65", "trainer.py:50-71"):
        assert cited in header
    assert _lib.ABI_VERSION == 4 and lib.cs_abi_version() == 4 and "#define CS_ABI_VERSION 4" in header


LOSS_GRAD_REFUSALS = [
    (dict(null="weights"), "null argument"),
    (dict(null="params"), "null argument"),
    (dict(null="rows"), "null argument"),
    (dict(null="targets"), "null argument"),
    (dict(null="grad"), "null argument"),
    (dict(null="loss"), "null argument"),
    (dict(null="scratch"), "null argument"),
    (dict(B=0), "B must be positive"),
    (dict(n=0), "n must be at least 1"),
    (dict(n=129), "at most 128 humans a sample (CS_VN_LSTM_MAX_N)"),
    (dict(blob_off=1), "the weight blob does not have the size of this network"),
    (dict(param_off=-1), "the flat parameters do not have the size of this network"),
    (dict(scratch_off=-1), "the scratch is too small"),
    (dict(cols=14), "rotated rows have 13 or 15 columns"),
    (dict(dims=[0] + NET1_DIMS[1:]), "the LSTM's hidden width must be between 1 and 256"),
    (dict(dims=NET2_DIMS[:-1]), "mlp1 has zero or more layers, mlp at least one"),
    (dict(dims=NET1_DIMS[:-1] + [2]), "mlp ends in one output"),
    (dict(dims=[256, 0, 1, 1]), "do not fit the 160 KiB of LDS"),
]
_BY_DESCRIPTION = ("rotated rows", "hidden width", "mlp1 has zero", "mlp ends", "do not fit")


@pytest.mark.parametrize("kw,fragment", LOSS_GRAD_REFUSALS, ids=[f"{i}-{f[:24]}" for i, (_, f) in enumerate(LOSS_GRAD_REFUSALS)])
def test_loss_grad_lstm_refuses_before_any_device_call(kw, fragment):
    from social_navigation_pyenvs_amd import _lib

    if any(part in fragment for part in _BY_DESCRIPTION):
        d = np.ascontiguousarray(kw.get("dims", NET2_DIMS), np.int32)      # (refused by the description: no sizes to ask for)
        a, b = C.c_size_t(0), C.c_size_t(0)
        rc = _lib.load().cs_value_net_grad_sizes_lstm(d.ctypes.data, len(d), kw.get("cols", 13), 7, 5, C.byref(a), C.byref(b))
        msg = _lib.load().cs_last_error().decode()
        assert (rc, fragment in msg) == (_lib.CS_ERR_ARG, True), msg
        rc = _lib.load().cs_value_net_loss_grad_lstm(d.ctypes.data, len(d), 0x1000, 1, 0x1000, 1, 7, 5, kw.get("cols", 13), 0x1000, 0x1000, 0x1000,
                                                     0x1000, None, 0x1000, 1, None)
        msg = _lib.load().cs_last_error().decode()
        assert (rc, fragment in msg) == (_lib.CS_ERR_ARG, True), msg
        return
    rc, msg = _loss_grad(**kw)
    assert (rc, fragment in msg) == (_lib.CS_ERR_ARG, True), msg
    if "n" in kw or "B" in kw:             # the sizes entry refuses the same shapes
        d = np.ascontiguousarray(NET2_DIMS, np.int32)
        a, b = C.c_size_t(0), C.c_size_t(0)
        rc = _lib.load().cs_value_net_grad_sizes_lstm(d.ctypes.data, len(d), 13, kw.get("B", 7), kw.get("n", 5), C.byref(a), C.byref(b))
        assert (rc, fragment in _lib.load().cs_last_error().decode()) == (_lib.CS_ERR_ARG, True)


PACK_DEVICE_REFUSALS = [
    (dict(params=None), "null argument"),
    (dict(blob=None), "null argument"),
    (dict(n_params=-1), "the flat parameters do not have the size of this network"),
    (dict(n_blob=4), "the weight blob does not have the size of this network"),
    (dict(cols=12), "rotated rows have 13 or 15 columns"),
]


@pytest.mark.parametrize("kw,fragment", PACK_DEVICE_REFUSALS, ids=[f"{i}" for i in range(len(PACK_DEVICE_REFUSALS))])
def test_pack_lstm_device_refuses_before_any_device_call(kw, fragment):
    from social_navigation_pyenvs_amd import _lib

    _, _, blob, params, _ = _sizes(NET2_DIMS)
    d = np.ascontiguousarray(NET2_DIMS, np.int32)
    rc = _lib.load().cs_value_net_pack_lstm_device(d.ctypes.data, len(d), kw.get("cols", 13), kw.get("params", 0x1000), params + kw.get("n_params", 0),
                                                   kw.get("blob", 0x1000), blob + kw.get("n_blob", 0), None)
    msg = _lib.load().cs_last_error().decode()
    assert (rc, fragment in msg) == (_lib.CS_ERR_ARG, True), msg


@pytest.mark.parametrize("net", lg.G24_NETS)
def test_the_sizes_are_the_flat_layout_and_a_tape_per_workgroup(net):
    from social_navigation_pyenvs_amd import _lib
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    model = lg.g24_module(net)
    dn = value_net.DeviceNet(model, int(lg.g24()[net]["cols"]))
    assert dn.family is value_net.RECURRENT
    tensors = [p for layer in value_net.describe(model)[2] for p in value_net.layer_params(layer)]
    want = np.concatenate([[0], np.cumsum([p.numel() for p in tensors])])
    assert list(value_net.param_offsets(dn)) == want.tolist()
    P = int(want[-1])
    assert P == sum(p.numel() for p in model.parameters())
    # one region a workgroup (32 samples a job, at most 256): the partial gradient and the loss term, then n steps of 6 x 32 x up(H, 8) floats
    region = lambda n: (P + 1 + 3) // 4 * 4 + n * 6 * 32 * 24
    for B, n, groups in ((7, 5, 1), (33, 3, 2), (100, 5, 4), (8193, 2, 256), (2, 128, 1)):
        assert value_net.grad_sizes_lstm(dn, B, n) == (P, groups * region(n)), (B, n)
    d = np.ascontiguousarray(dn.dims, np.int32)
    assert _lib.load().cs_value_net_grad_sizes_lstm(d.ctypes.data, len(d), dn.cols, 7, 5, None, None) == _lib.CS_ERR_ARG


# ---------------------------------------------------------------------------------------------------------------- the Python refusals
def test_the_predicates_and_the_refusals_name_each_family_once():
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    assert value_net.has_recurrent_gradient_kernel(value_net.RECURRENT)
    for family in (value_net.FEED_FORWARD, value_net.MAPPED, value_net.RECURRENT_MAPPED):
        assert not value_net.has_recurrent_gradient_kernel(family)
    assert not value_net.has_gradient_kernel(value_net.RECURRENT)
    assert "covers the feed-forward networks" in value_net.GRADIENT_REFUSAL and "device_lstm" in value_net.GRADIENT_REFUSAL
    sarl = value_net.DeviceNet(vg.sarl_module(13, True), 13)
    om = value_net.DeviceNet(lg.lstm_module(1, 13 + 48), 13, om_cols=48, om_grid=(4, 1.0, 3))
    assert om.family is value_net.RECURRENT_MAPPED
    for net in (sarl, om):
        for call in (lambda: value_net.pack_lstm_on_device(net, None), lambda: value_net.grad_sizes_lstm(net, 7, 5),
                     lambda: value_net.loss_and_grad_lstm(net, None, None, None, None)):
            with pytest.raises(ValueError, match="covers LSTM-RL's two networks"):
                call()
    with pytest.raises(ValueError, match="covers the feed-forward networks"):
        om.adopt_flat(object())
    lstm = value_net.DeviceNet(lg.lstm_module(2, 13), 13)
    with pytest.raises(ValueError, match="one contiguous CUDA float32 tensor of 8245 elements"):       # accepted as a family, refused as a tensor
        import torch

        lstm.adopt_flat(torch.zeros(8245))
    with pytest.raises(ValueError, match="covers the feed-forward networks"):
        value_net.grad_sizes(lstm, 7, 5)


def test_the_device_lstm_gradient_refuses_what_it_cannot_run():
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.utils.memory import ReplayMemory
    from social_navigation_pyenvs_amd.crowd_nav.utils.trainer import GRADIENTS, Trainer

    assert GRADIENTS == ("autograd", "device", "device_lstm")
    trainer = Trainer(lg.lstm_module(1, 13), ReplayMemory(8), torch.device("cpu"), 4)
    with pytest.raises(ValueError, match="one of 'autograd', 'device', 'device_lstm'"):
        trainer.set_gradient("fused")
    with pytest.raises(ValueError, match="the model is on the CPU"):
        trainer.set_gradient("device_lstm")
    assert trainer.gradient == "autograd" and trainer.net is None
    with pytest.raises(ValueError, match=r'the module has no LSTM; CADRL and SARL train with set_gradient\("device"\)'):
        Trainer(vg.sarl_module(13, True), ReplayMemory(8), torch.device("cpu"), 4).set_gradient("device_lstm")
    for network in (1, 2):              # OM-LSTM-RL: the rows carry 48 map columns
        with pytest.raises(ValueError, match="occupancy-map columns"):
            Trainer(lg.lstm_module(network, 13 + 48), ReplayMemory(8), torch.device("cpu"), 4).set_gradient("device_lstm")
    with pytest.raises(ValueError, match="the gradient kernel is float32|the model is on the CPU"):
        Trainer(lg.lstm_module(1, 13).double(), ReplayMemory(8), torch.device("cpu"), 4).set_gradient("device_lstm")
    trainer.set_gradient("autograd")


# ---------------------------------------------------------------------------------------------------------------- golden G24
@pytest.mark.parametrize("net", lg.G24_NETS)
def test_the_modules_under_cpu_autograd_reproduce_g24s_gradients_and_loss(net):
    """The reference's recorded .grad and loss against this project's module: the yardstick with G24's gradient in the candidate's place."""
    model = lg.g24_module(net)
    case = lg.g24()[net]
    x, v = lg.g24_batches(net)[0]
    (loss32, g32), (loss64, g64) = vg.references(model, x, v)
    vg.assert_within_yardstick(vg.split_like(case["grads"], vg.sorted_parameters(model)), g32, g64, f"{net} G24 gradients")
    lg.check_loss(case["loss"], loss32, loss64, f"{net} G24")


@pytest.mark.parametrize("net", lg.G24_NETS)
def test_g24s_minibatches_stay_away_from_the_relus_kinks(net):
    """A ReLU input within rounding of zero lets float32 and float64 take it on different sides, and every float32 gradient -- torch's, the
    reference's recording, the kernel's -- is then a sample's whole term from the float64 one: the comparisons on G24 would measure nothing."""
    model = lg.g24_module(net)
    for x, _ in lg.g24_batches(net):
        assert vg.relu_margins(model, x).min() >= vg.KINK_MARGIN


@pytest.mark.parametrize("net", lg.G24_NETS)
def test_the_trainer_in_autograd_mode_reproduces_g24s_training(net):
    model = lg.g24_module(net)
    case = lg.g24()[net]
    batches = lg.g24_batches(net)
    losses32, snaps32 = vg.train_steps(model, batches)
    losses64, snaps64 = vg.train_steps(model, batches, double=True)
    recorded = vg.split_like(case["trained"].astype(np.float64), vg.sorted_parameters(model))
    start = [p.detach().double().numpy() for p in vg.sorted_parameters(model)]
    vg.assert_within_yardstick([r - s for r, s in zip(recorded, start)], vg.updates(snaps32[-1], model), vg.updates(snaps64[-1], model),
                               f"{net} G24 trained parameters")
    lg.check_loss(case["average"], sum(losses32) / 3, sum(losses64) / 3, f"{net} G24 average")


@pytest.mark.parametrize("b", [0, 1, 2], ids=["B7n5", "B33n3", "B4n1"])
@pytest.mark.parametrize("net", lg.G24_NETS)
def test_the_numpy_restatement_of_the_backward_meets_the_yardstick(net, b):
    """Manual backpropagation through time in float32 with the kernel's sigmoid and tanh and the derivatives from the stored outputs, on all
    three of G24's minibatches: pins the formulas of the kernel's header without a GPU."""
    model = lg.g24_module(net)
    x, v = lg.g24_batches(net)[b]
    loss_n, g_n, _ = lg.numpy_loss_grad(model, x.numpy(), v.numpy())
    (loss32, g32), (loss64, g64) = vg.references(model, x, v)
    vg.assert_within_yardstick(g_n, g32, g64, f"{net} numpy restatement, batch {b}")
    lg.check_loss(loss_n, loss32, loss64, f"{net} numpy restatement, batch {b}")
    names = sorted(dict(model.named_parameters()))
    by = dict(zip(names, g_n))
    assert np.array_equal(by["lstm.bias_ih_l0"], by["lstm.bias_hh_l0"])
    if x.shape[1] == 1:
        assert not np.any(by["lstm.weight_hh_l0"])
    if b == 0:      # and it stands where G24's recorded gradient stands
        vg.assert_within_yardstick(g_n, vg.split_like(lg.g24()[net]["grads"], vg.sorted_parameters(model)), g64, f"{net} numpy restatement against G24")
