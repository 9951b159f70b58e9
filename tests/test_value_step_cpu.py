"""CPU suite of the fused optimiser step (cs_value_net_train_step, cs_value_net_train_step_lstm; ``Trainer.set_update``): the property the
update kernel's shape rests on -- the pack entries read every parameter exactly once --, the refusals of the trainer and of the C entries,
and the new symbols.  No GPU: the step itself is tests/test_gpu_value_step.py."""
import ctypes as C

import numpy as np
import pytest

import value_grad_cases as vg
import value_step_cases as vs

F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- the pack map
@pytest.mark.parametrize("key", list(vs.NETS))
def test_the_pack_reads_every_parameter_exactly_once(key):
    """The host pack of parameters set to distinct integers 1 .. P (the LSTM's biases: bias_ih = 1 .. 4H, bias_hh = 4096 times that, so a
    sum names its pair): every parameter's value lies in exactly one blob float, the LSTM's bias pairs as their sum, and every other blob
    float is 0 -- so a thread per parameter writes a blob float no other thread writes, and the padding never needs rewriting."""
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    model, cols, lstm = vs.model_of(key)
    net = value_net.DeviceNet(model, cols)
    offsets = value_net.param_offsets(net)
    P = offsets[-1]
    flat = np.arange(1, P + 1, dtype=F32)
    want = flat.copy()
    if lstm:
        tensors = [p for layer in net.layers for p in value_net.layer_params(layer)]
        at = dict(zip(map(id, tensors), offsets))
        ih, hh, rows = at[id(model.lstm.bias_ih_l0)], at[id(model.lstm.bias_hh_l0)], 4 * model.lstm.hidden_size
        assert rows < 4096
        flat += F32(4097 * rows)                  # every other parameter lies beyond the largest sum of a pair
        flat[ih:ih + rows] = np.arange(1, rows + 1)
        flat[hh:hh + rows] = 4096.0 * np.arange(1, rows + 1)
        want = np.concatenate([np.delete(flat, np.r_[ih:ih + rows, hh:hh + rows]), 4097.0 * np.arange(1, rows + 1)]).astype(F32)
    assert float(flat.max()) < 2 ** 24 and len(set(want.tolist())) == want.size
    blob = vs.host_pack(net, flat)
    filled = blob[blob != 0.0]
    assert filled.size == want.size and np.array_equal(np.sort(filled), np.sort(want))
    assert blob.size > filled.size                 # there is padding, and it is 0
    assert np.array_equal(vs.padding_of(net), blob == 0.0)


def _full(key):
    """The reference's widths: SARL (mlp1 150-100 .. mlp3 150-100-100-1), CADRL (150-100-100-1), LSTM-RL's two networks with H = 50; and
    H = 256, the widest the entries take"""
    import lstm_grad_cases as lg

    if key == "sarl":
        return vg.sarl_module(13, True, vg.SARL_FULL), 13
    if key == "sarl_15_plain":
        return vg.sarl_module(15, False, vg.SARL_FULL), 15
    if key == "cadrl":
        from social_navigation_pyenvs_amd.crowd_nav.policy.cadrl import ValueNetwork

        return ValueNetwork(13, [150, 100, 100, 1]), 13
    if key == "lstm_wide":
        return lg.lstm_module(2, 15, 256, (40, 33), (41, 27, 1)), 15
    return lg.lstm_module(int(key[-1]), 13, lg.H_FULL, lg.MLP1_FULL, lg.MLP_FULL), 13


@pytest.mark.parametrize("key", list(vs.NETS) + ["full:sarl", "full:sarl_15_plain", "full:cadrl", "full:lstm1", "full:lstm2", "full:lstm_wide"])
def test_the_update_kernels_map_is_the_pack_read_forwards(key):
    """cs_value_net_blob_index[_lstm] evaluates, on the host, the map k_vn_sgd writes the blob by (the same functor).  Against the host
    pack of distinct integers: every index lies in the blob, the float there is the parameter (the LSTM's bias pairs share a float that
    holds their sum), no other two parameters share a float, and every float no index names is 0.  At the test networks' widths and at
    the reference's: N = 150 and 100 (five and four 32-column blocks), K = 13, 15, 100 + 100 (the attention's two sources) and 150 (no
    multiples of 8), H = 50 (seven unit blocks, the last of two units), and H = 256."""
    from social_navigation_pyenvs_amd import _lib
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    model, cols = _full(key[5:]) if key.startswith("full:") else vs.model_of(key)[:2]
    net = value_net.DeviceNet(model, cols)
    offsets = value_net.param_offsets(net)
    P = offsets[-1]
    flat = np.arange(1, P + 1, dtype=F32)
    pairs = {}
    if net.lstm:
        at = dict(zip((id(p) for layer in net.layers for p in value_net.layer_params(layer)), offsets))
        ih, hh, rows = at[id(model.lstm.bias_ih_l0)], at[id(model.lstm.bias_hh_l0)], 4 * model.lstm.hidden_size
        pairs = {ih + r: hh + r for r in range(rows)}
    assert P < 2 ** 23                              # (a pair's sum is exact too)
    index = np.full(P, -7, np.int32)
    lead = (net.dims.ctypes.data, len(net.dims)) if net.lstm else (net.kind, net.dims.ctypes.data, len(net.dims))
    entry = _lib.load().cs_value_net_blob_index_lstm if net.lstm else _lib.load().cs_value_net_blob_index
    _lib.check(entry(*lead, cols, index.ctypes.data, P))
    blob = vs.host_pack(net, flat)
    assert index.min() >= 0 and index.max() < blob.size
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
    with pytest.raises(ValueError, match="the flat parameters do not have the size"):
        _lib.check(entry(*lead, cols, index.ctypes.data, P - 1))
    with pytest.raises(ValueError, match="null argument"):
        _lib.check(entry(*lead, cols, None, P))


# ---------------------------------------------------------------------------------------------------------------- the trainer's refusals
def _cpu_trainer():
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.utils.trainer import Trainer

    trainer = Trainer(vg.sarl_module(13, True), [], torch.device("cpu"), 4)
    trainer.set_learning_rate(0.01)
    return trainer


def test_updates_and_the_default_mode():
    from social_navigation_pyenvs_amd.crowd_nav.utils import trainer as tr

    assert tr.UPDATES == ("torch", "device")
    trainer = _cpu_trainer()
    assert trainer.update == "torch"
    trainer.set_update("torch")
    assert trainer.update == "torch"


def test_set_update_refuses_an_unknown_mode_and_device_under_autograd():
    trainer = _cpu_trainer()
    with pytest.raises(ValueError, match="one of 'torch', 'device'"):
        trainer.set_update("fused")
    with pytest.raises(ValueError, match="set_gradient"):
        trainer.set_update("device")
    assert trainer.update == "torch"
    trainer.set_gradient("autograd")
    assert trainer.update == "torch"


def test_the_fused_step_refuses_optimisers_it_does_not_cover():
    """What ``Trainer._step`` asks of ``self.optimizer`` in "device" update mode, on the CPU: lr and momentum of the one group of an SGD
    with momentum, read at every call; every other optimiser refused by name."""
    import torch.optim as optim

    from social_navigation_pyenvs_amd.crowd_nav.utils.trainer import fused_sgd_settings

    model = vg.sarl_module(13, True)
    params = list(model.parameters())
    sgd = optim.SGD(params, lr=0.01, momentum=0.9)
    assert fused_sgd_settings(sgd, params) == (0.01, 0.9)
    sgd.param_groups[0]["lr"] = 0.002
    assert fused_sgd_settings(sgd, params) == (0.002, 0.9)
    assert fused_sgd_settings(optim.SGD(params, lr=0.5), params) == (0.5, 0.0)
    with pytest.raises(ValueError, match="not Adam"):
        fused_sgd_settings(optim.Adam(params, lr=0.01), params)
    with pytest.raises(ValueError, match="no nesterov"):
        fused_sgd_settings(optim.SGD(params, lr=0.01, momentum=0.9, nesterov=True), params)
    with pytest.raises(ValueError, match="no weight_decay"):
        fused_sgd_settings(optim.SGD(params, lr=0.01, momentum=0.9, weight_decay=1e-4), params)
    with pytest.raises(ValueError, match="no dampening"):
        fused_sgd_settings(optim.SGD(params, lr=0.01, momentum=0.9, dampening=0.1), params)
    with pytest.raises(ValueError, match="no maximize"):
        fused_sgd_settings(optim.SGD(params, lr=0.01, momentum=0.9, maximize=True), params)
    with pytest.raises(ValueError, match="one parameter group"):
        fused_sgd_settings(optim.SGD([dict(params=params[:2]), dict(params=params[2:])], lr=0.01, momentum=0.9), params)
    with pytest.raises(ValueError, match="not exactly the model's"):
        fused_sgd_settings(optim.SGD(params[:-1], lr=0.01, momentum=0.9), params)
    with pytest.raises(ValueError, match="not NoneType"):
        fused_sgd_settings(None, params)


# ---------------------------------------------------------------------------------------------------------------- the C entries
def test_both_symbols_are_exported_and_bound():
    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    for name in ("cs_value_net_train_step", "cs_value_net_train_step_lstm"):
        assert name in _lib.ABI and hasattr(lib, name)
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(_lib.ABI[name][1])
        assert fn.argtypes.count(C.c_float) == 2 and len(fn.argtypes) == len(_lib.ABI[name.replace("train_step", "loss_grad")][1]) + 5
    assert lib.cs_abi_version() == 4


def _entry_call(key, **over):
    """cs_value_net_train_step[_lstm] for network `key` on dummy device addresses (the checks only compare them with NULL; every call here
    is refused before a device call): (status, message)."""
    from social_navigation_pyenvs_amd import _lib
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    lib = _lib.load()
    model, cols, lstm = vs.model_of(key)
    net = value_net.DeviceNet(model, cols)
    B, n = 4, 1 if vs.NETS[key][0] == "cadrl" else 3
    lead = (net.dims.ctypes.data, len(net.dims)) if lstm else (net.kind, net.dims.ctypes.data, len(net.dims))
    n_params, n_scratch, n_blob = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    sizes = lib.cs_value_net_grad_sizes_lstm if lstm else lib.cs_value_net_grad_sizes
    assert sizes(*lead, cols, B, n, C.byref(n_params), C.byref(n_scratch)) == 0
    assert (lib.cs_value_net_pack_lstm if lstm else lib.cs_value_net_pack)(*lead, cols, None, None, C.byref(n_blob)) == 0
    dev = 0x1000
    a = dict(weights=dev, n_weights=n_blob.value, params=dev, n_params=n_params.value, momentum=dev, n_momentum=n_params.value, lr=0.01, mu=0.9,
             B=B, n=n, cols=cols, rows=dev, targets=dev, grad=dev, loss=dev, loss_sum=None, values=None, scratch=dev, n_scratch=n_scratch.value)
    a.update(over)
    entry = lib.cs_value_net_train_step_lstm if lstm else lib.cs_value_net_train_step
    rc = entry(*lead, a["weights"], a["n_weights"], a["params"], a["n_params"], a["momentum"], a["n_momentum"], a["lr"], a["mu"], a["B"], a["n"],
               a["cols"], a["rows"], a["targets"], a["grad"], a["loss"], a["loss_sum"], a["values"], a["scratch"], a["n_scratch"], None)
    return rc, lib.cs_last_error().decode()


_BAD_ARGS = [
    (dict(momentum=None), "null argument"),
    (dict(n_momentum=7), "the momentum buffer does not have the size of the flat parameters"),
    (dict(mu=-0.5), "momentum must be finite and at least 0"),
    (dict(mu=float("nan")), "momentum must be finite and at least 0"),
    (dict(mu=float("inf")), "momentum must be finite and at least 0"),
    (dict(lr=-0.01), "lr must be finite and at least 0"),
    (dict(lr=float("nan")), "lr must be finite and at least 0"),
    (dict(lr=float("inf")), "lr must be finite and at least 0"),
    # the loss-and-gradient entry's own checks come first and keep their messages
    (dict(params=None), "null argument"),
    (dict(grad=None, momentum=None), "null argument"),
    (dict(n_params=5), "the flat parameters do not have the size of this network"),
    (dict(n_weights=5), "the weight blob does not have the size of this network"),
    (dict(n_scratch=3), "the scratch is too small for this minibatch"),
    (dict(B=0), "B must be positive"),
]


@pytest.mark.parametrize("key", ["sarl_13_g", "cadrl_13", "lstm1_13", "lstm2_13"])
@pytest.mark.parametrize("over,fragment", _BAD_ARGS, ids=[f"{i}-{'-'.join(o)}" for i, (o, _) in enumerate(_BAD_ARGS)])
def test_the_entries_refuse_bad_arguments_before_any_device_call(key, over, fragment):
    from social_navigation_pyenvs_amd import _lib

    rc, msg = _entry_call(key, **over)
    assert rc == _lib.CS_ERR_ARG and fragment in msg, (rc, msg)


def test_the_python_seam_makes_loss_and_grads_checks():
    """``train_step`` / ``train_step_lstm`` refuse the other family's network as ``loss_and_grad`` / ``loss_and_grad_lstm`` do, before
    anything touches a device."""
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    ff, rec = value_net.DeviceNet(vs.model_of("sarl_13_g")[0], 13), value_net.DeviceNet(vs.model_of("lstm1_13")[0], 13)
    with pytest.raises(ValueError, match="train_step: the fused loss-and-gradient kernel"):
        value_net.train_step(rec, None, None, None, None, None, 0.01, 0.9)
    with pytest.raises(ValueError, match="train_step_lstm: the recurrent loss-and-gradient kernel"):
        value_net.train_step_lstm(ff, None, None, None, None, None, 0.01, 0.9)
    with pytest.raises(ValueError, match="adopt_flat"):
        ff.updated_on_device()
