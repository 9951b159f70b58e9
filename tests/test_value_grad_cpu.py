"""CPU suite of the fused loss-and-gradient kernel and of the trainer around it (csrc/value_net_grad.hip, crowd_nav/utils/trainer.py,
crowd_nav/utils/memory.py): the three entries' refusals before any device call, the flat parameter layout, golden G23 (the
reference's own gradients, loss and Trainer) against this project's modules under CPU autograd, the replay memory, and the trainer's
refusals.  The kernel itself is tests/test_gpu_value_grad.py.  The error yardstick is stated in tests/value_grad_cases.py."""
import ctypes as C
import os

import numpy as np
import pytest

import value_grad_cases as vg

F32 = np.float32
SARL_DIMS = [1, 2, 40, 33, 2, 33, 20, 3, 36, 30, 1, 3, 41, 27, 1]
CADRL_DIMS = [3, 37, 29, 1]
NETS = ["sarl_13_1", "sarl_13_0", "sarl_15_1", "sarl_15_0", "cadrl_13_0"]


def _sizes(kind, dims, cols=13, B=7, n=5):
    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    d = np.ascontiguousarray(dims, np.int32)
    blob, params, scratch = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    assert lib.cs_value_net_pack(kind, d.ctypes.data, len(d), cols, None, None, C.byref(blob)) == 0, lib.cs_last_error()
    rc = lib.cs_value_net_grad_sizes(kind, d.ctypes.data, len(d), cols, B, n, C.byref(params), C.byref(scratch))
    return rc, lib.cs_last_error().decode(), blob.value, params.value, scratch.value


def _loss_grad(kind=1, dims=SARL_DIMS, cols=13, B=7, n=5, null=None, blob_off=0, param_off=0, scratch_off=0):
    """cs_value_net_loss_grad with dummy device addresses: only calls whose checks refuse them before any device call"""
    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    _, _, blob, params, scratch = _sizes(kind, dims, cols, max(B, 1), min(max(n, 1), 1 if kind == 0 else 32))
    d = np.ascontiguousarray(dims, np.int32)
    dev = {k: 0x1000 for k in ("weights", "params", "rows", "targets", "grad", "loss", "values", "scratch")}
    if null:
        dev[null] = None
    rc = lib.cs_value_net_loss_grad(kind, d.ctypes.data, len(d), dev["weights"], blob + blob_off, dev["params"], params + param_off, B, n, cols,
                                    dev["rows"], dev["targets"], dev["grad"], dev["loss"], dev["values"], dev["scratch"], scratch + scratch_off, None)
    return rc, lib.cs_last_error().decode()


def test_the_symbols_are_declared_listed_and_exported():
    from social_navigation_pyenvs_amd import _lib

    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(_lib._PKG), "include", "crowdstep.h")).read()
    for sym in ("cs_value_net_loss_grad", "cs_value_net_grad_sizes", "cs_value_net_pack_device"):
        assert sym in _lib.ABI_SYMBOLS and hasattr(lib, sym) and f"int {sym}(" in header, sym
    for cited in ("trainer.py:50-71", "sarl.py:28-65", "cadrl.py:116-123"):
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
    (dict(blob_off=1), "the weight blob does not have the size of this network"),
    (dict(param_off=-1), "the flat parameters do not have the size of this network"),
    (dict(scratch_off=-1), "the scratch is too small"),
    (dict(kind=0, dims=CADRL_DIMS, n=2), "CADRL's trainer stores one human's row per sample"),
    (dict(cols=14), "rotated rows have 13 or 15 columns"),
    (dict(kind=2), "unknown value network kind"),
    (dict(dims=SARL_DIMS[:-1]), "a chain needs at least one layer and its widths"),
    (dict(dims=[1, 1, 256, 1, 256, 2, 256, 1, 9] + [256] * 8 + [1]), "do not fit the 160 KiB of LDS"),
]


@pytest.mark.parametrize("kw,fragment", LOSS_GRAD_REFUSALS, ids=[f"{i}-{f[:24]}" for i, (_, f) in enumerate(LOSS_GRAD_REFUSALS)])
def test_loss_grad_refuses_before_any_device_call(kw, fragment):
    from social_navigation_pyenvs_amd import _lib

    if "do not fit" in fragment or kw.get("kind") == 2 or kw.get("cols") == 14 or kw.get("dims") == SARL_DIMS[:-1]:
        d = np.ascontiguousarray(kw.get("dims", SARL_DIMS), np.int32)      # (refused by the description: no sizes to ask for)
        a, b = C.c_size_t(0), C.c_size_t(0)
        rc = _lib.load().cs_value_net_grad_sizes(kw.get("kind", 1), d.ctypes.data, len(d), kw.get("cols", 13), 7, 5, C.byref(a), C.byref(b))
        msg = _lib.load().cs_last_error().decode()
        assert (rc, fragment in msg) == (_lib.CS_ERR_ARG, True), msg
        rc = _lib.load().cs_value_net_loss_grad(kw.get("kind", 1), d.ctypes.data, len(d), 0x1000, 1, 0x1000, 1, 7, 5, kw.get("cols", 13), 0x1000, 0x1000,
                                                0x1000, 0x1000, None, 0x1000, 1, None)
        msg = _lib.load().cs_last_error().decode()
        assert (rc, fragment in msg) == (_lib.CS_ERR_ARG, True), msg
        return
    rc, msg = _loss_grad(**kw)
    assert (rc, fragment in msg) == (_lib.CS_ERR_ARG, True), msg


def test_values_may_be_null_and_the_sizes_are_the_layout():
    from social_navigation_pyenvs_amd import _lib

    rc, msg, blob, params, scratch = _sizes(1, SARL_DIMS, 13, 100, 5)
    assert rc == 0, msg
    ins, outs = [13, 40, 33, 33, 66, 36, 30, 26, 41, 27], [40, 33, 33, 20, 36, 30, 1, 41, 27, 1]
    assert params == sum(k * n + n for k, n in zip(ins, outs))
    assert scratch >= 4 * (params + 1)                      # one region per workgroup: 100 samples are 4 jobs of 32
    d = np.ascontiguousarray(SARL_DIMS, np.int32)
    assert _lib.load().cs_value_net_grad_sizes(1, d.ctypes.data, len(d), 13, 7, 5, None, None) == _lib.CS_ERR_ARG


PACK_DEVICE_REFUSALS = [
    (dict(params=None), "null argument"),
    (dict(blob=None), "null argument"),
    (dict(n_params=-1), "the flat parameters do not have the size of this network"),
    (dict(n_blob=4), "the weight blob does not have the size of this network"),
    (dict(cols=12), "rotated rows have 13 or 15 columns"),
]


@pytest.mark.parametrize("kw,fragment", PACK_DEVICE_REFUSALS, ids=[f"{i}" for i in range(len(PACK_DEVICE_REFUSALS))])
def test_pack_device_refuses_before_any_device_call(kw, fragment):
    from social_navigation_pyenvs_amd import _lib

    _, _, blob, params, _ = _sizes(1, SARL_DIMS)
    d = np.ascontiguousarray(SARL_DIMS, np.int32)
    rc = _lib.load().cs_value_net_pack_device(1, d.ctypes.data, len(d), kw.get("cols", 13), kw.get("params", 0x1000), params + kw.get("n_params", 0),
                                              kw.get("blob", 0x1000), blob + kw.get("n_blob", 0), None)
    msg = _lib.load().cs_last_error().decode()
    assert (rc, fragment in msg) == (_lib.CS_ERR_ARG, True), msg


@pytest.mark.parametrize("net", NETS)
def test_param_offsets_is_the_running_sum_over_describes_layers(net):
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    model = vg.g23_module(net)
    dn = value_net.DeviceNet(model, int(vg.g23()[net]["cols"]))
    tensors = [p for layer in value_net.describe(model)[2] for p in value_net.layer_params(layer)]
    want = np.concatenate([[0], np.cumsum([p.numel() for p in tensors])])
    assert list(value_net.param_offsets(dn)) == want.tolist()
    rc, msg, _, params, _ = _sizes(dn.kind, dn.dims, dn.cols, 7, 1 if dn.kind == 0 else 5)
    assert rc == 0 and params == want[-1], msg


def test_the_families_without_a_gradient_kernel_are_refused():
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    assert value_net.has_gradient_kernel(value_net.FEED_FORWARD)
    for family in (value_net.MAPPED, value_net.RECURRENT, value_net.RECURRENT_MAPPED):
        assert not value_net.has_gradient_kernel(family)
    om = value_net.DeviceNet(vg.sarl_module(13 + 48, True), 13, om_cols=48, om_grid=(4, 1.0, 3))
    for call in (lambda: value_net.pack_on_device(om, None), lambda: value_net.grad_sizes(om, 7, 5), lambda: om.adopt_flat(object()),
                 lambda: value_net.loss_and_grad(om, None, None, None, None)):
        with pytest.raises(ValueError, match="covers the feed-forward networks"):
            call()
    import lstm_cases as lc

    lstm = value_net.DeviceNet(lc.lstm_policy(1).model, 13)
    with pytest.raises(ValueError, match="covers the feed-forward networks"):
        value_net.grad_sizes(lstm, 7, 5)


# ---------------------------------------------------------------------------------------------------------------- golden G23
@pytest.mark.parametrize("net", NETS)
def test_the_modules_under_cpu_autograd_reproduce_g23s_gradients_and_loss(net):
    """The reference's recorded .grad and loss against this project's module: the yardstick with G23's gradient in the candidate's place."""
    model = vg.g23_module(net)
    case = vg.g23()[net]
    x, v = vg.g23_batches(net)[0]
    loss32, g32 = vg.autograd(model, x, v)
    loss64, g64 = vg.autograd(model, x, v, double=True)
    recorded = vg.split_like(case["grads"], vg.sorted_parameters(model))
    vg.assert_within_yardstick(recorded, g32, g64, f"{net} G23 gradients")
    e_rec, e_t = abs(case["loss"] - loss64) / abs(loss64), abs(loss32 - loss64) / abs(loss64)
    assert e_rec <= vg.FACTOR * max(e_t, vg.FLOOR), (e_rec, e_t)


@pytest.mark.parametrize("net", NETS)
def test_the_trainer_in_autograd_mode_reproduces_g23s_training(net):
    """Three optimize_batch(1) steps over G23's minibatches in order: what the steps added to the parameters against a float64 run of the
    same trainer, with the reference's recorded final parameters in the candidate's place; the average loss likewise."""
    model = vg.g23_module(net)
    case = vg.g23()[net]
    batches = vg.g23_batches(net)
    losses32, snaps32 = vg.train_steps(model, batches)
    losses64, snaps64 = vg.train_steps(model, batches, double=True)
    recorded = vg.split_like(case["trained"].astype(np.float64), vg.sorted_parameters(model))
    start = [p.detach().double().numpy() for p in vg.sorted_parameters(model)]
    vg.assert_within_yardstick([r - s for r, s in zip(recorded, start)], vg.updates(snaps32[-1], model), vg.updates(snaps64[-1], model),
                               f"{net} G23 trained parameters")
    avg32, avg64 = sum(losses32) / 3, sum(losses64) / 3
    e_rec, e_t = abs(case["average"] - avg64) / abs(avg64), abs(avg32 - avg64) / abs(avg64)
    assert e_rec <= vg.FACTOR * max(e_t, vg.FLOOR), (e_rec, e_t)
    # and one optimize_batch(3) call returns losses / num_batches as the reference forms it
    import copy

    import torch

    from social_navigation_pyenvs_amd.crowd_nav.utils.trainer import Trainer

    m = copy.deepcopy(model)
    trainer = Trainer(m, [], torch.device("cpu"), 1)
    trainer.set_learning_rate(0.01)
    trainer.data_loader = vg.in_order_loader(batches)
    assert trainer.optimize_batch(3) == sum(losses32) / 3
    for p, s in zip(vg.sorted_parameters(m), snaps32[-1]):
        assert np.array_equal(p.detach().double().numpy(), s)


# ---------------------------------------------------------------------------------------------------------------- the replay memory
def _pairs(count, n=3, cols=13, seed=0):
    import torch

    rs = np.random.RandomState(seed)
    return torch.from_numpy(rs.uniform(-1, 1, (count, n, cols)).astype(F32)), torch.from_numpy(rs.uniform(-1, 1, count).astype(F32))


def test_replay_memory_is_a_ring_with_the_references_interface():
    import torch
    from torch.utils.data import Dataset

    from social_navigation_pyenvs_amd.crowd_nav.utils.memory import ReplayMemory

    mem = ReplayMemory(5)
    assert isinstance(mem, Dataset) and len(mem) == 0 and not mem.is_full()
    states, values = _pairs(8)
    for i in range(4):
        mem.push((states[i], torch.Tensor([float(values[i])])))
    assert len(mem) == 4 and not mem.is_full()
    s, v = mem[2]
    assert torch.equal(s, states[2]) and v.shape == (1,) and float(v) == float(values[2])
    for i in range(4, 8):
        mem.push((states[i], torch.Tensor([float(values[i])])))
    assert len(mem) == 5 and mem.is_full()
    # the ring: samples 5, 6, 7 overwrote slots 0, 1, 2; 3 and 4 stayed
    for slot, i in enumerate([5, 6, 7, 3, 4]):
        assert torch.equal(mem[slot][0], states[i]) and float(mem[slot][1]) == float(values[i])
    with pytest.raises(IndexError):
        mem[5]
    mem.clear()
    assert len(mem) == 0 and not mem.is_full()


def test_push_and_push_batch_agree_and_keep_masks():
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.utils.memory import ReplayMemory

    states, values = _pairs(9, seed=1)
    one, many = ReplayMemory(6), ReplayMemory(6)
    for i in range(9):
        one.push((states[i], values[i].reshape(1)))
    many.push_batch(states[:4], values[:4])
    many.push_batch(states[4:9], values[4:9].reshape(5, 1))
    assert len(one) == len(many) == 6
    for slot in range(6):
        assert torch.equal(one[slot][0], many[slot][0]) and torch.equal(one[slot][1], many[slot][1])
    keep = torch.tensor([True, False, False, True, True, False, True, False, False])
    masked, plain = ReplayMemory(6), ReplayMemory(6)
    masked.push_batch(states[:3], values[:3])
    plain.push_batch(states[:3], values[:3])
    masked.push_batch(states[3:], values[3:], keep=keep[3:])
    plain.push_batch(states[3:][keep[3:]], values[3:][keep[3:]])
    assert len(masked) == len(plain) == 6
    for slot in range(6):
        assert torch.equal(masked[slot][0], plain[slot][0]) and torch.equal(masked[slot][1], plain[slot][1])
    none = ReplayMemory(6)
    none.push_batch(states[:3], values[:3], keep=torch.zeros(3, dtype=torch.bool))
    assert len(none) == 0
    with pytest.raises(ValueError, match="exceed the capacity"):
        none.push_batch(states[:7], values[:7])
    with pytest.raises(ValueError, match="a state of shape"):
        many.push_batch(states[:2, :2], values[:2])


def test_sample_shapes_and_a_dataloader_over_the_memory():
    import torch
    from torch.utils.data import DataLoader

    from social_navigation_pyenvs_amd.crowd_nav.utils.memory import ReplayMemory

    states, values = _pairs(10, n=5, cols=15, seed=2)
    mem = ReplayMemory(16)
    with pytest.raises(ValueError, match="empty"):
        mem.sample(4)
    mem.push_batch(states, values)
    x, v = mem.sample(7, generator=torch.Generator().manual_seed(3))
    assert x.shape == (7, 5, 15) and v.shape == (7, 1) and x.dtype == torch.float32
    x2, _ = mem.sample(7, generator=torch.Generator().manual_seed(3))
    assert torch.equal(x, x2)
    rows = {tuple(r.reshape(-1).tolist()) for r in states}
    assert all(tuple(r.reshape(-1).tolist()) in rows for r in x)
    xs, vs = next(iter(DataLoader(mem, 4, shuffle=True)))
    assert xs.shape == (4, 5, 15) and vs.shape == (4, 1)


# ---------------------------------------------------------------------------------------------------------------- the trainer's refusals
def test_the_trainer_raises_as_the_reference_does_without_a_learning_rate():
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.utils.memory import ReplayMemory
    from social_navigation_pyenvs_amd.crowd_nav.utils.trainer import Trainer

    trainer = Trainer(vg.g23_module("sarl_13_1"), ReplayMemory(8), torch.device("cpu"), 4)
    with pytest.raises(ValueError, match="Learning rate is not set!"):
        trainer.optimize_batch(1)
    with pytest.raises(ValueError, match="Learning rate is not set!"):
        trainer.optimize_epoch(1)
    trainer.set_learning_rate(0.01)
    assert isinstance(trainer.optimizer, torch.optim.SGD) and trainer.optimizer.defaults["momentum"] == 0.9 and trainer.optimizer.defaults["lr"] == 0.01
    assert isinstance(trainer.criterion, torch.nn.MSELoss) and trainer.gradient == "autograd"


def test_optimize_epoch_divides_by_the_memory_as_the_reference_does():
    import copy

    import torch

    from social_navigation_pyenvs_amd.crowd_nav.utils.memory import ReplayMemory
    from social_navigation_pyenvs_amd.crowd_nav.utils.trainer import Trainer

    model = vg.g23_module("sarl_13_0")
    mem = ReplayMemory(16)
    mem.push_batch(*_pairs(10, n=3, cols=13, seed=4))
    batches = [(mem.states[:4], mem.values[:4]), (mem.states[4:8], mem.values[4:8]), (mem.states[8:10], mem.values[8:10])]
    trainer = Trainer(copy.deepcopy(model), mem, torch.device("cpu"), 4)
    trainer.set_learning_rate(0.01)
    trainer.data_loader = batches                    # a preset loader is honoured: one pass yields these three minibatches
    got = trainer.optimize_epoch(1)
    losses, _ = vg.train_steps(model, batches)
    assert got == sum(losses) / 10


def test_the_device_gradient_refuses_what_it_cannot_run():
    import torch

    import lstm_cases as lc
    from social_navigation_pyenvs_amd.crowd_nav.utils.memory import ReplayMemory
    from social_navigation_pyenvs_amd.crowd_nav.utils.trainer import Trainer

    trainer = Trainer(vg.g23_module("sarl_13_1"), ReplayMemory(8), torch.device("cpu"), 4)
    with pytest.raises(ValueError, match="one of 'autograd', 'device'"):
        trainer.set_gradient("fused")
    with pytest.raises(ValueError, match="the model is on the CPU"):
        trainer.set_gradient("device")
    assert trainer.gradient == "autograd"
    with pytest.raises(ValueError, match="covers the feed-forward networks"):
        Trainer(lc.lstm_policy(1).model, ReplayMemory(8), torch.device("cpu"), 4).set_gradient("device")
    with pytest.raises(ValueError, match="covers the feed-forward networks"):        # OM-SARL: mlp1 reads 13 + 48 columns
        Trainer(vg.sarl_module(13 + 48, True), ReplayMemory(8), torch.device("cpu"), 4).set_gradient("device")
    trainer.set_gradient("autograd")
