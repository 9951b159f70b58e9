"""What the suites of the fused optimiser step share (tests/test_value_step_cpu.py, tests/test_gpu_value_step.py;
cs_value_net_train_step[_lstm], ``Trainer.set_update("device")``): the test networks by a short key, the host pack of a flat parameter
array, the device state of one step, one fused step with everything read back (computed once per case), and a trainer driven over a
schedule of minibatches and learning rates.  Modules, minibatches and the yardstick are tests/value_grad_cases.py's and
tests/lstm_grad_cases.py's."""
import copy
import functools

import numpy as np

import lstm_grad_cases as lg
import value_grad_cases as vg

F32 = np.float32
LR, MU = 0.05, 0.9      # (neither is a float32: the kernel takes float32(lr), float32(mu))

# key -> the test networks the issue names: SARL with 13 | 15 columns with and without the global state, CADRL, LSTM-RL's two networks
NETS = {
    "sarl_13_g": ("sarl", 13, True), "sarl_13_p": ("sarl", 13, False), "sarl_15_g": ("sarl", 15, True), "sarl_15_p": ("sarl", 15, False),
    "cadrl_13": ("cadrl", 13, None), "lstm1_13": ("lstm", 13, 1), "lstm2_13": ("lstm", 13, 2),
}
# the shapes of the one-step and blob tests: one region; 33 x 3, four regions and P (odd for every net here) no multiple of the launch's
# 256 threads; a SARL sample in chunks; 33 x 2 for the recurrent networks (CADRL stores one human a sample: n = 1, two regions at B = 33)
ONE_STEP = ([(k, 1, 1) for k in NETS] + [(k, 33, 3) for k in NETS if k.startswith("sarl")] + [("cadrl_13", 33, 1)]
            + [("sarl_13_g", 257, 33), ("sarl_15_p", 257, 33), ("lstm1_13", 33, 2), ("lstm2_13", 33, 2)])


@functools.lru_cache(maxsize=None)
def model_of(key):
    """(module on the CPU with seeded weights, cols, whether recurrent)"""
    family, cols, arg = NETS[key]
    if family == "sarl":
        return vg.seeded_sarl(cols, arg), cols, False
    if family == "lstm":
        return lg.seeded(arg, cols), cols, True
    model = vg.cadrl_module(cols)
    vg.draw_weights(model, 2339, calm=False)
    return model, cols, False


def batch_of(key, B, n, salt=0):
    return vg.batch(NETS[key][1], B, n, cadrl=NETS[key][0] == "cadrl", salt=salt)


def split_flat(net, flat):
    """A flat parameter array cut into the arrays a pack entry takes, in value_net.param_offsets' order"""
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    offsets = value_net.param_offsets(net)
    shapes = [tuple(p.shape) for layer in net.layers for p in value_net.layer_params(layer)]
    return [np.asarray(flat[a:b], F32).reshape(s) for a, b, s in zip(offsets, offsets[1:], shapes)]


def host_pack(net, flat, precision="f32"):
    """cs_value_net_pack / _pack_lstm / _pack_bf16 of the flat parameters `flat` (numpy), on the host"""
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    return value_net.pack(net.kind, net.dims, net.cols, split_flat(net, flat), precision)


def padding_of(net):
    """bool [blob floats]: the blob floats no parameter reaches -- what the host pack of all-ones parameters leaves 0"""
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    return host_pack(net, np.ones(value_net.param_offsets(net)[-1], F32)) == 0.0


# ---------------------------------------------------------------------------------------------------------------- one step on the GPU
def device_state(key, momentum_seed=41):
    """(net, flat, momentum, grad) on the GPU for the network `key`: the DeviceNet has adopted `flat` and its float32 blob is current; the
    momentum is seeded N(0, 0.01) (None: zeros), the gradient buffer NaN-filled."""
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    model, cols, _ = model_of(key)
    net = value_net.DeviceNet(model, cols)
    flat = vg.flat_parameters(net, model)
    net.adopt_flat(flat)
    net.refresh("f32")
    if momentum_seed is None:
        momentum = torch.zeros_like(flat)
    else:
        momentum = vg.to_device((np.random.RandomState(momentum_seed).standard_normal(flat.numel()) * 0.01).astype(F32))
    return net, flat, momentum, torch.full_like(flat, np.nan)


def kernels_of(key):
    """(loss_and_grad, train_step) of the network's family"""
    from social_navigation_pyenvs_amd.crowd_nav.policy import value_net

    if model_of(key)[2]:
        return value_net.loss_and_grad_lstm, value_net.train_step_lstm
    return value_net.loss_and_grad, value_net.train_step


def read(*tensors):
    import torch

    torch.cuda.synchronize()
    return [t.cpu().numpy().copy() for t in tensors]


@functools.lru_cache(maxsize=None)
def one_step(key, B, n):
    """One fused step of network `key` on a seeded minibatch from seeded parameters and momentum, and cs_value_net_loss_grad[_lstm] on the
    same inputs: a dict of host arrays -- p0, buf0 (before), p1, buf1, grad, blob, loss, values, loss_sum (after; loss_sum started at 0.5),
    ref_grad, ref_loss, ref_values (the loss-and-gradient entry), host_blob (the host pack of p1), padding (bool per blob float)."""
    import torch

    loss_and_grad, train_step = kernels_of(key)
    x, v = batch_of(key, B, n)
    rows, targets = vg.to_device(x), vg.to_device(v).reshape(-1)
    net, flat, momentum, grad = device_state(key)
    out = dict(zip(("p0", "buf0"), read(flat, momentum)))
    ref_values, ref_grad = torch.full((B,), np.nan, device="cuda"), torch.full_like(flat, np.nan)
    ref_loss = loss_and_grad(net, flat, rows, targets, ref_grad, ref_values)
    out.update(zip(("ref_grad", "ref_loss", "ref_values"), read(ref_grad, ref_loss, ref_values)))
    values, loss_sum = torch.full((B,), np.nan, device="cuda"), torch.full((1,), 0.5, dtype=torch.float64, device="cuda")
    loss = train_step(net, flat, momentum, rows, targets, grad, LR, MU, values, loss_sum)
    out.update(zip(("p1", "buf1", "grad", "blob", "loss", "values", "loss_sum"), read(flat, momentum, grad, net.blob, loss, values, loss_sum)))
    out["host_blob"], out["padding"] = host_pack(net, out["p1"]), padding_of(net)
    return out


def three_steps(key, B, n):
    """Three consecutive fused steps (a minibatch each) from the seeded state: the bytes of parameters, momentum, gradient, blob, the last
    loss and loss_sum"""
    import torch

    _, train_step = kernels_of(key)
    net, flat, momentum, grad = device_state(key)
    loss_sum = torch.zeros(1, dtype=torch.float64, device="cuda")
    for salt in range(3):
        x, v = batch_of(key, B, n, salt)
        loss = train_step(net, flat, momentum, vg.to_device(x), vg.to_device(v).reshape(-1), grad, LR, MU, None, loss_sum)
    return [a.tobytes() for a in read(flat, momentum, grad, net.blob, loss, loss_sum)]


# ---------------------------------------------------------------------------------------------------------------- the trainer on a schedule
def trainer_for(model, gradient, update, memory=(), batch_size=1, device="cuda", double=False, net=None, lr=0.01, copy_model=True):
    import torch

    from social_navigation_pyenvs_amd.crowd_nav.utils.trainer import Trainer

    m = copy.deepcopy(model).to(device) if copy_model else model
    if double:
        m = m.double()
    trainer = Trainer(m, memory, torch.device(device), batch_size)
    trainer.set_learning_rate(lr)
    if gradient != "autograd":
        trainer.set_gradient(gradient, net=net)
    trainer.set_update(update)
    return trainer


def snapshot(trainer):
    return [p.detach().double().cpu().numpy().copy() for p in vg.sorted_parameters(trainer.model)]


def run_schedule(model, batches, gradient, update, double=False):
    """A trainer over `batches`, one ``optimize_batch(1)`` each, on the schedule of the trajectory test: step 0 at lr 0.01; the group's lr
    set to 0.005 (the momentum carries) before step 1; a new ``set_learning_rate(0.01)`` (the momentum starts from zero) before step 2;
    then, whatever the update mode was, ``set_update("torch")`` and one more step on the first minibatch.  `gradient` "autograd" runs on the
    CPU (`double`: in float64).  Returns ([loss per step], [parameter arrays in sorted-name order after each step], the trainer)."""
    device = "cpu" if gradient == "autograd" else "cuda"
    trainer = trainer_for(model, gradient, update, device=device, double=double)
    batches = list(batches) + [batches[0]]
    if double:
        batches = [(x.double(), v.double()) for x, v in batches]
    trainer.data_loader = vg.in_order_loader([(x.to(device), v.to(device)) for x, v in batches])
    losses, snaps = [], []
    for step in range(len(batches)):
        if step == 1:
            trainer.optimizer.param_groups[0]["lr"] = 0.005
        if step == 2:
            trainer.set_learning_rate(0.01)
        if step == len(batches) - 1:
            trainer.set_update("torch")
        losses.append(trainer.optimize_batch(1))
        snaps.append(snapshot(trainer))
    return losses, snaps, trainer
