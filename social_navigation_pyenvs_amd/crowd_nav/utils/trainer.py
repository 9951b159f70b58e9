"""The trainer of the value-based policies, with the interface and the arithmetic of crowd_nav/utils/trainer.py: SGD with momentum 0.9 on
the mean-squared error between model(inputs) and the stored target values, an epoch over the memory (``optimize_epoch``) or a number of
minibatches (``optimize_batch``).

Three ways to the gradient, ``set_gradient``:

  "autograd"  (the default) zero_grad, model(inputs), MSELoss, backward -- torch throughout, on any device.
  "device"    for a CADRL / SARL network on the GPU: the module's parameters become views of one flat CUDA tensor and their .grad views of
              another, and a minibatch runs cs_value_net_pack_device (the decision kernels' blob from the flat parameters),
              cs_value_net_loss_grad (forward, loss and the whole gradient, csrc/value_net_grad.hip) and
              optimizer.step().  The optimiser is torch's and the caller's to replace (``self.optimizer``).
  "device_lstm"  the same mechanics for an LSTM-RL network (lstm_rl.ValueNetwork1 / ValueNetwork2 on rows of 13 or 15 columns) on the GPU:
              cs_value_net_pack_lstm_device and cs_value_net_loss_grad_lstm (backpropagation through time over a sample's rows as they lie,
              csrc/value_net_lstm_grad.hip).

  "device_om", "device_lstm_om"  (MAP_GRADIENTS) the same mechanics for the networks with occupancy-map columns, OM-SARL's and OM-LSTM-RL's, on
              stored rows of cols + om_cols columns (the rotated columns, then the human's map, as ``transform`` stores a state):
              cs_value_net_pack_om_device / cs_value_net_loss_grad_om and their `_lstm_om` siblings, the kernels above with a wide input
              tile.  They need `net=`, the policy's own ``policy.device_net()``: a first layer of 61 inputs does not say how many of them
              are map columns.

Two ways to the update, ``set_update``:

  "torch"     (the default) ``self.optimizer.step()``, whatever optimiser the caller put there, and the loss read back per minibatch.
  "device"    for the device gradient modes (the map modes included) and torch.optim.SGD with momentum (one parameter group, dampening 0, no Nesterov, no weight
              decay, not maximize -- what ``set_learning_rate`` builds): a minibatch is cs_value_net_train_step[_lstm], two launches -- the
              gradient kernel, then one kernel that sums the gradient, takes the optimiser's step and rewrites the decision kernels' blob
              (csrc/value_net_grad.h k_vn_sgd).  lr and momentum are read from the optimiser's group at every step; its
              momentum buffers are views of one flat tensor the kernel updates, so ``optimizer.state_dict()`` holds them and a switch back to
              "torch" goes on from them.  The loss is added to a float64 on the device: ``optimize_epoch`` reads it once an epoch,
              ``optimize_batch`` once a call, nothing else crosses to the host."""
from __future__ import annotations

import logging
from typing import NamedTuple

import torch
import torch.nn as nn
import torch.optim as optim
from torch.utils.data import DataLoader

from ..policy import value_net

GRADIENTS = ("autograd", "device", "device_lstm")
MAP_GRADIENTS = ("device_om", "device_lstm_om")     # the device modes of the networks with occupancy-map columns
UPDATES = ("torch", "device")


class _Mode(NamedTuple):
    """What a device gradient mode states about itself; ``set_gradient`` and the steps ask its row of _MODES."""
    kinds: tuple                # ``describe``'s kinds of the modules it trains
    other_kind: str             # the refusal of any other module ({who}: the caller)
    wide_rows: str              # the refusal of a first layer that reads more than 13 | 15 columns ({who}, {cols}); a map mode has none
    has_kernel: object          # value_net's predicate of the families it trains
    which: str                  # what the messages call a DeviceNet of those families
    narrow: str                 # a map mode's sibling for the same network without map columns
    needs_net: bool             # `net=` is required: the first layer does not say how many of its inputs are map columns
    loss_and_grad: object       # value_net's two seams
    train_step: object


_MODES = {
    "device": _Mode((value_net.CS_VN_CADRL, value_net.CS_VN_SARL), value_net.GRADIENT_REFUSAL.format("{who}"), value_net.GRADIENT_REFUSAL.format("{who}"),
                    value_net.has_gradient_kernel, "feed-forward", "", False, value_net.loss_and_grad, value_net.train_step),
    "device_lstm": _Mode((value_net.CS_VN_LSTM,), '{who}: the module has no LSTM; CADRL and SARL train with set_gradient("device")',
                         value_net.RECURRENT_GRADIENT_REFUSAL.format("{who} on rows of {cols} columns"), value_net.has_recurrent_gradient_kernel,
                         "recurrent", "", False, value_net.loss_and_grad_lstm, value_net.train_step_lstm),
    "device_om": _Mode((value_net.CS_VN_SARL,), '{who}: the module is not SARL\'s network; OM-LSTM-RL trains with set_gradient("device_lstm_om")', "",
                       value_net.has_mapped_gradient_kernel, "mapped", "device", True, value_net.loss_and_grad_om, value_net.train_step_om),
    "device_lstm_om": _Mode((value_net.CS_VN_LSTM,), '{who}: the module has no LSTM; OM-SARL trains with set_gradient("device_om")', "",
                            value_net.has_mapped_gradient_kernel, "mapped", "device_lstm", True, value_net.loss_and_grad_om, value_net.train_step_om),
}


class _MemoryLoader:
    """What a DataLoader(memory, batch_size, shuffle=True) yields, drawn on the memory's device: every iteration is one pass over a fresh
    permutation of the stored samples in minibatches, the last one short."""

    def __init__(self, memory, batch_size):
        self.memory, self.batch_size = memory, int(batch_size)

    def __iter__(self):
        count = len(self.memory)
        order = torch.randperm(count, device=self.memory.device)
        for at in range(0, count, self.batch_size):
            index = order[at:at + self.batch_size]
            yield self.memory.states[index], self.memory.values[index]


def fused_sgd_settings(optimizer, params=None):
    """(lr, momentum) of `optimizer` for the fused step ("device" update mode), read from its one parameter group; ValueError, naming what
    it is, for an optimiser the fused step does not cover: anything but torch.optim.SGD over exactly `params` (None: not compared) in one
    group with dampening 0, no Nesterov, no weight decay and not maximize.  No device work."""
    who = 'Trainer.set_update("device")'
    if not isinstance(optimizer, optim.SGD):
        raise ValueError(f'{who}: the fused step is torch.optim.SGD with momentum, not {type(optimizer).__name__}; set_update("torch") runs any optimiser')
    if len(optimizer.param_groups) != 1:
        raise ValueError(f"{who}: the fused step takes one parameter group, the optimiser has {len(optimizer.param_groups)}")
    group = optimizer.param_groups[0]
    for name in ("dampening", "nesterov", "weight_decay", "maximize"):
        if group.get(name):
            raise ValueError(f'{who}: the fused step has no {name} ({name} = {group[name]!r}); set_update("torch") runs this optimiser')
    if params is not None and (len(group["params"]) != len(params) or {id(p) for p in group["params"]} != {id(p) for p in params}):
        raise ValueError(f"{who}: the optimiser's parameters are not exactly the model's")
    return float(group["lr"]), float(group["momentum"])


class Trainer(object):
    def __init__(self, model, memory, device, batch_size):
        """Train the trainable model of a policy"""
        self.model = model
        self.device = device
        self.criterion = nn.MSELoss().to(device)
        self.memory = memory
        self.data_loader = None
        self.batch_size = batch_size
        self.optimizer = None
        self.gradient = "autograd"
        self.net = self.flat = self.flat_grad = None
        self.update = "torch"
        self.momentum = self.loss_sum = self.last_loss = None
        self._momentum_views, self._sgd_bound = (), None

    def set_learning_rate(self, learning_rate):
        logging.info('Current learning rate: %f', learning_rate)
        self.optimizer = optim.SGD(self.model.parameters(), lr=learning_rate, momentum=0.9)

    # ------------------------------------------------------------------ the gradient's path
    def set_gradient(self, gradient, net=None):
        """"autograd", "device" or "device_lstm" (the module's docstring).  `net`: the value_net.DeviceNet whose blob the device modes keep
        current -- a policy's own (``policy.device_net()``), so that its decisions read the trained weights without a host round trip;
        None: one of the trainer's.  "device" refuses a module that is not CADRL's or SARL's network, "device_lstm" one without an LSTM or
        with map columns (OM-LSTM-RL); both a model on the CPU, a model that is not float32, a memory whose stored states are not
        [., n, 13 | 15] float32 rows and a `net` that is not this model's.  "device_om" and "device_lstm_om" (MAP_GRADIENTS) are those two
        for a network with map columns: `net` is required (it says how many of the first layer's inputs are map columns), the rows are
        [., n, cols + om_cols]."""
        if gradient not in GRADIENTS + MAP_GRADIENTS:
            raise ValueError(f"gradient {gradient!r}: one of {', '.join(map(repr, GRADIENTS))}, or for a network with occupancy-map "
                             f"columns {', '.join(map(repr, MAP_GRADIENTS))}")
        if gradient == "autograd":
            if self.net is not None:
                self.net.adopt_flat(None)
            self.gradient, self.net, self.flat, self.flat_grad = gradient, None, None, None
            self.update = "torch"
            return
        kind, _, layers = value_net.describe(self.model)
        params = [p for layer in layers for p in value_net.layer_params(layer)]
        first = layers[0] if layers else None
        cols = getattr(first, "in_features", getattr(first, "input_size", 0))       # (network 1's first layer is the nn.LSTM itself)
        who = f'Trainer.set_gradient("{gradient}")'
        mode = _MODES[gradient]
        has_kernel, which = mode.has_kernel, mode.which
        if kind not in mode.kinds:
            raise ValueError(mode.other_kind.format(who=who))
        if mode.needs_net:
            no_maps = f'{who}: the network has no occupancy-map columns; it trains with set_gradient("{mode.narrow}")'
            if net is None:
                if cols in (13, 15):
                    raise ValueError(no_maps)
                raise ValueError(f"{who}: a first layer of {cols} inputs does not say how many of them are map columns; pass net=, the "
                                 "policy's own policy.device_net()")
            if net.model is not self.model:
                raise ValueError(f"{who}: the DeviceNet given is not this model's {which} one")
            if not has_kernel(net.family):
                raise ValueError(no_maps)
            if net.cols + net.om_cols != cols:
                raise ValueError(f"{who}: the DeviceNet's {net.cols} + {net.om_cols} columns are not the first layer's {cols} inputs")
        elif cols not in (13, 15):
            raise ValueError(mode.wide_rows.format(who=who, cols=cols))
        if any(not p.is_cuda for p in params):
            raise ValueError(f'{who}: the model is on the CPU; the gradient kernel runs on the GPU (model.to("cuda"))')
        if any(p.dtype != torch.float32 for p in params):
            raise ValueError(f'{who}: the gradient kernel is float32')
        self._check_states(getattr(self.memory, "states", None), cols, kind, who)
        if net is None:
            net = value_net.DeviceNet(self.model, cols)
        elif net.model is not self.model or not has_kernel(net.family):
            raise ValueError(f"{who}: the DeviceNet given is not this model's {which} one")
        offsets = value_net.param_offsets(net)
        flat = torch.empty(offsets[-1], dtype=torch.float32, device=params[0].device)
        grad = torch.zeros_like(flat)
        with torch.no_grad():
            for p, at in zip(params, offsets):
                flat[at:at + p.numel()].copy_(p.detach().reshape(-1))
                p.data = flat[at:at + p.numel()].view(p.shape)
                p.grad = grad[at:at + p.numel()].view(p.shape)
        net.adopt_flat(flat, mapped=mode.needs_net)
        self.gradient, self.net, self.flat, self.flat_grad = gradient, net, flat, grad

    # ------------------------------------------------------------------ the update's path
    def set_update(self, update):
        """"torch" or "device" (the module's docstring).  "device" needs a device gradient mode (``set_gradient`` first); the optimiser is
        checked at every step, so it may still be replaced -- by one the fused step covers.  ``set_gradient("autograd")`` takes the mode back
        to "torch"."""
        if update not in UPDATES:
            raise ValueError(f"update {update!r}: one of {', '.join(map(repr, UPDATES))}")
        if update == "device" and self.gradient == "autograd":
            raise ValueError('Trainer.set_update("device"): the fused step runs behind a device gradient; call set_gradient("device") '
                             'or set_gradient("device_lstm") first (with occupancy-map columns: "device_om" or "device_lstm_om")')
        self.update = update

    def _sgd(self):
        """``fused_sgd_settings`` of ``self.optimizer``, its momentum buffers bound to ``self.momentum`` as views.  The binding (and the
        check of the optimiser's parameters against the model's) is made when the optimiser, its state or its group is another object than
        at the step before -- a new optimiser, ``load_state_dict``, ``set_gradient`` -- or a buffer is no longer the view bound (torch's
        first step of its own clones the gradient); a step on the same objects only reads the group's settings again."""
        opt = self.optimizer
        bound = self._sgd_bound
        if (bound is not None and bound[0] is opt and bound[1] is opt.state and bound[2] is opt.param_groups[0] and bound[3] is self.flat
                and opt.state[bound[4]].get("momentum_buffer") is self._momentum_views[0]):
            return fused_sgd_settings(opt)
        params = [p for layer in self.net.layers for p in value_net.layer_params(layer)]
        settings = fused_sgd_settings(opt, params)
        if self.momentum is None or self.momentum.numel() != self.flat.numel() or self.momentum.device != self.flat.device:
            self.momentum = torch.zeros_like(self.flat)
        # a fresh optimiser starts from zero momentum, buffers that torch's step or load_state_dict made are taken over
        views = []
        with torch.no_grad():
            for p, at in zip(params, value_net.param_offsets(self.net)):
                view, old = self.momentum[at:at + p.numel()].view(p.shape), opt.state[p].get("momentum_buffer")
                if old is None:
                    view.zero_()
                elif old.data_ptr() != view.data_ptr():
                    view.copy_(old)
                opt.state[p]["momentum_buffer"] = view
                views.append(view)
        self._momentum_views = tuple(views)
        self._sgd_bound = (opt, opt.state, opt.param_groups[0], self.flat, params[0])
        return settings

    @staticmethod
    def _check_states(states, cols, kind, who='Trainer.set_gradient("device")'):
        """The stored states the gradient kernels take: float32 [., n, cols] on the GPU ([., cols] as well for CADRL, whose n is 1)."""
        if states is None:
            return
        dims = (2, 3) if kind == value_net.CS_VN_CADRL else (3,)
        if states.dim() not in dims or states.shape[-1] != cols or states.dtype != torch.float32:
            raise ValueError(f"{who}: the memory's states are {tuple(states.shape[1:])} {states.dtype} rows; the gradient "
                             f"kernel takes float32 [n, {cols}]")

    def _loader(self):
        if self.data_loader is None:
            if self.gradient != "autograd" and hasattr(self.memory, "sample"):
                self.data_loader = _MemoryLoader(self.memory, self.batch_size)
            else:
                self.data_loader = DataLoader(self.memory, self.batch_size, shuffle=True)
        return self.data_loader

    def _device_inputs(self, inputs):
        """What a minibatch of either device gradient mode is checked for before its launches; leaves the float32 blob current."""
        self._check_states(inputs, self.net.cols + self.net.om_cols, self.net.kind, f'Trainer.set_gradient("{self.gradient}")')
        self.net.refresh("f32")
        for p in self.model.parameters():       # (an optimiser's zero_grad(set_to_none) dropped the views: the kernel writes them whole)
            if p.grad is None:
                raise ValueError(f'Trainer: a parameter lost its gradient view; call set_gradient("{self.gradient}") again')

    def _enqueue_fused_step(self, inputs, values):
        """One optimiser step of "device" update mode on a minibatch, enqueued: nothing is read back, the loss is added to
        ``self.loss_sum`` on the device and left in ``self.last_loss`` (a CUDA tensor of one element)."""
        self._device_inputs(inputs)
        lr, momentum = self._sgd()
        self.last_loss = _MODES[self.gradient].train_step(self.net, self.flat, self.momentum, inputs.contiguous(), values.reshape(-1).contiguous(),
                                                          self.flat_grad, lr, momentum, loss_sum=self._device_sum())

    def _step(self, inputs, values):
        """One optimiser step on a minibatch; returns the loss as a Python float (a read-back in every mode: the loops of "device" update
        mode enqueue their steps with ``_enqueue_fused_step`` instead)."""
        if self.update == "device":
            self._enqueue_fused_step(inputs, values)
            return self.last_loss.item()
        if self.gradient != "autograd":
            self._device_inputs(inputs)
            loss = _MODES[self.gradient].loss_and_grad(self.net, self.flat, inputs.contiguous(), values.reshape(-1).contiguous(), self.flat_grad)
            self.optimizer.step()
            return loss.item()
        self.optimizer.zero_grad()
        outputs = self.model(inputs)
        loss = self.criterion(outputs, values)
        loss.backward()
        self.optimizer.step()
        return loss.data.item()

    def _device_sum(self):
        """The float64 the fused steps add their losses to, on the parameters' device"""
        if self.loss_sum is None or self.loss_sum.device != self.flat.device:
            self.loss_sum = torch.zeros(1, dtype=torch.float64, device=self.flat.device)
        return self.loss_sum

    def _run(self, minibatches):
        """One optimiser step per minibatch; the sum of their losses as the reference forms it (a Python float grown by loss.item()).  In
        "device" update mode the steps are only enqueued and the same float64 sum, formed on the device in the same order, is read once."""
        fused = self.update == "device"
        if fused:
            self._device_sum().zero_()
        total = 0
        for inputs, values in minibatches:
            if fused:
                self._enqueue_fused_step(inputs, values)
            else:
                total += self._step(inputs, values)
        return self.loss_sum.item() if fused else total

    # ------------------------------------------------------------------ the reference's two loops
    def optimize_epoch(self, num_epochs):
        if self.optimizer is None:
            raise ValueError('Learning rate is not set!')
        loader = self._loader()
        average_epoch_loss = 0
        for epoch in range(num_epochs):
            epoch_loss = self._run(loader)
            average_epoch_loss = epoch_loss / len(self.memory)
            logging.debug('Average loss in epoch %d: %.2E', epoch, average_epoch_loss)
        return average_epoch_loss

    def optimize_batch(self, num_batches):
        if self.optimizer is None:
            raise ValueError('Learning rate is not set!')
        loader = self._loader()
        losses = self._run(next(iter(loader)) for _ in range(num_batches))
        average_loss = losses / num_batches
        logging.debug('Average loss : %.2E', average_loss)
        return average_loss
