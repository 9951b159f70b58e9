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
              csrc/value_net_lstm_grad.hip)."""
from __future__ import annotations

import logging

import torch
import torch.nn as nn
import torch.optim as optim
from torch.utils.data import DataLoader

from ..policy import value_net

GRADIENTS = ("autograd", "device", "device_lstm")


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

    def set_learning_rate(self, learning_rate):
        logging.info('Current learning rate: %f', learning_rate)
        self.optimizer = optim.SGD(self.model.parameters(), lr=learning_rate, momentum=0.9)

    # ------------------------------------------------------------------ the gradient's path
    def set_gradient(self, gradient, net=None):
        """"autograd", "device" or "device_lstm" (the module's docstring).  `net`: the value_net.DeviceNet whose blob the device modes keep
        current -- a policy's own (``policy.device_net()``), so that its decisions read the trained weights without a host round trip;
        None: one of the trainer's.  "device" refuses a module that is not CADRL's or SARL's network, "device_lstm" one without an LSTM or
        with map columns (OM-LSTM-RL); both a model on the CPU, a model that is not float32, a memory whose stored states are not
        [., n, 13 | 15] float32 rows and a `net` that is not this model's."""
        if gradient not in GRADIENTS:
            raise ValueError(f"gradient {gradient!r}: one of {', '.join(map(repr, GRADIENTS))}")
        if gradient == "autograd":
            if self.net is not None:
                self.net.adopt_flat(None)
            self.gradient, self.net, self.flat, self.flat_grad = gradient, None, None, None
            return
        kind, _, layers = value_net.describe(self.model)
        params = [p for layer in layers for p in value_net.layer_params(layer)]
        first = layers[0] if layers else None
        cols = getattr(first, "in_features", getattr(first, "input_size", 0))       # (network 1's first layer is the nn.LSTM itself)
        who = f'Trainer.set_gradient("{gradient}")'
        if gradient == "device_lstm":
            has_kernel, which = value_net.has_recurrent_gradient_kernel, "recurrent"
            if kind != value_net.CS_VN_LSTM:
                raise ValueError(f'{who}: the module has no LSTM; CADRL and SARL train with set_gradient("device")')
            if cols not in (13, 15):
                raise ValueError(value_net.RECURRENT_GRADIENT_REFUSAL.format(f"{who} on rows of {cols} columns"))
        else:
            has_kernel, which = value_net.has_gradient_kernel, "feed-forward"
            if kind == value_net.CS_VN_LSTM or cols not in (13, 15) or not has_kernel(value_net.family_of(kind, 0)):
                raise ValueError(value_net.GRADIENT_REFUSAL.format(who))
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
        net.adopt_flat(flat)
        self.gradient, self.net, self.flat, self.flat_grad = gradient, net, flat, grad

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

    def _step(self, inputs, values):
        """One optimiser step on a minibatch; returns the loss as a Python float."""
        if self.gradient != "autograd":
            self._check_states(inputs, self.net.cols, self.net.kind, f'Trainer.set_gradient("{self.gradient}")')
            self.net.refresh("f32")
            for p in self.model.parameters():       # (an optimiser's zero_grad(set_to_none) dropped the views: the kernel writes them whole)
                if p.grad is None:
                    raise ValueError(f'Trainer: a parameter lost its gradient view; call set_gradient("{self.gradient}") again')
            kernel = value_net.loss_and_grad_lstm if self.gradient == "device_lstm" else value_net.loss_and_grad
            loss = kernel(self.net, self.flat, inputs.contiguous(), values.reshape(-1).contiguous(), self.flat_grad)
            self.optimizer.step()
            return loss.item()
        self.optimizer.zero_grad()
        outputs = self.model(inputs)
        loss = self.criterion(outputs, values)
        loss.backward()
        self.optimizer.step()
        return loss.data.item()

    # ------------------------------------------------------------------ the reference's two loops
    def optimize_epoch(self, num_epochs):
        if self.optimizer is None:
            raise ValueError('Learning rate is not set!')
        loader = self._loader()
        average_epoch_loss = 0
        for epoch in range(num_epochs):
            epoch_loss = 0
            for inputs, values in loader:
                epoch_loss += self._step(inputs, values)
            average_epoch_loss = epoch_loss / len(self.memory)
            logging.debug('Average loss in epoch %d: %.2E', epoch, average_epoch_loss)
        return average_epoch_loss

    def optimize_batch(self, num_batches):
        if self.optimizer is None:
            raise ValueError('Learning rate is not set!')
        loader = self._loader()
        losses = 0
        for _ in range(num_batches):
            inputs, values = next(iter(loader))
            losses += self._step(inputs, values)
        average_loss = losses / num_batches
        logging.debug('Average loss : %.2E', average_loss)
        return average_loss
