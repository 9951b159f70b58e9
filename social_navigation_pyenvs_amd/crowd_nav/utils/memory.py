"""The replay memory of the value-based trainers (the interface of crowd_nav/utils/memory.py: ``push((state, value))``, ``is_full``,
``__getitem__``, ``__len__``, ``clear``, a torch ``Dataset``), kept as a ring in two preallocated tensors on one device -- states
[capacity, ...] and values [capacity, 1] -- so that W worlds' joint states and targets go in with ``push_batch`` straight from
``joint_state_device`` / ``value_device`` and a minibatch comes out with ``sample``, nothing crossing to the host.

The ring's write position and fill count live on the device as well: ``push_batch`` with a ``keep`` mask stores a number of samples the host
never learns.  ``len()`` (and what needs it: ``is_full``, ``sample``, a DataLoader) reads the count back when a masked push left it
unknown, and remembers it until the next one."""
from __future__ import annotations

import torch
from torch.utils.data import Dataset


class ReplayMemory(Dataset):
    def __init__(self, capacity):
        self.capacity = int(capacity)
        if self.capacity < 1:
            raise ValueError("ReplayMemory: the capacity must be at least 1")
        self.states = self.values = None        # [capacity + 1, ...]: the last row takes what a keep mask drops
        self._position = self._count = None     # int64 device scalars
        self._len = 0                           # the host's copy of the count; None: unknown since a masked push

    # ------------------------------------------------------------------ storage
    def _allocate(self, state, value_dtype):
        self.states = torch.zeros((self.capacity + 1,) + tuple(state.shape), dtype=state.dtype, device=state.device)
        self.values = torch.zeros((self.capacity + 1, 1), dtype=value_dtype, device=state.device)
        self._position = torch.zeros((), dtype=torch.int64, device=state.device)
        self._count = torch.zeros((), dtype=torch.int64, device=state.device)

    def _attach(self, state_shape, dtype, device):
        """What a writer that fills the ring itself (crowd_nav.utils.episodes.EpisodeBuffer.flush) needs first: the tensors of an empty
        memory allocated for states of `state_shape`, as push_batch does on first use, and a memory of another state shape, dtype or device
        refused."""
        if self.states is None:
            self._allocate(torch.empty(tuple(state_shape), dtype=dtype, device=device), torch.float32)
        have = (tuple(self.states.shape[1:]), self.states.dtype, self.values.dtype, self.states.device)
        if have != (tuple(state_shape), dtype, torch.float32, torch.device(device)):
            raise ValueError(f"ReplayMemory: states {tuple(state_shape)} {dtype} on {device} in a memory of {have[0]} {have[1]} (values {have[2]}) "
                             f"on {have[3]}")

    @property
    def device(self):
        return None if self.states is None else self.states.device

    def push_batch(self, states, values, keep=None):
        """Store states [W, ...] with values [W] (or [W, 1]) behind what the ring holds, the oldest samples giving way at capacity; with
        `keep` (bool [W]) only the worlds where it is true, in their order.  W may not exceed the capacity.  Device work only."""
        W = states.shape[0]
        if W > self.capacity:
            raise ValueError(f"ReplayMemory.push_batch: {W} samples at once exceed the capacity {self.capacity}")
        values = values.reshape(W, 1)
        if self.states is None:
            self._allocate(states[0], values.dtype)
        if tuple(states.shape[1:]) != tuple(self.states.shape[1:]):
            raise ValueError(f"ReplayMemory: a state of shape {tuple(states.shape[1:])} in a memory of {tuple(self.states.shape[1:])}")
        states, values = states.to(self.states.device, self.states.dtype), values.to(self.values.device, self.values.dtype)
        if keep is None:
            slot = (self._position + torch.arange(W, device=self.states.device)) % self.capacity
            kept = W
            if self._len is not None:
                self._len = min(self._len + W, self.capacity)
        else:
            keep = keep.to(self.states.device).reshape(W).bool()
            order = torch.cumsum(keep, 0) - 1
            slot = torch.where(keep, (self._position + order) % self.capacity, torch.full_like(order, self.capacity))
            kept = keep.sum()
            self._len = None
        self.states.index_copy_(0, slot, states)
        self.values.index_copy_(0, slot, values)
        self._position = (self._position + kept) % self.capacity
        self._count = torch.clamp(self._count + kept, max=self.capacity)

    def push(self, item):
        """One (state, value) pair, as the reference's trainer and explorer push them."""
        state, value = item
        state = torch.as_tensor(state)
        value = torch.as_tensor(value, dtype=torch.float32 if not torch.is_tensor(value) else None)
        self.push_batch(state[None], value.reshape(1).to(state.device))

    # ------------------------------------------------------------------ the reference's interface
    def __len__(self):
        if self._len is None:
            self._len = int(self._count.item())
        return self._len

    def is_full(self):
        return len(self) == self.capacity

    def __getitem__(self, item):
        if not -len(self) <= item < len(self):
            raise IndexError(item)
        return self.states[item % len(self)], self.values[item % len(self)]

    def clear(self):
        self.states = self.values = self._position = self._count = None
        self._len = 0

    # ------------------------------------------------------------------ minibatches
    def sample(self, batch_size, generator=None):
        """(inputs [B, ...], values [B, 1]) of `batch_size` stored samples drawn with replacement (`generator`: a torch.Generator on the
        memory's device)."""
        if len(self) == 0:
            raise ValueError("ReplayMemory.sample: the memory is empty")
        index = torch.randint(len(self), (int(batch_size),), generator=generator, device=self.states.device)
        return self.states[index], self.values[index]
