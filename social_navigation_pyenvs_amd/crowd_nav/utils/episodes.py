"""The episode-level half of the reference's ``Explorer`` (crowd_nav/utils/explorer.py:80-153: ``update_memory`` and the bookkeeping of
``run_k_episodes``) for W resident worlds: a per-world trajectory store on the device, and one flush that turns the episodes that just
ended into ``ReplayMemory`` samples -- only those whose outcome is kept (the reference: ReachGoal and Collision, never Timeout), with the
discounted return-to-go of imitation learning or the bootstrapped target given at each step, in the order and with the ring semantics of
the reference's ``push`` applied sample by sample, world-ascending then step-ascending.  Kernels: csrc/episodes.hip (cs_episode_append,
cs_episode_flush); nothing crosses to the host except in ``figures()``."""
from __future__ import annotations

from ...social_gym.src.info import INFO_BY_CODE
from ... import _lib
from .memory import ReplayMemory

TARGET_MODES = {"returns": 0, "stored": 1}      # include/crowdstep.h CS_EPISODE_RETURNS, CS_EPISODE_STORED
_CODE_BY_NAME = {cls.__name__: code for code, cls in enumerate(INFO_BY_CODE)}
MAX_STEPS = 2048                                 # a world's discount table and rewards live in LDS


class EpisodeBuffer:
    def __init__(self, n_worlds, max_steps, gamma, time_step, keep=("ReachGoal", "Collision")):
        self.W, self.T = int(n_worlds), int(max_steps)
        if self.W < 1:
            raise ValueError("EpisodeBuffer: n_worlds must be at least 1")
        if self.T < 1:
            raise ValueError("EpisodeBuffer: max_steps must be at least 1")
        if self.T > MAX_STEPS:
            raise ValueError(f"EpisodeBuffer: max_steps above {MAX_STEPS}")
        self.gamma, self.time_step = float(gamma), float(time_step)
        if not 0.0 < self.gamma <= 1.0:
            raise ValueError("EpisodeBuffer: gamma must lie in (0, 1]")
        if not self.time_step > 0.0:
            raise ValueError("EpisodeBuffer: time_step must be positive")
        self.keep_mask = 0
        for name in keep:
            name = name if isinstance(name, str) else name.__name__
            if name not in _CODE_BY_NAME:
                raise ValueError(f"EpisodeBuffer: keep names an unknown outcome {name!r} ({', '.join(_CODE_BY_NAME)})")
            self.keep_mask |= 1 << _CODE_BY_NAME[name]
        self.states = self.rewards = self.targets = self.cursor = self.overflow = self._figures = self._scratch = None
        self.state_shape = None

    # ------------------------------------------------------------------ storage
    def _allocate(self, state):
        import torch

        dev = state.device
        self.state_shape = tuple(state.shape[1:])
        self.F = 1
        for s in self.state_shape:
            self.F *= int(s)
        self.states = torch.zeros((self.W, self.T, self.F), dtype=torch.float32, device=dev)
        self.rewards = torch.zeros((self.W, self.T), dtype=torch.float32, device=dev)
        self.cursor = torch.zeros(self.W, dtype=torch.int32, device=dev)
        self.overflow = torch.zeros(self.W, dtype=torch.int32, device=dev)
        self._figures = torch.zeros(6, dtype=torch.float64, device=dev)
        self._scratch = torch.zeros(2 * (self.W + 1), dtype=torch.float64, device=dev)      # 16 (W + 1) bytes

    @property
    def device(self):
        return None if self.states is None else self.states.device

    def _vector(self, what, t, dtype):
        import torch

        if not torch.is_tensor(t):
            raise ValueError(f"EpisodeBuffer: {what} must be a tensor")
        if t.dtype != dtype:
            raise ValueError(f"EpisodeBuffer: {what} must be {dtype}, not {t.dtype}")
        if t.numel() != self.W or t.dim() > 2:
            raise ValueError(f"EpisodeBuffer: {what} of shape {tuple(t.shape)} for {self.W} worlds")
        if self.states is not None and t.device != self.states.device:
            raise ValueError(f"EpisodeBuffer: {what} on {t.device}, the buffer on {self.states.device}")
        return t.reshape(self.W).contiguous()

    def _need_gpu(self, what):
        """The buffer takes its shape from the first append wherever that tensor lives, so that every refusal above comes before this one;
        the kernels are the only path."""
        if self.states.device.type != "cuda":
            raise _lib.CrowdstepError(f"EpisodeBuffer.{what}: the tensors are on {self.states.device}; the episode buffer has no host path")

    @staticmethod
    def _stream():
        import torch

        return torch.cuda.current_stream().cuda_stream

    def append(self, state, reward, target=None):
        """One step of every world: ``state`` [W, ...] float32 CUDA (what the robot acted from), ``reward`` [W], and with ``target`` [W] the
        value ``flush(targets="stored")`` will store for it.  A world that already holds ``max_steps`` steps stores nothing and is flagged
        (``overflowed()``).  Device work only, on the current stream."""
        import torch

        if not torch.is_tensor(state):
            raise ValueError("EpisodeBuffer.append: the state must be a tensor")
        if state.dtype != torch.float32:
            raise ValueError(f"EpisodeBuffer.append: the state must be float32, not {state.dtype}")
        if state.dim() < 2 or state.shape[0] != self.W or state.numel() == 0:
            raise ValueError(f"EpisodeBuffer.append: a state of shape {tuple(state.shape)} for {self.W} worlds")
        if self.states is None:
            self._allocate(state)
        elif tuple(state.shape[1:]) != self.state_shape:
            raise ValueError(f"EpisodeBuffer.append: a state of shape {tuple(state.shape[1:])} in a buffer of {self.state_shape}")
        elif state.device != self.states.device:
            raise ValueError(f"EpisodeBuffer.append: a state on {state.device}, the buffer on {self.states.device}")
        reward = self._vector("the reward", reward, torch.float32)
        if target is not None:
            target = self._vector("the target", target, torch.float32)
            if self.targets is None:
                self.targets = torch.zeros((self.W, self.T), dtype=torch.float32, device=self.states.device)
        self._need_gpu("append")
        state = state.contiguous()
        _lib.check(_lib.load().cs_episode_append(self.W, self.T, self.F, state.data_ptr(), reward.data_ptr(),
                                                 None if target is None else target.data_ptr(), self.states.data_ptr(), self.rewards.data_ptr(),
                                                 None if self.targets is None else self.targets.data_ptr(), self.cursor.data_ptr(),
                                                 self.overflow.data_ptr(), self._stream()))

    def flush(self, memory, done, info_code, v_pref=1.0, targets="returns"):
        """The episodes of the worlds where ``done`` (bool / uint8 [W]) is set leave the buffer: those whose ``info_code`` (int32 [W], an
        index into ``info.INFO_BY_CODE``) is kept and that never overflowed go into ``memory`` sample by sample, the others are dropped;
        either way the world starts its next episode empty.  ``targets="returns"``: the value of a step is the discounted return-to-go
        with ``gamma^(k * time_step * v_pref)`` (``v_pref``: a number, or float [W]); ``"stored"``: the target given at append.  Device
        work only; ``len(memory)`` is unknown to the host afterwards, as after a masked ``push_batch``."""
        import torch

        if targets not in TARGET_MODES:
            raise ValueError(f"EpisodeBuffer.flush: targets must be one of {sorted(TARGET_MODES)}, not {targets!r}")
        if not isinstance(memory, ReplayMemory):
            raise ValueError("EpisodeBuffer.flush: the memory must be a crowd_nav.utils.memory.ReplayMemory")
        if self.states is None:
            raise ValueError("EpisodeBuffer.flush: nothing was appended yet")
        if targets == "stored" and self.targets is None:
            raise ValueError('EpisodeBuffer.flush: targets="stored" needs the targets given at append')
        if torch.is_tensor(done) and done.dtype == torch.bool:
            done = done.view(torch.uint8) if done.is_contiguous() else done.to(torch.uint8)
        done = self._vector("done", done, torch.uint8)
        info_code = self._vector("info_code", info_code, torch.int32)
        if torch.is_tensor(v_pref):
            if v_pref.device != self.states.device or v_pref.numel() != self.W:
                raise ValueError(f"EpisodeBuffer.flush: v_pref of shape {tuple(v_pref.shape)} on {v_pref.device} for {self.W} worlds")
            v_tensor, v_scalar = v_pref.reshape(self.W).to(torch.float64).contiguous(), 1.0
        else:
            v_tensor, v_scalar = None, float(v_pref)
        memory._attach(self.state_shape, torch.float32, self.states.device)
        self._need_gpu("flush")
        _lib.check(_lib.load().cs_episode_flush(self.W, self.T, self.F, self.states.data_ptr(), self.rewards.data_ptr(),
                                                None if self.targets is None else self.targets.data_ptr(), self.cursor.data_ptr(),
                                                self.overflow.data_ptr(), done.data_ptr(), info_code.data_ptr(), self.keep_mask,
                                                TARGET_MODES[targets], self.gamma, self.time_step, v_scalar,
                                                None if v_tensor is None else v_tensor.data_ptr(), memory.capacity, memory.states.data_ptr(),
                                                memory.values.data_ptr(), memory._position.data_ptr(), memory._count.data_ptr(),
                                                self._figures.data_ptr(), self._scratch.data_ptr(), self._stream()))
        memory._len = None

    # ------------------------------------------------------------------ what the reference logs
    def figures(self, time_limit=None):
        """The figures ``run_k_episodes`` logs, over the episodes flushed since the last ``reset()``: a dict of episodes, success,
        collision, timeout, success_rate, collision_rate, avg_nav_time (``time_limit`` when nobody arrived, explorer.py:105) and
        avg_discounted_reward, with the two float64 sums the averages come from (nav_time_sum, discounted_reward_sum).  Synchronises."""
        if self._figures is None:
            f = [0.0] * 6
        else:
            f = self._figures.tolist()
        episodes, success, collision, timeout = (int(x) for x in f[:4])
        return dict(episodes=episodes, success=success, collision=collision, timeout=timeout,
                    success_rate=success / episodes if episodes else 0.0, collision_rate=collision / episodes if episodes else 0.0,
                    avg_nav_time=f[4] / success if success else time_limit, avg_discounted_reward=f[5] / episodes if episodes else 0.0,
                    nav_time_sum=f[4], discounted_reward_sum=f[5])

    def overflowed(self):
        """int32 CUDA [W]: 1 where the running episode was stepped beyond ``max_steps`` (it will not be stored).  No synchronisation."""
        if self.overflow is None:
            raise ValueError("EpisodeBuffer.overflowed: nothing was appended yet")
        return self.overflow

    def reset(self):
        """Forget the running episodes and the figures; the allocation and its state shape stay."""
        if self.states is not None:
            self.cursor.zero_()
            self.overflow.zero_()
            self._figures.zero_()
