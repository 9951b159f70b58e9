"""DeviceLoop -- what ``BatchedSocialNavGym`` keeps on the GPU between two calls of its device-resident loop, every field declared once.

Built by ``BatchedSocialNavGym._device_loop_state()`` for one world batch; it holds no reference to the Gym.  An unknown field name is an
``AttributeError``; a field that exists only after some call starts as ``None`` / ``False``.  ``SideStream`` is the one stream scope of
the Gym's device methods.  torch is imported where the device is first touched, as in the Gym's module.
"""
from __future__ import annotations

import numpy as np

from .. import _lib


def clock_table(time_limit, time_step, factor):
    """``global_time`` after k Gym steps for every k an episode can reach: accumulated in float32, ``factor`` additions of ``time_step``
    per step (social_nav_gym.py:244) -- the same sequence as a table indexed by the per-world step counter."""
    max_steps = int(time_limit / (time_step * factor)) + 8
    clock = np.zeros(max_steps, np.float32)
    t = np.float32(0)
    for k in range(1, max_steps):
        for _ in range(factor):
            t = t + np.float32(time_step)
        clock[k] = t
    return clock


def stage_depth(level_bytes, depth, cap):
    """Episodes staged ahead per world: ``depth`` halved while the staging batch (``level_bytes`` a level) exceeds ``cap`` bytes -- never
    below 2 for that reason --, rounded down to a power of two."""
    d = max(1, int(depth))
    while d > 2 and d * level_bytes > cap:
        d //= 2
    return 1 << (d.bit_length() - 1)


class StepPieces:
    """The ctypes argument tuples of one (result set, auto-reset mode), bound once: ``step`` (cs_gym_step), ``tail`` (cs_consume_staged_worlds,
    or None), ``fold`` (cs_gym_step_staged, or None), ``keep`` -- the structs the byref arguments point into -- and the ``results`` a step returns."""
    __slots__ = ("step", "tail", "fold", "keep", "results")

    def __init__(self, step, tail, fold, keep, results):
        self.step, self.tail, self.fold, self.keep, self.results = step, tail, fold, keep, results

    __getitem__ = object.__getattribute__      # pieces["fold"]: how the nested dictionary this record replaces was read


class DeviceLoop:
    """Per-world step counters, seeds, the float32 clock table and the pre-staged next episodes, resident on the GPU."""
    __slots__ = (
        # the batch and the two streams: the step runs on a torch side stream (ordered against the caller's stream by SideStream); a
        # library stream carries the refill passes of the staging batch
        "cw", "stream", "stream_b", "released",
        # bookkeeping of the live worlds (cs_gym_book) and the persistent action / observation / result tensors
        "counter", "seeds", "stride", "gtime", "clock", "mask", "act", "obs", "out", "state", "cols", "results",
        # pre-staged episodes (include/crowdstep.h cs_stage_book) and their refill pass
        "depth", "base_seed", "epoch", "staged_seed", "staged_status", "failed", "pending", "staging", "stage_book", "staging_desc", "gen",
        "refill_args", "refill_ev", "since_refill",
        # what a call leaves for the next one
        "parity", "mode", "obs_fresh",
        # made by the first call that needs them: NEXT_STEP's two masks, a value-based decision's outputs, the look-ahead's gathers
        "ns_masks", "vn_values", "vn_choice", "la_cols", "la_robot_cols", "la_robot",
        # bound once: StepPieces per (parity, mode), no-train policies per factory name, their ctypes arguments per (id, time step, parameters)
        "pieces", "pnt_named", "pnt_args",
    )

    def __init__(self, cw, *, n, headed_obs, clock, seeds_host, stride, depth, gen, refill_priority):
        import ctypes as C

        import torch

        self.released = True            # (nothing to release before the library stream exists)
        W = cw.W
        self.cw, self.depth, self.gen = cw, depth, gen
        self.clock = torch.as_tensor(clock, device="cuda")
        self.counter = torch.zeros(W, dtype=torch.int32, device="cuda")
        self.parity = 0
        self.results = [(torch.zeros(W, dtype=torch.float32, device="cuda"), torch.zeros(W, dtype=torch.bool, device="cuda"),
                         torch.zeros(W, dtype=torch.bool, device="cuda"), torch.zeros(W, dtype=torch.int32, device="cuda"))
                        for _ in range(2)]
        self.gtime = torch.zeros(W, dtype=torch.float32, device="cuda")
        self.seeds = torch.as_tensor(seeds_host.astype(np.int64), device="cuda").to(torch.int32)
        # a world's seed moves on by the worlds of the WHOLE job when its episode ends: world w walks s + w + k * stride on
        # any rank count (ShardedBatchedSocialNavGym sets seed_stride = total_worlds; a single process: W)
        self.stride = int(stride)
        self.mask = torch.zeros(W, dtype=torch.int32, device="cuda")
        # episode e of world w draws base_seed[w] + e * stride; no slot's tag is the seed of the episode that belongs in it, so the
        # first refill pass generates every slot
        self.base_seed, self.epoch = self.seeds.clone(), torch.zeros(W, dtype=torch.int32, device="cuda")
        self.staged_seed = self.seeds.repeat(depth).contiguous()
        self.staged_status = torch.zeros(W * depth, dtype=torch.int32, device="cuda")
        self.failed = torch.zeros(W, dtype=torch.int32, device="cuda")
        self.pending = torch.zeros(W, dtype=torch.int32, device="cuda")     # cs_gym_step_staged: take-overs deferred to a later step
        self.out = cw._buffer("reward_out", (W, 7)).torch()
        self.state = cw.d_state.torch().view(W, cw.rows, 13)
        self.cols = torch.as_tensor([0, 1, 3, 4, 8] + ([2, 7] if headed_obs else []), device="cuda")
        self.mode, self.obs_fresh, self.since_refill = None, False, 0
        self.ns_masks = self.vn_values = self.vn_choice = self.la_cols = self.la_robot_cols = self.la_robot = None
        self.pieces, self.pnt_named, self.pnt_args = {}, {}, {}
        self.stream = torch.cuda.Stream()
        self.stream_b = _lib.stream_create(priority=refill_priority)
        self.released = False
        try:
            self.act = torch.zeros((W, 2), dtype=torch.float32, device="cuda")
            self.obs = torch.zeros((W, n, 7 if headed_obs else 5), dtype=torch.float32, device="cuda")
            self.staging = cw.staging_copy(depth)
            self.staging.stream = self.stream_b
            P = lambda t: t.data_ptr()
            self.stage_book = _lib.cs_stage_book(d_seeds=P(self.seeds), d_base_seed=P(self.base_seed), d_epoch=P(self.epoch),
                                                 d_staged_seed=P(self.staged_seed), d_staged_status=P(self.staged_status), d_failed=P(self.failed),
                                                 seed_stride=self.stride, depth=depth, d_pending=P(self.pending))
            self.staging_desc = self.staging.descriptor()
            self.refill_args = (C.byref(self.gen), C.byref(self.staging_desc), C.byref(self.stage_book), C.c_void_p(self.stream_b))
            self.refill_ev = _lib.Event()
            cw.stream = self.stream.cuda_stream
            torch.cuda.synchronize()
            # every world's next ``depth`` episodes, generated once up front; from here on a pass only regenerates the consumed slots
            self._refill()
            _lib.stream_sync(self.stream_b)
        except BaseException:
            self.release()
            raise

    def __getitem__(self, key):
        """``loop["name"]`` reads the field ``name`` and ``loop["pieces", parity, mode]`` the pieces bound for them: how the dictionary this
        object replaces was read, kept for callers outside the package.  An unknown name is an ``AttributeError`` here too."""
        return self.pieces[key[1:]] if isinstance(key, tuple) else getattr(self, key)

    def release(self):
        """The refill passes run on a library stream torch's allocator knows nothing about, on tensors torch owns (epoch, base_seed, the
        staging tags): before those tensors can go back to the allocator the stream must have drained -- and it is destroyed, not leaked."""
        if self.released:
            return
        self.released = True
        try:
            _lib.stream_sync(self.stream_b)
            _lib.stream_destroy(self.stream_b)
        except Exception:
            pass

    def _refill(self):
        _lib.check(_lib.load().cs_refill_staged_worlds(*self.refill_args))
        self.refill_ev.record(self.stream_b)
        self.since_refill = 0

    def maybe_refill(self, every):
        """Every ``every`` steps: one pass of cs_refill_staged_worlds on the side stream (at most one in flight).  Nothing orders it
        against the step's stream -- the staging slots carry tags (cs_stage_book) -- so it costs the step no wait and no event."""
        self.since_refill += 1
        if self.since_refill >= every and self.refill_ev.done():
            self._refill()

    def gym_book(self, parity, mask, prev_mask, auto_reset):
        reward, terminated, truncated, info = self.results[parity]
        return _lib.cs_gym_book(d_counter=self.counter.data_ptr(), d_seeds=self.seeds.data_ptr(), d_mask=mask.data_ptr(),
                                d_prev_mask=None if prev_mask is None else prev_mask.data_ptr(), d_clock=self.clock.data_ptr(),
                                clock_len=self.clock.numel(), auto_reset=int(bool(auto_reset)), d_reward=reward.data_ptr(),
                                d_terminated=terminated.data_ptr(), d_truncated=truncated.data_ptr(), d_info=info.data_ptr(),
                                seed_stride=self.stride)


class SideStream:
    """``with SideStream(loop) as s:`` -- a call's work on the loop's stream, ordered on the device with the caller's stream: before it with
    whatever produced the call's arguments, after it with whoever reads its results; the loop's stream is the current one inside.  On the
    way out the tensors in ``s.inputs`` (None entries skipped) are recorded on the loop's stream and those in ``s.outputs`` on the caller's,
    which is what lets torch's allocator take either back.  No wait and no stream switch where the caller already works on the loop's
    stream (``device_stream()``); after an exception nothing is recorded or waited for."""
    __slots__ = ("loop", "cur", "ctx", "inputs", "outputs")

    def __init__(self, loop):
        self.loop = loop
        self.inputs = self.outputs = ()

    def __enter__(self):
        import torch

        side = self.loop.stream
        cur = self.cur = torch.cuda.current_stream()
        self.ctx = None
        if cur.cuda_stream != side.cuda_stream:
            side.wait_stream(cur)
            self.ctx = torch.cuda.stream(side)
            self.ctx.__enter__()
        return self

    def __exit__(self, exc_type, exc, tb):
        side, cur = self.loop.stream, self.cur
        if exc_type is None:
            for t in self.inputs:
                if t is not None:
                    t.record_stream(side)
            for t in self.outputs:
                if t is not None:
                    t.record_stream(cur)
        if self.ctx is not None:
            self.ctx.__exit__(exc_type, exc, tb)
            if exc_type is None:
                cur.wait_stream(side)
        return False
