"""Policy base class (reference: crowd_nav/policy_no_train/policy.py) and the seam to the batched kernel (cs_policy_no_train).

``predict(JointState)`` packs the robot's FullState into a 13-column safe-state record and the humans into [1][n][5|7] observation rows
-- the layouts the batched Gym keeps resident -- and runs the same kernel with W = 1, so one robot alone and a batch of 4096 give the
same bits.  There is no host implementation of the policies: without a GPU ``predict`` raises ``CrowdstepError``."""
from __future__ import annotations

import numpy as np

from ..utils.action import ActionXY

# include/crowdstep.h CS_PNT_*
CS_PNT_BP, CS_PNT_SSP, CS_PNT_SFM_HELBING, CS_PNT_SFM_GUO, CS_PNT_SFM_MOUSSAID = 0, 1, 2, 3, 4
CS_PNT_MASS, CS_PNT_N_PARAMS = 20, 21
# agent.py:269 slot order of the 20-parameter row
PARAM_SLOTS = ["relaxation_time", "Ai", "Aw", "Bi", "Bw", "Ci", "Cw", "Di", "Dw", "Ei", "k1", "k2", "agent_lambda", "gamma", "ns",
               "ns1", "ko", "kd", "alpha", "k_lambda"]


class Policy:
    def __init__(self):
        self.trainable = False
        self.phase = None
        self.model = None
        self.device = None
        self.last_state = None
        self.time_step = None
        self.env = None

    def configure(self, config):
        return

    def set_phase(self, phase):
        self.phase = phase

    def set_device(self, device):
        self.device = device

    def set_env(self, env):
        self.env = env

    def get_model(self):
        return self.model

    def predict(self, state):
        raise NotImplementedError

    @staticmethod
    def reach_destination(state):
        s = state.self_state
        return bool(np.linalg.norm((s.py - s.gy, s.px - s.gx)) < s.radius)


def pack_params(params: dict) -> np.ndarray:
    """The policy's parameter dict in the kernel's layout: the 20 agent.py slots, the mass in slot CS_PNT_MASS (absent keys: 0)."""
    out = np.zeros(CS_PNT_N_PARAMS, np.float32)
    for k, v in params.items():
        if k in PARAM_SLOTS:
            out[PARAM_SLOTS.index(k)] = v
    out[CS_PNT_MASS] = params.get("mass", 0.0)
    return out


def robot_record(self_state) -> np.ndarray:
    """FullState -> one safe-state row (agent.py:256-258): x, y, yaw, Vx, Vy, BVx, BVy, Omega, radius, mass, gx, gy, v_pref."""
    s = self_state
    return np.array([s.px, s.py, s.theta, s.vx, s.vy, 0.0, 0.0, 0.0, s.radius, 0.0, s.gx, s.gy, s.v_pref], np.float32)


def observation_rows(human_states) -> np.ndarray:
    """ObservableState(Headed) list -> [n][5] rows px, py, vx, vy, radius (theta / omega are not read by these policies)."""
    return np.array([[h.px, h.py, h.vx, h.vy, h.radius] for h in human_states], np.float32).reshape(len(human_states), 5)


def launch(policy_id: int, W: int, n: int, d_robot13: int, d_obs: int, obs_cols: int, time_step: float, params, d_action: int,
           stream=None) -> None:
    """cs_policy_no_train on device pointers; ``params`` a float32 [CS_PNT_N_PARAMS] host array or None (bp / ssp)."""
    from ... import _lib

    p = None if params is None else np.ascontiguousarray(params, np.float32)
    _lib.check(_lib.load().cs_policy_no_train(policy_id, W, n, d_robot13, d_obs, obs_cols, 0.0 if time_step is None else time_step,
                                              None if p is None else p.ctypes.data, d_action, stream))


class NoTrainPolicy(Policy):
    """A policy whose ``predict`` is one W = 1 launch of cs_policy_no_train."""
    pnt_id = None
    params: dict = {}

    def packed_params(self):
        """The kernel's parameter array (None for bp / ssp), repacked only when the params dict changed."""
        if self.pnt_id < CS_PNT_SFM_HELBING:
            return None
        key = tuple(self.params.items())
        if getattr(self, "_packed_key", None) != key:
            self._packed, self._packed_key = pack_params(self.params), key
        return self._packed

    def _buffers(self, n):
        from ... import _lib

        bufs = getattr(self, "_bufs", None)
        if bufs is None or bufs["n"] != n:
            bufs = dict(n=n, robot=_lib.DeviceBuffer((1, 13)), obs=_lib.DeviceBuffer((1, max(n, 1), 5)), act=_lib.DeviceBuffer((1, 2)))
            self._bufs = bufs
        return bufs

    def predict(self, state):
        rows = observation_rows(state.human_states)
        n = rows.shape[0]
        b = self._buffers(n)
        b["robot"].upload(robot_record(state.self_state)[None])
        if n:
            b["obs"].upload(rows.reshape(1, n, 5))
        launch(self.pnt_id, 1, n, b["robot"].ptr, b["obs"].ptr, 5, self.time_step, self.packed_params(), b["act"].ptr)
        a = b["act"].download()[0]
        self.last_state = state
        return ActionXY(float(a[0]), float(a[1]))
