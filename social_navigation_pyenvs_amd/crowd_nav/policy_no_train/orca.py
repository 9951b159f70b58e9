"""ORCA robot policy (reference: crowd_nav/policy_no_train/orca.py): one RVO2 doStep in which the robot is agent 0, on the device.

The reference builds a ``rvo2.PyRVOSimulator`` per decision; this class runs csrc/policy_orca.hip instead -- the float32 restatement of
RVO2's computeNeighbors / computeNewVelocity this project carries, solved for agent 0 only (cs_policy_orca).  ``predict`` is one W = 1
launch of the kernel ``BatchedSocialNavGym.act_device`` runs for a whole batch, so one robot alone and a batch of 4096 give the same bits:
those of oracle/orca_oracle.c.  Parity with the rvo2 library itself stays unpinned, as for every ORCA path here.  It is built
by ``crowd_nav.policy.policy_factory["orca_device"]``; the no-train factory's ``"orca"`` keeps raising, as its tests pin.  There is no host
implementation: without a GPU ``predict`` raises ``CrowdstepError``."""
from __future__ import annotations

import numpy as np

from ..utils.action import ActionXY
from .policy import Policy, observation_rows, robot_record

KMAX = 10        # neighbours the kernel keeps at most (csrc/policy_orca.hip)


def orca_margin(safety_space) -> np.float32:
    """What the policy adds to every agent's radius (orca.py:100, :103), as the float32 the kernel adds."""
    return np.float32(0.01 + safety_space)


def launch(W: int, n: int, d_robot13: int, d_obs: int, obs_cols: int, time_step: float, neighbor_dist: float, max_neighbors: int,
           time_horizon: float, safety_space: float, d_action: int, stream=None) -> None:
    """cs_policy_orca on device pointers."""
    from ... import _lib

    _lib.check(_lib.load().cs_policy_orca(W, n, d_robot13, d_obs, obs_cols, 0.0 if time_step is None else time_step, neighbor_dist,
                                          max_neighbors, time_horizon, float(orca_margin(safety_space)), d_action, stream))


class ORCA(Policy):
    name = 'ORCA'
    trainable = False
    multiagent_training = None
    kinematics = 'holonomic'
    safety_space = 0
    neighbor_dist = 10
    max_neighbors = 10
    time_horizon = 5
    time_horizon_obst = 5          # no obstacles: unused
    radius = 0.3
    max_speed = 1
    sim = None

    def __init__(self):
        super().__init__()
        self.trainable = False

    def configure(self, config):
        return

    def set_phase(self, phase):
        return

    def _buffers(self, n):
        from ... import _lib

        bufs = getattr(self, "_bufs", None)
        if bufs is None or bufs["n"] != n:
            bufs = dict(n=n, robot=_lib.DeviceBuffer((1, 13)), obs=_lib.DeviceBuffer((1, max(n, 1), 5)), act=_lib.DeviceBuffer((1, 2)))
            self._bufs = bufs
        return bufs

    def predict(self, state):
        """One doStep for agent 0 (orca.py:82-132): the robot row and the [1][n][5] observation rows through the kernel with W = 1."""
        rows = observation_rows(state.human_states)
        n = rows.shape[0]
        b = self._buffers(n)
        b["robot"].upload(robot_record(state.self_state)[None])
        if n:
            b["obs"].upload(rows.reshape(1, n, 5))
        launch(1, n, b["robot"].ptr, b["obs"].ptr, 5, self.time_step, self.neighbor_dist, self.max_neighbors, self.time_horizon,
               self.safety_space, b["act"].ptr)
        a = b["act"].download()[0]
        self.last_state = state
        return ActionXY(float(a[0]), float(a[1]))
