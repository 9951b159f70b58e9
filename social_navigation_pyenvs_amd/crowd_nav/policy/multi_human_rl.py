"""MultiHumanRL: the base of the value-based policies whose network takes all the humans' joint states at once ([batch, humans, joint
state]).  The decision is CADRL's W = 1 kernel launch with the subclass's network; what differs is the state handed to a trainer."""
from __future__ import annotations

import torch

from .cadrl import CADRL, joint_rows


class MultiHumanRL(CADRL):
    def input_dim(self):
        """Columns of one network input row.  OM-SARL (om_sarl.py) widens it by its occupancy maps."""
        return self.joint_state_dim

    def transform(self, state):
        """What a trainer stores for this decision: the rotated joint state of the robot with every human, tensor [humans, 13 | 15]."""
        rows = torch.from_numpy(joint_rows(state, self.with_theta_and_omega_visible)).to(self.device)
        return self.rotate(rows, theta_and_omega_visible=self.with_theta_and_omega_visible)
