"""OM-LSTM-RL (the reference's LSTM-RL with ``lstm_rl.with_om = true``): LSTM-RL whose per-human rows are widened by the local occupancy map
of the OTHER humans ([om] section; om_sarl.py describes the maps).  Fixed from outside: the [lstm_rl] and [om] configuration keys, the
attributes, ``build_occupancy_maps``' signature and result, the name -- the reference renames nothing: ``policy.name`` stays "LSTM-RL" --
and the checkpoint's keys and shapes (network 1: lstm.weight_ih_l0 is [4 H, joint_state_dim + C]; network 2: mlp1.0.weight is
[.., joint_state_dim + C]), so a reference checkpoint loads with strict=True.

The decision is cs_lookahead -> cs_occupancy_maps on the NEXT human states -> cs_value_net_decide_lstm_om (csrc/value_net_lstm.hip).  Which
map a step's row is paired with has two answers in the reference, and ``set_map_order`` chooses:

  "reference"  (the default) its serial decision (multi_human_rl.py:46-78): every action's next humans are sorted by decreasing distance to
               the robot's position under that action, but the maps are built once, on the first action's -- ActionXY(0, 0) -- sorted
               humans, and attached by position to every later action's rows.  The t-th row in an action's order carries the map of the
               human that was t-th in action 0's order.  (Its parallel branch reads a name it never binds)
  "own"        every human beside its own map: what ``transform`` (multi_human_rl.py:115-128) stores and a trainer evaluates, so what the
               network was trained on.

``set_mapped_precision("bf16")`` moves ``predict`` and the batched Gym's ``act_device`` to the opt-in bf16 arithmetic
(cs_value_net_decide_lstm_om_bf16, csrc/value_net_lstm_om_bf16.hip): the map columns and what LSTM-RL's bf16 kernel runs in
bf16, the rotated columns float32, the same order and pairing.  ``set_recurrent_precision("bf16")`` keeps refusing: that is the kernel
without map columns.

``transform``, ``state_value``, ``joint_state_device``, the Gym's ``value_device`` and the trainers stay float32 and evaluate the rows in
the humans' own order beside their own maps, whatever the map order and the precision.  It is a key of its own in policy_factory, "om_lstm_rl": ``policy_factory["lstm_rl_device"]`` with with_om = true keeps
raising."""
from __future__ import annotations

import logging

import torch

from . import value_net
from .cadrl import width_list
from .lstm_rl import LstmRL, ValueNetwork1, ValueNetwork2
from .om_sarl import OMSARL


class OMLstmRL(LstmRL):
    family = value_net.RECURRENT_MAPPED  # (two humans at least for ``predict`` and ``state_value``: a lone human has nobody to map)

    def __init__(self):
        super().__init__()
        self.map_order = "reference"

    def configure(self, config):
        self.set_common_parameters(config)
        section = self.config_section
        if not config.getboolean(section, "with_om"):
            raise ValueError("OM-LSTM-RL is LSTM-RL with occupancy maps: lstm_rl.with_om = false is policy_factory['lstm_rl_device']")
        if self.om_channel_size not in (1, 2, 3):
            raise NotImplementedError(f"om_channel_size {self.om_channel_size}: 1 (occupancy), 2 (mean velocity) or 3 (both)")
        if self.cell_num < 1 or not self.cell_size > 0:
            raise ValueError(f"{self.name}: om.cell_num must be positive and om.cell_size > 0")
        self.with_om = True
        mlp_dims = width_list(config.get(section, "mlp2_dims"))
        hidden = config.getint(section, "global_state_dim")
        self.with_interaction_module = config.getboolean(section, "with_interaction_module")
        if self.with_interaction_module:
            self.interaction_module_dims = width_list(config.get(section, "mlp1_dims"))
            self.model = ValueNetwork2(self.input_dim(), self.self_state_dim, self.interaction_module_dims, mlp_dims, hidden)
        else:
            self.model = ValueNetwork1(self.input_dim(), self.self_state_dim, mlp_dims, hidden)
        self.multiagent_training = config.getboolean(section, "multiagent_training")
        logging.debug("%s: %d map columns, %s pairwise interaction module, hidden width %d", self.name, self.map_columns(),
                      "with" if self.with_interaction_module else "without", hidden)

    def set_map_order(self, map_order):
        """Which map a step's row is paired with in ``predict`` and ``act_device``: "reference" (the default) or "own" (the module's
        docstring)."""
        self.map_order = value_net.check_map_order(map_order)
        for net in [self._net] + list(self._state_nets):
            if net is not None:
                net.map_order = map_order

    def set_mapped_precision(self, precision):
        """The arithmetic of the decision kernel on rows with map columns, for ``predict`` and ``act_device`` alike: "f32" (the default) or
        the opt-in "bf16" (DESIGN.md 4.5).  ``decision_precision``, ``decision_input`` and ``recurrent_precision`` stay ("f32", "tensor",
        "f32"); ``set_map_order`` keeps its meaning."""
        self.mapped_precision = value_net.check_mapped_precision(precision, self.family)

    map_columns = OMSARL.map_columns
    input_dim = OMSARL.input_dim
    om_grid = OMSARL.om_grid
    build_occupancy_maps = OMSARL.build_occupancy_maps

    def _new_device_net(self, model):
        return value_net.DeviceNet(model, self.joint_state_dim, self.map_columns(), self.om_grid(), self.map_order)

    def transform(self, state):
        """What a trainer stores for this decision: tensor [humans, 13 | 15 + C], every human's rotated joint state, in the humans' own
        order, and its own map."""
        maps = self.build_occupancy_maps(state.human_states).to(self.device)
        return torch.cat([super().transform(state), maps], dim=1)
