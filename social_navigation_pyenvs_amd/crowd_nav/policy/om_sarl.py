"""OM-SARL (Chen et al. 2019; the reference's SARL with ``sarl.with_om = true``): SARL whose per-human rows are widened by a local occupancy
map of the OTHER humans -- cell_num x cell_num cells of cell_size metres around the human, in the frame of its velocity, om_channel_size
values a cell ([om] section).  Fixed from outside: the [sarl] and [om] configuration keys, the attributes (with_om, cell_num, cell_size,
om_channel_size), ``build_occupancy_maps``' signature and result, and the checkpoint's keys and shapes (mlp1's first layer is
joint_state_dim + cell_num^2 * om_channel_size wide), so a reference OM-SARL checkpoint loads with strict=True.

The maps are cs_occupancy_maps (csrc/occupancy_map.hip), the decision cs_lookahead -> cs_occupancy_maps on the NEXT human states ->
cs_value_net_decide_om (csrc/value_net_om.hip): SARL's decision from the same rows and rewards with the maps the reference's serial branch
builds (multi_human_rl.py:75-78; its parallel branch reads a name it never binds).

``set_wide_precision("bf16")`` moves ``predict`` and the batched Gym's ``act_device`` to the opt-in bf16 arithmetic
(cs_value_net_decide_om_bf16, csrc/value_net_om_bf16.hip): mlp1's layer 0 keeps the rotated columns float32 and takes the
map columns in bf16, everything behind it is SARL's bf16 decision.  ``set_decision_precision("bf16")`` and ``set_decision_input("fused")``
keep refusing: those are the kernels without map columns.  ``transform``, ``state_value``, ``joint_state_device``, the Gym's
``value_device`` and the trainers stay float32.

It is a key of its own in policy_factory, "om_sarl": ``policy_factory["sarl"]`` with with_om = true keeps raising."""
from __future__ import annotations

import logging

import numpy as np
import torch

from ... import _lib
from . import value_net
from .cadrl import width_list
from .sarl import SARL, ValueNetwork


class OMSARL(SARL):
    display_name = "OM-SARL"
    family = value_net.MAPPED            # (two humans at least for ``predict`` and ``state_value``: a lone human has nobody to map)

    def configure(self, config):
        self.set_common_parameters(config)
        section = self.config_section
        if not config.getboolean(section, "with_om"):
            raise ValueError("OM-SARL is SARL with occupancy maps: sarl.with_om = false is policy_factory['sarl']")
        if self.om_channel_size not in (1, 2, 3):
            raise NotImplementedError(f"om_channel_size {self.om_channel_size}: 1 (occupancy), 2 (mean velocity) or 3 (both)")
        if self.cell_num < 1 or not self.cell_size > 0:
            raise ValueError(f"{self.name}: om.cell_num must be positive and om.cell_size > 0")
        self.with_om = True
        widths = {key: width_list(config.get(section, key)) for key in ("mlp1_dims", "mlp2_dims", "mlp3_dims", "attention_dims")}
        self.model = ValueNetwork(self.input_dim(), self.self_state_dim, widths["mlp1_dims"], widths["mlp2_dims"], widths["mlp3_dims"],
                                  widths["attention_dims"], config.getboolean(section, "with_global_state"))
        self.multiagent_training = config.getboolean(section, "multiagent_training")
        logging.debug("%s: %d map columns, widths %s", self.name, self.map_columns(), widths)

    def set_wide_precision(self, precision):
        """The arithmetic of the decision kernel on the rows with map columns, for ``predict`` and ``act_device`` alike: "f32" (the
        default) or the opt-in "bf16" (DESIGN.md 4.5).  ``decision_precision`` and ``decision_input`` stay ("f32", "tensor")."""
        self.wide_precision = value_net.check_wide_precision(precision, self.family)

    def map_columns(self):
        return int(self.cell_num) ** 2 * int(self.om_channel_size) if self.with_om else 0

    def input_dim(self):
        return self.joint_state_dim + self.map_columns()

    def om_grid(self):
        return int(self.cell_num), float(self.cell_size), int(self.om_channel_size)

    def _new_device_net(self, model):
        return value_net.DeviceNet(model, self.joint_state_dim, self.map_columns(), self.om_grid())

    # ------------------------------------------------------------------ the maps
    def build_occupancy_maps(self, human_states):
        """The reference's method (multi_human_rl.py:133-187): float32 tensor [humans, cell_num^2 * om_channel_size], row i the map around
        human i of the other humans.  The W = 1 launch of cs_occupancy_maps.  One human has nobody to map: ValueError, as there."""
        if len(human_states) < 2:
            raise ValueError("build_occupancy_maps needs at least two humans: a lone human has no other human to map")
        _lib.require_gpu()
        rows = np.array([[h.px, h.py, h.vx, h.vy] for h in human_states], np.float32)
        humans = torch.as_tensor(rows, device="cuda")[None].contiguous()
        return value_net.maps_of(humans, 2, self.om_grid(), torch.cuda.current_stream().cuda_stream)[0].cpu()

    def transform(self, state):
        """What a trainer stores for this decision: tensor [humans, 13 | 15 + C], every human's rotated joint state and its map."""
        maps = self.build_occupancy_maps(state.human_states).to(self.device)
        return torch.cat([super().transform(state), maps], dim=1)

    def get_attention_weights(self):
        """SARL's, on the wide rows: the last action's rotated rows beside the maps of that decision."""
        rot = getattr(self, "_last_rotated", None)
        if rot is not None and not callable(rot):
            with torch.no_grad():
                self.model(torch.cat([rot[0, -1], self._net.last_maps[0]], dim=1)[None].to(next(self.model.parameters()).device))
            self._last_rotated = None
        return self.model.attention_weights
