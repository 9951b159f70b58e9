"""SARL (Chen et al. 2019, "Crowd-Robot Interaction: Crowd-aware Robot Navigation with Attention-based Deep Reinforcement Learning"):
a pairwise MLP per human, attention over the humans, a value MLP on (robot state, attended crowd feature).  Fixed from outside: the
[sarl] configuration keys and the checkpoint's submodule names (mlp1, mlp2, attention, mlp3), so a reference checkpoint loads."""
from __future__ import annotations

import logging

import torch
import torch.nn as nn

from .cadrl import mlp, width_list
from .multi_human_rl import MultiHumanRL


class ValueNetwork(nn.Module):
    def __init__(self, input_dim, self_state_dim, mlp1_dims, mlp2_dims, mlp3_dims, attention_dims, with_global_state):
        super().__init__()
        embed = int(mlp1_dims[-1])
        self.self_state_dim = int(self_state_dim)
        self.global_state_dim = embed
        self.with_global_state = bool(with_global_state)
        self.attention_weights = None
        # submodules in the order of a reference checkpoint's keys
        self.mlp1 = mlp(input_dim, mlp1_dims, last_relu=True)                           # per-human embedding
        self.mlp2 = mlp(embed, mlp2_dims)                                               # per-human feature
        self.attention = mlp(embed * 2 if self.with_global_state else embed, attention_dims)   # score from (embedding[, crowd mean])
        self.mlp3 = mlp(int(mlp2_dims[-1]) + self.self_state_dim, mlp3_dims)            # value

    def forward(self, state):
        """state [batch, humans, joint state] -> value [batch, 1]"""
        batch, humans, _ = state.shape
        embedding = self.mlp1(state.flatten(0, 1)).view(batch, humans, -1)
        feature = self.mlp2(embedding)
        if self.with_global_state:      # every human's embedding next to the crowd's mean embedding
            crowd = embedding.mean(dim=1, keepdim=True).expand_as(embedding)
            scores = self.attention(torch.cat([embedding, crowd], dim=2))
        else:
            scores = self.attention(embedding)
        # the masked softmax as published: a score of exactly 0 marks a padded human, and no maximum is subtracted
        e = torch.where(scores != 0, torch.exp(scores), torch.zeros_like(scores))
        weights = e / e.sum(dim=1, keepdim=True)
        self.attention_weights = weights[0].detach().squeeze(-1).cpu().numpy()
        crowd_feature = (weights * feature).sum(dim=1)
        return self.mlp3(torch.cat([state[:, 0, :self.self_state_dim], crowd_feature], dim=1))


class SARL(MultiHumanRL):
    display_name = "SARL"
    config_section = "sarl"

    def configure(self, config):
        self.set_common_parameters(config)
        section = self.config_section
        self.with_om = config.getboolean(section, "with_om")
        if self.with_om:
            raise NotImplementedError("OM-SARL (sarl.with_om = true) is a policy of its own here: the rows widened by the humans' occupancy maps "
                                      "have their own decision kernel; build it with policy_factory[\"om_sarl\"]")
        widths = {key: width_list(config.get(section, key)) for key in ("mlp1_dims", "mlp2_dims", "mlp3_dims", "attention_dims")}
        self.model = ValueNetwork(self.input_dim(), self.self_state_dim, widths["mlp1_dims"], widths["mlp2_dims"], widths["mlp3_dims"],
                                  widths["attention_dims"], config.getboolean(section, "with_global_state"))
        self.multiagent_training = config.getboolean(section, "multiagent_training")
        logging.debug("%s: attention %s the crowd's mean embedding, widths %s", self.name, "with" if self.model.with_global_state else "without", widths)

    def get_attention_weights(self):
        """The attention over the humans for the LAST action of the last decision (what a per-action model() loop leaves behind, and what
        the reference's renderer shows): one forward of the torch module on that action's rows, on demand -- not on the hot path."""
        rot = getattr(self, "_last_rotated", None)
        if callable(rot):               # a "fused" decision wrote no rows: the last action's are generated now
            rot = rot()[0]
        if rot is not None:
            with torch.no_grad():
                self.model(rot[0, -1:].to(next(self.model.parameters()).device))
            self._last_rotated = None
        return self.model.attention_weights
