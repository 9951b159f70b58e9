"""LSTM-RL (Everett et al. 2018; reference: crowd_nav/policy/lstm_rl.py): the humans' rotated joint states, sorted by decreasing distance to
the robot's next position, go through an LSTM whose last hidden state, next to the robot's own state, feeds the value MLP.  ValueNetwork1
reads the rows themselves, ValueNetwork2 puts a pairwise interaction module (mlp1) in front of the LSTM.  Fixed from outside: the module,
class and attribute names, the [lstm_rl] configuration keys and the checkpoint's keys and shapes (lstm.weight_ih_l0, lstm.weight_hh_l0,
lstm.bias_ih_l0, lstm.bias_hh_l0, mlp.<2 i>.*, mlp1.<2 i>.*), so a reference checkpoint loads with strict=True.

The decision is cs_lookahead -> cs_value_net_decide_lstm (csrc/value_net_lstm.hip): the sort by column 11, the interaction module, the n
dependent LSTM steps and the value MLP of all (world, action) pairs in one kernel, float32 on the look-ahead tensor; ``predict`` is its
W = 1 launch.  ``set_recurrent_precision("bf16")`` moves ``predict`` and the batched Gym's ``act_device`` to the opt-in bf16 arithmetic
(cs_value_net_decide_lstm_bf16, csrc/value_net_lstm_bf16.hip); ``state_value``, ``value_device``, ``joint_state_device`` and
the trainers stay float32.  ``set_recurrent_input("fused")`` moves both, in either precision, to cs_value_net_decide_lstm_worlds[_bf16]
(csrc/value_net_lstm_worlds.hip): the kernel generates its rows from the worlds' own, no look-ahead tensor, bit for bit the same decision.
The reference sorts inside ``predict`` only: ``transform`` keeps the humans' own order, and its trainer evaluates the target
network on those rows as stored, so ``state_value`` and ``value_device`` evaluate the rows in the order given.  It is a key of its own in
policy_factory, "lstm_rl_device": ``policy_factory["lstm_rl"]`` keeps raising."""
from __future__ import annotations

import logging

import torch
import torch.nn as nn

from . import value_net
from .cadrl import mlp, width_list
from .multi_human_rl import MultiHumanRL


class ValueNetwork1(nn.Module):
    def __init__(self, input_dim, self_state_dim, mlp_dims, lstm_hidden_dim):
        super().__init__()
        self.self_state_dim = int(self_state_dim)
        self.lstm_hidden_dim = int(lstm_hidden_dim)
        # submodules in the order of a reference checkpoint's keys
        self.mlp = mlp(self.self_state_dim + self.lstm_hidden_dim, mlp_dims)
        self.lstm = nn.LSTM(int(input_dim), self.lstm_hidden_dim, batch_first=True)

    def forward(self, state):
        """state [batch, humans, joint state], the humans in the order to scan -> value [batch, 1]"""
        _, (h_n, _) = self.lstm(state)                      # from zero (h0, c0)
        return self.mlp(torch.cat([state[:, 0, :self.self_state_dim], h_n.squeeze(0)], dim=1))


class ValueNetwork2(nn.Module):
    def __init__(self, input_dim, self_state_dim, mlp1_dims, mlp_dims, lstm_hidden_dim):
        super().__init__()
        self.self_state_dim = int(self_state_dim)
        self.lstm_hidden_dim = int(lstm_hidden_dim)
        self.mlp1 = mlp(input_dim, mlp1_dims)               # the pairwise interaction module (no ReLU behind its last layer)
        self.mlp = mlp(self.self_state_dim + self.lstm_hidden_dim, mlp_dims)
        self.lstm = nn.LSTM(int(mlp1_dims[-1]), self.lstm_hidden_dim, batch_first=True)

    def forward(self, state):
        batch, humans, _ = state.shape
        embedding = self.mlp1(state.flatten(0, 1)).view(batch, humans, -1)
        _, (h_n, _) = self.lstm(embedding)
        return self.mlp(torch.cat([state[:, 0, :self.self_state_dim], h_n.squeeze(0)], dim=1))


class LstmRL(MultiHumanRL):
    display_name = "LSTM-RL"
    config_section = "lstm_rl"
    family = value_net.RECURRENT         # the one kernel: float32 on the look-ahead tensor

    def __init__(self):
        super().__init__()
        self.with_interaction_module = None
        self.interaction_module_dims = None

    def set_recurrent_precision(self, precision):
        """The arithmetic of the recurrent decision kernel, for ``predict`` and ``act_device`` alike: "f32" (the default) or the opt-in
        "bf16" (W_hh, network 2's W_ih and the layers behind each chain's first on bf16 matrix instructions, h rounded once a
        step, c and the accumulation float32).  ``decision_precision`` and ``decision_input`` stay ("f32", "tensor"); combines freely with
        ``set_recurrent_input`` (cadrl.py: the setter lies beside the attribute, and refuses every policy but this one)."""
        self.recurrent_precision = value_net.check_recurrent_precision(precision, self.family)

    def configure(self, config):
        self.set_common_parameters(config)
        section = self.config_section
        self.with_om = config.getboolean(section, "with_om")
        if self.with_om:
            raise NotImplementedError("OM-LSTM-RL (lstm_rl.with_om = true) is a policy of its own here: the rows widened by the humans' occupancy "
                                      "maps have their own recurrent decision kernel; build it with policy_factory[\"om_lstm_rl\"]")
        mlp_dims = width_list(config.get(section, "mlp2_dims"))
        hidden = config.getint(section, "global_state_dim")
        self.with_interaction_module = config.getboolean(section, "with_interaction_module")
        if self.with_interaction_module:
            self.interaction_module_dims = width_list(config.get(section, "mlp1_dims"))
            self.model = ValueNetwork2(self.input_dim(), self.self_state_dim, self.interaction_module_dims, mlp_dims, hidden)
        else:
            self.model = ValueNetwork1(self.input_dim(), self.self_state_dim, mlp_dims, hidden)
        self.multiagent_training = config.getboolean(section, "multiagent_training")
        logging.debug("%s: %s pairwise interaction module, hidden width %d", self.name, "with" if self.with_interaction_module else "without", hidden)
