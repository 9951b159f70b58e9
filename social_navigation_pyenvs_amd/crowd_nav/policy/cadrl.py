"""CADRL (reference: crowd_nav/policy/cadrl.py) and the device versions of the array helpers CADRL / SARL call once per robot decision
(cadrl.py:13-105).  ``CADRL`` keeps the reference's attributes, configuration keys and ``state_dict`` layout; its ``predict`` is the
W = 1 launch of the fused decision kernel (cs_lookahead + cs_value_net_decide) the batched Gym runs for W worlds
(``BatchedSocialNavGym.act_device``), so one robot alone and a batch give the same bits.  There is no host path for the decision."""
from __future__ import annotations

import itertools
import logging

import numpy as np
import torch
import torch.nn as nn

from ... import _lib
from ..._lib import DeviceBuffer, check
from ..policy_no_train.policy import Policy
from ..utils.action import ActionXY
from . import value_net


def build_action_space_array(v_pref: float, speed_samples: int = 5, rotation_samples: int = 16) -> np.ndarray:
    """The holonomic action set of CADRL.build_action_space (cadrl.py:181-206): (0, 0) + rotations x speeds."""
    speeds = [(np.exp((i + 1) / speed_samples) - 1) / (np.e - 1) * v_pref for i in range(speed_samples)]
    rotations = np.linspace(0, 2 * np.pi, rotation_samples, endpoint=False)
    acts = [[0.0, 0.0]] + [[s * np.cos(r), s * np.sin(r)] for r, s in itertools.product(rotations, speeds)]
    return np.array(acts, dtype=np.float64)


def compute_rotated_states_and_reward(action_space, next_humans_state, current_humans_state, current_robot_state, dt,
                                      theta_and_omega_visible=False):
    """Same signature and return as the reference function (cadrl.py:42-83): (rotated_states [A, N, 13|15],
    rewards [A]).  A leading world axis on the three state arrays batches W robots:
    next [W,N,4|6], current [W,N,5|7], robot [W,8+] -> ([W,A,N,13|15], [W,A])."""
    _lib.require_gpu()
    cur = np.asarray(current_humans_state)
    single = cur.ndim == 2
    f = np.float32
    acts = np.ascontiguousarray(action_space, dtype=f)
    nxt = np.ascontiguousarray(next_humans_state, dtype=f)
    cur32 = np.ascontiguousarray(cur, dtype=f)
    rob = np.ascontiguousarray(current_robot_state, dtype=f)
    if single:
        nxt, cur32, rob = nxt[None], cur32[None], rob[None]
    W, n, A = cur32.shape[0], cur32.shape[1], acts.shape[0]
    oc = 15 if theta_and_omega_visible else 13
    if nxt.shape[-1] != (6 if theta_and_omega_visible else 4) or cur32.shape[-1] != (7 if theta_and_omega_visible else 5):
        raise ValueError("state column counts do not match theta_and_omega_visible")
    d_a, d_n, d_c, d_r = (DeviceBuffer.from_numpy(x) for x in (acts, nxt, cur32, rob))
    d_rot, d_rew = DeviceBuffer((W, A, n, oc)), DeviceBuffer((W, A))
    check(_lib.load().cs_lookahead(W, n, A, int(bool(theta_and_omega_visible)), d_a.ptr, d_n.ptr, d_c.ptr, d_r.ptr, rob.shape[-1], dt, d_rot.ptr,
                                   d_rew.ptr, None))
    dtype = cur.dtype if cur.dtype in (np.float32, np.float64) else np.float64
    rot, rew = d_rot.download().astype(dtype), d_rew.download().astype(dtype)
    return (rot[0], rew[0]) if single else (rot, rew)


def compute_action_value(rewards, value_network_min_outputs, dt, gamma, vpref):
    """cadrl.py:85-90 (host numpy: A scalars)."""
    return np.asarray(rewards) + pow(gamma, dt * vpref) * np.asarray(value_network_min_outputs)


def propagate_humans_state_with_constant_velocity_model(current_humans_state, dt, theta_and_omega_visible=False):
    """cadrl.py:92-105 (host numpy)."""
    c = np.asarray(current_humans_state)
    if theta_and_omega_visible:
        return np.stack([c[:, 0] + c[:, 2] * dt, c[:, 1] + c[:, 3] * dt, c[:, 5] + c[:, 6] * dt, c[:, 2], c[:, 3], c[:, 6]], 1)
    return np.stack([c[:, 0] + c[:, 2] * dt, c[:, 1] + c[:, 3] * dt, c[:, 2], c[:, 3]], 1)


# ---------------------------------------------------------------------------------------------------------------------
# The policy.  What is fixed from outside: the names a CrowdNav trainer / explorer / robot reads and calls (attributes, methods,
# configuration sections and keys), the state_dict keys of a checkpoint (`value_network.<2 i>.weight|bias`), and the order of the two
# numpy random draws of an exploring decision.  Everything else is this project's.

ROBOT_FIELDS = ("px", "py", "vx", "vy", "radius", "gx", "gy", "v_pref", "theta")
HUMAN_FIELDS = ("px", "py", "vx", "vy", "radius")
HEADED_FIELDS = HUMAN_FIELDS + ("theta", "omega")

# public attributes a freshly built policy carries (name -> initial value); CrowdNav code tests several of them against None
_INITIAL_ATTRIBUTES = {
    "trainable": True, "parallelize": False, "with_theta_and_omega_visible": False,
    "self_state_dim": 6, "human_state_dim": 7, "joint_state_dim": 13,
    **dict.fromkeys(("multiagent_training", "kinematics", "epsilon", "gamma", "sampling", "speed_samples", "rotation_samples", "query_env",
                     "action_space", "action_space_ndarray", "speeds", "rotations", "action_values", "with_om", "cell_num", "cell_size",
                     "om_channel_size"), None),
}

# policy.config entries every value-based policy reads: attribute <- (section, key, parser method of the config object)
_COMMON_SCHEMA = {
    "gamma": ("rl", "gamma", "getfloat"),
    "kinematics": ("action_space", "kinematics", "get"),
    "sampling": ("action_space", "sampling", "get"),
    "speed_samples": ("action_space", "speed_samples", "getint"),
    "rotation_samples": ("action_space", "rotation_samples", "getint"),
    "query_env": ("action_space", "query_env", "getboolean"),
    "cell_num": ("om", "cell_num", "getint"),
    "cell_size": ("om", "cell_size", "getfloat"),
    "om_channel_size": ("om", "om_channel_size", "getint"),
}


def read_config(policy, config, schema):
    """Set the attributes named in `schema` on `policy` from a ConfigParser-like object."""
    for attribute, (section, key, parser) in schema.items():
        setattr(policy, attribute, getattr(config, parser)(section, key))


def width_list(text):
    """'150, 100, 100, 1' -> [150, 100, 100, 1]"""
    return [int(tok) for tok in str(text).replace(",", " ").split()]


def mlp(input_dim, mlp_dims, last_relu=False):
    """A Linear stack with a ReLU between consecutive layers (and behind the last one when last_relu).  The Linear layers sit at the even
    indices of the Sequential: that is where a reference checkpoint's keys (`<name>.0.weight`, `<name>.2.weight`, ...) expect them."""
    widths = [int(input_dim)] + [int(w) for w in mlp_dims]
    net = nn.Sequential()
    for k, (fan_in, fan_out) in enumerate(zip(widths, widths[1:])):
        net.append(nn.Linear(fan_in, fan_out))
        if last_relu or k + 2 < len(widths):
            net.append(nn.ReLU())
    return net


class ValueNetwork(nn.Module):
    """The CADRL value network (Chen et al. 2017): one MLP on the 13- (15-) column agent-centric joint state of the robot and ONE human.
    The submodule's name is the prefix of the checkpoint keys."""

    def __init__(self, input_dim, mlp_dims):
        super().__init__()
        self.value_network = mlp(input_dim, mlp_dims)

    def forward(self, state):
        return self.value_network(state)


def joint_rows(state, headed):
    """JointState -> float32 array [humans, 14 | 16]: the robot's full state followed by one human's observable state per row."""
    robot = [float(getattr(state.self_state, f)) for f in ROBOT_FIELDS]
    fields = HEADED_FIELDS if headed else HUMAN_FIELDS
    return np.array([robot + [float(getattr(h, f)) for f in fields] for h in state.human_states], np.float32).reshape(len(state.human_states), -1)


class CADRL(Policy):
    display_name = "CADRL"
    config_section = "cadrl"
    family = value_net.FEED_FORWARD      # the row of value_net.Family the policy's network belongs to

    def __init__(self):
        super().__init__()
        self.name = self.display_name
        for attribute, value in _INITIAL_ATTRIBUTES.items():
            setattr(self, attribute, value)
        self._net = None
        self._state_nets = []
        self._acts_device = None
        self.decision_precision = "f32"
        self.decision_input = "tensor"
        self.recurrent_precision = "f32"         # (LSTM-RL's own choice, lstm_rl.py set_recurrent_precision; "f32" for every other policy)
        self.recurrent_input = "tensor"          # (LSTM-RL's own choice, set_recurrent_input below; "tensor" for every other policy)
        self.mapped_precision = "f32"            # (OM-LSTM-RL's own choice, om_lstm_rl.py set_mapped_precision; "f32" for every other policy)
        self.wide_precision = "f32"              # (OM-SARL's own choice, om_sarl.py set_wide_precision; "f32" for every other policy)

    # ------------------------------------------------------------------ configuration
    def configure(self, config):
        self.set_common_parameters(config)
        self.model = ValueNetwork(self.joint_state_dim, width_list(config.get(self.config_section, "mlp_dims")))
        self.multiagent_training = config.getboolean(self.config_section, "multiagent_training")
        logging.debug("%s: value network %s", self.name, [m.out_features for m in self.model.value_network if isinstance(m, nn.Linear)])

    def set_common_parameters(self, config):
        read_config(self, config, _COMMON_SCHEMA)
        if self.kinematics != "holonomic":
            raise ValueError(f"{self.name}: kinematics {self.kinematics!r} is not supported: the decision kernel acts in ActionXY (holonomic)")
        # (the reference keeps this switch in the [sarl] section for every policy)
        self.with_theta_and_omega_visible = config.getboolean("sarl", "with_theta_and_omega_visible", fallback=False)
        extra = 2 if self.with_theta_and_omega_visible else 0
        self.human_state_dim, self.joint_state_dim = 7 + extra, 13 + extra

    def set_device(self, device):
        self.device = device
        self.model = self.model.to(device)

    def set_epsilon(self, epsilon):
        self.epsilon = epsilon

    def set_decision_precision(self, precision):
        """The arithmetic of the decision kernel, for ``predict`` and ``act_device`` alike: "f32" (the default) or the opt-in "bf16"
        (bf16 matrix instructions behind the first layer, float32 accumulation and reductions)."""
        value_net.check_mode(self.family, self.decision_input, value_net.check_precision(precision))
        self.decision_precision = precision

    def set_decision_input(self, decision_input):
        """Where the decision kernel's rows come from, for ``predict`` and ``act_device`` alike: "tensor" (the default: cs_lookahead writes
        rotated [W][A][n][13|15] to HBM, cs_value_net_decide reads it back) or the opt-in "fused" (cs_value_net_decide_worlds generates
        the rows in LDS from the worlds' own rows, bit for bit the same decision).  "fused" is float32 only."""
        self.decision_input = value_net.check_mode(self.family, decision_input, self.decision_precision)

    def set_recurrent_input(self, recurrent_input):
        """Where the recurrent decision kernel's rows come from, for ``predict`` and ``act_device`` alike: "tensor" (the default: cs_lookahead
        writes rotated [W][A][n][13|15], the kernel gathers it back one sorted row at a time) or the opt-in "fused"
        (cs_value_net_decide_lstm_worlds[_bf16] generates every step's rows in LDS from the worlds' own rows, bit for bit the same decision
        in either ``recurrent_precision``).  "fused" is LSTM-RL's alone: every other policy is refused with the reason (CADRL
        and SARL have ``set_decision_input``), before anything touches the device."""
        self.recurrent_input = value_net.check_recurrent_input(recurrent_input, self.family)

    def build_action_space(self, v_pref):
        """(0, 0) plus rotation_samples headings x speed_samples exponentially spaced speeds up to v_pref."""
        self.action_space_ndarray = build_action_space_array(v_pref, self.speed_samples, self.rotation_samples)
        grid = self.action_space_ndarray[1:].reshape(self.rotation_samples, self.speed_samples, 2)
        self.speeds = [float(np.hypot(*grid[0, k])) for k in range(self.speed_samples)]
        self.rotations = np.arange(self.rotation_samples) * (2 * np.pi / self.rotation_samples)
        self.action_space = [ActionXY(float(vx), float(vy)) for vx, vy in self.action_space_ndarray]

    # ------------------------------------------------------------------ the decision
    def map_columns(self):
        """Occupancy-map columns behind the rotated ones in a network input row: none but for OM-SARL."""
        return 0

    def _new_device_net(self, model):
        return value_net.DeviceNet(model, self.joint_state_dim)

    def device_net(self):
        """The network as the kernel reads it (value_net.DeviceNet), the blob of ``decision_precision`` repacked only after a parameter changed."""
        if self._net is None or self._net.model is not self.model:
            self._net = self._new_device_net(self.model)
        self._net.refresh_selected(self.decision_precision, self.recurrent_precision, self.mapped_precision, self.wide_precision)
        return self._net

    _STATE_NETS_KEPT = 4

    def state_net(self, model=None):
        """The float32 DeviceNet that evaluates states (cs_value_net_state) with ``model``'s weights -- None: the policy's own module, the
        DeviceNet of ``device_net()``.  Another module (a trainer's deep-copied target network) must have the policy's architecture; its
        DeviceNet is kept per module, apart from the policy's own, and repacked only after a parameter changed."""
        if self._net is None or self._net.model is not self.model:
            self._net = self._new_device_net(self.model)
        net = own = self._net
        if model is not None and model is not self.model:
            net = next((kept for kept in self._state_nets if kept.model is model), None)
            if net is None:
                net = self._new_device_net(model)
                if net.kind != own.kind or not np.array_equal(net.dims, own.dims):
                    raise ValueError(f"{self.name}: the module to evaluate has another architecture than the policy's "
                                     f"({net.dims.tolist()} against {own.dims.tolist()})")
                self._state_nets = (self._state_nets + [net])[-self._STATE_NETS_KEPT:]
        net.refresh("f32")
        return net

    def _world_of(self, state, what):
        """The W = 1 tensors of a JointState, for `what` ("predict", "state_value"): (the current humans [n, 5 | 7] on the host, the same [1, n, 5 | 7]
        and the robot's row [1, 9] on the device); ValueError when the state has fewer humans than the policy's family needs."""
        least = self.family.min_humans
        if len(state.human_states) < least:
            raise ValueError(f"{self.name}.{what} needs at least " + ("one human" if least == 1 else
                                                                     "two humans: a lone human has no other human to map"))
        _lib.require_gpu()
        rows = joint_rows(state, bool(self.with_theta_and_omega_visible))
        up = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device="cuda")
        cur = rows[:, len(ROBOT_FIELDS):]
        return cur, up(cur)[None], up(rows[:1, :len(ROBOT_FIELDS)])

    def state_value(self, state, model=None):
        """V(state): the value network (``model``: another module of the same architecture, e.g. a target network) on the rotated joint
        state of ``state`` as it stands -- no look-ahead, no reward, the humans in their own order; CADRL: the minimum over the humans;
        OM-SARL: on the wide rows of ``transform``.  The W = 1 launches behind ``BatchedSocialNavGym.value_device``
        (value_net.state_values_for_worlds), float32; returns a Python float."""
        if self.model is None:
            raise AttributeError(f"{self.name}: configure() the policy before it evaluates a state")
        _, d_c, d_r = self._world_of(state, "state_value")
        values, _ = value_net.state_values_for_worlds(self.state_net(model), d_c, d_r, None, self.gamma, 0.0, False, torch.cuda.current_stream().cuda_stream)
        return float(values.item())

    def device_action_space(self):
        """The action table as a CUDA tensor [A, 2], uploaded again only when action_space_ndarray holds other values."""
        table = np.asarray(self.action_space_ndarray, np.float32)
        cached = self._acts_device
        if cached is None or cached[0].shape != table.shape or not np.array_equal(cached[0], table):
            cached = self._acts_device = (table.copy(), torch.as_tensor(table, device="cuda").contiguous())
        return cached[1]

    def _next_humans(self, current):
        headed = self.with_theta_and_omega_visible
        if not self.query_env:
            return propagate_humans_state_with_constant_velocity_model(current, self.time_step, headed)
        manager = self.env.motion_model_manager          # the crowd's own model, one robot step ahead (cs_peek)
        if headed:
            return np.asarray(manager.get_next_human_observable_states(self.time_step, theta_and_omega_visible=True))[:, :6]
        return np.asarray(manager.get_next_human_observable_states(self.time_step))

    def _decide_one(self, state, override=-1):
        """value_net.decide_for_worlds for this one robot (W = 1) on the current stream: (action values [A], chosen index, ActionXY row
        float32)."""
        cur, d_c, d_r = self._world_of(state, "predict")
        A = len(self.action_space_ndarray)
        net = self.device_net()
        up = lambda a, dtype=torch.float32: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")
        d_a, d_n = self.device_action_space(), up(np.asarray(self._next_humans(cur.astype(np.float64)), np.float32))[None]
        vals = torch.empty((1, A), dtype=torch.float32, device="cuda")
        pick = torch.empty(1, dtype=torch.int32, device="cuda")
        act = torch.empty((1, 2), dtype=torch.float32, device="cuda")
        stream = lambda: torch.cuda.current_stream().cuda_stream
        rot, _ = value_net.decide_for_worlds(net, self.decision_input, self.decision_precision, d_a, d_n, d_c, d_r, self.gamma, self.time_step,
                                             up(np.array([override]), torch.int32), vals, pick, act, stream(),
                                             recurrent_precision=self.recurrent_precision, mapped_precision=self.mapped_precision,
                                             wide_precision=self.wide_precision, recurrent_input=self.recurrent_input)
        # (SARL's attention weights read the last action's rows; without the look-ahead tensor they are made when asked for)
        self._last_rotated = rot if rot is not None else (lambda: value_net.lookahead(d_a[-1:].contiguous(), d_n, d_c, d_r, self.time_step, stream()))
        return vals[0].cpu().numpy(), int(pick.item()), act[0].cpu().numpy()

    def _require_ready(self):
        missing = [what for what in ("phase", "device") if getattr(self, what) is None]
        if missing:
            raise AttributeError(f"{self.name}.predict: call set_{missing[0]}() first ({', '.join(missing)} not set)")
        if self.phase == "train" and self.epsilon is None:
            raise AttributeError(f"{self.name}.predict: the training phase needs set_epsilon()")

    def predict(self, state):
        """The action with the best one-step look-ahead value.  A robot within its radius of the goal stands still.  One uniform draw is
        taken for every decision; in the training phase a draw below epsilon replaces the decision by a uniformly chosen action (a second
        draw, np.random.choice) -- the order a seeded reference run consumes the numpy stream in.  Otherwise the W = 1 kernel decides."""
        self._require_ready()
        if self.reach_destination(state):
            return ActionXY(0, 0)
        if self.action_space is None:
            self.build_action_space(state.self_state.v_pref)
        draw = np.random.random()
        if self.phase == "train" and draw < self.epsilon:
            chosen = self.action_space[int(np.random.choice(len(self.action_space)))]
        else:
            values, index, _ = self._decide_one(state)
            self.action_values = values.astype(float).tolist()
            chosen = ActionXY(*self.action_space_ndarray[index])
        if self.phase == "train":
            self.last_state = self.transform(state)
        return chosen

    def transform(self, state):
        """What a trainer stores for this decision: the network's input row of the robot and its ONE human, tensor [13 | 15]."""
        if len(state.human_states) != 1:
            raise AssertionError(f"{self.name} is a one-human network: got {len(state.human_states)} humans")
        rows = torch.from_numpy(joint_rows(state, self.with_theta_and_omega_visible)).to(self.device)
        return self.rotate(rows, theta_and_omega_visible=self.with_theta_and_omega_visible)[0]

    def rotate(self, state, theta_and_omega_visible=False):
        """World frame -> the agent-centric frame whose x axis points from the robot to its goal.
        state [batch, 14 | 16]: ROBOT_FIELDS then HUMAN_FIELDS | HEADED_FIELDS; result [batch, 13 | 15]:
        dg, v_pref, theta (0: holonomic), radius, vx, vy, px1, py1, vx1, vy1, radius1, da, radius + radius1 [, theta1, omega1]."""
        s = state
        col = lambda i: s[:, i:i + 1]
        dx, dy = col(5) - col(0), col(6) - col(1)
        rot = torch.atan2(dy, dx)
        c, sn = torch.cos(rot), torch.sin(rot)
        turn = lambda x, y: (x * c + y * sn, y * c - x * sn)
        vx, vy = turn(col(2), col(3))
        px1, py1 = turn(col(9) - col(0), col(10) - col(1))
        vx1, vy1 = turn(col(11), col(12))
        theta = torch.zeros_like(col(7))
        out = [torch.hypot(dx, dy), col(7), theta, col(4), vx, vy, px1, py1, vx1, vy1, col(13), torch.hypot(col(0) - col(9), col(1) - col(10)),
               col(4) + col(13)]
        if theta_and_omega_visible:
            out += [col(14) - theta, col(15)]
        return torch.cat(out, dim=1)
