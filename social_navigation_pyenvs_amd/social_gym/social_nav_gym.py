"""SocialNavGym -- the drop-in Gym boundary (reference: social_gym/social_nav_gym.py:14-277).

``configure(config)``, ``set_robot(robot)``, ``set_safety_space(s)``, ``reset(phase, test_case)``,
``step(action)``, ``render()`` and the attributes CrowdNav reads (``global_time, time_limit, time_step,
robot_time_step, case_size, case_counter, humans, robot, motion_model, states, updated,
motion_model_manager``) keep the reference's names, argument meaning, return shapes and error
behaviour (``AttributeError`` without a robot, ``ValueError`` for a robot time step that is not a
multiple of the time step, ``NotImplementedError`` for an unknown human policy).

What differs underneath: the ``time_step_factor`` substeps of ``step()`` (robot move + ``update_humans``
+ respawn, :240-245) are ONE fused kernel launch on the MI355X; PyGame is gone (``render`` is a no-op as
with the reference's ``HEADLESS = True``); gymnasium is optional (the class subclasses ``gym.Env`` when
the package is importable).  ``BatchedSocialNavGym`` below runs W such worlds in lock-step.
"""
from __future__ import annotations

import logging

import numpy as np

from .. import _lib
from ..batched import CrowdWorlds, HUMAN_MODELS as _MODELS
from .device_loop import DeviceLoop, SideStream, StepPieces, clock_table, stage_depth
from .social_nav_sim import SocialNavSim
from .src.info import INFO_BY_CODE, Collision, Danger, Nothing, ReachGoal, Timeout  # noqa: F401
from .src.utils import is_multiple

try:  # optional: register / subclass when gymnasium exists (it is not part of this image)
    import gymnasium as gym

    _EnvBase = gym.Env
except Exception:  # pragma: no cover
    gym = None

    class _EnvBase:  # minimal stand-in so isinstance checks on the API shape still work
        pass

HEADLESS = True
PARALLELIZE_ROBOT = True
PARALLELIZE_HUMANS = True
HUMAN_MODELS = list(_MODELS)


class SocialNavGym(_EnvBase, SocialNavSim):
    def __init__(self):
        # the reference builds a throw-away 10-human world here (:25); an empty shell is enough
        self.config_data = {"humans": {}, "walls": [], "headless": True}
        self.humans = []
        self.walls = []
        self.mode = "circular_crossing"
        self.parallelize_robot = PARALLELIZE_ROBOT
        self.parallelize_humans = PARALLELIZE_HUMANS
        self.sampling_time = 1 / 60
        self.robot_sampling_time = 1 / 4
        self.real_size = 15
        self.display_to_real_ratio = 1.0
        self.updated = True
        self.sim_t = 0.0
        self.time_limit = None
        self.time_step = None
        self.robot = None
        self.global_time = None
        self.human_times = None
        self.success_reward = None
        self.collision_penalty = None
        self.discomfort_dist = None
        self.discomfort_penalty_factor = None
        self.config = None
        self.case_capacity = None
        self.case_size = None
        self.case_counter = None
        self.randomize_attributes = None
        self.train_val_sim = None
        self.test_sim = None
        self.square_width = None
        self.circle_radius = None
        self.human_num = None
        self.safety_space = 0
        self.states = None
        self.action_values = None
        self.attention_weights = None
        self.action_space = gym.spaces.Discrete(1) if gym is not None else None
        self.observation_space = gym.spaces.Discrete(1) if gym is not None else None

    # ------------------------------------------------------------------ configuration (:59-98)
    def configure(self, config):
        self.config = config
        self.time_limit = config.getint("env", "time_limit")
        self.time_step = config.getfloat("env", "time_step")
        self.robot_time_step = config.getfloat("env", "robot_time_step")
        if not is_multiple(self.robot_time_step, self.time_step):
            raise ValueError("Robot time step must be a multiple of time step")
        self.time_step_factor = int(self.robot_time_step / self.time_step)
        self.randomize_attributes = config.getboolean("env", "randomize_attributes")
        self.success_reward = config.getfloat("reward", "success_reward")
        self.collision_penalty = config.getfloat("reward", "collision_penalty")
        self.discomfort_dist = config.getfloat("reward", "discomfort_dist")
        self.discomfort_penalty_factor = config.getfloat("reward", "discomfort_penalty_factor")
        self.human_policy = config.get("humans", "policy")
        self.robot_radius = config.getfloat("robot", "radius")
        if self.human_policy not in HUMAN_MODELS:
            raise NotImplementedError
        u32 = np.iinfo(np.uint32).max
        self.case_capacity = {"train": u32 - 2000, "val": 1000, "test": 1000}
        self.case_size = {"train": u32 - 2000, "val": config.getint("env", "val_size"), "test": config.getint("env", "test_size")}
        self.train_val_sim = config.get("sim", "train_val_sim")
        self.test_sim = config.get("sim", "test_sim")
        self.traffic_height = config.getfloat("sim", "traffic_height")
        self.traffic_length = config.getfloat("sim", "traffic_length")
        self.circle_radius = config.getfloat("sim", "circle_radius")
        self.human_num = config.getint("sim", "human_num")
        self.case_counter = {"train": 0, "test": 0, "val": 0}
        logging.info("human number: {}".format(self.human_num))
        logging.info("Human policy: {}".format(self.human_policy))

    def set_safety_space(self, safety_space: float):
        self.safety_space = safety_space

    def set_robot(self, robot):
        self.robot = robot
        if PARALLELIZE_ROBOT:
            self.robot.parallelize = True

    def compute_humans_observable_state(self):
        if self.robot.sensor == "coordinates":
            headed = self.robot.policy.with_theta_and_omega_visible
            return [h.get_observable_state(visible_theta_and_omega=True) if headed else h.get_observable_state() for h in self.humans]
        raise NotImplementedError

    def check_actual_collisions_and_goal(self):
        dmin, collision = 10000.0, False
        for h in self.humans:
            d = np.linalg.norm(h.position - self.robot.position) - h.radius - self.robot.radius
            dmin = d if d < dmin else dmin
            if dmin <= 0:
                collision = True
        reaching_goal = np.linalg.norm(self.robot.position - self.robot.get_goal_position()) < self.robot.radius
        return collision, dmin, reaching_goal

    # ------------------------------------------------------------------ reset (:120-225)
    def _generate(self, scenario, human_num):
        kw = dict(insert_robot=True, human_policy=self.human_policy, headless=HEADLESS, runge_kutta=False,
                  robot_visible=self.robot.visible, robot_radius=self.robot_radius, n_actors=human_num,
                  randomize_human_attributes=self.randomize_attributes)
        if scenario == "circle_crossing":
            self.generate_circular_crossing_setting(circle_radius=self.circle_radius, randomize_human_positions=True, **kw)
        elif scenario == "parallel_traffic":
            self.generate_parallel_traffic_scenario(traffic_length=self.traffic_length, traffic_height=self.traffic_height, **kw)
        elif scenario == "circular_crossing_with_static_obstacles":
            self.generate_circular_crossing_with_static_obstacles(circle_radius=self.circle_radius, randomize_human_positions=True, **kw)
        # any other name: the reference falls through its elif chain and keeps the previous config_data

    def reset(self, phase="test", test_case=None):
        if self.robot is None:
            raise AttributeError("robot has to be set!")
        assert phase in ["train", "val", "test"]
        if test_case is not None:
            self.case_counter[phase] = test_case
        if self.robot.parallelize:
            self.robot.policy.parallelize = True
        self.global_time = 0
        multi = self.robot.policy.multiagent_training
        self.human_times = [0] * (self.human_num if (phase == "test" or multi) else 1)
        if self.config.get("humans", "policy") == "trajnet":
            raise NotImplementedError
        counter_offset = {"train": self.case_capacity["val"] + self.case_capacity["test"], "val": 0, "test": self.case_capacity["val"]}
        if self.case_counter[phase] >= 0:
            seed = counter_offset[phase] + self.case_counter[phase]
            np.random.seed(seed)
            if phase in ["train", "val"]:
                human_num = self.human_num if multi else 1
                scenario = self.train_val_sim
            else:
                human_num = self.human_num
                scenario = self.test_sim
            if scenario == "hybrid_scenario":
                scenario = np.random.choice(["circle_crossing", "parallel_traffic"])
                np.random.seed(seed)  # the choice draw is discarded: the generator restarts the stream (:156-157)
            self._generate(str(scenario), human_num)
            self.case_counter[phase] = (self.case_counter[phase] + 1) % self.case_size[phase]
        else:
            assert phase == "test"
            if self.case_counter[phase] == -1:  # the reference's debugging case (:199-209)
                self.human_num = 3
                humans = {0: {"pos": [0, -6], "yaw": np.pi / 2, "goals": [[0, 5], [0, -6]]},
                          1: {"pos": [-5, -5], "yaw": np.pi / 2, "goals": [[-5, 5], [-5, -5]]},
                          2: {"pos": [5, -5], "yaw": np.pi / 2, "goals": [[5, 5], [5, -5]]}}
                robot = {"pos": [7.5, 7.5], "yaw": 0.0, "radius": 0.25, "goals": [[7.5, 7.5]]}
                self.config_data = {"headless": False, "motion_model": "sfm_helbing", "runge_kutta": False, "insert_robot": True,
                                    "grid": True, "humans": humans, "walls": [], "robot": robot}
            else:
                raise NotImplementedError
        self.robot.set_radius_and_update_graphics(self.robot_radius)
        r = self.config_data["robot"]
        self.robot.set(r["pos"][0], r["pos"][1], r["goals"][0][0], r["goals"][0][1], 0, 0, r["yaw"], w=0)
        self.reset_sim(reset_robot=False)
        if self.safety_space > 0:
            self.motion_model_manager.set_safety_space(self.safety_space)
        self.set_time_step(self.time_step)
        self.set_robot_time_step(self.robot_time_step)
        self.states = list()
        if hasattr(self.robot.policy, "action_values"):
            self.action_values = list()
        if hasattr(self.robot.policy, "get_attention_weights"):
            self.attention_weights = list()
        return self.compute_humans_observable_state(), {0: Nothing()}

    # ------------------------------------------------------------------ step (:227-250)
    def step(self, action):
        collision, dmin, reaching_goal = self.collision_detection_and_reaching_goal(action, self.robot_time_step)
        reward, terminated, truncated, info = self.compute_reward_and_infos(collision, dmin, reaching_goal, self.global_time,
                                                                            self.robot_time_step)
        self.states.append([self.robot.get_full_state(), [h.get_full_state() for h in self.humans]])
        if hasattr(self.robot.policy, "action_values"):
            self.action_values.append(self.robot.policy.action_values)
        if hasattr(self.robot.policy, "get_attention_weights"):
            self.attention_weights.append(self.robot.policy.get_attention_weights())
        # time_step_factor x { robot.step(action, dt) ; update_humans(t, dt) } -> one fused launch
        self.robot.check_validity(action)
        unicycle = self.robot.kinematics != "holonomic"
        act = (action.v, action.r) if unicycle else (action.vx, action.vy)
        self.motion_model_manager.update_humans_block(self.time_step, self.time_step_factor, act, unicycle=unicycle)
        for _ in range(self.time_step_factor):
            self.global_time += self.time_step
        self.updated = True
        return self.compute_humans_observable_state(), reward, terminated, truncated, {0: info}

    def imitation_learning_step(self):
        """One environment step with the robot following a human motion model (:252-274): reward and info come from the
        ACTUAL state at the end of the update."""
        self.states.append([self.robot.get_full_state(), [h.get_full_state() for h in self.humans]])
        # time_step_factor x { update_robot(t, dt) ; update_humans(t, dt) } on the device, one read-back
        self.motion_model_manager.imitation_block(self.time_step, self.time_step_factor)
        for _ in range(self.time_step_factor):
            self.global_time += self.time_step
        ob = self.compute_humans_observable_state()
        collision, dmin, reaching_goal = self.check_actual_collisions_and_goal()
        reward, terminated, truncated, info = self.compute_reward_and_infos(collision, dmin, reaching_goal, self.global_time,
                                                                            self.robot_time_step)
        self.updated = True
        return ob, reward, terminated, truncated, {0: info}

    def render(self):
        return None


class BatchedSocialNavGym:
    """W independent SocialNavGym worlds advanced in lock-step on one GPU.

    Same episode logic as ``SocialNavGym.step`` -- reward / termination from the swept collision test on the
    CURRENT state (cs_collision_reward), then ``time_step_factor`` fused substeps (cs_step) -- with arrays
    instead of object lists: observations ``[W, N, 5]`` (px, py, vx, vy, radius) or ``[W, N, 7]`` (+ theta,
    omega), rewards ``[W]``, terminated / truncated ``[W]`` bool, ``info_code [W]`` (index into
    ``social_gym.src.info.INFO_BY_CODE``).  Worlds are generated by the exact reference generators from
    seeds ``offset[phase] + case`` (one per world) through a scratch ``SocialNavGym``; every world needs the
    same human count and goal-slot count (a hybrid batch pads traffic goals with NaN).

    This class is float32 whatever the world precision of the W = 1 facade (``SocialNavSim.set_world_precision``): its Gym head, device
    generators and auto-reset are float32 kernels.  A batch of float64 worlds is ``batched.CrowdWorlds64`` with float64 initial states
    from the host generators.
    """

    def __init__(self, config, n_worlds: int, robot_visible=False, robot_radius=None, headed_obs=False):
        self.W = int(n_worlds)
        self.headed_obs = bool(headed_obs)
        self._proto = SocialNavGym()
        self._proto.configure(config)
        self.config = config
        self.time_step = self._proto.time_step
        self.robot_time_step = self._proto.robot_time_step
        self.time_step_factor = self._proto.time_step_factor
        self.time_limit = self._proto.time_limit
        self.robot_visible = bool(robot_visible)
        self.reward_cfg = (float(self.time_limit), self._proto.success_reward, self._proto.collision_penalty,
                           self._proto.discomfort_dist, self._proto.discomfort_penalty_factor)
        self.global_time = None
        self.cw = None

    def reset(self, phase="test", first_case=0, safety_space=0.0, device=False):
        """Generate W worlds from the seeds ``offset[phase] + (first_case + w) % case_size``.  ``device=False`` runs the
        host generators world by world (W serial rejection-sampling loops); ``device=True`` runs them in one launch of
        ``cs_generate_worlds`` (one GPU lane per world, same legacy random stream, same rows)."""
        if device:
            return self._reset_on_device(phase, first_case, safety_space)
        from .src.agent import RobotAgent
        from types import SimpleNamespace

        proto = self._proto
        rows_s, rows_g, rows_p, rows_r, respawn = [], [], [], [], []
        model = proto.human_policy
        for w in range(self.W):
            robot = RobotAgent(proto)
            robot.visible, robot.sensor, robot.kinematics = self.robot_visible, "coordinates", "holonomic"
            robot.policy = SimpleNamespace(multiagent_training=True, with_theta_and_omega_visible=self.headed_obs, kinematics="holonomic")
            proto.parallel_traffic_humans_respawn = False  # one fresh env per world: no sticky respawn flag
            proto.set_robot(robot)
            proto.reset(phase=phase, test_case=first_case + w)
            mm = proto.motion_model_manager
            rows_s.append(mm.states.copy())
            rows_g.append(mm.goals.copy())
            rows_p.append(None if mm.params is None else mm.params.copy())
            rows_r.append(robot.get_safe_state())
            respawn.append(1 if mm.parallel_traffic_humans_respawn else 0)
            bounds = mm.respawn_bounds if mm.parallel_traffic_humans_respawn else None
            if bounds is not None:
                self._bounds = bounds
        gmax = max(g.shape[1] for g in rows_g)
        n = rows_g[0].shape[0]
        goals = np.full((self.W, n, gmax, 2), np.nan)
        for w, g in enumerate(rows_g):
            goals[w, :, :g.shape[1]] = g
        S = np.stack(rows_s)
        P = None if rows_p[0] is None else np.stack(rows_p)
        self.n = n
        self.radius = S[:, :n, 8].astype(np.float32)
        margin = np.zeros((self.W, S.shape[1]))
        if model == "orca":
            margin += 0.01 + safety_space
        elif safety_space > 0:
            margin[:, :n] = 0.01 + safety_space
        any_respawn = any(respawn)
        self.cw = CrowdWorlds(S, goals, P, margin, None, type=model, all_params_equal=True, robot_row=self.robot_visible,
                              robot=np.stack(rows_r), respawn_bounds=self._bounds if any_respawn else None,
                              respawn_worlds=np.array(respawn, np.int32) if any_respawn else None)
        self.global_time = np.zeros(self.W, np.float32)
        return self.observe()

    def _reset_on_device(self, phase, first_case, safety_space):
        from .. import generators as gen
        from .. import scenarios as sc
        from .src.agent import RobotAgent

        proto = self._proto
        assert phase in ["train", "val", "test"]
        scenario = proto.train_val_sim if phase in ("train", "val") else proto.test_sim
        if scenario not in gen.SCENARIOS:
            raise NotImplementedError(f"no device generator for scenario {scenario!r}")
        model = proto.human_policy
        n = proto.human_num
        robot = RobotAgent(proto)
        robot.set_radius_and_update_graphics(proto.robot_radius)
        traffic = scenario in ("parallel_traffic", "hybrid_scenario")
        G = 1 if scenario == "parallel_traffic" else 2
        rows = n + int(self.robot_visible)
        margin = np.zeros((self.W, rows))
        if model == "orca":
            margin += 0.01 + safety_space
        elif safety_space > 0:
            margin[:, :n] = 0.01 + safety_space
        P = None if model == "orca" else np.tile(sc.default_params(model), (n, 1))
        self._bounds = (proto.traffic_length / 2, proto.traffic_height / 2)
        self.cw = CrowdWorlds(np.zeros((self.W, rows, 13), np.float32), np.full((self.W, n, G, 2), np.nan, np.float32), P, margin,
                              None, type=model, all_params_equal=True, robot_row=self.robot_visible,
                              robot=np.zeros((self.W, 13), np.float32), respawn_bounds=self._bounds if traffic else None,
                              respawn_worlds=np.zeros(self.W, np.int32) if traffic else None)
        seeds = gen.phase_seeds(phase, first_case, self.W, proto.case_capacity)
        self._gen_kw = dict(insert_robot=True, randomize_attributes=proto.randomize_attributes, randomize_positions=True,
                            circle_radius=proto.circle_radius, traffic_length=proto.traffic_length,
                            traffic_height=proto.traffic_height, robot_radius=proto.robot_radius, human_mass=75,
                            robot_mass=robot.mass, robot_desired_speed=robot.desired_speed)
        self._gen_scenario, self._seeds_host = scenario, seeds
        status, scn = gen.generate_worlds(self.cw, scenario, seeds, **self._gen_kw)
        # (the respawn rule stays armed for a hybrid batch even when it drew no traffic world: d_world_flags gates it per
        #  world, and step_device's auto-reset may regenerate any world as a traffic world later)
        if model == "orca":  # RVO2 preferred velocity lives in columns 5:7 (set_state_orca, motion_model_manager.py:105-123)
            S = self.cw.get_states()
            d = S[:, :n, 10:12] - S[:, :n, 0:2]
            dn = np.linalg.norm(d, axis=-1, keepdims=True)
            S[:, :n, 5:7] = np.where(dn > S[:, :n, 12:13], d / np.maximum(dn, 1e-30), d)
            self.cw.set_states(S)
        self.n = n
        self.radius = self.cw.get_states()[:, :n, 8].astype(np.float32)
        self.global_time = np.zeros(self.W, np.float32)
        return self.observe()

    # ------------------------------------------------------------------ device-resident loop (torch tensors in HBM)
    # Every world keeps its next STAGE_DEPTH episodes staged ahead (a power of two; capped so that the staging batch stays below
    # STAGE_BYTES), and every REFILL_EVERY steps one pass of cs_refill_staged_worlds regenerates the consumed slots on a side stream.
    # Measured at 4096 x 25 hybrid worlds with a random policy (tools/gym_step_variants.py; 1 % of the worlds end per step, some of them
    # every five steps -- a robot driven into its neighbour again and again), us per batched step with every finished episode regenerated:
    #   depth 16, pass every 4 steps 95.5 | depth 32, every 16: 65.6 | depth 64, every 32 or 64: 56.6 | depth 128, every 128: 56.1
    #   (no resets at all: 45.5; round 3: 144 same-step, 88 NEXT_STEP).  A pass disturbs the step stream for about its own duration
    #   (~0.2 ms: the generator's wavefronts share SIMDs and the instruction cache with the step kernel), so passes are made rare and
    #   the ring deep; 4096 x 25 worlds take 5.4 MB per level.
    REFILL_EVERY = 32
    STAGE_DEPTH = 64
    STAGE_BYTES = 1 << 30
    REFILL_PRIORITY = 0      # stream priority of the refill passes (1 = the device's lowest: no measurable difference)
    FOLD_RESET = True        # the take-over of the staged episodes inside the step's launch (cs_gym_step_staged) where the step kernel allows it
    _dl = None               # the batch's DeviceLoop once a device method has run

    def _device_loop_state(self):
        """The batch's ``DeviceLoop`` (device_loop.py), built with the first call after ``reset(..., device=True)``."""
        from .. import generators as gen

        dl = self._dl
        if dl is not None and dl.cw is self.cw:
            return dl
        if getattr(self, "_gen_scenario", None) is None:
            raise RuntimeError("step_device needs a world batch generated on the device: reset(..., device=True)")
        self._release_device_loop()      # a new batch: the old one's refill pass may still be writing its staging worlds
        try:
            import torch

            torch.zeros(1, device="cuda")
        except RuntimeError as e:  # _lib.load() maps torch's bundled HIP runtime for both, whatever the import order
            raise _lib.CrowdstepError("torch cannot see the GPU in this process (HIP runtime in use: "
                                      f"{_lib.hip_runtime_path or 'system'}; CROWDSTEP_HIP_RUNTIME=system forces two runtimes): {e}") from e
        cw = self.cw
        level = self.W * (cw.rows * 13 + self.n * cw.G * 2 + 13 + 1) * 4
        self._dl = DeviceLoop(cw, n=self.n, headed_obs=self.headed_obs, clock=clock_table(self.time_limit, self.time_step, self.time_step_factor),
                              seeds_host=self._seeds_host, stride=getattr(self, "seed_stride", None) or self.W,
                              depth=stage_depth(level, self.STAGE_DEPTH, self.STAGE_BYTES),
                              gen=gen.make_generator(cw, self._gen_scenario, **self._gen_kw), refill_priority=self.REFILL_PRIORITY)
        return self._dl

    def _release_device_loop(self):
        """Drains and destroys the loop's refill stream (``DeviceLoop.release``) and lets the loop go."""
        dl, self._dl = self._dl, None
        if dl is not None:
            dl.release()

    def close(self):
        """End of the environment's device-resident loop (also run when the object is collected): drains and destroys the refill stream."""
        self._release_device_loop()

    def __del__(self):
        try:
            self._release_device_loop()
        except Exception:
            pass

    def observe_device(self):
        """Observations [W, N, 5|7] as a torch CUDA tensor gathered from the resident state (no host copy)."""
        dl = self._device_loop_state()
        return dl.state[:, :self.n].index_select(2, dl.cols)

    def _step_pieces(self, dl, parity, mode):
        r"""One vectorised Gym step = ONE library launch (cs_gym_step_staged; SFM / HSFM crowds on the one-wavefront kernels) or two on one
        stream, every ctypes argument bound once per (result set, mode):

            cs_gym_step (reward + bookkeeping in the step kernel's prologue, substeps, observation)  ->  cs_consume_staged_worlds

        Which worlds end is known from the reward of the state BEFORE the substeps (social_nav_gym.py:229-233); their next episode
        was generated ahead (its seed is the live one + stride), so the reset is a masked copy.  The regeneration of the consumed
        staging slots (one latency-bound wavefront per world, ~0.15 ms) runs on a side stream with a whole episode to finish
        (DeviceLoop.maybe_refill) -- round 3 had it on the critical path (144 us per step) or beside the next step (NEXT_STEP mode, 88 us).

        mode "same_step": the worlds whose episode ends NOW take over their staged episode before the observation is returned;
        mode "next_step" (Gymnasium's default since 1.0): the bookkeeping of this parity writes mask_p and reads prev = mask_{1-p};
        the tail resets the worlds that ended in the PREVIOUS step; mode "none": no tail.

        Plain launches, not a HIP graph: two consecutive replays of a graph leave the stream idle for 8.5 us (rocprofv3 kernel trace,
        profiles/r4ae_gym_step_timeline.txt: 8.6 us between the consume kernel of one replay and the step kernel of the next, 8.4 us
        between one-kernel graphs) where two plain launches follow each other within 0.3 us -- with two launches per step the graph
        saves the host nothing it needs (28 us of host time per step against 44 us on the GPU)."""
        import ctypes as C

        c = dl.pieces.get((parity, mode))
        if c is not None:
            return c
        cw = self.cw
        A = C.c_void_p(dl.stream.cuda_stream)
        d = cw.descriptor()
        dref = C.byref(d)
        cfg = (C.c_float * 5)(*[float(x) for x in self.reward_cfg])
        P = lambda t: C.c_void_p(t.data_ptr())
        if mode == "next_step":
            masks = dl.ns_masks
            book = dl.gym_book(parity, masks[parity], masks[parity ^ 1], True)
            tail_mask = masks[parity ^ 1]
        else:
            book = dl.gym_book(parity, dl.mask, None, mode == "same_step")
            tail_mask = dl.mask if mode == "same_step" else None
        # cs_gym_step: reward of the state before the substeps + typed results, step counter, float32 clock, reset mask and next seeds
        # (the head: the step kernel's prologue), the substeps, and the observation of the stepped crowd from the kernel's registers
        a_step = (dref, C.c_float(self.time_step), C.c_int(self.time_step_factor), P(dl.act), C.c_float(self.robot_time_step), P(dl.gtime), cfg,
                  P(dl.out), C.byref(book), C.c_int(int(self.headed_obs)), P(dl.obs), A)
        # ... rewritten for the worlds that take over their staged episode (a world whose generation failed keeps its rows and is
        # flagged in reset_failed_mask())
        a_tail = None if tail_mask is None else (C.byref(dl.gen), C.byref(dl.staging_desc), dref, P(tail_mask), C.byref(dl.stage_book),
                                                 C.c_int(int(self.headed_obs)), P(dl.obs), A)
        # ... or both in ONE launch (cs_gym_step_staged: the take-over in the step kernel's epilogue) where the step is the one-wavefront
        # SFM / HSFM kernel; FOLD_RESET = False keeps the two launches (the bit-equality reference of the tests)
        a_fold = None
        if tail_mask is not None and self.FOLD_RESET and _lib.load().cs_gym_step_is_one_launch(dref) == 2:
            a_fold = a_step[:-1] + (C.byref(dl.gen), C.byref(dl.staging_desc), C.byref(dl.stage_book), A)
        keep = (d, cfg, book)              # the structs the byref arguments point into
        c = dl.pieces[parity, mode] = StepPieces(a_step, a_tail, a_fold, keep, (dl.obs,) + dl.results[parity])
        return c

    def _open_step(self, dl, auto_reset):
        """The head of a step: the auto-reset mode (no change while a NEXT_STEP reset is pending), the parity flip, its _step_pieces."""
        import torch

        mode = "next_step" if auto_reset == "next_step" else ("same_step" if auto_reset else "none")
        if mode == "next_step":
            if dl.ns_masks is None:
                dl.ns_masks = [torch.zeros(self.W, dtype=torch.int32, device="cuda") for _ in range(2)]
                torch.cuda.synchronize()
        elif dl.mode == "next_step" and dl.ns_masks is not None and any(bool(m.any().item()) for m in dl.ns_masks):
            raise RuntimeError("a NEXT_STEP auto-reset is pending for some world: keep auto_reset=\"next_step\" (or reset()) before changing the mode")
        dl.mode = mode
        parity = dl.parity
        dl.parity = parity ^ 1
        return self._step_pieces(dl, parity, mode)

    def _issue_step(self, dl, c, pargs=None):
        """One step's library calls: the one-launch fold, or the step + tail; with ``pargs`` the entries that decide the action first."""
        lib, chk = _lib.load(), _lib.check
        if c.fold is not None:
            if pargs is None:
                chk(lib.cs_gym_step_staged(*c.fold))
            else:
                chk(lib.cs_gym_step_staged_policy(*c.fold[:-1], *pargs, c.fold[-1]))
            dl.maybe_refill(self.REFILL_EVERY)
            return
        if pargs is None:
            chk(lib.cs_gym_step(*c.step))
        else:
            chk(lib.cs_gym_step_policy(*c.step[:-1], *pargs, c.step[-1]))
        if c.tail is not None:
            chk(lib.cs_consume_staged_worlds(*c.tail))
            dl.maybe_refill(self.REFILL_EVERY)

    def _no_train_policy(self, dl, policy, who):
        """The no-train policy behind a policy_factory name or an instance, refused where this batch cannot take it (``who`` asks)."""
        from ..crowd_nav.policy_no_train.policy import NoTrainPolicy

        if isinstance(policy, str):
            from ..crowd_nav.policy_no_train.policy_factory import policy_factory

            pol = dl.pnt_named.get(policy) or dl.pnt_named.setdefault(policy, policy_factory[policy]())
        else:
            pol = policy
        if not isinstance(pol, NoTrainPolicy):
            raise TypeError(f"{who} takes a no-train policy (bp, ssp, sfm_helbing, sfm_guo, sfm_moussaid), not {policy!r}")
        if pol.kinematics != "holonomic" or self.cw.unicycle:
            raise ValueError(f"{who}: the no-train policies act in ActionXY and need a holonomic robot")
        if self.cw.d_robot is None:
            raise ValueError(f"{who} needs the robot rows")
        return pol

    def _policy_args(self, dl, pol):
        """The policy's ctypes arguments, bound once per (id, time step, parameters): for the Gym step's policy entries, for cs_policy_no_train."""
        import ctypes as C

        ts = self.robot_time_step if pol.time_step is None else pol.time_step
        prm = pol.packed_params()
        key = (pol.pnt_id, ts, None if prm is None else prm.ctypes.data)
        bound = dl.pnt_args
        b = bound.get(key)
        if b is None:
            P = lambda t: C.c_void_p(t.data_ptr())
            step = (C.c_int(pol.pnt_id), C.c_float(ts), None if prm is None else prm.ctypes.data_as(C.c_void_p))
            act = (step[0], C.c_int(self.W), C.c_int(self.n), C.c_void_p(self.cw.d_robot.ptr), P(dl.obs), C.c_int(dl.obs.shape[2]), step[1], step[2],
                   P(dl.act), C.c_void_p(dl.stream.cuda_stream))
            b = bound[key] = dict(step=step, act=act, keep=prm)
        return b

    @staticmethod
    def _is_orca_policy(policy):
        """``policy`` asks for the ORCA robot of crowd_nav/policy_no_train/orca.py: an instance, or its key in the combined factory."""
        from ..crowd_nav.policy_no_train.orca import ORCA

        return isinstance(policy, ORCA) or (isinstance(policy, str) and policy == "orca_device")

    def _orca_policy(self, policy, who, explore=None):
        """The ORCA policy behind ``"orca_device"`` or an instance, with the no-train policies' refusals -- made before anything touches the
        device (``who`` asks)."""
        if explore is not None:
            raise ValueError(f"{who}: explore= belongs to the value-based policies (CADRL, SARL)")
        if isinstance(policy, str):
            from ..crowd_nav.policy_no_train.orca import ORCA

            policy = ORCA()                      # (the class's constants: no state, no device)
        if policy.kinematics != "holonomic" or (self.cw is not None and self.cw.unicycle):
            raise ValueError(f"{who}: the ORCA policy acts in ActionXY and needs a holonomic robot")
        if self.cw is not None and self.cw.d_robot is None:
            raise ValueError(f"{who} needs the robot rows")
        return policy

    def _orca_launch(self, dl, pol):
        """One launch of cs_policy_orca for the W resident worlds on the device stream (called inside its scope): the decision is one library call."""
        from ..crowd_nav.policy_no_train.orca import launch

        launch(self.W, self.n, self.cw.d_robot.ptr, dl.obs.data_ptr(), dl.obs.shape[2], self.robot_time_step if pol.time_step is None else pol.time_step,
               pol.neighbor_dist, pol.max_neighbors, pol.time_horizon, pol.safety_space, dl.act.data_ptr(), dl.stream.cuda_stream)

    def _observe_if_stale(self, dl):
        """No step since the batch was generated: the observation of the resident rows (what a decision in a launch of its own reads)."""
        if dl.obs_fresh:
            return
        d = self.cw.descriptor(respawn=False)
        _lib.check(_lib.load().cs_gym_observe(d, self.headed_obs, dl.obs.data_ptr(), dl.stream.cuda_stream))
        dl.obs_fresh = True

    def step_device(self, actions, auto_reset=True):
        """``step`` without leaving the GPU: ``actions`` is a float32 torch CUDA tensor [W, 2] (holonomic vx, vy) -- or
        ``env.action_buffer()`` itself, filled in place (no copy).  Returns torch CUDA tensors (obs [W, N, 5|7], reward [W],
        terminated [W], truncated [W], info_code [W]); obs is a persistent buffer rewritten by the next call, the other four
        alternate between two sets (those of the previous step stay valid for one more call).
        With ``auto_reset=True`` the worlds whose episode ended take over their next episode -- generated ahead on the device from
        the next unused seed -- before the observation is taken (same-step autoreset).  ``auto_reset="next_step"`` is Gymnasium's
        NEXT_STEP mode: a world that ended at step t returns its terminal observation at t and the first observation of its next
        episode -- with reward 0 and no termination -- at t + 1, taken over from the staging batch at the end of step t + 1.
        ``auto_reset=False``: no resets (a finished world keeps stepping)."""
        dl = self._device_loop_state()
        c = self._open_step(dl, auto_reset)
        with SideStream(dl):
            if actions is not dl.act:
                import torch

                dl.act.copy_(actions.to(device="cuda", dtype=torch.float32), non_blocking=True)
            self._issue_step(dl, c)
        dl.obs_fresh = True                        # the step wrote the observation buffer act_device reads
        return c.results

    def reset_failed_mask(self):
        """int32 CUDA tensor [W], no synchronisation: 1 where the world's LAST device-side auto-reset could not be generated
        (cs_generate_worlds status != 0: the bounded rejection sampling gave up, or the traffic is too dense -- the reference loops
        forever / raises there).  Such a world keeps its finished rows and starts a new episode FROM them (its step counter and clock
        were reset with the others'): after a collision or a reached goal it ends again at once and tries the following seed of its
        sequence; after a time-limit truncation it runs a further episode from where it stands.  The flag returns to 0 with the first
        reset that succeeds.  2: the take-over was DEFERRED (one-launch step, cs_gym_step_staged: the staged episode was not ready; the
        world is between two episodes -- reward 0, no flags -- until a later step finds it; with the refill cadence of this class that does
        not happen)."""
        return self._device_loop_state().failed

    def failed_resets(self) -> int:
        """Number of worlds flagged in ``reset_failed_mask()``.  Synchronises."""
        return int((self._device_loop_state().failed != 0).sum().item())

    def device_stream(self):
        """The torch stream the device-resident step runs on.  A loop that does its own GPU work inside ``with torch.cuda.stream(env.device_stream())``
        is ordered with the step by the stream itself: step_device then skips its two cross-stream waits (four HIP calls per step)."""
        return self._device_loop_state().stream

    def action_buffer(self):
        """The persistent [W, 2] action tensor the step kernel reads: write actions into it and pass it to ``step_device``."""
        return self._device_loop_state().act

    def act_device(self, policy, explore=None):
        """Every world's robot decides with a no-train CrowdNav policy (``policy``: a name of crowd_nav.policy_no_train.policy_factory or
        an instance of its classes) -- ``predict`` for W robots in ONE launch of cs_policy_no_train on ``device_stream()``, reading the
        resident robot rows and the current observation, writing ActionXY rows into ``action_buffer()``.  Returns that buffer, ready
        for ``step_device(env.action_buffer())``; nothing crosses to the host.  The policy's ``time_step`` (None: the robot time step)
        is the social-force policies' integration step.  Needs worlds generated on the device (``reset(..., device=True)``) and a
        holonomic robot (the policies act in ActionXY, robot_agent.py:112-114).

        A ``crowd_nav.policy`` CADRL / SARL instance decides with its value network instead: cs_peek (or the constant-velocity model
        when the policy's ``query_env`` is false) -> cs_lookahead -> cs_value_net_decide (cs_value_net_decide_bf16 after the policy's
        ``set_decision_precision("bf16")``), all on ``device_stream()``; after the policy's ``set_decision_input("fused")``, cs_peek ->
        cs_value_net_decide_worlds, which generates the look-ahead rows in the kernel and allocates no look-ahead tensor.  ``explore``: an
        int32 CUDA tensor [W] of action indices forced on their worlds, -1 = greedy (the caller's epsilon-greedy draw).  The action
        values and choices of that decision stay readable through ``last_values_device()``.  An OM-SARL instance
        (``policy_factory["om_sarl"]``) runs cs_peek -> cs_lookahead -> cs_occupancy_maps on the next humans -> cs_value_net_decide_om
        (cs_value_net_decide_om_bf16 after the policy's ``set_wide_precision("bf16")``), an
        LSTM-RL instance (``policy_factory["lstm_rl_device"]``) cs_peek -> cs_lookahead -> cs_value_net_decide_lstm, which sorts every
        (world, action)'s humans by decreasing distance inside the kernel (cs_value_net_decide_lstm_bf16 after the policy's
        ``set_recurrent_precision("bf16")``; after its ``set_recurrent_input("fused")``, cs_peek -> cs_value_net_decide_lstm_worlds[_bf16] alone,
        which allocates no look-ahead tensor); an OM-LSTM-RL instance (``policy_factory["om_lstm_rl"]``) both:
        the maps of the next humans, then cs_value_net_decide_lstm_om with the policy's map order (cs_value_net_decide_lstm_om_bf16 after the
        policy's ``set_mapped_precision("bf16")``).

        An ``ORCA`` instance (crowd_nav/policy_no_train/orca.py) or the name ``"orca_device"`` -- its key in crowd_nav.policy.policy_factory --
        decides with one launch of cs_policy_orca instead (csrc/policy_orca.hip: one RVO2 doStep for agent 0, a wavefront per world), with the
        same inputs, the same output buffer and the same refusals as the no-train policies; the policy's ``time_step`` (None: the robot time
        step) is the simulator's.  The no-train factory's ``"orca"`` keeps raising NotImplementedError."""
        if self._is_orca_policy(policy):
            pol = self._orca_policy(policy, "act_device", explore)      # (refused before anything touches the device)
            dl = self._device_loop_state()
            with SideStream(dl):
                self._observe_if_stale(dl)
                self._orca_launch(dl, pol)
            return dl.act
        if not isinstance(policy, str):
            from ..crowd_nav.policy.cadrl import CADRL

            if isinstance(policy, CADRL):
                return self._act_device_value(policy, explore)
        dl = self._device_loop_state()
        if explore is not None:
            raise ValueError("act_device: explore= belongs to the value-based policies (CADRL, SARL)")
        pol = self._no_train_policy(dl, policy, "act_device")
        with SideStream(dl):
            self._observe_if_stale(dl)
            _lib.check(_lib.load().cs_policy_no_train(*self._policy_args(dl, pol)["act"]))     # a decision is one library call
        return dl.act

    def act_step_device(self, policy, auto_reset=True):
        """``act_device(policy)`` and ``step_device(action_buffer(), auto_reset)`` as ONE library call -- and, for the SFM / HSFM crowds of
        the one-wavefront step kernels, ONE launch (cs_gym_step_policy / cs_gym_step_staged_policy): the step kernel's head decides every
        world's ActionXY from the rows it has loaded before it consumes it.  ``policy``: a no-train CrowdNav policy as ``act_device``
        takes it (a name of policy_factory or an instance of its classes).  Returns what ``step_device`` returns and leaves the decided
        actions in ``action_buffer()``; runs on ``device_stream()``, nothing crosses to the host.  Bit for bit the results of the two
        calls.  The other crowds (ORCA, social momentum, walls, the smallest worlds) run the decision kernel and the step's launches
        inside the same call.  A CADRL / SARL instance decides in milliseconds and gains nothing here: ``act_device``, then ``step_device``.
        An ``ORCA`` instance or ``"orca_device"`` (see ``act_device``) takes the second form for every crowd: no step build decides ORCA in
        its head, so the decision launch (cs_policy_orca) and the plain step run behind each other inside one stream scope and one call."""
        from ..crowd_nav.policy_no_train.policy import NoTrainPolicy

        if self._is_orca_policy(policy):
            pol = self._orca_policy(policy, "act_step_device")          # (refused before anything touches the device)
            dl = self._device_loop_state()
            c = self._open_step(dl, auto_reset)
            with SideStream(dl):
                self._observe_if_stale(dl)
                self._orca_launch(dl, pol)
                self._issue_step(dl, c)
            dl.obs_fresh = True
            return c.results

        if not isinstance(policy, (str, NoTrainPolicy)):   # (refused before anything touches the device)
            raise TypeError(f"act_step_device takes a no-train policy (bp, ssp, sfm_helbing, sfm_guo, sfm_moussaid), not {policy!r}: "
                            "a value-based policy (CADRL, SARL) decides with act_device, then step_device")
        dl = self._device_loop_state()
        pol = self._no_train_policy(dl, policy, "act_step_device")
        c = self._open_step(dl, auto_reset)
        pargs = self._policy_args(dl, pol)["step"]
        with SideStream(dl):
            self._observe_if_stale(dl)
            self._issue_step(dl, c, pargs)
        return c.results

    def act_step_variant(self) -> str:
        """Which kernels ``act_step_device`` runs for this batch (cs_gym_step_policy_variant): the step build that decides in its head, or
        ``k_policy_no_train + `` the plain step's build."""
        import ctypes as C

        d = self.cw.descriptor()
        buf = C.create_string_buffer(320)
        _lib.check(_lib.load().cs_gym_step_policy_variant(d, buf, 320))
        return buf.value.decode()

    def _refuse_value_policy(self, who, pol, before, kinematics_first=False):
        """What ``who`` cannot take as a value-based policy of this batch, refused before anything touches the device.  ``before``: what the
        policy was about to do unconfigured; ``kinematics_first``: act_device's order, the robot's kinematics ahead of the missing model."""
        from ..crowd_nav.policy.cadrl import CADRL

        if not isinstance(pol, CADRL):
            raise TypeError(f"{who} takes a value-based policy (CADRL, SARL), not {pol!r}")
        refusals = [(pol.model is None, AttributeError(f"{pol.name}: configure() the policy before it {before}")),
                    (pol.kinematics != "holonomic" or (self.cw is not None and self.cw.unicycle),
                     ValueError(f"{who}: the value-based policies act in ActionXY and need a holonomic robot"))]
        for refused, error in reversed(refusals) if kinematics_first else refusals:
            if refused:
                raise error
        if bool(pol.with_theta_and_omega_visible) != self.headed_obs:
            raise ValueError(f"{who}: the policy's with_theta_and_omega_visible and the batch's headed_obs differ")
        if self.cw is not None and self.cw.d_robot is None:
            raise ValueError(f"{who} needs the robot rows")
        if 1 < pol.family.min_humans and self._human_count() < pol.family.min_humans:      # (only a family with maps asks for more than one)
            raise ValueError(f"{who}: {pol.name}'s occupancy maps need at least two humans a world")

    def _act_device_value(self, pol, explore):
        """act_device for a CADRL / SARL instance: W decisions of its value network, nothing crosses to the host."""
        import torch

        from ..crowd_nav.policy import value_net

        self._refuse_value_policy("act_device", pol, "decides", kinematics_first=True)
        dl = self._device_loop_state()
        if pol.action_space_ndarray is None:
            pol.build_action_space(float(self._gen_kw["robot_desired_speed"]))
        W = self.W
        acts = pol.device_action_space()            # (kept on the policy beside action_space_ndarray, uploaded again when its values change)
        A = acts.shape[0]
        if explore is not None:
            if not (torch.is_tensor(explore) and explore.is_cuda and explore.dtype == torch.int32 and tuple(explore.shape) == (W,)):
                raise ValueError("act_device: explore is an int32 CUDA tensor [W] of action indices (-1 = greedy)")
            explore = explore.contiguous()
        net = pol.device_net()                       # (repacked here, on the caller's stream, only when a parameter changed)
        if dl.vn_values is None or dl.vn_values.shape[1] != A:
            dl.vn_values = torch.zeros((W, A), dtype=torch.float32, device="cuda")
            dl.vn_choice = torch.zeros(W, dtype=torch.int32, device="cuda")
        with SideStream(dl) as s:
            nxt = None
            if not pol.query_env:                    # cadrl.py:92-105: the humans keep their velocity over the robot's step
                o, T = self.observe_device(), self.robot_time_step
                nxt = (torch.stack([o[..., 0] + o[..., 2] * T, o[..., 1] + o[..., 3] * T, o[..., 5] + o[..., 6] * T, o[..., 2], o[..., 3], o[..., 6]], -1)
                       if self.headed_obs else torch.stack([o[..., 0] + o[..., 2] * T, o[..., 1] + o[..., 3] * T, o[..., 2], o[..., 3]], -1)).contiguous()
            nxt, cur_, rob = self._worlds_on_side_stream(dl, nxt)
            rot, rew = value_net.decide_for_worlds(net, pol.decision_input, pol.decision_precision, acts, nxt, cur_, rob, pol.gamma, self.robot_time_step,
                                                   explore, dl.vn_values, dl.vn_choice, dl.act, dl.stream.cuda_stream,
                                                   recurrent_precision=pol.recurrent_precision, mapped_precision=pol.mapped_precision,
                                                   wide_precision=pol.wide_precision, recurrent_input=pol.recurrent_input)
            s.inputs = (nxt, cur_, rob, rot, rew, explore)
        return dl.act

    def last_values_device(self):
        """(action values [W, A] float32, chosen action index [W] int32) of the last value-based ``act_device`` decision, as CUDA tensors
        rewritten by the next one; None before the first."""
        dl = self._device_loop_state()
        if dl.vn_values is None:
            return None
        return dl.vn_values, dl.vn_choice

    def joint_state_device(self, policy):
        """What a trainer stores for the decision every robot is about to take: ``policy.transform`` of every world's resident state -- the
        rotated joint state of the robot with each human, what ``predict`` leaves in ``last_state`` -- as a new CUDA tensor [W, n, 13|15].
        ``policy``: a configured CADRL / SARL instance.  One launch of cs_value_net_state on ``device_stream()`` (which also evaluates the
        network: ``value_device(policy, with_state=True)`` returns both); nothing crosses to the host.  For an OM-SARL instance the rows are
        [W, n, 13|15 + C]: the maps of the CURRENT humans appended, as its ``transform`` gives them per world (three launches, see
        ``value_device``)."""
        return self._state_values_device("joint_state_device", policy, None, None, 0.0, True)[1]

    def value_device(self, policy, model=None, rewards=None, bootstrap=False, with_state=False):
        """The value network on every world's resident state: a new float32 CUDA tensor [W] of V(s) -- CADRL: the minimum over the humans,
        SARL: the network's output --, with ``with_state`` the pair (values, rows [W, n, 13|15] as ``joint_state_device`` returns them).
        ``model``: the module to evaluate instead of ``policy.model`` -- any module of the policy's architecture, such as a trainer's
        ``copy.deepcopy`` target network; its packed weights are kept per module and repacked only after a parameter changed.
        ``bootstrap=True`` evaluates the trainer's target of the state the worlds are in, ``rewards + gamma^(robot_time_step * v_pref) * V``
        (crowd_nav/utils/explorer.py:120-153; ``rewards``: a float32 CUDA tensor [W], None = 0); a terminal step's target is its reward
        alone: ``torch.where(done, rewards, target)``.  Without ``bootstrap`` ``rewards`` must be None.  float32 arithmetic whatever the
        policy's decision precision.  One launch of cs_value_net_state on ``device_stream()``; nothing crosses to the host.  An OM-SARL
        instance gives the same quantities from THREE launches instead of one: cs_value_net_state for the rotated rows, cs_occupancy_maps
        on the current humans, cs_value_net_decide_om with A = 1 (a one-row action table, no choice); its rows are [W, n, 13|15 + C].  An
        LSTM-RL instance takes TWO: cs_value_net_state for the rows, cs_value_net_decide_lstm with A = 1 on them in the humans' own order
        (``transform`` does not sort; the reference's trainer evaluates its target network on the rows as stored)."""
        if rewards is not None and not bootstrap:
            raise ValueError("value_device: rewards= belongs to bootstrap=True (rewards + gamma^(robot_time_step * v_pref) * V)")
        values, rows = self._state_values_device("value_device", policy, model, rewards, self.robot_time_step if bootstrap else 0.0, with_state)
        return (values, rows) if with_state else values

    def _state_values_device(self, who, pol, model, rewards, dt, with_rows):
        """cs_value_net_state on the resident worlds, with act_device's refusals and stream scope: (values [W], rows [W, n, cols] or None)."""
        self._refuse_value_policy(who, pol, "evaluates a state")
        import torch

        from ..crowd_nav.policy import value_net

        dl = self._device_loop_state()
        if rewards is not None:
            if not (torch.is_tensor(rewards) and rewards.is_cuda and rewards.dtype == torch.float32 and tuple(rewards.shape) == (self.W,)):
                raise ValueError(f"{who}: rewards is a float32 CUDA tensor [W]")
            rewards = rewards.contiguous()
        net = pol.state_net(model)                   # (repacked here, on the caller's stream, only when a parameter changed)
        with SideStream(dl) as s:
            _, cur_, rob = self._worlds_on_side_stream(dl, peek=False)
            values, rows = value_net.state_values_for_worlds(net, cur_, rob, rewards, pol.gamma, dt, with_rows, dl.stream.cuda_stream)
            s.inputs, s.outputs = (cur_, rob, rewards), (values, rows)
        return values, rows

    def _human_count(self):
        """Humans a world: of the generated batch, or what the configuration will generate"""
        n = getattr(self, "n", None)
        return int(n) if n is not None else self.config.getint("sim", "human_num")

    def occupancy_maps_device(self, cell_num, cell_size, channels, which="current"):
        """OM-SARL's local occupancy maps of every world's humans (cs_occupancy_maps; ``build_occupancy_maps`` for W worlds), for a network
        of the caller's own: a new float32 CUDA tensor [W, n, cell_num^2 * channels].  ``which``: "current" -- the humans as they stand,
        what ``transform`` appends -- or "next" -- one robot step ahead (cs_peek), what a decision appends.  On ``device_stream()``;
        nothing crosses to the host.  Worlds of one human have nobody to map: ValueError, before anything touches the device."""
        import torch

        from ..crowd_nav.policy import value_net

        if which not in ("current", "next"):
            raise ValueError(f'occupancy_maps_device: which={which!r}: "current" or "next"')
        if self._human_count() < 2:
            raise ValueError("occupancy_maps_device: occupancy maps need at least two humans a world")
        grid = (int(cell_num), float(cell_size), int(channels))
        dl = self._device_loop_state()
        with SideStream(dl) as s:
            nxt, cur_, _ = self._worlds_on_side_stream(dl, peek=which == "next")
            maps = value_net.maps_of(*((nxt, 3 if self.headed_obs else 2) if which == "next" else (cur_, 2)), grid, dl.stream.cuda_stream)
            s.inputs, s.outputs = (nxt, cur_), (maps,)
        return maps

    def lookahead_device(self, action_space):
        """The per-decision array work of CADRL / SARL for every world, on the device: one-step look-ahead of the humans
        (``get_next_human_observable_states``, cadrl.py:258-259 -> cs_peek) and ``compute_rotated_states_and_reward``
        (cadrl.py:42-83 -> cs_lookahead) for all actions.  ``action_space`` [A, 2] (numpy or CUDA tensor).  Returns torch CUDA
        tensors (rotated_states [W, A, N, 13] -- 15 columns with ``headed_obs`` (theta and omega visible) --, rewards [W, A]) ready for ONE
        batched value-network call -- no host copy.
        Needs worlds generated on the device (``reset(..., device=True)``), like ``step_device``."""
        import torch

        from ..crowd_nav.policy import value_net

        dl = self._device_loop_state()
        if self.cw.d_robot is None:
            raise ValueError("lookahead_device needs the robot rows")
        with SideStream(dl) as s:                   # the library launches on this stream (cw.stream); the torch ops between them follow
            acts = torch.as_tensor(np.asarray(action_space, dtype=np.float32) if not torch.is_tensor(action_space) else action_space,
                                   dtype=torch.float32, device="cuda").contiguous()
            out = s.outputs = value_net.lookahead(acts, *self._worlds_on_side_stream(dl), self.robot_time_step, dl.stream.cuda_stream)
        return out

    def _worlds_on_side_stream(self, dl, next_humans=None, peek=True):
        """What a look-ahead reads of the resident worlds, as contiguous CUDA tensors: (next humans [W, n, 4 | 6] -- cs_peek's, or the caller's;
        None without ``peek``: the current state alone is asked for --, current humans [W, n, 5 | 7], robot rows [W, 9] in FullState order)."""
        import torch

        cw, W, n = self.cw, self.W, self.n
        lib = _lib.load()
        d = cw.descriptor(respawn=False)
        peek_buf = cw._buffer("peek", (W, n, 8))
        if next_humans is None and peek:
            _lib.check(lib.cs_peek(d, self.robot_time_step, peek_buf.ptr, cw.stream))
        if dl.la_cols is None:
            # next humans: (px, py, vx, vy), or (x, y, yaw, Vx, Vy, Omega) with theta / omega visible (cadrl.py:42-83) = cs_peek's first six
            dl.la_cols = torch.as_tensor([0, 1, 2, 3, 4, 5] if self.headed_obs else [0, 1, 3, 4], device="cuda")
            dl.la_robot_cols = torch.as_tensor([0, 1, 3, 4, 8, 10, 11, 12, 2], device="cuda")   # FullState order
            dl.la_robot = cw.d_robot.torch().view(W, 13)
        nxt = peek_buf.torch().view(W, n, 8).index_select(2, dl.la_cols).contiguous() if next_humans is None and peek else next_humans
        cur = dl.state[:, :n].index_select(2, dl.cols).contiguous()
        rob = dl.la_robot.index_select(1, dl.la_robot_cols).contiguous()
        return nxt, cur, rob

    # ------------------------------------------------------------------ imitation learning, W worlds at once
    def set_human_motion_model_as_robot_policy(self, policy_name, runge_kutta=False, safety_space=0.0):
        """Every world's robot follows a human motion model (SocialNavGym.set_human_motion_model_as_robot_policy,
        social_nav_sim.py:862-873); call after ``reset``.  ``safety_space``: the value the Gym hands to set_safety_space
        (motion_model_manager.py:147-170) -- pass the one used at ``reset``."""
        from .. import scenarios as sc
        from ..batched import HUMAN_MODELS

        if runge_kutta and policy_name == "orca":
            raise NotImplementedError                              # ORCA is Euler only (motion_model_manager.py:579)
        if policy_name not in HUMAN_MODELS:
            raise Exception(f"The robot motion model '{policy_name}' does not exist")
        if self.cw is None:
            raise RuntimeError("reset() first: the robot model is attached to the resident worlds")
        cw, n = self.cw, self.n
        hm = np.zeros((self.W, cw.rows), np.float32)
        if policy_name == "orca":
            hm[:] = 0.01 + safety_space          # robot_sim radii: radius + 0.01 (+ safety space) for humans and robot (:585-587)
            cw.set_robot_model("orca", None, 0.01 + safety_space, hm)
        else:
            # human.safety_space as the single-agent force functions read it: only set_safety_space touches it (:151-153)
            if safety_space > 0 and self._proto.human_policy != "orca":
                hm[:, :n] = 0.01 + safety_space
            cw.set_robot_model(policy_name, sc.default_params(policy_name), (0.01 + safety_space) if safety_space > 0 else 0.0, hm)
        self.robot_motion_model_title = policy_name
        self.robot_runge_kutta = bool(runge_kutta)    # every substep's update_robot is an RK45 solve over dt (cs_robot_model_rk45)

    def imitation_learning_step(self):
        """SocialNavGym.imitation_learning_step (social_nav_gym.py:252-274) for every world: time_step_factor x
        { update_robot ; update_humans }, then reward / termination from the ACTUAL distances of the new state.
        Returns (obs, reward [W], terminated [W], truncated [W], info_code [W])."""
        if getattr(self.cw, "robot_model", None) is None:
            raise AttributeError("set_human_motion_model_as_robot_policy has not been called")
        if getattr(self, "robot_runge_kutta", False):
            # motion_model_manager.py:631-640: the robot's SFM / HSFM model integrated by RK45 over every substep, the humans standing
            # during the solve; then the crowd's Euler substep -- the reference's alternation, launch by launch
            for _ in range(self.time_step_factor):
                self.cw.robot_model_rk45(self.time_step, download=False)
                self.cw.step(self.time_step, 1, None)
        else:
            self.cw.imitation_block(self.time_step, self.time_step_factor)
        for _ in range(self.time_step_factor):
            self.global_time += np.float32(self.time_step)
        out = self.cw.actual_collision_reward(self.robot_time_step, self.global_time, self.reward_cfg)
        return self.observe(), out[:, 3].copy(), out[:, 4] > 0, out[:, 5] > 0, out[:, 6].astype(np.int32)

    def observe(self):
        S = self.cw.get_states()[:, :self.n]
        cols = [0, 1, 3, 4, 8] + ([2, 7] if self.headed_obs else [])
        return S[:, :, cols]

    def step(self, actions):
        """actions [W, 2] holonomic (vx, vy).  Returns (obs, reward [W], terminated [W], truncated [W], info_code [W])."""
        actions = np.ascontiguousarray(np.broadcast_to(np.asarray(actions, np.float32), (self.W, 2)))
        out = self.cw.collision_reward(actions, self.robot_time_step, self.global_time, self.reward_cfg)
        self.cw.step(self.time_step, self.time_step_factor, actions)
        for _ in range(self.time_step_factor):
            self.global_time += np.float32(self.time_step)
        return self.observe(), out[:, 3].copy(), out[:, 4] > 0, out[:, 5] > 0, out[:, 6].astype(np.int32)
