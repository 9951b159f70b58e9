/*
 * crowdstep.h -- C ABI of libcrowdstep.so, the MI355X (gfx950) batched crowd-stepper.
 *
 * The reference (TommasoVandermeer/Social-Navigation-PyEnvs) has no FFI: its seam for this path is
 * the pure-array Python function  update_humans_parallel()  (social_gym/src/forces_parallel.py:185,
 * called from exactly one site, social_gym/src/motion_model_manager.py:360) plus the rvo2
 * PyRVOSimulator object API for ORCA (motion_model_manager.py:237-246, 386-394).  Every entry point
 * below names the reference interface it replaces.  All of them are batched over W independent
 * worlds; W = 1 with the reference's [N,13] arrays is the drop-in case.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.  Pointers named d_* are DEVICE
 *     pointers (hipMalloc / cs_malloc / torch.Tensor.data_ptr()); h_* are host pointers.
 *   - return 0 (CS_OK) or a negative cs_status; cs_last_error() gives the message (thread-local).
 *     Nothing throws or aborts across the ABI.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls are
 *     asynchronous on that stream unless stated otherwise.
 *   - arithmetic type: float32 ("f32").  Array layouts are the reference's row layouts:
 *       state row  S[13]  = px,py,theta,vx,vy,bvx,bvy,omega,r,m,gx,gy,vd       (agent.py:256-258)
 *       param row  P[20]  = relax_t,Ai,Aw,Bi,Bw,Ci,Cw,Di,Dw,Ei,k1,k2,lambda,gamma,ns,ns1,ko,kd,
 *                           alpha,k_lambda                                      (agent.py:268-388)
 *       goals [n][G][2] NaN padded; obstacles [O][Smax][2][2] NaN padded
 *   - a world has n humans (+1 trailing robot row when `robot_row` is set) = `rows` rows.
 */
#ifndef CROWDSTEP_H
#define CROWDSTEP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum cs_status {
    CS_OK = 0,
    CS_ERR_ARG = -1,      /* bad shape / null pointer / unsupported size                       */
    CS_ERR_TYPE = -2,     /* model type outside 0..8 (the reference raises ValueError, :211)    */
    CS_ERR_HIP = -3,      /* HIP runtime error, message in cs_last_error()                      */
    CS_ERR_NO_DEVICE = -4 /* no gfx950 device visible                                           */
} cs_status;

/* model ids = index into the reference's SFMS list (motion_model_manager.py:15-17) */
enum {
    CS_SFM_HELBING = 0, CS_SFM_GUO = 1, CS_SFM_MOUSSAID = 2,
    CS_HSFM_FARINA = 3, CS_HSFM_GUO = 4, CS_HSFM_MOUSSAID = 5,
    CS_HSFM_NEW = 6, CS_HSFM_NEW_GUO = 7, CS_HSFM_NEW_MOUSSAID = 8,
    CS_ORCA = 9, /* HUMAN_MODELS[9] (social_nav_gym.py:11-12); only cs_step / cs_peek accept it */
    CS_SOCIAL_MOMENTUM = 10 /* MotionModelManager("social_momentum") (motion_model_manager.py:247-251, 395-404;
                               social_gym/src/social_momentum.py); only cs_step / cs_peek accept it */
};

/* memory layout of a state array: element (world w, row a, field f) lives at
 *   base[(w*rows + a) * agent_stride + f * field_stride]
 * CS_LAYOUT_AOS: the reference's [W][rows][13]   (agent_stride 13, field_stride 1)
 * CS_LAYOUT_SOA: 13 planes [13][W*rows]          (agent_stride 1,  field_stride W*rows) */
enum { CS_LAYOUT_AOS = 0, CS_LAYOUT_SOA = 1 };

/* flag bits of cs_worlds.flags */
enum {
    CS_ALL_PARAMS_EQUAL = 1 << 0, /* update_humans_parallel(all_params_equal=True): pair forces use P[0]  */
    CS_ROBOT_ROW        = 1 << 1, /* last_is_robot=True: last row is the robot, never updated by the model */
    CS_PARAMS_SHARED    = 1 << 2, /* d_params is one [n][20] block shared by all worlds                    */
    CS_OBSTACLES_SHARED = 1 << 3, /* d_obstacles is one [O][Smax][2][2] block shared by all worlds         */
    CS_RESPAWN          = 1 << 4, /* parallel-traffic respawn after every substep (mmm.py:407-422)         */
    CS_ROBOT_UNICYCLE   = 1 << 5  /* d_action rows are (v, r) instead of (vx, vy) (robot_agent.py:119-136) */
};

/* Descriptor of W resident worlds; every pointer is a caller-owned device buffer. */
typedef struct cs_worlds {
    int32_t W;          /* worlds                                                                */
    int32_t n;          /* humans per world                                                      */
    int32_t G;          /* goal slots per human                                                  */
    int32_t O;          /* polygons (0 = no walls)                                               */
    int32_t Smax;       /* segment slots per polygon                                             */
    int32_t type;       /* 0..8                                                                  */
    int32_t flags;      /* CS_* bits                                                             */
    int32_t layout;     /* CS_LAYOUT_*  of d_state                                               */
    float*  d_state;    /* [W][rows][13] (or SoA planes)  in/out                                 */
    float*  d_goals;    /* [W][n][G][2]                   in/out (rotated on goal switch)        */
    const float* d_params;    /* [W][n][20] or [n][20]                                           */
    const float* d_safety;    /* [W][rows]                                                       */
    const float* d_obstacles; /* [W][O][Smax][2][2] or shared, NULL when O == 0                  */
    float*  d_robot;    /* [W][13] robot safe-state rows or NULL.  With CS_ROBOT_ROW it is the
                           source of the last row before every substep (mmm.py:359)             */
    const int32_t* d_world_flags; /* optional [W]: bit0 = respawn enabled in this world (NULL: the
                           CS_RESPAWN bit applies to every world; hybrid batches mix both kinds)   */
    float   respawn_bound_x, respawn_bound_y; /* respawn_bounds (social_nav_sim.py:360)           */
    /* ORCA only (type == CS_ORCA): ORCA_DEFAULTS of motion_model_manager.py:14 */
    float   orca_neighbor_dist, orca_time_horizon, orca_time_horizon_obst;
    int32_t orca_max_neighbors;
    /* social momentum only (type == CS_SOCIAL_MOMENTUM): n_actions of motion_model_manager.py:249 (0 = 20) */
    int32_t sm_n_actions;
    /* ORCA only: static obstacles as RVO2 keeps them after addObstacle / processObstacles (motion_model_manager.py:244-246):
     * [orca_n_vertices][8] records  point.x, point.y, unitDir.x, unitDir.y, isConvex, next, prev, 0  (polygon vertices in
     * the order given, counter-clockwise; next / prev = vertex indices), shared by all worlds.  NULL / 0 = no obstacles. */
    const float* d_orca_vertices;
    int32_t orca_n_vertices;
    /* ORCA only: RVO2 keeps neighborDist, maxNeighbors, timeHorizon, timeHorizonObst PER AGENT (RVOSimulator::addAgent(position,
     * neighborDist, maxNeighbors, timeHorizon, timeHorizonObst, radius, maxSpeed, velocity): the call at motion_model_manager.py:241,
     * where the reference passes ORCA_DEFAULTS for everyone).  [W][rows][4] floats in that order, or NULL = the four scalars above for
     * every agent.  With it, orca_max_neighbors must be the LARGEST maxNeighbors and orca_neighbor_dist the largest neighborDist. */
    const float* d_orca_agent_params;
    /* ORCA only (ABI 4): the arithmetic of the register-resident build for THESE worlds -- CS_ORCA_MATH_* below.  0 (a zeroed struct) = the
     * process default: CROWDSTEP_ORCA_MATH=exact|fast|fma if set, else exact.  A field of the context, not a process-wide switch: two
     * environments of one process may differ, and the mode is part of what a captured HIP graph froze. */
    int32_t orca_math;
} cs_worlds;

/* cs_worlds.orca_math: how the register-resident ORCA build (k_orca_step<FAST10>: maxNeighbors = 10, no static obstacles, one RVO2
 * parameter set -- what motion_model_manager.py:14, 237-246 always creates) divides and takes square roots in RVO2's linearProgram1 / 2 / 3
 * and line construction (reached through rvo2.PyRVOSimulator.doStep, motion_model_manager.py:387; float32 like RVO2):
 *   EXACT  correctly rounded divide / sqrt, no FMA contraction: bit-identical to oracle/orca_oracle.c.  THE DEFAULT.
 *   FAST   v_rcp_f32 / v_sqrt_f32 / v_rsq_f32 (1 ulp each);
 *   FMA    fast, and determinants / dot products / point + t * direction as mul + fma.
 * FAST / FMA are opt-in: they stay within north_star's 1e-5 per step except on the agent-substeps float32 does not determine (a decision
 * edge of the linear programme or an ill-conditioned intersection; tests/test_gpu_orca_fast.py classifies every one).  The generic ORCA
 * builds (other maxNeighbors, static obstacles, per-agent parameters, the grid path, the robot's own ORCA model) are always exact. */
enum { CS_ORCA_MATH_DEFAULT = 0, CS_ORCA_MATH_EXACT = 1, CS_ORCA_MATH_FAST = 2, CS_ORCA_MATH_FMA = 3 };

/* ---------------------------------------------------------------- runtime / memory helpers */
const char* cs_last_error(void);
/* The ABI this header describes.  A host binding must refuse a library whose cs_abi_version() differs: struct layouts (cs_worlds,
 * cs_gym_book, cs_stage_book) and argument lists change between versions (social_navigation_pyenvs_amd/_lib.py load() does). */
#define CS_ABI_VERSION 4
int cs_abi_version(void);
int cs_device_count(int* count);
int cs_set_device(int device);
int cs_device_name(int device, char* buf, size_t buflen);
/* PCI address "domain:bus:device.function" of a device: bench.py reports it per rank, so that a multi-GPU line proves which
 * card every rank sat on (one process per GPU, no collective on the data path) */
int cs_device_pci_bus_id(int device, char* buf, size_t buflen);
int cs_malloc(void** d_ptr, size_t bytes);
int cs_free(void* d_ptr);
int cs_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes, void* stream);
int cs_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes, void* stream);
int cs_memcpy_d2d(void* d_dst, const void* d_src, size_t bytes, void* stream);
int cs_memset(void* d_ptr, int value, size_t bytes, void* stream);
int cs_stream_create(void** stream);
/* priority: 0 = default, < 0 = the device's highest, > 0 = its lowest (background work beside a step stream: the refill passes of
 * cs_refill_staged_worlds); a stream of another priority also lands on another hardware queue */
int cs_stream_create_with_priority(void** stream, int priority);
int cs_stream_destroy(void* stream);
int cs_stream_sync(void* stream);
/* HIP events on the launch stream (bench.py times kernels with these) */
int cs_event_create(void** event);
int cs_event_destroy(void* event);
int cs_event_record(void* event, void* stream);
int cs_event_elapsed_ms(void* start, void* stop, float* ms); /* synchronises on `stop` */
int cs_event_query(void* event, int* done);                  /* *done = 1 when the work recorded before `event` has finished; never blocks */
int cs_stream_wait_event(void* stream, void* event);         /* later work of `stream` waits for `event` (no host sync) */

/* HIP graphs: capture the launches issued on `stream` between begin and end (e.g. K cs_step calls of a rollout) and
 * replay them with one launch -- removes the per-launch host gap of a launch-bound loop. */
int cs_graph_begin_capture(void* stream);
int cs_graph_end_capture(void* stream, void** graph_exec);
int cs_graph_launch(void* graph_exec, void* stream);
int cs_graph_destroy(void* graph_exec);

/* ---------------------------------------------------------------- the hot path
 *
 * cs_update_humans_parallel  replaces  update_humans_parallel(type, agents_state, goals, obstacles,
 *   agents_params, dt, safety_space, all_params_equal, last_is_robot) -> updated_state
 *   (forces_parallel.py:185-284), for W worlds at once, one Euler substep.
 *   d_state is read and mutated exactly like `agents_state` (goal columns on a goal switch and, for
 *   headed types, columns 3:5 = R(theta)*bv); d_goals is rotated in place; d_out receives the
 *   returned copy (robot row copied through).  d_out may equal w->d_state (in-place update, what
 *   `self.states = update_humans_parallel(...)` amounts to, motion_model_manager.py:360).
 *   w->d_robot is ignored here (the last row of d_state IS the robot row).
 */
int cs_update_humans_parallel(const cs_worlds* w, float dt, float* d_out, void* stream);

/*
 * cs_step  replaces the substep loop of SocialNavGym.step (social_nav_gym.py:240-245) /
 *   MotionModelManager.update_humans (motion_model_manager.py:354-367, 407-422), fused in ONE
 *   launch:  n_substeps x { robot.step(action, dt) ; states[-1] = robot row ; update_humans ;
 *   respawn }.  State is updated in place.
 *   d_action: [W][2] robot action held for the whole block, or NULL (robot does not move).
 */
int cs_step(const cs_worlds* w, float dt, int n_substeps, const float* d_action, void* stream);

/*
 * cs_step_trace  cs_step (same kernel build, same arithmetic, same in-place update -- the launch differs only in one non-NULL
 *   kernel argument) that also records every human's row AFTER every fused substep, so that a test can check each substep of a
 *   fused launch on its own against the reference's single-substep function (forces_parallel.py:185-284 + the respawn rule,
 *   motion_model_manager.py:407-422) restarted from the previous record.
 *   d_trace [n_substeps][W][rows][12] = px, py, theta, vx, vy, bvx, bvy, omega, gx, gy (state columns 10:12), goals[0].x, goals[0].y
 *   (rows = n + 1 with CS_ROBOT_ROW: the robot's record k is the robot as substep k + 1 sees it -- it moves before the humans,
 *   social_nav_gym.py:240-243 -- and as it stands at the end for the last record).
 *   Types 0..8, any world size (worlds beyond one block: the grid path records from HBM after every substep).
 */
int cs_step_trace(const cs_worlds* w, float dt, int n_substeps, const float* d_action, float* d_trace, void* stream);

/*
 * cs_peek  replaces MotionModelManager.get_next_human_observable_states(dt, theta_and_omega_visible)
 *   (motion_model_manager.py:691-709): one Euler step of size dt WITHOUT committing it.
 *   d_next: [W][n][8] rows  x, y, yaw, Vx, Vy, Omega, Gx, Gy  (get_human_states(include_goal=True,
 *   headed=False), :294-298); the caller slices [0,1,3,4] for the 4-column form.
 */
int cs_peek(const cs_worlds* w, float dt, float* d_next, void* stream);

/*
 * cs_collision_reward  replaces SocialNavSim.collision_detection_and_reaching_goal
 *   (social_nav_sim.py:949-984) + compute_reward_and_infos (:986-1029) for W worlds.
 *   Reads humans from w->d_state and the robot from w->d_robot (position, radius, goal).
 *   d_action [W][2] holonomic (vx, vy).  d_global_time [W].
 *   reward_cfg = {time_limit, success_reward, collision_penalty, discomfort_dist,
 *                 discomfort_penalty_factor}
 *   d_out [W][7] = collision, dmin, reaching_goal, reward, terminated, truncated, info_code
 *   (info_code: 0 Nothing, 1 Danger, 2 ReachGoal, 3 Collision, 4 Timeout; social_gym/src/info.py)
 */
int cs_collision_reward(const cs_worlds* w, const float* d_action, float T, const float* d_global_time,
                        const float* reward_cfg /* host, 5 floats */, float* d_out, void* stream);

/*
 * cs_lookahead  replaces compute_rotated_states_and_reward(action_space, next_humans_state, current_humans_state,
 *   current_robot_state, dt, theta_and_omega_visible) -> (rotated_states, rewards)
 *   (crowd_nav/policy/cadrl.py:42-83, with transform_state_to_agent_centric :13-39) for W robots at once.
 *   d_actions [A][2]; d_next [W][n][4] (px,py,vx,vy) or [W][n][6] (x,y,yaw,Vx,Vy,Omega) when theta_and_omega_visible;
 *   d_current [W][n][5] (px,py,vx,vy,r) or [W][n][7] (+theta,omega); d_robot [W][robot_stride] rows starting with
 *   px,py,vx,vy,r,gx,gy,v_pref.  Outputs d_rotated [W][A][n][13|15] (the value-network input), d_rewards [W][A].
 */
int cs_lookahead(int W, int n, int A, int theta_and_omega_visible, const float* d_actions, const float* d_next,
                 const float* d_current, const float* d_robot, int robot_stride, float dt, float* d_rotated,
                 float* d_rewards, void* stream);

/*
 * cs_generate_worlds  replaces, for W worlds at once and on the device, what SocialNavGym.reset does per world on the
 *   host (social_nav_gym.py:135-197):  np.random.seed(seed) ; [hybrid: np.random.choice + re-seed] ;
 *   generate_circular_crossing_setting / generate_parallel_traffic_scenario /
 *   generate_circular_crossing_with_static_obstacles (social_nav_sim.py:200-431) ; the HumanAgent rows reset_sim
 *   builds (:97-198) ; robot.set(...) (social_nav_gym.py:211-213).
 *   One lane per world restates numpy's legacy MT19937 stream (init_genrand seeding, 53-bit random_sample,
 *   uniform, choice-of-two) and the generators' rejection loops in f64, draw for draw; rows are rounded to f32 when
 *   stored.  d_seeds [W] = offset[phase] + case (social_nav_gym.py:135-137).  Writes w->d_state (humans, and the
 *   robot row with CS_ROBOT_ROW), w->d_goals ([W][n][G][2], NaN-padded), w->d_robot (if not NULL), w->d_world_flags
 *   (if not NULL: 1 for parallel-traffic worlds = respawn rule on).
 *   d_mask     optional [W]: only worlds with a non-zero entry are regenerated (auto-reset of finished episodes).
 *   d_status   optional [W]: 0 ok, 1 = a human could not be placed within max_tries (the reference loops forever),
 *              2 = parallel traffic too dense (ValueError in the reference, :318-319); such worlds are left untouched.
 *   d_scenario optional [W]: the scenario each world got (the hybrid choice).
 *   d_scratch  cs_generate_scratch_bytes(W) bytes (624 MT19937 words per world).
 */
enum {
    CS_SCN_CIRCULAR_CROSSING = 0,                  /* 'circle_crossing'                          */
    CS_SCN_PARALLEL_TRAFFIC = 1,                   /* 'parallel_traffic'                         */
    CS_SCN_CIRCULAR_CROSSING_STATIC_OBSTACLES = 2, /* 'circular_crossing_with_static_obstacles'  */
    CS_SCN_HYBRID = 3                              /* 'hybrid_scenario': choice of the first two */
};
typedef struct cs_generator {
    int32_t scenario;             /* CS_SCN_*                                                               */
    int32_t n;                    /* n_actors                                                               */
    int32_t insert_robot;         /* robot start / goal take part in the rejection tests (:284-287)         */
    int32_t randomize_attributes; /* uniform(0.5,1.5) speed and uniform(0.3,0.5) radius per human (:217-220) */
    int32_t randomize_positions;  /* circular crossing only: 0 = evenly spaced (:231-251)                    */
    int32_t max_tries;            /* bound of every rejection loop                                           */
    double  circle_radius, traffic_length, traffic_height, robot_radius;
    double  human_mass;           /* 75 (reset_sim, :167)                                                    */
    double  robot_mass, robot_desired_speed; /* RobotAgent defaults (agent.py)                               */
} cs_generator;
/* (an ORCA batch -- w->type == CS_ORCA -- also gets RVO2's preferred velocity in columns 5:7 of every generated row: update_goals_orca,
 * motion_model_manager.py:125-133, as the reference sets it when it builds the simulator) */
size_t cs_generate_scratch_bytes(int W);
int cs_generate_worlds(const cs_generator* gen, const cs_worlds* w, const uint32_t* d_seeds, const int32_t* d_mask,
                       int32_t* d_status, int32_t* d_scenario, void* d_scratch, void* stream);

/*
 * cs_laser_scan  replaces LaserSensor.get_laser_measurements(humans, walls) without the noise term
 *   (social_gym/src/sensors.py:51-66; disc hit :24-33, one-sided segment hit :35-49) for W sensors at once.
 *   Humans (x, y, radius) are read from w->d_state, walls from w->d_obstacles.  Sensor poses (x, y, yaw in columns
 *   0..2 of rows of `pose_stride` floats) come from d_pose, or from w->d_robot (robot safe-state rows) when d_pose
 *   is NULL.  Ray k of `samples` points at linspace(yaw - range/2, yaw + range/2, samples)[k] (:53).
 *   d_out [W][samples] = min(hit distance, max_distance); RobotAgent.get_laser_readings subtracts the robot radius
 *   afterwards (robot_agent.py:77-82) -- the host mirror does that.
 *   Errors: max_distance > 10 -> CS_ERR_ARG with the reference's message (sensors.py:13).
 */
int cs_laser_scan(const cs_worlds* w, const float* d_pose, int pose_stride, float range, int samples,
                  float max_distance, float* d_out, void* stream);

/*
 * cs_robot_model_step  replaces MotionModelManager.update_robot(t, dt) (motion_model_manager.py:615-653) for a robot that
 *   follows a HUMAN motion model, as set by set_robot_motion_model / SocialNavGym.set_human_motion_model_as_robot_policy
 *   (motion_model_manager.py:552-589, social_nav_sim.py:862-873): ONE Euler substep of the robot of every world, the robot half
 *   of the substep loop of SocialNavGym.imitation_learning_step (social_nav_gym.py:259-263; the human half is cs_step with
 *   n_substeps = 1 and no action, which picks the moved robot up from w->d_robot when it is visible).
 *   robot_type 0..8: compute_robot_forces (:591-613) with the single-agent force functions of forces.py and the Euler update
 *     (:72-86); robot_params = the robot's 20 parameters (agent.py:269 slots; host pointer).  d_robot_memory [W][2] keeps
 *     robot.desired_force between substeps (the reference leaves it untouched within one radius of the goal, forces.py:12-16);
 *     zero it when the robot is created.  Walls: w->d_obstacles.
 *   robot_type CS_ORCA: one doStep of the robot's own RVO2 simulator (:580-589, :641-653: humans with preferred velocity 0,
 *     the robot last) = the robot's ORCA solve against the humans and w->d_orca_vertices, with w->orca_* parameters;
 *     robot_params and d_robot_memory are ignored.  PARITY UNPINNED like cs_step with CS_ORCA.
 *   robot_margin: robot.safety_space (SFM: 0 or 0.01 + safety_space; ORCA: 0.01 + safety_space, :147-170, :588).
 *   d_human_margin [W][rows]: the humans' safety_space as the ROBOT's model sees it (SFM robot: human.safety_space;
 *     ORCA robot: 0.01 + safety_space); NULL = w->d_safety.
 *   Reads the humans from w->d_state; updates w->d_robot rows (x, y, yaw, Vx, Vy, BVx, BVy, Omega) and, with CS_ROBOT_ROW,
 *   the last state row.  Errors: robot_type outside 0..9 -> CS_ERR_TYPE (the reference raises, :589).
 */
int cs_robot_model_step(const cs_worlds* w, int32_t robot_type, const float* robot_params, float robot_margin,
                        const float* d_human_margin, float* d_robot_memory, float dt, void* stream);

/*
 * cs_robot_model_velocities  replaces MotionModelManager.update_robot(t, dt, just_velocities=True) (motion_model_manager.py:615-629
 *   with euler_*_single_agent_update(..., just_velocities=True), :72-85): the robot's velocities (linear or body + angular) are
 *   integrated by its SFM / HSFM model, its position and yaw stay (SocialNavSim moves the pose at its own rate with
 *   update_robot_pose, :655-659).  Arguments as cs_robot_model_step; robot_type 0..8, or CS_ORCA: the robot's doStep gives the new
 *   velocity and the robot's simulator agent is put back on robot.position (:641-653).
 */
int cs_robot_model_velocities(const cs_worlds* w, int32_t robot_type, const float* robot_params, float robot_margin,
                              const float* d_human_margin, float* d_robot_memory, float dt, void* stream);

/*
 * cs_imitation_block  replaces the substep loop of SocialNavGym.imitation_learning_step (social_nav_gym.py:259-263):
 *   n_substeps x { motion_model_manager.update_robot(t, dt) ; motion_model_manager.update_humans(t, dt) }, arguments as
 *   cs_robot_model_step.  With an invisible robot (no CS_ROBOT_ROW: the crowd does not see it) and SFM / HSFM models on both sides
 *   this is TWO launches: the crowd's n fused substeps, which also record what the robot's integrator sees of the humans at the
 *   start of every substep (positions and linear velocities, library-owned scratch: see cs_reserve_scratch), and the robot's n substeps against those
 *   records -- bit-identical to the alternating launches.  Otherwise (visible robot, ORCA on either side) the 2 n launches are
 *   issued in the reference's order.
 */
int cs_imitation_block(const cs_worlds* w, int32_t robot_type, const float* robot_params, float robot_margin,
                       const float* d_human_margin, float* d_robot_memory, float dt, int n_substeps, void* stream);

/*
 * Library-owned scratch.  Three entry points keep device scratch of their own: cs_imitation_block's fused form (what the robot sees
 * of the crowd, [n_substeps][W][n] x 16 B) and cs_step / cs_update_humans_parallel for worlds beyond one block (double-buffered
 * rows + the neighbour grid).  The block belongs to (device, stream, use): batches driven on different streams never share one.
 * Nothing is allocated, grown or freed while `stream` is capturing: an entry point that would have to returns CS_ERR_ARG
 * -- call cs_reserve_scratch(w, n_substeps, stream) (or the entry point itself once) before cs_graph_begin_capture.  A block
 * handed out during a capture is never freed behind a graph's back (growing it later retires the old block); cs_release_scratch
 * synchronises EVERY device that holds a block and frees them all -- only when no captured graph that used them will be replayed again.
 * Threads: one host thread per (device, stream) at a time; different streams never share a block.
 */
int cs_reserve_scratch(const cs_worlds* w, int n_substeps, void* stream);
int cs_release_scratch(void);

/*
 * cs_actual_collision_reward  replaces SocialNavGym.check_actual_collisions_and_goal (social_nav_gym.py:107-118) +
 *   compute_reward_and_infos (social_nav_sim.py:986-1029) for W worlds: distances of the CURRENT state (no swept test;
 *   collision when the smallest distance is <= 0).  Same reward_cfg and d_out layout as cs_collision_reward.
 */
int cs_actual_collision_reward(const cs_worlds* w, float T, const float* d_global_time, const float* reward_cfg /* host, 5 floats */,
                               float* d_out, void* stream);

/*
 * cs_update_humans_rk45  replaces MotionModelManager(runge_kutta=True).update_humans(t, dt) (motion_model_manager.py:374-384):
 *   scipy.integrate.solve_ivp(f_rk45_headed | f_rk45_not_headed, (t, t + dt), y0, method='RK45') of every world, i.e. the
 *   Dormand-Prince 5(4) pair with scipy's step-size control (rtol 1e-3, atol 1e-6, error norm over the whole world) around a
 *   right-hand side with side effects (:500-550, :437-460): trial states are written with the speed clamp / angle wrap, goal
 *   lists rotate at trial positions, the single-agent force functions of forces.py are used (with the pair force of the
 *   lower index mirrored onto the higher one under CS_ALL_PARAMS_EQUAL, forces.py:130-151).
 *   type 0..8; rows <= 64.  The robot row (CS_ROBOT_ROW) is a fixed entity for the whole call.
 *   d_memory [W][n][2]: agent.desired_force between calls (kept within one radius of the goal, forces.py:12-16); zero it
 *   when the humans are created.  d_nfev [W] or NULL: number of right-hand-side evaluations (2 + 6 per attempted step).
 *   Updates rows (x, y, yaw, Vx, Vy, BVx, BVy, Omega, goal columns) and rotates d_goals in place.
 */
int cs_update_humans_rk45(const cs_worlds* w, float dt, float* d_memory, int32_t* d_nfev, void* stream);
/*   With CS_RESPAWN the parallel-traffic respawn rule runs behind the solve, as update_humans(post_update=True) does on the agent
 *   objects (motion_model_manager.py:405-422, the non-parallel form: positions and goal lists; max over radius + safety space).
 *
 * cs_complete_rk45_simulation  replaces MotionModelManager.complete_rk45_simulation(t, dt, final_time) (motion_model_manager.py:461-498):
 *   ONE solve_ivp(f_rk45_*, (t, t + final_time), y0, method='RK45', t_eval=np.arange(t, final_time, dt)) per world -- the same
 *   right-hand side and step-size control as cs_update_humans_rk45, the solution at the n_eval = len(arange(t, final_time, dt)) times
 *   k * dt taken from scipy's RK45 dense output (rk.py RkDenseOutput: y_old + h Q [x, x^2, x^3, x^4], Q = K^T P) of the step that
 *   contains them.  d_human_states [W][n_eval][n][6] (x, y, yaw, BVx, BVy, Omega: headed types) or [..][4] (x, y, Vx, Vy): the raw
 *   solution components, as the reference returns them.  The rows of w->d_state are left at the state of t + final_time.
 *
 * cs_robot_model_rk45  replaces MotionModelManager.update_robot(t, dt) for a robot whose SFM / HSFM motion model was set with
 *   runge_kutta=True (motion_model_manager.py:631-640, f_rk45_robot_* :661-687): scipy's RK45 around compute_robot_forces (:591-613,
 *   the single-agent force functions; the humans stand still during the solve).  Arguments as cs_robot_model_step; robot_type 0..8;
 *   up to 64 humans per world.  d_nfev [W] or NULL.
 */
int cs_complete_rk45_simulation(const cs_worlds* w, float dt, float final_time, float* d_memory, float* d_human_states, int n_eval,
                                int32_t* d_nfev, void* stream);
int cs_robot_model_rk45(const cs_worlds* w, int32_t robot_type, const float* robot_params, float robot_margin, const float* d_human_margin,
                        float* d_robot_memory, float dt, int32_t* d_nfev, void* stream);

/*
 * cs_gym_bookkeeping  the host bookkeeping of SocialNavGym between two steps, for W worlds on the device (one lane per world):
 *   typed copies of cs_collision_reward's rows (d_out [W][7] -> d_reward [W], d_terminated / d_truncated [W] bytes 0 / 1,
 *   d_info [W]); the per-world step counter and global_time = clock[counter] (social_nav_gym.py:244 accumulates time_step in
 *   float32: the caller tabulates those sums in d_clock [clock_len]); with auto_reset, d_mask [W] = episode ended, the counter
 *   of such a world restarts at 0 and its seed moves on by seed_stride (the next unused seed of its arithmetic sequence) -- the inputs
 *   of the masked cs_generate_worlds that follows.
 */
int cs_gym_bookkeeping(int W, const float* d_out, int32_t* d_counter, uint32_t* d_seeds, int32_t* d_mask, float* d_global_time,
                       const float* d_clock, int clock_len, int auto_reset, float* d_reward, uint8_t* d_terminated,
                       uint8_t* d_truncated, int32_t* d_info, uint32_t seed_stride /* 0 = W */, void* stream);

/*
 * cs_gym_observe  replaces SocialNavGym.compute_humans_observable_state (social_nav_gym.py:100-105: the list of
 *   human.get_observable_state() / get_observable_state_headed(), agent.py:247-253) for W worlds: d_obs [W][n][5] rows
 *   px, py, vx, vy, radius, or [W][n][7] with theta, omega appended when theta_and_omega_visible.
 * cs_copy_worlds_masked  the second half of a masked auto-reset: the worlds with d_mask[w] != 0 are copied from `src` (a staging
 *   batch cs_generate_worlds filled, possibly on another stream beside cs_step) over those of `dst`: state rows, goal lists,
 *   robot rows, world flags.  Both descriptors have the same shape and layout.
 * With cs_collision_reward, cs_gym_bookkeeping, cs_step and cs_generate_worlds these make a whole vectorised Gym step a
 * sequence of library launches with fixed arguments: capture it once (cs_graph_begin_capture), replay it per step.
 */
int cs_gym_observe(const cs_worlds* w, int theta_and_omega_visible, float* d_obs, void* stream);
int cs_copy_worlds_masked(const cs_worlds* src, const cs_worlds* dst, const int32_t* d_mask, void* stream);
/* the same with the generator's per-world status (cs_generate_worlds d_status): a world whose generation failed (status != 0: the
 * bounded rejection sampling gave up, or the traffic is too dense) is NOT copied over the live one -- the caller sees the status. */
int cs_copy_worlds_masked_status(const cs_worlds* src, const cs_worlds* dst, const int32_t* d_mask, const int32_t* d_status, void* stream);

/*
 * cs_step_observe  cs_step followed by cs_gym_observe in ONE launch: the SFM / HSFM step kernels write the observation of the stepped
 *   humans from their registers (other crowd models and worlds beyond one block: the two launches).  d_obs as in cs_gym_observe.
 * cs_copy_worlds_masked_observe  cs_copy_worlds_masked_status that also rewrites the observation rows of the worlds it copies (d_obs
 *   [W][n][5|7], NULL: plain copy) -- with cs_step_observe a vectorised Gym step with auto-reset needs no separate observation launch.
 */
int cs_step_observe(const cs_worlds* w, float dt, int n_substeps, const float* d_action, int theta_and_omega_visible, float* d_obs,
                    void* stream);
int cs_copy_worlds_masked_observe(const cs_worlds* src, const cs_worlds* dst, const int32_t* d_mask, const int32_t* d_status,
                                  int theta_and_omega_visible, float* d_obs, void* stream);

/*
 * cs_gym_bookkeeping_next_step  cs_gym_bookkeeping for Gymnasium's NEXT_STEP autoreset mode: a world whose episode ended in the
 *   previous step (d_prev_mask[w] != 0) spends this step being reset -- its results are those of a reset step (reward 0, not
 *   terminated, not truncated, Nothing), its step counter and clock restart -- and a world that ends now is flagged in d_mask
 *   and moves to the next seed of its sequence; its replacement can then be generated BESIDE the next step (cs_generate_worlds
 *   into a staging batch on another stream) and copied in at that step's end (cs_copy_worlds_masked), off the critical path.
 */
int cs_gym_bookkeeping_next_step(int W, const float* d_out, int32_t* d_counter, uint32_t* d_seeds, int32_t* d_mask, const int32_t* d_prev_mask,
                                 float* d_global_time, const float* d_clock, int clock_len, float* d_reward, uint8_t* d_terminated,
                                 uint8_t* d_truncated, int32_t* d_info, uint32_t seed_stride /* 0 = W */, void* stream);

/*
 * cs_collision_reward_gym  cs_collision_reward and the episode bookkeeping behind it in ONE launch (the lane that writes a world's
 *   reward row also does that world's bookkeeping): what cs_collision_reward + cs_gym_bookkeeping (book->d_prev_mask == NULL) or
 *   cs_collision_reward + cs_gym_bookkeeping_next_step (d_prev_mask given) leave behind, bit for bit, with one graph node less on
 *   the critical path of a vectorised Gym step (a dependent kernel node costs ~8 us in a HIP graph replay).  d_global_time is
 *   read (time-limit test) and then advanced.  Worlds of more than 64 humans take the two launches.
 */
typedef struct cs_gym_book {
    int32_t* d_counter;          /* [W] steps of the running episode */
    uint32_t* d_seeds;           /* [W] seed of the running episode: += seed_stride when the episode ends */
    int32_t* d_mask;             /* [W] out: episode ended in this step */
    const int32_t* d_prev_mask;  /* [W] NEXT_STEP mode: worlds being reset during this step; NULL: same-step rules */
    const float* d_clock;        /* [clock_len] float32 sums of the time step */
    int32_t clock_len;
    int32_t auto_reset;          /* same-step rules: restart counter / advance seed of finished worlds */
    float* d_reward;             /* [W] typed copies of the reward row */
    uint8_t* d_terminated;
    uint8_t* d_truncated;
    int32_t* d_info;
    uint32_t seed_stride;        /* what a finished world's seed moves on by: the number of worlds of the WHOLE job, so that world w walks
                                  * s + w + k * total on any rank count (ShardedBatchedSocialNavGym); 0 = W, the single-process batch */
} cs_gym_book;
int cs_collision_reward_gym(const cs_worlds* w, const float* d_action, float T, float* d_global_time,
                            const float* reward_cfg /* host, 5 floats */, float* d_out, const cs_gym_book* book, void* stream);

/*
 * cs_gym_step  cs_collision_reward_gym followed by cs_step_observe -- the head and the body of SocialNavGym.step (social_nav_gym.py:
 *   227-250: reward / termination of the CURRENT state, then the substeps, then the observation) -- in ONE launch: the step kernel's
 *   prologue computes the swept robot-human distances of the incoming rows, writes the reward row and does the episode bookkeeping
 *   (the very code of cs_collision_reward_gym, bit for bit), then runs the fused substeps and writes the observation from its registers.
 *   One launch and one graph node less on the critical path of a vectorised Gym step.  SFM / HSFM worlds of up to 64 rows on the LDS
 *   kernel; every other world: the two launches, internally.  Arguments as the two calls'.
 */
int cs_gym_step(const cs_worlds* w, float dt, int n_substeps, const float* d_action, float T, float* d_global_time,
                const float* reward_cfg /* host, 5 floats */, float* d_out, const cs_gym_book* book, int theta_and_omega_visible,
                float* d_obs, void* stream);

/*
 * Pre-staged episodes: the reset of a finished world (SocialNavGym.reset, social_nav_gym.py:120-225: seed -> generator -> rows) taken
 * off the critical path of a vectorised Gym step.  A world's episodes are a function of their seeds, and the seeds are known ahead:
 * episode e of world w draws d_base_seed[w] + e * seed_stride.  So every world keeps its next `depth` episodes generated ahead in a
 * staging batch of depth * W worlds (slot j of world w = staging world j * W + w holds the one episode e in (epoch, epoch + depth] with
 * e = j mod depth); an episode end is then a copy, and the consumed slots are regenerated on a side stream, several steps later, without
 * anybody waiting for them -- a world that ends a few steps after its reset (a robot driven into its neighbour) finds the following
 * episodes staged as well.  No event orders the two streams: the slots carry tags.
 *   d_staged_seed[j][w]  the seed slot j of world w was generated from -- stored LAST by the generator (release, device scope)
 *   d_epoch[w]           the episode the live world w is in (0 after reset) -- stored LAST by the consumer, once every load of the slot
 *                        has returned (relaxed, device scope; the obligations of the protocol are listed in csrc/generate.hip)
 * cs_refill_staged_worlds   (side stream) regenerates every slot whose tag differs from the seed of the episode that belongs in it now
 *   (one wavefront per slot; the other blocks leave at once); d_staged_status[j][w] = cs_generate_worlds' status.  Launches of it must
 *   be ordered among themselves (one stream).  n <= 64.
 * cs_consume_staged_worlds  (the step's stream, behind the substeps) for every world with d_mask[w] != 0: episode e = epoch + 1; if the
 *   tag of slot e mod depth (a device-scope relaxed load; the slot's words are read with device-scope loads under a control dependency
 *   on it) equals d_seeds[w] -- the seed the bookkeeping just moved the world to -- the staged world is copied
 *   over the live one, observation rows included (cs_copy_worlds_masked_observe); if the refill has not got to it yet the world is
 *   generated in place from d_seeds[w] by the same generator code: the same rows either way, a function of the seed.
 *   A world that cannot be generated (status != 0) keeps its rows and gets d_failed[w] = 1 (0 after a successful reset): it starts a new
 *   episode FROM its finished rows (step counter and clock were reset by the bookkeeping) -- after a collision or a reached goal it ends
 *   again at the next step and then tries the following seed of its sequence; after a time-limit truncation it runs a further episode
 *   from where it stands, flagged in d_failed the whole time.
 */
typedef struct cs_stage_book {
    const uint32_t* d_seeds;      /* [W] cs_gym_book.d_seeds: == d_base_seed + d_epoch * seed_stride between two steps */
    const uint32_t* d_base_seed;  /* [W] seed of episode 0 */
    uint32_t* d_epoch;            /* [W] */
    uint32_t* d_staged_seed;      /* [depth][W] */
    int32_t* d_staged_status;     /* [depth][W] */
    int32_t* d_failed;            /* [W] 0 = the last take-over succeeded, 1 = the staged episode could not be generated, 2 = deferred (cs_gym_step_staged) */
    uint32_t seed_stride;         /* 0 = W */
    int32_t depth;                /* episodes staged ahead per world: a power of two */
    int32_t* d_pending;           /* [W] cs_gym_step_staged only (may be NULL otherwise): 1 = the world's episode is over and its take-over deferred */
} cs_stage_book;
/* `staging` describes depth * W worlds of the shape of the live batch (same n, G, layout, robot row) */
int cs_refill_staged_worlds(const cs_generator* gen, const cs_worlds* staging, const cs_stage_book* book, void* stream);
int cs_consume_staged_worlds(const cs_generator* gen, const cs_worlds* staging, const cs_worlds* live, const int32_t* d_mask,
                             const cs_stage_book* book, int theta_and_omega_visible, float* d_obs, void* stream);

/* cs_gym_step followed by cs_consume_staged_worlds in ONE launch (SocialNavGym.step + the reset of the worlds that ended,
 * social_nav_gym.py:227-250, :120-225): the head of the step kernel decides which worlds take over their staged episode at the end of this
 * launch -- same-step rules (book->auto_reset): the worlds that end now; NEXT_STEP rules (book->d_prev_mask): those that ended in the
 * previous step -- and the wavefront that stepped such a world copies the staged episode over it (rows, goal lists, robot row, world
 * flag, observation rows) instead of writing the stepped rows.  Same results as the two launches, bit for bit, whenever the slot is staged.
 * A slot the refill has NOT staged yet is not generated in place (cs_consume_staged_worlds does that): the take-over is DEFERRED --
 * d_pending[w] = 1, d_failed[w] = 2, the world is between two episodes (reward 0, no flags, observation of its finished rows) until a later
 * cs_gym_step_staged finds the slot.  With the refill cadence of social_gym/social_nav_gym.py (a pass whenever a world may have ended, `depth`
 * episodes ahead) that does not happen.  Only for worlds cs_gym_step runs as one launch (cs_gym_step_is_one_launch: SFM / HSFM worlds of
 * up to 64 rows on the one-wavefront builds) and without polygon walls; CS_ERR_ARG otherwise -- take the two launches there.
 * cs_gym_step_is_one_launch: 0 = cs_gym_step is two launches for these worlds, 1 = one launch, 2 = one launch and cs_gym_step_staged too. */
int cs_gym_step_is_one_launch(const cs_worlds* w);
int cs_gym_step_staged(const cs_worlds* w, float dt, int n_substeps, const float* d_action, float T, float* d_global_time, const float* reward_cfg,
                       float* d_out, const cs_gym_book* book, int theta_and_omega_visible, float* d_obs, const cs_generator* gen,
                       const cs_worlds* staging, const cs_stage_book* stage_book, void* stream);

/*
 * cs_policy_no_train  the CrowdNav baseline robot policies that need no training (crowd_nav/policy_no_train/: blind_planner.py,
 *   simple_social_planner.py, sfm_helbing.py, sfm_guo.py, sfm_moussaid.py with forces.py) -- Policy.predict(JointState) for the robots
 *   of W worlds in one launch.  d_robot13 [W][13] robot safe-state rows (cs_worlds.d_robot: x, y, yaw, Vx, Vy, BVx, BVy, Omega, radius,
 *   mass, gx, gy, v_pref); d_obs [W][n][obs_cols] observation rows (cs_gym_observe: px, py, vx, vy, radius[, theta, omega]; obs_cols 5 or
 *   7); d_action [W][2] out: ActionXY (vx, vy).  time_step: the policy's (ROBOT_SAMPLING_TIME in the simulator); only the social-force
 *   policies read it.  params (host, CS_PNT_N_PARAMS floats, read before the call returns): the policy's own dict packed into the 20
 *   agent.py slots [relax_t, Ai, Aw, Bi, Bw, Ci, Cw, Di, Dw, Ei, k1, k2, a_lambda, gamma, ns, ns1, ko, kd, alpha, k_lambda] and its
 *   mass in slot CS_PNT_MASS; required by the social-force policies, ignored (may be NULL) by bp / ssp.
 *   Errors (CS_ERR_ARG, before any device call): unknown policy id, W < 1, n < 0, obs_cols not 5 or 7, null pointers.
 */
enum { CS_PNT_BP = 0, CS_PNT_SSP = 1, CS_PNT_SFM_HELBING = 2, CS_PNT_SFM_GUO = 3, CS_PNT_SFM_MOUSSAID = 4 };
enum { CS_PNT_MASS = 20, CS_PNT_N_PARAMS = 21 };
int cs_policy_no_train(int policy, int W, int n, const float* d_robot13, const float* d_obs, int obs_cols, float time_step,
                       const float* params /* host, CS_PNT_N_PARAMS floats */, float* d_action, void* stream);

/*
 * cs_policy_orca  the CrowdNav ORCA robot policy (crowd_nav/policy_no_train/orca.py:82-132, ORCA.predict) for the robots of W worlds in
 *   one launch: one doStep of a fresh RVO2 simulator in which the robot is agent 0 and human j agent j + 1, of which only agent 0's new
 *   velocity is read.  d_robot13 / d_obs / obs_cols / d_action as cs_policy_no_train's.  Agent 0 has radius `radius + margin` and
 *   maxSpeed v_pref; human j has radius `radius_j + margin` (margin = float32(0.01 + safety_space), added in float32).  Preferred
 *   velocity: d = goal - position, s = sqrt(d.x * d.x + d.y * d.y), d / s where s > 1 (strict; an IEEE division), d otherwise.
 *   Neighbours: the humans with distSq < neighbor_dist^2 (strict), the first max_neighbors of them in ascending (distSq, index) order --
 *   the list RVO2's insertion leaves after a walk in index order; one half-plane each in that order (a colliding pair uses
 *   1 / time_step instead of 1 / time_horizon), linearProgram2, linearProgram3 where that is infeasible.  Exact arithmetic only (IEEE
 *   divide and square root, no contraction): bit for bit what oracle/orca_oracle.c computes for agent 0, for a world alone (W = 1) and
 *   in any batch.  Parity with the rvo2 library itself is unpinned, as for every ORCA path here.  One launch of
 *   k_policy_orca on `stream` (a wavefront per world, lanes over humans); only d_action is written.
 *   Errors (CS_ERR_ARG with a message, before any device call): W < 1, n < 0, obs_cols not 5 or 7, a null d_robot13 or d_action, a null
 *   d_obs with n > 0, time_step <= 0, time_horizon <= 0, neighbor_dist < 0, max_neighbors outside 0..10 (the kernel keeps at most ten
 *   neighbours; the reference's value is 10).
 */
int cs_policy_orca(int W, int n, const float* d_robot13, const float* d_obs, int obs_cols, float time_step, float neighbor_dist,
                   int max_neighbors, float time_horizon, float margin, float* d_action, void* stream);

/*
 * cs_gym_step_policycs_policy_no_train followed by cs_gym_step -- `action = robot.act(ob); ob, reward, done, info = env.step(action)`, the
 *   seam of Explorer.run_k_episodes (crowd_nav/utils/explorer.py:57-58) with a robot of crowd_nav/policy_no_train/ (*.py) -- in ONE launch: the
 *   step kernel's prologue decides every world's ActionXY from the rows it has loaded (the robot row of cs_worlds.d_robot and the humans'
 *   state rows: the values cs_policy_no_train reads from d_robot13 and from the observation rows), BEFORE the Gym head, the swept collision
 *   test and the robot's advance consume it; the decided action is also stored to d_action [W][2] (out: no action row is read).  Bit for
 *   bit what the two calls leave, in every buffer.  Arguments as cs_gym_step's, then policy / policy_time_step / policy_params as
 *   cs_policy_no_train's policy / time_step / params.  One launch for the worlds cs_gym_step runs as one launch on the plain crowd
 *   batch's builds without walls (all_params_equal, <= 2 goal slots; 25 humans, 25 or 5 humans + a visible robot, and every row count of
 *   the run-time partner loop); everywhere else (ORCA, social momentum, walls, the DPP-row kernel's small worlds, the grid path) the
 *   decision kernel and the Gym step's launches follow each other on `stream` inside this call: one entry, the same results.
 *   d_obs must hold the current observation (cs_gym_observe / the previous step's) -- the worlds of the second kind decide from it.
 *   Errors (CS_ERR_ARG, before any device call): unknown policy id, policy_time_step <= 0, a unicycle batch (CS_ROBOT_UNICYCLE: the
 *   policies act in ActionXY), cs_worlds.d_robot null, d_action null, a social-force policy without parameters, null cs_gym_book buffers.
 * cs_gym_step_staged_policy  the same in front of cs_gym_step_staged (its arguments, its conditions and its errors; then the three policy
 *   arguments): decision, reward, bookkeeping, substeps, observation and the take-over of the staged episodes in ONE launch.
 * cs_gym_step_policy_variant  which kernels cs_gym_step_policy runs for these worlds: "k_sfm_step<...,LEAN=8+k> ... (policy decided in the
 *   head)" for the one launch, "k_policy_no_train + " and cs_step_variant's answer otherwise (the tests assert which build they compared).
 */
int cs_gym_step_policy(const cs_worlds* w, float dt, int n_substeps, float* d_action, float T, float* d_global_time,
                       const float* reward_cfg /* host, 5 floats */, float* d_out, const cs_gym_book* book, int theta_and_omega_visible,
                       float* d_obs, int policy, float policy_time_step, const float* policy_params /* host, CS_PNT_N_PARAMS floats */,
                       void* stream);
int cs_gym_step_staged_policy(const cs_worlds* w, float dt, int n_substeps, float* d_action, float T, float* d_global_time,
                              const float* reward_cfg, float* d_out, const cs_gym_book* book, int theta_and_omega_visible, float* d_obs,
                              const cs_generator* gen, const cs_worlds* staging, const cs_stage_book* stage_book, int policy,
                              float policy_time_step, const float* policy_params, void* stream);
int cs_gym_step_policy_variant(const cs_worlds* w, char* buf, size_t buflen);

/*
 * cs_value_net_decide  the decision of the trained value-based robots for W worlds: the per-action model() loop, compute_action_value
 *   and the arg-max of CADRL.predict (crowd_nav/policy/cadrl.py:264-273, :85-90: value_network on every (action, human) row, minimum over
 *   the humans) and of MultiHumanRL.predict with SARL's network (crowd_nav/policy/multi_human_rl.py:52-63, crowd_nav/policy/sarl.py:28-65:
 *   mlp1 -> mlp2, attention on (mlp1, mean of mlp1) or on mlp1 alone, the masked softmax exp(s) * (s != 0) normalised, mlp3 on (the first
 *   six columns of the first human's row, the weighted feature)), with reach_destination (cadrl.py:244).  Reads cs_lookahead's output:
 *   d_rotated [W][A][n][cols] (cols 13 or 15), d_rewards [W][A]; d_actions [A][2]; d_robot [W][robot_stride] as cs_lookahead takes it
 *   (px, py, vx, vy, radius, gx, gy, v_pref, ...).  Writes d_values [W][A] = reward + gamma^(dt * v_pref) * V, d_choice [W] (may be
 *   NULL) = the first maximum of a world's values (np.argmax), or d_override[w] where that is in 0..A-1 (d_override may be NULL; -1 =
 *   greedy: the caller's epsilon-greedy draw), and d_action_out [W][2] = the chosen action, (0, 0) for a robot within its radius of its
 *   goal.  float32 on the f32-input matrix instructions; the activations of a row tile stay in LDS from the input columns to the value;
 *   a (world, action) gives the same bits for W = 1 as inside any batch.  Two kernels on `stream`: the network, then the per-world pick.
 *
 *   The network is described by `dims` (host):  CS_VN_CADRL: [L, w_1 .. w_L] (the output widths of value_network's Linear layers,
 *   w_L = 1);  CS_VN_SARL: [with_global_state, L1, mlp1 widths.., L2, mlp2 widths.., La, attention widths.., L3, mlp3 widths..]
 *   (attention and mlp3 end in 1).  ReLU follows every layer but a chain's last, and mlp1's last too.  Widths 1..256, at most 16 layers.
 *   d_weights is the blob cs_value_net_pack writes, n_weight_floats its length.
 * cs_value_net_pack  (host only, no device) lays the Linear layers out for the kernel: params[2 l] = weight of layer l ([out][in], row
 *   major, as torch.nn.Linear holds it), params[2 l + 1] = its bias, layers in the order of `dims`.  blob == NULL: only *n_floats is set.
 *   Errors of both (CS_ERR_ARG, before any device call): unknown kind, cols not 13 or 15, a width outside 1..256, a malformed `dims`,
 *   n < 1, W or A < 1, null pointers, a blob of another size, a network whose tile does not fit the LDS.
 */
enum { CS_VN_CADRL = 0, CS_VN_SARL = 1 };
int cs_value_net_pack(int kind, const int32_t* dims, int n_dims, int cols, const float* const* params, float* blob, size_t* n_floats);
int cs_value_net_decide(int kind, const int32_t* dims, int n_dims, const float* d_weights, size_t n_weight_floats, int W, int A, int n,
                        int cols, const float* d_rotated, const float* d_rewards, const float* d_actions, const float* d_robot,
                        int robot_stride, float gamma, float dt, const int32_t* d_override, float* d_values, int32_t* d_choice,
                        float* d_action_out, void* stream);

/*
 * cs_value_net_decide_bf16  the same decision with the opt-in bf16 arithmetic (csrc/value_net_bf16.hip): the arguments,
 *   results, errors and messages of cs_value_net_decide, with d_weights the blob cs_value_net_pack_bf16 writes and n_weight_bytes its
 *   length in bytes; the LDS-fit check is made for this entry's own tile buffers.  A layer whose input holds raw rotated-state columns
 *   (CADRL value_network layer 0, SARL mlp1 layer 0, all of mlp3) stays float32; every other layer runs on v_mfma_f32_32x32x16_bf16
 *   with bf16 weights (rounded to nearest even at pack time), float32 biases and float32 accumulation in a fixed k order.  An
 *   activation is rounded to bf16 once, when it is stored as the operand of a bf16 layer (after bias and ReLU); what a reduction
 *   consumes (attention scores, mlp2 features, CADRL's per-human value) is not rounded; the crowd mean is summed in float32 from the
 *   rounded mlp1 outputs and rounded once.  Softmax, minimum, weighted sum, the action value and the pick are cs_value_net_decide's.
 *   A (world, action) gives the same bits for W = 1 as inside any batch.
 * cs_value_net_pack_bf16  (host only) params as cs_value_net_pack; blob == NULL: only *n_bytes is set.  Layout, layer after layer in
 *   the order of `dims`, every offset a multiple of 16 bytes:
 *     a float32 layer   as cs_value_net_pack lays it out: float [ncb][kg][64 lanes][4] with ncb = ceil(N / 32) column blocks and kg =
 *                       ceil(K / 8) k-groups -- lane l holds Wt[k = 8 g + 4 (l >> 5) + s][column 32 cb + (l & 31)], s = 0..3 --, then
 *                       float bias[32 ncb];
 *     a bf16 layer      bfloat16 [ncb][ks][64 lanes][8] with ks = ceil(K1 / 16) + ceil(K2 / 16) k-steps (K2: the attention's
 *                       crowd-mean half, its k-steps behind the first source's) -- lane l holds Wt[k = 16 s + 8 (l >> 5) + e][column
 *                       32 cb + (l & 31)], e = 0..7, of k-step s --, then float bias[32 ncb].
 *   Weights and biases beyond N or K are zero.
 */
int cs_value_net_pack_bf16(int kind, const int32_t* dims, int n_dims, int cols, const float* const* params, void* blob, size_t* n_bytes);
int cs_value_net_decide_bf16(int kind, const int32_t* dims, int n_dims, const void* d_weights, size_t n_weight_bytes, int W, int A, int n,
                             int cols, const float* d_rotated, const float* d_rewards, const float* d_actions, const float* d_robot,
                             int robot_stride, float gamma, float dt, const int32_t* d_override, float* d_values, int32_t* d_choice,
                             float* d_action_out, void* stream);

/*
 * cs_value_net_decide_worlds  cs_lookahead followed by cs_value_net_decide as ONE entry point, without the look-ahead tensor
 *   (csrc/value_net_worlds.hip): the network kernel generates a tile's input rows in LDS from the worlds' own rows, so
 *   rotated [W][A][n][13|15] -- an A-fold expansion of its inputs, 431 MB at 4096 worlds x 81 actions x 25 humans -- is never written.
 *   d_actions [A][2], d_next [W][n][4|6], d_current [W][n][5|7], d_robot [W][robot_stride], robot_stride and dt are exactly what
 *   cs_lookahead takes; kind, dims, d_weights (cs_value_net_pack's blob for cols = 13, or 15 with theta_and_omega_visible), gamma,
 *   d_override, d_values, d_choice and d_action_out exactly what cs_value_net_decide takes.  d_rewards_out (may be NULL) receives
 *   [W][A], the rewards the kernel computed.  d_values, d_choice, d_action_out and d_rewards_out are, bit for bit, those of
 *   cs_lookahead followed by cs_value_net_decide on the same inputs; a (world, action) gives the same bits for W = 1 as inside any
 *   batch.  Device memory touched: the inputs above, the blob, and one float per (world, action) (two with d_rewards_out).  Two kernels
 *   on `stream`: the network, then the per-world pick.  Errors (CS_ERR_ARG, before any device call): those of cs_value_net_decide and
 *   of cs_lookahead with their messages (d_next and d_current are required; robot_stride >= 8); the LDS-fit check is made for this
 *   kernel's own LDS (the tile buffers and a table of 32 x 8 floats).
 */
int cs_value_net_decide_worlds(int kind, const int32_t* dims, int n_dims, const float* d_weights, size_t n_weight_floats, int W, int A, int n,
                               int theta_and_omega_visible, const float* d_actions, const float* d_next, const float* d_current,
                               const float* d_robot, int robot_stride, float gamma, float dt, const int32_t* d_override,
                               float* d_rewards_out /* may be NULL */, float* d_values, int32_t* d_choice, float* d_action_out, void* stream);

/*
 * cs_value_net_state  the value network on the worlds' CURRENT state, for a trainer (csrc/value_net_state.hip): what
 *   policy.transform hands to a replay memory (crowd_nav/policy/multi_human_rl.py:115-128 -> cadrl.py rotate) and the target value
 *   reward + gamma^(time_step * v_pref) * V(state) (crowd_nav/utils/explorer.py:120-153), for W worlds in one kernel on `stream`.
 *   d_current [W][n][5|7] (px, py, vx, vy, radius [, theta, omega]) and d_robot [W][robot_stride] (px, py, vx, vy, radius, gx, gy,
 *   v_pref, ...) are what cs_lookahead takes; kind, dims and d_weights (cs_value_net_pack's float32 blob for cols = 13, or 15 with
 *   theta_and_omega_visible) what cs_value_net_decide takes.  A world's n rows are, by definition and bit for bit, cs_lookahead's rows
 *   for the one action (robot vx, vy), dt = 0 and d_next = the humans' current (px, py, vx, vy | px, py, theta, vx, vy, omega).
 *   d_rotated_out (may be NULL) receives them, dense [W][n][13|15].  d_values [W] = d_rewards[w] + gamma^(dt * v_pref[w]) * V(w), with
 *   V the network's output on the world's rows (CADRL: the minimum over the humans) exactly as cs_value_net_decide computes it on such
 *   rows; d_rewards may be NULL (0): with it NULL and dt = 0 the value is the network's output itself.  A world gives the same bits
 *   for W = 1 as inside any batch.  float32 only.  Device memory touched: the inputs, the blob, d_values, d_rotated_out.
 *   Errors (CS_ERR_ARG, before any device call): those of cs_value_net_decide's network description with their messages, W < 1,
 *   n < 1, a null d_weights, d_current, d_robot or d_values, a blob of another size, robot_stride < 8, a network whose tile buffers
 *   (with this kernel's table of 32 x 8 floats) do not fit the LDS.
 */
int cs_value_net_state(int kind, const int32_t* dims, int n_dims, const float* d_weights, size_t n_weight_floats, int W, int n,
                       int theta_and_omega_visible, const float* d_current, const float* d_robot, int robot_stride,
                       const float* d_rewards /* may be NULL */, float gamma, float dt, float* d_rotated_out /* may be NULL */,
                       float* d_values, void* stream);

/*
 * cs_value_net_loss_grad  one optimisation step's loss and gradient for a CADRL / SARL network, fused (csrc/value_net_grad.hip, DESIGN.md
 *   4.5): what crowd_nav/utils/trainer.py:50-71 does per minibatch before optimizer.step() -- zero_grad, outputs = model(inputs), loss =
 *   MSELoss(outputs, values), loss.backward() -- for the networks of crowd_nav/policy/sarl.py:28-65 (mlp1, the crowd mean, the attention
 *   chain, the masked softmax, mlp2's weighted sum, mlp3) and crowd_nav/policy/cadrl.py:116-123 (value_network), in two launches on
 *   `stream`.  kind, dims, d_weights are what cs_value_net_decide takes (cs_value_net_pack's float32 blob for `cols`).  d_params holds
 *   the same parameters flat, in torch's own layout: for every layer in dims' order weight [N][K] row-major, then bias [N]
 *   (n_param_floats: cs_value_net_grad_sizes).  d_rows [B][n][cols] are B stored states (policy.transform's rows, the humans in their own
 *   order; cols 13 or 15), d_targets [B] their target values.  CADRL's trainer stores one human's row per sample: n must be 1 for it.
 *   d_grad (the layout of d_params; written, not accumulated) = d/dtheta mean_b (V_b - target_b)^2, d_loss the loss, d_values [B] (may be
 *   NULL) the network's outputs: bit for bit what cs_value_net_state returns for such rows with d_rewards NULL and dt 0.  d_scratch of
 *   n_scratch_floats (at least cs_value_net_grad_sizes' figure) holds one partial gradient per workgroup, summed in a fixed order: no
 *   atomics, the same call gives the same bytes; the bits may depend on B.  float32.
 *   Errors (CS_ERR_ARG, before any device call): those of cs_value_net_decide's network description, B < 1, n < 1, CADRL with n > 1,
 *   a null pointer other than d_values, a blob or parameter array of another size, a scratch that is too small, a network whose
 *   tile (every layer's activations of 32 rows and two gradient buffers) does not fit the 160 KiB of LDS.
 * cs_value_net_grad_sizes  (host only) the lengths of d_params and of d_scratch for such a call, in floats.
 * cs_value_net_pack_device  cs_value_net_pack on the device, one launch on `stream`: d_blob (n_blob_floats = cs_value_net_pack's figure)
 *   from the flat d_params, byte for byte what cs_value_net_pack writes for the same numbers, zero padding included -- the refresh after
 *   every optimiser step of trainer.py:50-71 without a host round trip.
 */
int cs_value_net_grad_sizes(int kind, const int32_t* dims, int n_dims, int cols, int B, int n, size_t* n_param_floats, size_t* n_scratch_floats);
int cs_value_net_loss_grad(int kind, const int32_t* dims, int n_dims, const float* d_weights, size_t n_weight_floats, const float* d_params,
                           size_t n_param_floats, int B, int n, int cols, const float* d_rows, const float* d_targets, float* d_grad,
                           float* d_loss, float* d_values /* may be NULL */, float* d_scratch, size_t n_scratch_floats, void* stream);
int cs_value_net_pack_device(int kind, const int32_t* dims, int n_dims, int cols, const float* d_params, size_t n_param_floats, float* d_blob,
                             size_t n_blob_floats, void* stream);

/*
 * cs_value_net_train_step  one whole optimisation step of trainer.py:50-71 for a CADRL / SARL network in two launches on `stream`:
 *   cs_value_net_loss_grad's job kernel, unchanged, then one kernel (csrc/value_net_grad.h k_vn_sgd) that per parameter i of
 *   the flat layout sums the workgroups' partial gradients in their fixed order -- d_grad, d_loss and d_values receive the bytes
 *   cs_value_net_loss_grad gives for the same inputs --, takes torch.optim.SGD's step with momentum (dampening 0, no Nesterov, no weight
 *   decay): d_momentum[i] = momentum * d_momentum[i] + d_grad[i], d_params[i] -= lr * d_momentum[i], each one float32 fused multiply-add,
 *   and rewrites the float of d_weights that reads parameter i: afterwards d_weights is byte for byte cs_value_net_pack's blob of the
 *   updated parameters, its zero padding untouched.  d_params and d_weights are in/out; on entry d_weights must be the blob of d_params
 *   (cs_value_net_pack_device).  d_momentum (n_momentum_floats = n_param_floats; zeros before the first step, as torch's first step
 *   takes buf = grad) is in/out.  d_loss_sum (may be NULL): a device double to which the step adds (double)*d_loss -- the float64 sum the
 *   reference's loops form on the host from loss.item(), without a read-back per minibatch.  No atomics: the same call from the same
 *   state gives the same bytes everywhere.
 *   Errors (CS_ERR_ARG, before any device call): cs_value_net_loss_grad's, a null d_momentum, a momentum buffer of another size, an lr
 *   that is not finite or negative, a momentum that is not finite or negative.
 * cs_value_net_blob_index  (host only) the map the update kernel writes the blob by, evaluated by the same code: index[i] (n_param_floats
 *   entries, cs_value_net_grad_sizes) is the float of cs_value_net_pack's blob that holds parameter i of the flat layout.  Every
 *   parameter has a float of its own; the blob's other floats are its zero padding.
 */
int cs_value_net_train_step(int kind, const int32_t* dims, int n_dims, float* d_weights, size_t n_weight_floats, float* d_params,
                            size_t n_param_floats, float* d_momentum, size_t n_momentum_floats, float lr, float momentum, int B, int n,
                            int cols, const float* d_rows, const float* d_targets, float* d_grad, float* d_loss,
                            double* d_loss_sum /* may be NULL */, float* d_values /* may be NULL */, float* d_scratch,
                            size_t n_scratch_floats, void* stream);
int cs_value_net_blob_index(int kind, const int32_t* dims, int n_dims, int cols, int32_t* index, size_t n_param_floats);

/*
 * cs_occupancy_maps OM-SARL's local occupancy maps (crowd_nav/policy/multi_human_rl.py:133-187 build_occupancy_maps) for W worlds in
 *   one kernel on `stream` (csrc/occupancy_map.hip).  d_humans [W][n][stride] holds a human's position at columns 0, 1
 *   and its velocity at vel_col, vel_col + 1: cs_lookahead's d_next [W][n][4|6] (vel_col 2 | 3) and d_current [W][n][5|7] (vel_col 2)
 *   are read in place.  d_maps [W][n][C], C = cell_num^2 * channels, laid out [cell][channel]: for centre human i and every other human j
 *   of its world, d = p_j - p_i is taken into the frame whose x axis is v_i (the world's frame when v_i = 0), its cell is
 *   cell_num * floor(y / cell_size + cell_num / 2) + floor(x / cell_size + cell_num / 2) when both indices lie in 0..cell_num-1 (a NaN
 *   lies nowhere; a coincident pair is (0, 0)).  channels 1: 1 for an occupied cell, else 0;  2: the mean of the members' velocities in
 *   that frame, (0, 0) for an empty cell;  3: (occupied, mean vx, mean vy).  The means are summed in ascending j by one lane per cell:
 *   no atomics, and a world gives the same bits for W = 1 as inside any batch.  n = 1 writes zeros.  float32.
 *   Errors (CS_ERR_ARG, before any device call): W or n < 1, null pointers, stride < 4, vel_col outside 2..stride-2, cell_num < 1,
 *   cell_size not > 0, channels outside 1..3, C > 241 (so that 15 + C <= 256, the widest layer input), W * n * C beyond an int.
 * cs_value_net_decide_om  cs_value_net_decide for OM-SARL (sarl.with_om = true; csrc/value_net_om.hip): row (w, a, j) of the network's
 *   input is d_rotated[w][a][j][0..cols) followed by d_maps[w][j][0..om_cols) -- one map row serves the A actions of its world, the
 *   maps are never expanded A-fold.  Every other argument, the results, the two kernels on `stream`, the position independence and the
 *   errors are cs_value_net_decide's, the LDS-fit check made for this kernel's own LDS (its input tile has rows of cols + om_cols rounded
 *   up to 8, plus 4 floats).  d_weights is cs_value_net_pack_om's blob.  float32, CS_VN_SARL only.  mlp3's self state is still the first
 *   six columns of the first human's row.
 * cs_value_net_pack_om  (host only) cs_value_net_pack for a SARL network whose mlp1 reads cols + om_cols columns: the same layout, the
 *   first layer with ceil((cols + om_cols) / 8) k-groups.
 *   Further errors of both (CS_ERR_ARG): kind != CS_VN_SARL, om_cols < 1, cols + om_cols > 256, a null d_maps.
 */
int cs_occupancy_maps(int W, int n, const float* d_humans, int stride, int vel_col, int cell_num, float cell_size, int channels,
                      float* d_maps /* [W][n][cell_num^2 * channels] */, void* stream);
int cs_value_net_pack_om(int kind, const int32_t* dims, int n_dims, int cols, int om_cols, const float* const* params, float* blob,
                         size_t* n_floats);
int cs_value_net_decide_om(int kind, const int32_t* dims, int n_dims, const float* d_weights, size_t n_weight_floats, int W, int A, int n,
                           int cols, int om_cols, const float* d_rotated, const float* d_maps, const float* d_rewards,
                           const float* d_actions, const float* d_robot, int robot_stride, float gamma, float dt,
                           const int32_t* d_override, float* d_values, int32_t* d_choice, float* d_action_out, void* stream);

/*
 * cs_value_net_decide_lstm  cs_value_net_decide for LSTM-RL (crowd_nav/policy/lstm_rl.py; csrc/value_net_lstm.hip): per
 *   (world, action) the n rows of d_rotated [W][A][n][cols], [mlp1 on every row,] torch.nn.LSTM(batch_first) over the rows from zero
 *   (h0, c0) -- gates = W_ih x_t + b_ih + W_hh h + b_hh in torch's order i, f, g, o; c = sigmoid(f) c + sigmoid(i) tanh(g); h =
 *   sigmoid(o) tanh(c) --, then mlp on (the first six columns of the first row in evaluation order, h_n).  sorted_by_distance = 1 is the
 *   decision's order (multi_human_rl.py:48-50): the rows sorted by column 11 descending, ties by DECREASING human index
 *   (np.flip(np.argsort(da, kind="stable"))); a NaN distance sorts first.  sorted_by_distance = 0 evaluates the rows as they lie (what a
 *   trainer's stored states ask for: A = 1, a one-row action table, d_choice NULL).  Every other argument, the results (d_values =
 *   reward + gamma^(dt * v_pref) * V, d_choice, d_override, d_action_out, reach-destination), the two kernels on `stream` and the
 *   position independence (a (world, action) gives the same bits for W = 1 as inside any batch) are cs_value_net_decide's.  float32.
 *   `dims` (host): [H, L1, mlp1 widths.., L2, mlp widths..] -- H the LSTM's hidden width 1..256; L1 = 0: no interaction module
 *   (ValueNetwork1), else mlp1 (ValueNetwork2; the LSTM reads its last width); mlp ends in 1.  ReLU follows every layer but a chain's
 *   last.  Widths 1..256, at most 16 Linear layers.  n is at most CS_VN_LSTM_MAX_N humans a world.
 * cs_value_net_pack_lstm  (host only) params in the order of `dims`: mlp1's (weight, bias) pairs; then weight_ih [4H][in], weight_hh
 *   [4H][H], bias_ih [4H], bias_hh [4H] as torch holds them; then mlp's pairs.  blob == NULL: only *n_floats is set.  Layout, one piece
 *   after the other, weights and biases beyond a width zero:
 *     every mlp1 layer  as cs_value_net_pack lays a float32 layer out (cs_value_net_pack_bf16's comment states it): float
 *                       [ncb][kg][64 lanes][4], then float bias[32 ncb];
 *     the gates         float [nb][kg][64 lanes][4] with nb = ceil(H / 8) blocks of 8 hidden units and kg = ceil(H / 8) + ceil(in / 8)
 *                       k-groups (h's, then the input's): lane l, element s of k-group g of block b holds W[row][k] with row = (j >> 3) * H +
 *                       8 b + (j & 7) for j = l & 31 (gate j >> 3 of unit 8 b + (j & 7)), W = weight_hh and k = 8 g + 4 (l >> 5) + s for
 *                       g < ceil(H / 8), else W = weight_ih and k = 8 (g - ceil(H / 8)) + 4 (l >> 5) + s; then float bias[32 nb],
 *                       bias[32 b + j] = bias_ih[row] + bias_hh[row] summed in float32;
 *     every mlp layer   as the mlp1 layers; the first reads K = 6 + H columns.
 *   Errors of both (CS_ERR_ARG, before any device call): cols not 13 or 15, H or a width outside 1..256, a malformed `dims`, more than
 *   16 layers, an mlp that does not end in 1, null pointers; of the decision also cs_value_net_decide's (W, A, n < 1, a blob of another
 *   size, robot_stride < 8), sorted_by_distance outside 0..1, n > CS_VN_LSTM_MAX_N, a network whose tile buffers do not fit the LDS.
 */
#define CS_VN_LSTM_MAX_N 128
int cs_value_net_pack_lstm(const int32_t* dims, int n_dims, int cols, const float* const* params, float* blob, size_t* n_floats);
int cs_value_net_decide_lstm(const int32_t* dims, int n_dims, const float* d_weights, size_t n_weight_floats, int W, int A, int n, int cols,
                             int sorted_by_distance, const float* d_rotated, const float* d_rewards, const float* d_actions,
                             const float* d_robot, int robot_stride, float gamma, float dt, const int32_t* d_override, float* d_values,
                             int32_t* d_choice, float* d_action_out, void* stream);

/*
 * cs_value_net_decide_lstm_bf16  cs_value_net_decide_lstm with the opt-in bf16 arithmetic (csrc/value_net_lstm_bf16.hip): the
 *   same arguments, results, errors and messages, with the blob of cs_value_net_pack_lstm_bf16 and its length in bytes.  float32 layers
 *   (full weights, unrounded inputs): network 1's weight_ih on the raw row, network 2's mlp1 layer 0, mlp's layer 0.  bf16 layers (weights
 *   rounded to bf16, nearest even, by the pack; float32 biases and accumulation): weight_hh, network 2's weight_ih, every mlp1 / mlp layer
 *   behind the first.  Rounded once, nearest even, when stored as a bf16 operand: h_t after o * tanh(c) (the next step's operand and what
 *   mlp reads as h_n), an mlp1 / mlp activation behind bias and ReLU that a bf16 layer reads, mlp1's last output.  Never rounded: c, the
 *   gate pre-activations, sigmoid, tanh, mlp's last output, the value.  A gate pre-activation is one chain: the bias, the input's part,
 *   then weight_hh's.  Position independence, the order rule, the pick and d_override are cs_value_net_decide_lstm's.
 * cs_value_net_pack_lstm_bf16  (host only) params as cs_value_net_pack_lstm takes them.  blob == NULL: only *n_bytes is set.  Layout, one
 *   piece after the other, each a whole number of floats, weights and biases beyond a width zero:
 *     mlp1's layer 0, mlp's layer 0   float32 layers as cs_value_net_pack lays them out: float [ncb][kg][64 lanes][4], float bias[32 ncb];
 *     every other mlp1 / mlp layer    as cs_value_net_pack_bf16 lays a bf16 layer out: bf16 [ncb][ks][64 lanes][8] with ncb = ceil(N / 32),
 *                       ks = ceil(K / 16): lane l, element e of k-step s of block b holds weight[32 b + (l & 31)][16 s + 8 (l >> 5) + e];
 *                       then float bias[32 ncb];
 *     the gates (between mlp1's layers and mlp's)   [nb][ksh + ksx][64 lanes] slots of 16 bytes, nb = ceil(H / 8) blocks of 8 hidden units;
 *                       lane l of block b stands for row = (j >> 3) * H + 8 b + (j & 7), j = l & 31.  Slot s < ksh = ceil(H / 16): 8 bf16,
 *                       element e = weight_hh[row][16 s + 8 (l >> 5) + e].  The ksx slots behind them hold weight_ih: network 2, ksx =
 *                       ceil(in / 16), 8 bf16, element e = weight_ih[row][16 (s - ksh) + 8 (l >> 5) + e]; network 1, ksx = ceil(cols / 8),
 *                       4 floats, element e = weight_ih[row][8 (s - ksh) + 4 (l >> 5) + e].  Then float bias[32 nb], bias[32 b + j] =
 *                       bias_ih[row] + bias_hh[row] summed in float32.
 *   A NaN weight becomes the quiet NaN 0x7fc0.
 */
int cs_value_net_pack_lstm_bf16(const int32_t* dims, int n_dims, int cols, const float* const* params, void* blob, size_t* n_bytes);
int cs_value_net_decide_lstm_bf16(const int32_t* dims, int n_dims, const void* d_weights, size_t n_weight_bytes, int W, int A, int n, int cols,
                                  int sorted_by_distance, const float* d_rotated, const float* d_rewards, const float* d_actions,
                                  const float* d_robot, int robot_stride, float gamma, float dt, const int32_t* d_override, float* d_values,
                                  int32_t* d_choice, float* d_action_out, void* stream);

/*
 * cs_value_net_decide_lstm_worlds  cs_lookahead followed by cs_value_net_decide_lstm as ONE entry point, without the look-ahead tensor
 *   (csrc/value_net_lstm_worlds.hip), as cs_value_net_decide_worlds is for CADRL and SARL: the recurrent kernel computes a
 *   job's frames, rewards and sort keys and generates every step's rows in LDS from the worlds' own rows, so rotated [W][A][n][13|15] --
 *   431 MB at 4096 worlds x 81 actions x 25 humans -- is neither allocated, written nor gathered back; nothing of size W * A * n is read
 *   or written.  d_actions [A][2], d_next [W][n][4|6], d_current [W][n][5|7], d_robot [W][robot_stride], robot_stride and dt are exactly
 *   what cs_lookahead takes; dims, d_weights (cs_value_net_pack_lstm's blob for cols = 13, or 15 with theta_and_omega_visible),
 *   sorted_by_distance, gamma, d_override, d_values, d_choice and d_action_out exactly what cs_value_net_decide_lstm takes.
 *   d_rewards_out (may be NULL) receives [W][A], the rewards the kernel computed.  d_values, d_choice, d_action_out and d_rewards_out
 *   are, bit for bit, those of cs_lookahead followed by cs_value_net_decide_lstm on the same inputs -- the order of tied distances
 *   included: the sort key is the tensor's column 11, computed by the same function --; a (world, action) gives the same bits for W = 1
 *   as inside any batch.  Two kernels on `stream`: the network, then the per-world pick.  Errors (CS_ERR_ARG, before any device call):
 *   those of cs_value_net_decide_lstm and of cs_lookahead with their messages (d_next and d_current are required; robot_stride >= 8;
 *   sorted_by_distance outside 0..1; n > CS_VN_LSTM_MAX_N, in this entry's name); the LDS-fit check is made for this kernel's own LDS
 *   (cs_value_net_decide_lstm's buffers and a table of 32 x 8 floats).  The entry takes no `cols`: the column count follows from
 *   theta_and_omega_visible, and a blob packed for the other count cannot be detected here -- the blobs of 13 and of 15 columns have the
 *   same size (both round up to two k-groups of 8), the two columns' weights are then zero or unread.  The caller pairs the flag with
 *   the `cols` it packed for (the Python binding does: decide_lstm_worlds refuses a DeviceNet of the other count).
 * cs_value_net_decide_lstm_worlds_bf16  the same for cs_value_net_decide_lstm_bf16 (csrc/value_net_lstm_worlds_bf16.hip): that entry's
 *   arithmetic on the blob of cs_value_net_pack_lstm_bf16 and its length in bytes, bit for bit cs_lookahead followed by
 *   cs_value_net_decide_lstm_bf16.  No pack entry of their own: the blobs are the tensor entries'.
 */
int cs_value_net_decide_lstm_worlds(const int32_t* dims, int n_dims, const float* d_weights, size_t n_weight_floats, int W, int A, int n,
                                    int theta_and_omega_visible, int sorted_by_distance, const float* d_actions, const float* d_next,
                                    const float* d_current, const float* d_robot, int robot_stride, float gamma, float dt,
                                    const int32_t* d_override, float* d_rewards_out /* may be NULL */, float* d_values, int32_t* d_choice,
                                    float* d_action_out, void* stream);
int cs_value_net_decide_lstm_worlds_bf16(const int32_t* dims, int n_dims, const void* d_weights, size_t n_weight_bytes, int W, int A, int n,
                                         int theta_and_omega_visible, int sorted_by_distance, const float* d_actions, const float* d_next,
                                         const float* d_current, const float* d_robot, int robot_stride, float gamma, float dt,
                                         const int32_t* d_override, float* d_rewards_out /* may be NULL */, float* d_values,
                                         int32_t* d_choice, float* d_action_out, void* stream);

/*
 * cs_value_net_loss_grad_lstm  cs_value_net_loss_grad for LSTM-RL (crowd_nav/policy/lstm_rl.py:9-65, ValueNetwork1 and ValueNetwork2;
 *   csrc/value_net_lstm_grad.hip): what crowd_nav/utils/trainer.py:50-71 does per minibatch before optimizer.step() -- zero_grad,
 *   outputs = model(inputs), loss = MSELoss(outputs, values), loss.backward() -- by backpropagation through time, in two launches on `stream`.
 *   dims, d_weights are what cs_value_net_decide_lstm takes (cs_value_net_pack_lstm's blob for `cols`).  d_params holds the same parameters
 *   flat, in torch's own layout and cs_value_net_pack_lstm's order: mlp1's (weight [N][K] row-major, bias [N]) pairs, weight_ih [4H][in],
 *   weight_hh [4H][H], bias_ih [4H], bias_hh [4H], mlp's pairs (n_param_floats: cs_value_net_grad_sizes_lstm).  d_rows [B][n][cols] are B
 *   stored states, n <= CS_VN_LSTM_MAX_N; a sample's rows are evaluated as they lie (cs_value_net_decide_lstm's sorted_by_distance = 0; the
 *   kernel does not sort), its self state is the first six columns of its first row.  d_targets [B] are the target values.  d_grad (the
 *   layout of d_params; written, not accumulated) = d/dtheta mean_b (V_b - target_b)^2, d_loss the loss, d_values [B] (may be NULL) the
 *   network's outputs: number for number what cs_value_net_decide_lstm returns for these rows with A = 1, sorted_by_distance = 0, zero
 *   rewards and dt = 0 (the same fmaf chain per gate from b_ih + b_hh, the same sigmoid and tanh on v_exp_f32 / v_rcp_f32).  The backward
 *   takes the derivatives from the stored activations (sigma' = s (1 - s), tanh' = 1 - t^2); bias_ih's and bias_hh's gradients are the same
 *   bytes; with n = 1 weight_hh's gradient is exactly 0; hidden units beyond H (the blob's padding to 8) contribute and receive nothing.
 *   d_scratch of n_scratch_floats (at least cs_value_net_grad_sizes_lstm's figure) holds per workgroup (one per 32 samples, at most 256) its
 *   partial gradient [P + 1, rounded up to 4] and behind it its TAPE, the gates, the cell state and h of every step, [n][6][32][H rounded up
 *   to 8] floats, which the workgroup writes in its forward and reads back itself in its backward.  The partial gradients are summed in a
 *   fixed order: no atomics, the same call gives the same bytes; the bits may depend on B.  float32.
 *   Errors (CS_ERR_ARG, before any device call): those of cs_value_net_decide_lstm's network description, B < 1, n < 1,
 *   n > CS_VN_LSTM_MAX_N, a null pointer other than d_values, a blob or parameter array of another size, a scratch that is too small, a
 *   network whose tile (every layer's activations of 32 rows, two gradient buffers, the gate gradients [32][4H]) does not fit the 160 KiB of LDS.
 * cs_value_net_grad_sizes_lstm  (host only) the lengths of d_params and of d_scratch for such a call, in floats.
 * cs_value_net_pack_lstm_device  cs_value_net_pack_lstm on the device, one launch on `stream`: d_blob (n_blob_floats =
 *   cs_value_net_pack_lstm's figure) from the flat d_params, byte for byte what cs_value_net_pack_lstm writes for the same numbers -- the gate
 *   rows in the order 8 * gate + unit, bias_ih + bias_hh summed in float32, the zero padding.
 */
int cs_value_net_grad_sizes_lstm(const int32_t* dims, int n_dims, int cols, int B, int n, size_t* n_param_floats, size_t* n_scratch_floats);
int cs_value_net_loss_grad_lstm(const int32_t* dims, int n_dims, const float* d_weights, size_t n_weight_floats, const float* d_params,
                                size_t n_param_floats, int B, int n, int cols, const float* d_rows, const float* d_targets, float* d_grad,
                                float* d_loss, float* d_values /* may be NULL */, float* d_scratch, size_t n_scratch_floats, void* stream);
int cs_value_net_pack_lstm_device(const int32_t* dims, int n_dims, int cols, const float* d_params, size_t n_param_floats, float* d_blob,
                                  size_t n_blob_floats, void* stream);

/*
 * cs_value_net_train_step_lstm  cs_value_net_train_step for LSTM-RL: cs_value_net_loss_grad_lstm's job kernel, unchanged, then the same
 *   update kernel on the recurrent blob's map -- the gate rows in the order 8 * gate + unit, and the gates' bias float rewritten as
 *   bias_ih + bias_hh of the two updated values, summed in float32 as cs_value_net_pack_lstm sums it.  Arguments, results and errors are
 *   cs_value_net_train_step's with cs_value_net_loss_grad_lstm's in the place of cs_value_net_loss_grad's.
 * cs_value_net_blob_index_lstm  (host only) cs_value_net_blob_index for the recurrent blob: index[i] is the float of
 *   cs_value_net_pack_lstm's blob that holds parameter i; bias_ih[row] and bias_hh[row] name the same float, which holds their sum.
 */
int cs_value_net_train_step_lstm(const int32_t* dims, int n_dims, float* d_weights, size_t n_weight_floats, float* d_params,
                                 size_t n_param_floats, float* d_momentum, size_t n_momentum_floats, float lr, float momentum, int B, int n,
                                 int cols, const float* d_rows, const float* d_targets, float* d_grad, float* d_loss,
                                 double* d_loss_sum /* may be NULL */, float* d_values /* may be NULL */, float* d_scratch,
                                 size_t n_scratch_floats, void* stream);
int cs_value_net_blob_index_lstm(const int32_t* dims, int n_dims, int cols, int32_t* index, size_t n_param_floats);

/*
 * cs_value_net_decide_lstm_om  cs_value_net_decide_lstm for OM-LSTM-RL (lstm_rl.with_om = true; csrc/value_net_lstm.hip
 *   k_value_net_lstm_om): the rows of the recurrent network carry om_cols occupancy-map columns behind the rotated ones.
 *   With perm_a the evaluation order of (w, a) -- cs_value_net_decide_lstm's rank rule on column 11 of that pair's rows, the identity
 *   for sorted_by_distance = 0 -- the input row at step t of (w, a) is d_rotated[w][a][perm_a[t]][0..cols) followed by
 *   d_maps[w][m][0..om_cols), d_maps [W][n][om_cols] being cs_occupancy_maps' output, read in place and never expanded A-fold:
 *     map_order = CS_VN_MAPS_OWN           m = perm_a[t]: every human beside its own map (what multi_human_rl.py:115-128 transform stores
 *                                          and a trainer evaluates);
 *     map_order = CS_VN_MAPS_FIRST_ACTION  m = perm_0[t], perm_0 the order of (w, action index 0) under the same rule, computed from that
 *                                          pair's own rows of d_rotated whichever tile they lie in: the reference's serial decision
 *                                          (multi_human_rl.py:75-78 builds the maps once, on the first action's sorted humans, and attaches
 *                                          them by position to every later action's rows).
 *   With sorted_by_distance = 0 both orders are the identity.  Network 1: the LSTM reads cols + om_cols columns, its gates
 *   ceil(H / 8) + ceil((cols + om_cols) / 8) k-groups in the same descending order; network 2: mlp1's first layer reads cols + om_cols
 *   columns, the gates are cs_value_net_decide_lstm's.  Everything else -- dims, the NaN key, the self state from the first row in
 *   evaluation order, the pick, d_override, reach-destination, the two kernels on `stream` -- is cs_value_net_decide_lstm's.  A world
 *   alone (W = 1, all A actions) gives the bits it gives inside any batch; with CS_VN_MAPS_OWN a single (world, action) does too.  No
 *   atomics.  float32.  With all-zero map weights and finite maps the values equal cs_value_net_decide_lstm's bit for bit.
 * cs_value_net_pack_lstm_om  (host only) cs_value_net_pack_lstm's layout with the one wider K: weight_ih (network 1) or mlp1's first
 *   weight (network 2) is [..][cols + om_cols].
 *   Further errors of both (CS_ERR_ARG, before any device call): om_cols < 1, cols + om_cols > 256; of the decision a null d_maps,
 *   map_order outside 0..1, and the LDS-fit refusal made for this kernel's own LDS (joint rows or gather tile of cols + om_cols rounded
 *   up to 8, plus 4 floats; the keys and the order of action 0, 2 x 32 n words).
 */
enum { CS_VN_MAPS_OWN = 0, CS_VN_MAPS_FIRST_ACTION = 1 };
int cs_value_net_pack_lstm_om(const int32_t* dims, int n_dims, int cols, int om_cols, const float* const* params, float* blob,
                              size_t* n_floats);
int cs_value_net_decide_lstm_om(const int32_t* dims, int n_dims, const float* d_weights, size_t n_weight_floats, int W, int A, int n,
                                int cols, int om_cols, int sorted_by_distance, int map_order, const float* d_rotated,
                                const float* d_maps /* [W][n][om_cols] */, const float* d_rewards, const float* d_actions,
                                const float* d_robot, int robot_stride, float gamma, float dt, const int32_t* d_override,
                                float* d_values, int32_t* d_choice, float* d_action_out, void* stream);

/*
 * cs_value_net_decide_lstm_om_bf16  cs_value_net_decide_lstm_om with the opt-in bf16 arithmetic (csrc/value_net_lstm_om_bf16.hip):
 *   the same arguments, results, errors and messages -- om_cols < 1, cols + om_cols > 256, a null d_maps, map_order outside 0..1, the LDS-fit
 *   refusal for this kernel's own LDS --, with the blob of cs_value_net_pack_lstm_om_bf16 and its length in bytes.  The first layer that
 *   reads a row (network 1: weight_ih; network 2: mlp1's layer 0) is split by column: its cols rotated columns stay float32 (full weights,
 *   unrounded inputs); its om_cols map columns are bf16 operands with float32 accumulation -- the weights [:, cols:] rounded to bf16, nearest
 *   even, by the pack, a map value rounded once, nearest even, when it is staged, zeros up to a multiple of 16 columns.  mlp's layer 0 is
 *   float32; weight_hh, network 2's weight_ih and every mlp1 / mlp layer behind the first are bf16 layers; the rounding points (h_t once a
 *   step) and what is never rounded (c, the pre-activations, sigmoid, tanh, mlp's last output, the value) are
 *   cs_value_net_decide_lstm_bf16's.  A first-layer pre-activation is one chain: the bias, the float32 k-groups of the rotated columns
 *   ascending, the map k-steps of 16 ascending, for network 1's gates then weight_hh's k-steps ascending.  The order of a sequence's rows,
 *   the map pairing, ties, NaN distances, d_override and the pick are cs_value_net_decide_lstm_om's: the arithmetic never touches the order.
 *   A (world, action)'s value depends on its own rows and the map rows it reads: W = 1 gives the bits of any batch.  With all-zero map
 *   weights and finite maps the values equal cs_value_net_decide_lstm_bf16's on the narrow network bit for bit.  No atomics.
 * cs_value_net_pack_lstm_om_bf16  (host only) params as cs_value_net_pack_lstm_om takes them.  blob == NULL: only *n_bytes is set.  The
 *   blob is zeroed, then written.  Layout: cs_value_net_pack_lstm_bf16's, piece for piece, with the one wider layer:
 *     network 2's mlp1 layer 0   [ncb][2 + ksm][64 lanes] slots of 16 bytes, ksm = ceil(om_cols / 16): slot s < 2 holds 4 floats, element
 *                       e = weight[32 b + (l & 31)][8 s + 4 (l >> 5) + e] for k < cols; slot s >= 2 holds 8 bf16, element e =
 *                       weight[32 b + (l & 31)][cols + 16 (s - 2) + 8 (l >> 5) + e] for k < cols + om_cols; then float bias[32 ncb];
 *     network 1's gates   [nb][ksh + 2 + ksm][64 lanes] slots: the ksh slots of weight_hh as in cs_value_net_pack_lstm_bf16; then 2 slots of
 *                       4 floats, element e = weight_ih[row][8 (s - ksh) + 4 (l >> 5) + e] for k < cols; then ksm slots of 8 bf16, element e
 *                       = weight_ih[row][cols + 16 (s - ksh - 2) + 8 (l >> 5) + e]; then float bias[32 nb] = bias_ih + bias_hh.
 *   Network 2's gates and every other layer are cs_value_net_pack_lstm_bf16's.  A NaN weight becomes the quiet NaN 0x7fc0.
 */
int cs_value_net_pack_lstm_om_bf16(const int32_t* dims, int n_dims, int cols, int om_cols, const float* const* params, void* blob,
                                   size_t* n_bytes);
int cs_value_net_decide_lstm_om_bf16(const int32_t* dims, int n_dims, const void* d_weights, size_t n_weight_bytes, int W, int A, int n,
                                     int cols, int om_cols, int sorted_by_distance, int map_order, const float* d_rotated,
                                     const float* d_maps /* [W][n][om_cols] */, const float* d_rewards, const float* d_actions,
                                     const float* d_robot, int robot_stride, float gamma, float dt, const int32_t* d_override,
                                     float* d_values, int32_t* d_choice, float* d_action_out, void* stream);

/*
 * cs_value_net_decide_om_bf16  cs_value_net_decide_om with the opt-in bf16 arithmetic (csrc/value_net_om_bf16.hip): the same
 *   arguments, results, errors and messages -- kind != CS_VN_SARL, om_cols < 1, cols + om_cols > 256, a null d_maps, the LDS-fit refusal for
 *   this kernel's own LDS --, with the blob of cs_value_net_pack_om_bf16 and its length in bytes.  mlp1's layer 0 is split by column: its
 *   cols rotated columns stay float32 (full weights, unrounded inputs, v_mfma_f32_32x32x2_f32); its om_cols map columns are bf16 operands
 *   with float32 accumulation -- the weights [:, cols:] rounded to bf16, nearest even, by the pack, a map value rounded once, nearest even,
 *   when it is staged, zeros up to a multiple of 16 columns.  A pre-activation of that layer is one chain: the bias, the two float32
 *   k-groups of the rotated columns ascending, the ksm = ceil(om_cols / 16) map k-steps ascending; then the ReLU; then it is rounded once
 *   as the next layer's operand.  Everything else is cs_value_net_decide_bf16's contract: every later layer outside mlp3 a bf16 layer, mlp3
 *   float32 on the unrounded self state (the first six columns of the first human's row), what a reduction consumes not rounded, the
 *   crowd mean summed in human order from the rounded mlp1 outputs and rounded once, the softmax, the weighted sum, the action value and
 *   the pick float32.  One map row serves the A actions of its world.  A (world, action) gives the same bits for W = 1 as inside any
 *   batch.  With all-zero map weights and finite maps the values equal cs_value_net_decide_bf16's on the narrow network.  No atomics.
 * cs_value_net_pack_om_bf16  (host only) params as cs_value_net_pack_om takes them.  blob == NULL: only *n_bytes is set.  The blob is
 *   zeroed, then written.  Layout: cs_value_net_pack_bf16's, layer after layer, with the one wider layer:
 *     mlp1 layer 0      [ncb][2 + ksm][64 lanes] slots of 16 bytes, ncb = ceil(N / 32): slot s < 2 holds 4 floats, element e =
 *                       weight[32 b + (l & 31)][8 s + 4 (l >> 5) + e] for k < cols; slot s >= 2 holds 8 bf16, element e =
 *                       weight[32 b + (l & 31)][cols + 16 (s - 2) + 8 (l >> 5) + e] for k < cols + om_cols; then float bias[32 ncb].
 *   Weights and biases beyond N or K are zero.  A NaN weight becomes the quiet NaN 0x7fc0.
 */
int cs_value_net_pack_om_bf16(int kind, const int32_t* dims, int n_dims, int cols, int om_cols, const float* const* params, void* blob,
                              size_t* n_bytes);
int cs_value_net_decide_om_bf16(int kind, const int32_t* dims, int n_dims, const void* d_weights, size_t n_weight_bytes, int W, int A, int n,
                                int cols, int om_cols, const float* d_rotated, const float* d_maps /* [W][n][om_cols] */,
                                const float* d_rewards, const float* d_actions, const float* d_robot, int robot_stride, float gamma, float dt,
                                const int32_t* d_override, float* d_values, int32_t* d_choice, float* d_action_out, void* stream);

/*
 * The optimisation step of the networks with occupancy-map columns, OM-SARL and OM-LSTM-RL (csrc/value_net_grad.hip,
 * csrc/value_net_lstm_grad.hip): every entry below is its sibling without `_om` -- the same kernels, launches, results,
 * determinism and errors -- with `int om_cols` behind `cols`, 1 <= om_cols and cols + om_cols <= 256.
 *   Row layout.  d_rows is [B][n][cols + om_cols], float32 and dense: a row is the cols (13 | 15) rotated columns of a human followed by
 *   the om_cols columns of that human's occupancy map -- what multi_human_rl.py:115-128 transform stores for a state, what
 *   joint_state_device returns and a replay memory holds.  The maps are not a separate array here.  The self state is columns 0..5 of a
 *   sample's first row.
 * cs_value_net_grad_sizes_om, cs_value_net_loss_grad_om, cs_value_net_train_step_om  (kind = CS_VN_SARL alone) d_weights is
 *   cs_value_net_pack_om's blob, d_params the flat parameters with mlp1's first weight [N][cols + om_cols]; the gradient of that weight
 *   covers its map columns.  d_values are cs_value_net_decide_om's numbers for these rows and maps with A = 1, zero rewards and dt = 0.
 *   Row layout: d_rows [B][n][cols + om_cols] as above.
 * cs_value_net_pack_om_device  byte for byte cs_value_net_pack_om's blob from the flat d_params.
 * cs_value_net_blob_index_om  (host only) index[i] is the float of cs_value_net_pack_om's blob that holds parameter i; the columns of the
 *   first layer's k-group padding (cols + om_cols up to a multiple of 8) belong to no parameter and stay zero.
 * cs_value_net_grad_sizes_lstm_om, cs_value_net_loss_grad_lstm_om, cs_value_net_train_step_lstm_om  d_weights is
 *   cs_value_net_pack_lstm_om's blob; network 1: weight_ih is [4H][cols + om_cols] and the LSTM reads the row itself, network 2: mlp1's
 *   first weight is [N][cols + om_cols].  d_values are cs_value_net_decide_lstm_om's numbers with A = 1 and sorted_by_distance = 0 (the
 *   same descending k-group order over the wider joint row).  The tape does not depend on the row's width.  Row layout: d_rows
 *   [B][n][cols + om_cols] as above, a sample's rows evaluated as they lie.
 * cs_value_net_pack_lstm_om_device, cs_value_net_blob_index_lstm_om  cs_value_net_pack_lstm_device and cs_value_net_blob_index_lstm for
 *   cs_value_net_pack_lstm_om's blob.
 *   Further errors of all (CS_ERR_ARG, before any device call): om_cols < 1, cols + om_cols > 256, kind != CS_VN_SARL for the feed-forward
 *   entries; the LDS-fit refusal names the widths and the bytes asked for (the input tile has rows of cols + om_cols rounded up to 8, plus 4
 *   floats).
 */
int cs_value_net_grad_sizes_om(int kind, const int32_t* dims, int n_dims, int cols, int om_cols, int B, int n, size_t* n_param_floats,
                               size_t* n_scratch_floats);
int cs_value_net_loss_grad_om(int kind, const int32_t* dims, int n_dims, const float* d_weights, size_t n_weight_floats, const float* d_params,
                              size_t n_param_floats, int B, int n, int cols, int om_cols, const float* d_rows /* [B][n][cols + om_cols] */,
                              const float* d_targets, float* d_grad, float* d_loss, float* d_values /* may be NULL */, float* d_scratch,
                              size_t n_scratch_floats, void* stream);
int cs_value_net_pack_om_device(int kind, const int32_t* dims, int n_dims, int cols, int om_cols, const float* d_params, size_t n_param_floats,
                                float* d_blob, size_t n_blob_floats, void* stream);
int cs_value_net_train_step_om(int kind, const int32_t* dims, int n_dims, float* d_weights, size_t n_weight_floats, float* d_params,
                               size_t n_param_floats, float* d_momentum, size_t n_momentum_floats, float lr, float momentum, int B, int n,
                               int cols, int om_cols, const float* d_rows /* [B][n][cols + om_cols] */, const float* d_targets, float* d_grad,
                               float* d_loss, double* d_loss_sum /* may be NULL */, float* d_values /* may be NULL */, float* d_scratch,
                               size_t n_scratch_floats, void* stream);
int cs_value_net_blob_index_om(int kind, const int32_t* dims, int n_dims, int cols, int om_cols, int32_t* index, size_t n_param_floats);
int cs_value_net_grad_sizes_lstm_om(const int32_t* dims, int n_dims, int cols, int om_cols, int B, int n, size_t* n_param_floats,
                                    size_t* n_scratch_floats);
int cs_value_net_loss_grad_lstm_om(const int32_t* dims, int n_dims, const float* d_weights, size_t n_weight_floats, const float* d_params,
                                   size_t n_param_floats, int B, int n, int cols, int om_cols,
                                   const float* d_rows /* [B][n][cols + om_cols] */, const float* d_targets, float* d_grad, float* d_loss,
                                   float* d_values /* may be NULL */, float* d_scratch, size_t n_scratch_floats, void* stream);
int cs_value_net_pack_lstm_om_device(const int32_t* dims, int n_dims, int cols, int om_cols, const float* d_params, size_t n_param_floats,
                                     float* d_blob, size_t n_blob_floats, void* stream);
int cs_value_net_train_step_lstm_om(const int32_t* dims, int n_dims, float* d_weights, size_t n_weight_floats, float* d_params,
                                    size_t n_param_floats, float* d_momentum, size_t n_momentum_floats, float lr, float momentum, int B,
                                    int n, int cols, int om_cols, const float* d_rows /* [B][n][cols + om_cols] */, const float* d_targets,
                                    float* d_grad, float* d_loss, double* d_loss_sum /* may be NULL */, float* d_values /* may be NULL */,
                                    float* d_scratch, size_t n_scratch_floats, void* stream);
int cs_value_net_blob_index_lstm_om(const int32_t* dims, int n_dims, int cols, int om_cols, int32_t* index, size_t n_param_floats);

/*
 * Float64 worlds (csrc/sfmstep_f64.hip): the SFM / HSFM substep in the reference's own precision (PRECISION = np.float64),
 * an opt-in arithmetic beside the float32 entries above.  cs_worlds_f64 carries the fields of cs_worlds that apply, with double buffers:
 * the state is CS_LAYOUT_AOS [W][rows][13] only, a world holds up to 64 rows (one wavefront per world), the types are 0..8, the robot is
 * holonomic.  Flag bits: CS_ALL_PARAMS_EQUAL, CS_ROBOT_ROW, CS_PARAMS_SHARED, CS_OBSTACLES_SHARED, CS_RESPAWN.  IEEE division and square
 * root, the device library's double exp / atan2 / sin / cos (the two atan2 of Moussaid's theta_ij correctly rounded: their last bit decides
 * its sign in a crowd at rest), no contraction and no float32 intermediate: a world tracks the float64 CPU
 * restatement (oracle/sfm_step.inc) to ~1e-10 m over a 2000-substep episode, where a float32 world is centimetres to metres away.
 *   cs_step_f64                    cs_step: n_substeps x { robot.step(action, dt) ; states[-1] = robot row ; update_humans ; respawn } in one
 *                                  launch, in place.  d_action [W][2] (vx, vy) held for the block, or NULL.
 *   cs_update_humans_parallel_f64  cs_update_humans_parallel: one substep of update_humans_parallel (forces_parallel.py:185-284) with its
 *                                  in-place side effects on d_state / d_goals; d_out may equal w->d_state.  w->d_robot is ignored.
 *   cs_peek_f64                    cs_peek: one step of dt into d_next [W][n][8] = x, y, yaw, Vx, Vy, Omega, Gx, Gy; state and goals untouched.
 * Errors (CS_ERR_ARG with a message, before any device call): a type outside 0..8 ("Type <t> does not exist for this implementation", the
 * reference's text), W, n or G < 1, more than 64 rows, n_substeps < 1, a null d_state / d_goals / d_params / d_safety, a layout other than
 * CS_LAYOUT_AOS, CS_ROBOT_UNICYCLE, a bad obstacle description, an action without d_robot, a null output.
 */
typedef struct cs_worlds_f64 {
    int32_t W;          /* worlds                                                                */
    int32_t n;          /* humans per world (rows = n + 1 with CS_ROBOT_ROW; rows <= 64)         */
    int32_t G;          /* goal slots per human                                                  */
    int32_t O;          /* polygons (0 = no walls)                                               */
    int32_t Smax;       /* segment slots per polygon                                             */
    int32_t type;       /* 0..8                                                                  */
    int32_t flags;      /* CS_* bits                                                             */
    int32_t layout;     /* CS_LAYOUT_AOS                                                         */
    double* d_state;    /* [W][rows][13]                  in/out                                 */
    double* d_goals;    /* [W][n][G][2] NaN padded        in/out (rotated on goal switch)        */
    const double* d_params;    /* [W][n][20] or [n][20]                                          */
    const double* d_safety;    /* [W][rows]                                                      */
    const double* d_obstacles; /* [W][O][Smax][2][2] or shared, NULL when O == 0                 */
    double* d_robot;    /* [W][13] robot safe-state rows or NULL (as cs_worlds.d_robot)          */
    const int32_t* d_world_flags; /* optional [W]: bit0 = respawn enabled in this world          */
    double  respawn_bound_x, respawn_bound_y;
} cs_worlds_f64;
int cs_step_f64(const cs_worlds_f64* w, double dt, int n_substeps, const double* d_action, void* stream);
int cs_update_humans_parallel_f64(const cs_worlds_f64* w, double dt, double* d_out, void* stream);
int cs_peek_f64(const cs_worlds_f64* w, double dt, double* d_next /* [W][n][8] */, void* stream);

/*
 * Device episode buffer (csrc/episodes.hip): the per-world trajectory store behind crowd_nav/utils/explorer.py's
 * update_memory / run_k_episodes, and the flush that turns finished episodes into replay-memory samples.  The store is the caller's:
 * states [W][T][F], rewards [W][T], targets [W][T] float32, cursor [W] and overflow [W] int32 (all zero at the start).
 *   cs_episode_append   every world w with t = cursor[w] < T stores d_state[w] (F floats), d_reward[w] and, when given, d_target[w] at
 *                       [w][t] and advances its cursor; a world already at T stores nothing and sets overflow[w] = 1.  Two launches: the
 *                       copy reads the cursors, the advance follows it on the stream.  d_target / d_targets may both be NULL.
 *   cs_episode_flush    L_w = cursor[w]; kept_w = L_w where d_done[w], (keep_mask >> d_code[w]) & 1 and overflow[w] == 0, else 0.  Sample
 *                       (w, i), i < kept_w, has the index g = sum_{u<w} kept_u + i of K = sum_w kept_w and goes to ring slot
 *                       (position + g) mod capacity of d_mem_states [capacity + 1][F] / d_mem_values [capacity + 1] when g >= K - capacity:
 *                       what K single pushes in the order world-ascending, step-ascending leave behind.  Row `capacity` is never written.
 *                       Then position = (position + K) mod capacity, count = min(count + K, capacity) (int64 device scalars), and
 *                       cursor[w] = overflow[w] = 0 for every done world.  The value of a sample: CS_EPISODE_RETURNS -- the discounted
 *                       return-to-go sum_{t>=i} gamma^((t-i) * dt * v_w) * r_t, float64 products and sums in ascending t (explorer.py:132)
 *                       rounded once to float32, v_w = d_v_pref[w] or v_pref when d_v_pref is NULL; CS_EPISODE_STORED -- the target given
 *                       at append.  d_figures [6] float64 accumulates over the done worlds: episodes, those of code 2 / 3 / 4 (ReachGoal,
 *                       Collision, Timeout), sum of L_w * dt over code 2, sum of sum_t gamma^(t * dt * v_w) * r_t (explorer.py:99); an
 *                       overflowed episode counts with the T steps it stored.  d_scratch: 16 * (W + 1) bytes, 8-byte aligned.  Three
 *                       launches on `stream`, integer prefix sum and fixed-shape float64 sums: no atomics on floats, nothing read back.
 * Errors (CS_ERR_ARG with a message, before any device call): a null pointer (d_target / d_targets / d_v_pref excepted; CS_EPISODE_STORED
 * needs d_targets; a d_target needs d_targets), W, T, F or capacity < 1, T above 2048 (the discount table and the rewards of a world live
 * in LDS), W * T beyond 2^31 - 1, an unknown target mode, gamma outside (0, 1], dt <= 0, a d_scratch that is not 8-byte aligned.
 */
#define CS_EPISODE_RETURNS 0
#define CS_EPISODE_STORED 1
int cs_episode_append(int W, int T, int F, const float* d_state /* [W][F] */, const float* d_reward /* [W] */,
                      const float* d_target /* [W] or NULL */, float* d_states, float* d_rewards, float* d_targets /* may be NULL */,
                      int32_t* d_cursor, int32_t* d_overflow, void* stream);
int cs_episode_flush(int W, int T, int F, const float* d_states, const float* d_rewards, const float* d_targets /* may be NULL */,
                     int32_t* d_cursor, int32_t* d_overflow, const uint8_t* d_done /* [W] */, const int32_t* d_code /* [W] */,
                     unsigned keep_mask, int target_mode, double gamma, double dt, double v_pref, const double* d_v_pref /* [W] or NULL */,
                     int capacity, float* d_mem_states, float* d_mem_values, void* d_position /* int64 */, void* d_count /* int64 */,
                     double* d_figures /* [6] */, void* d_scratch, void* stream);

/* layout conversion of a state array between the reference's AoS rows and SoA planes */
int cs_state_aos_to_soa(const float* d_aos, float* d_soa, int W, int rows, void* stream);
int cs_state_soa_to_aos(const float* d_soa, float* d_aos, int W, int rows, void* stream);

/* kernel launch geometry the library would use for `w` (diagnostics / DESIGN.md numbers) */
int cs_launch_geometry(const cs_worlds* w, int* grid, int* block, int* worlds_per_block);

/* Name of the kernel build the library runs for `w` (diagnostics; the parity tests assert through it that the build a
 * published number comes from is the build they compared with the oracle).  entry: 0 = cs_step, 1 = cs_update_humans_parallel
 * with d_out != d_state, 2 = cs_peek.  buf receives e.g. "k_sfm_step<SOC=0,HEADED=1,PEQ=1,MAXT=64,OCC=1,ROWS_CT=25,LEAN=1> grid=2048 block=64 wpb=2
 * lds=6032 wg=4" (lds: the dynamic LDS of a block in bytes -- what decides how many blocks a CU holds; wg: how many one-wavefront blocks go to the
 * dispatcher as one workgroup; the ORCA builds also name their arithmetic, "math=exact|fast|fma"). */
int cs_step_variant(const cs_worlds* w, int entry, char* buf, size_t buflen);

/* What CS_ORCA_MATH_DEFAULT resolves to in this process (CS_ORCA_MATH_EXACT unless CROWDSTEP_ORCA_MATH=fast|fma is set; read once). */
int cs_orca_default_math(void);

/* Diagnostic: the ORCA kernels' correctly rounded divide / square root sequences (csrc/orca.hip ieee_div, ieee_sqrt: the
 * compiler's FMA sequences without the exponent-range handling) against the compiler's operators on n_pairs random operand
 * pairs of the linear programmes' range.  h_out[0], h_out[1] = number of quotients / roots that differ in any bit (must be 0),
 * h_out[2], h_out[3] = bit patterns of the first differing operand pair.  Synchronises. */
int cs_debug_divsqrt_check(unsigned long long n_pairs, unsigned seed, unsigned long long* h_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CROWDSTEP_H */
