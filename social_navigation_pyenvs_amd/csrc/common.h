// Shared host-side helpers of libcrowdstep.so (error reporting across the C ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "crowdstep.h"

namespace cstep { struct KArgs; struct GymFold; }

namespace csimpl {

extern thread_local std::string g_err;

inline int fail(int code, const std::string& msg)
{
    g_err = msg;
    return code;
}

// ---- what every entry point works out about a cs_worlds ----
// rows per world: the humans, and the robot as the last row with CS_ROBOT_ROW
inline int rows_of(const cs_worlds* w) { return w->n + ((w->flags & CS_ROBOT_ROW) ? 1 : 0); }
// agent / field strides of d_state (crowdstep.h CS_LAYOUT_*); the layout has been checked
inline void state_strides(const cs_worlds* w, long& as, long& fs)
{
    if (w->layout == CS_LAYOUT_AOS) { as = 13; fs = 1; }
    else { as = 1; fs = (long)w->W * rows_of(w); }
}

// Argument checks the entry points combine, each CS_OK or the fail() status and message; an entry runs the ones it needs in its own order
inline int check_shape(const cs_worlds* w) { return w->W > 0 && w->n > 0 && w->G > 0 ? CS_OK : fail(CS_ERR_ARG, "W, n, G must be positive"); }
// d_state, d_goals, d_safety and (with_params: the force models) d_params
inline int check_buffers(const cs_worlds* w, bool with_params)
{
    return w->d_state && w->d_goals && (w->d_params || !with_params) && w->d_safety ? CS_OK : fail(CS_ERR_ARG, "null device buffer in cs_worlds");
}
// the entries that only read rows (rewards, observations, the robot's models: with_robot asks for d_robot as well)
inline int check_rows(const cs_worlds* w, bool with_robot)
{
    if (w->W > 0 && w->n > 0 && w->d_state && (w->d_robot || !with_robot)) return CS_OK;
    return fail(CS_ERR_ARG, with_robot ? "bad cs_worlds (a robot needs d_robot)" : "bad cs_worlds");
}
inline int check_layout(const cs_worlds* w) { return w->layout == CS_LAYOUT_AOS || w->layout == CS_LAYOUT_SOA ? CS_OK : fail(CS_ERR_ARG, "bad layout"); }
inline int check_obstacles(const cs_worlds* w)
{
    return w->O == 0 || (w->O > 0 && w->d_obstacles && w->Smax > 0) ? CS_OK : fail(CS_ERR_ARG, "bad obstacle description");
}
// the nine SFM / HSFM models (forces_parallel.py:211 raises ValueError for any other type)
inline int check_sfm_type(const cs_worlds* w)
{
    return w->type >= 0 && w->type <= 8 ? CS_OK : fail(CS_ERR_TYPE, "Type " + std::to_string(w->type) + " does not exist for this implementation");
}
// RVO2's parameters, for the crowd's ORCA steps and the robot's own ORCA model (up to 16 neighbours: ORCA_DEFAULTS uses 10)
inline int check_orca(const cs_worlds* w)
{
    if (w->orca_max_neighbors < 0 || w->orca_max_neighbors > 16) return fail(CS_ERR_ARG, "orca_max_neighbors must be in 0..16");
    if (!(w->orca_time_horizon > 0.0f) || !(w->orca_neighbor_dist >= 0.0f)) return fail(CS_ERR_ARG, "bad ORCA parameters");
    if (w->orca_n_vertices < 0 || (w->orca_n_vertices > 0 && !w->d_orca_vertices)) return fail(CS_ERR_ARG, "bad ORCA obstacle vertices");
    if (w->orca_n_vertices > 0 && !(w->orca_time_horizon_obst > 0.0f)) return fail(CS_ERR_ARG, "bad ORCA parameters");
    return CS_OK;
}
// the arithmetic of the crowd's register-resident ORCA build (CS_ORCA_MATH_*)
inline int check_orca_math(const cs_worlds* w)
{
    if (w->orca_math >= CS_ORCA_MATH_DEFAULT && w->orca_math <= CS_ORCA_MATH_FMA) return CS_OK;
    return fail(CS_ERR_ARG, "cs_worlds.orca_math: CS_ORCA_MATH_DEFAULT / EXACT / FAST / FMA");
}
inline int check_gym_book(const cs_gym_book* b)
{
    if (b->clock_len > 0 && b->d_counter && b->d_seeds && b->d_mask && b->d_clock && b->d_reward && b->d_terminated && b->d_truncated && b->d_info) return CS_OK;
    return fail(CS_ERR_ARG, "null buffer in cs_gym_book");
}
inline int check_stage_book(const cs_stage_book* b)
{
    return b->d_staged_seed && b->d_epoch && b->d_base_seed && b->d_staged_status ? CS_OK : fail(CS_ERR_ARG, "null buffer in cs_stage_book");
}

#ifdef CS_STAMPS
extern unsigned long long* g_stamp_buf; // diagnostic build only (tools/stamp_probe.py)
#endif

// cs_gym_step_staged (crowdstep.hip): the staged-episode take-over's arguments for the step kernel's epilogue, built and checked where
// the pre-staged episodes live (generate.hip)
int stage_fold(const cs_generator* gen, const cs_worlds* staging, const cs_worlds* live, const cs_stage_book* book, int obs_cols, float* d_obs,
               cstep::GymFold& out);

// ORCA branch (orca.hip)
int orca_launch(const cs_worlds* w, float dt, int n_substeps, const float* d_action, float* d_peek, hipStream_t stream);
// name of the k_orca_step build orca_launch would run for `w` (cs_step_variant)
int orca_variant(const cs_worlds* w, char* buf, size_t buflen);
// the robot's own ORCA model, one doStep of the robot per world (orca.hip; cs_robot_model_step with CS_ORCA)
int orca_robot_launch(const cs_worlds* w, float robot_margin, const float* d_human_margin, float dt, hipStream_t stream, int just_velocities = 0);
// library-owned device scratch, one block per (device, stream, use); never allocated, grown or freed while `stream` is capturing
// (CS_ERR_ARG then -- cs_reserve_scratch first), a block handed out during a capture is never freed before cs_release_scratch
enum { SCRATCH_ORCA_BIG = 0, SCRATCH_SFM_BIG = 1, SCRATCH_IMITATION = 2 };
int scratch(void** out, size_t bytes, int slot, hipStream_t stream);
int scratch_release_all();
inline size_t imitation_scratch_bytes(const cs_worlds* w, int n_substeps) { return (size_t)n_substeps * w->W * w->n * 4 * sizeof(float); }
size_t sfm_big_scratch_bytes(const cs_worlds* w);
size_t orca_big_scratch_bytes(const cs_worlds* w);
bool orca_uses_grid(const cs_worlds* w);   // ORCA worlds that take the grid path (more than 512 rows, or LDS columns beyond a block)
int big_world_min_rows(int dflt);
int device_simds();   // CUs x 4 of the current device
// the uniform grid of worlds beyond one block (bigworld.hip): rows binned into hashed buckets of square cells, every bucket's rows in
// index order (hand-written counting sort, bigworld.hip); start[w * NB + b] .. start[w * NB + b + 1] = bucket b of world w in `sorted` (row indices)
struct GridView { int W, rows, NB; int2* cellxy; unsigned* keys; int* tmp; int* sorted; int* start; int* fill; };
__host__ __device__ inline int cell_bucket(int cx, int cy, int NB) { return (int)(((unsigned)cx * 73856093u) ^ ((unsigned)cy * 19349663u)) & (NB - 1); }
size_t grid_bytes(int W, int rows, int NB);
// the parallel-traffic respawn rule on the stepped rows of worlds beyond one block (bigworld.hip k_bw_respawn); orca: RVO2 agent rows
void big_respawn_launch(float* S, long as, long fs, int W, int n, int rows, float* goals, int G, const float* extra, int orca, float bx, float by,
                        const int* world_flags, hipStream_t stream);
int big_world_buckets(int rows);   // hashed buckets of a world's grid: the power of two >= 2 * rows (1024 .. 2^20)
int grid_build(const float* S, long as, long fs, int W, int rows, int NB, const float* d_inv_cell, float inv_cell, void* mem, GridView& g, hipStream_t stream);
// SFM / HSFM worlds beyond one block (bigworld.hip)
int sfm_big_launch(const cs_worlds* w, float dt, int n_substeps, float* d_out, int mutate_input, bool robot_from_array, const float* d_action,
                   float* d_peek, hipStream_t stream, float* d_trace = nullptr);
// small worlds, one per 16-lane DPP row (rowstep.hip)
bool row16_supports(int rows);
int row16_launch(const cstep::KArgs& a, hipStream_t stream);
// the robot's n substeps against the crowd snapshots of an imitation block (robot_model.hip)
int robot_block_launch(const cs_worlds* w, int robot_type, const float* robot_params, float robot_margin, const float* d_human_margin,
                       float* d_robot_memory, float dt, int n_substeps, const float4* d_snap, hipStream_t stream);
// social-momentum branch (social_momentum.hip)
int social_momentum_launch(const cs_worlds* w, float dt, int n_substeps, const float* d_action, float* d_peek, hipStream_t stream);

} // namespace csimpl

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e__ = (expr);                                                                        \
        if (e__ != hipSuccess)                                                                          \
            return ::csimpl::fail(CS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));      \
    } while (0)
