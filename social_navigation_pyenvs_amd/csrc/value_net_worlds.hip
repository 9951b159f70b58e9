// value_net_worlds.hip -- the value-network decision of value_net.hip with its input rows generated inside the kernel: CADRL and SARL decide
// for W worlds from the resident rows, and the look-ahead tensor rotated [W][A][n][13|15] (an A-fold expansion of the ~1 KB a world's
// look-ahead reads: 431 MB at 4096 worlds x 81 actions x 25 humans) is never written.  Replaces cs_lookahead + cs_value_net_decide, whose
// results it reproduces bit for bit.
//
// The kernel is value_net.hip's (value_net_body.inc: the same groups, tiles, workgroups, layers and reductions) with another tile loader,
// built from lookahead_math.h's pieces.  Once per job, la_job_table computes the frames and rewards of the job's groups into a table of
// 32 x LA_FRAME_FLOATS floats behind the LDS map; the job's first barrier publishes it.  A tile is then written by one lane per (row, four
// columns): wavefront Q (la_wave_quad) writes columns [4 Q, 4 Q + 4) of row r = lane, la_world_quad<Q> of the row's world and human, with
// one ds_write_b128 (rows are 80 bytes apart), zero beyond the rows and the columns as load_tile pads.  A group in chunks (n > 32)
// regenerates the rows of a chunk at each of SARL's three passes (human ch * 32 + r); its frame is computed once.  The arithmetic is the
// one k_lookahead runs, so the rows are cs_lookahead's to the last bit.  HBM traffic: the worlds' rows, the weight blob, one float per
// group (two with d_rewards_out).  No atomics.  gfx950 only.
#include <hip/hip_runtime.h>

#include "lookahead_math.h"
#include "value_net_f32.h"

namespace {

// columns [4 Q, 4 Q + 4) of the tile's rows: row r belongs to the tile's group r / per (the job's group t0 + r / per, the launch's g0 + r / per)
// and is its human ch * M + r % per
template <int Q>
__device__ __forceinline__ void generate_quad(const LaWorlds& s, const float* frames, const VnBufs& b, int t0, int g0, int ch, int rows, int per, int M)
{
    const int r = threadIdx.x & 63;
    if (r >= M) return;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (r < rows) {
        const int k = r / per, j = ch * M + r - k * per;
        v = la_world_quad<Q>(s, frames + LA_FRAME_FLOATS * (t0 + k), (g0 + k) / s.A, j);
    }
    *reinterpret_cast<float4*>(b.X0 + r * LDX + 4 * Q) = v;
    if (Q == 0) b.grp[r] = r < rows ? r / per : 0;
}

__device__ __forceinline__ void generate_tile(const LaWorlds& s, const float* frames, const VnBufs& b, int t0, int g0, int ch, int rows, int per, int M)
{
    la_wave_quad([&](auto Q) { generate_quad<Q()>(s, frames, b, t0, g0, ch, rows, per, M); });
}

// `frames`: floats from the start of the dynamic block to the frame table, behind the map m that the other two kernels share
__global__ __launch_bounds__(NT) void k_value_net_worlds(VnPlan p, VnLds m, int frames, int M, const float* __restrict__ wb, int NG, int A, int n,
                                                         int headed, const float* __restrict__ actions, const float* __restrict__ next,
                                                         const float* __restrict__ cur, const float* __restrict__ robot, int rstride, float gamma,
                                                         float dt, float* __restrict__ rewards_out, float* __restrict__ values)
{
    extern __shared__ float lds[];
    const int gsum = m.G;
    const LaWorlds world{actions, next, cur, robot, rewards_out, rstride, headed, A, n};
    float* const table = lds + frames;
#define VN_BEGIN_JOB(gbase, ng) la_job_table(world, table, gbase, ng, dt)
#define VN_TILE_SOURCE(g0) const int tile_g0 = (g0)
#define VN_LOAD_TILE(ch, rows, per) generate_tile(world, table, b, t0, tile_g0, ch, rows, per, M)
#define VN_REWARD(g, k) table[LA_FRAME_FLOATS * (k) + LA_REWARD]
#include "value_net_body.inc"
#undef VN_BEGIN_JOB
#undef VN_TILE_SOURCE
#undef VN_LOAD_TILE
#undef VN_REWARD
}

} // namespace

#include "value_net_pick.h"

extern "C" int cs_value_net_decide_worlds(int kind, const int32_t* dims, int n_dims, const float* d_weights, size_t n_weight_floats, int W, int A, int n,
                                          int theta_and_omega_visible, const float* d_actions, const float* d_next, const float* d_current,
                                          const float* d_robot, int robot_stride, float gamma, float dt, const int32_t* d_override,
                                          float* d_rewards_out, float* d_values, int32_t* d_choice, float* d_action_out, void* stream)
{
    VnPlan p;
    const int rc = build_plan(kind, dims, n_dims, theta_and_omega_visible ? 15 : 13, 0, p);
    if (rc != CS_OK) return rc;
    // (the worlds' two arrays stand where cs_value_net_decide has cs_lookahead's two outputs: cs_lookahead's own checks are among these)
    const int rc2 = check_decide_args(p, d_weights, n_weight_floats, W, A, n, d_next, d_current, d_actions, d_robot, robot_stride, d_values, d_action_out);
    if (rc2 != CS_OK) return rc2;
    VnLaunch q;
    const int rc3 = prepare_launch<k_value_net_worlds>(p, n, JROWS * LA_FRAME_FLOATS, W, A, q);      // (the tail: the frame table)
    if (rc3 != CS_OK) return rc3;
    hipLaunchKernelGGL(k_value_net_worlds, dim3(q.grid), dim3(NT), q.shmem, (hipStream_t)stream, p, q.m, q.tail, TILE_M, d_weights, q.NG, A, n,
                       theta_and_omega_visible ? 1 : 0, d_actions, d_next, d_current, d_robot, robot_stride, gamma, dt, d_rewards_out, d_values);
    return launch_pick(W, A, d_values, d_actions, d_robot, robot_stride, d_override, d_choice, d_action_out, stream);
}
