// value_net_lstm_worlds.h -- LSTM-RL's decision with its input rows generated inside the kernel, as value_net_worlds.hip does it for CADRL and
// SARL: what k_value_net_lstm_worlds (value_net_lstm_worlds.hip, float32) and k_value_net_lstm_worlds_bf16 (value_net_lstm_worlds_bf16.hip) share.
// The look-ahead tensor rotated [W][A][n][13|15] is never written, nor read back one sorted row at a time; the results are those of
// cs_lookahead followed by cs_value_net_decide_lstm[_bf16], bit for bit.
//
// The kernels are the two recurrent kernel texts (value_net_lstm_body.inc, value_net_lstm_bf16_body.inc, LSTM_OM 0) included once more with
// the three seams of a job's input (value_net_lstm_kernel.h) redefined at the end of this header, on lookahead_math.h's pieces:
//   LSTM_BEGIN_JOB     la_job_table: the frames and rewards of the job's sequences into a table of JROWS x LA_FRAME_FLOATS floats behind the
//                      kernel's LDS map; d_rewards_out is written there.  A barrier, then the sort keys: lstm_key of column 11 as
//                      la_world_quad<2> computes it -- the function that wrote the tensor's column, so that ties fall as they do there.
//   LSTM_STEP_ROWS     one lane per (sequence, four columns): lane s of wavefront Q (la_wave_quad) calls la_world_quad<Q> for human
//                      perm[s][t] and writes a float4 where lstm_gather writes the row, zeros beyond the columns and the sequences as it
//                      pads.  The human's next row and radius come from HBM / L2, the frame from LDS; the lane's world index is computed
//                      once a job (`lane_world`, declared by LSTM_BEGIN_JOB in the job's scope beside the LaWorlds): the division stays out of the step loop.
//   LSTM_STORE_VALUES  lstm_store_values with the reward from the table.
// No atomics.  gfx950 only.
#pragma once
#include "lookahead_math.h"
#include "value_net_lstm_kernel.h"

namespace {

// what LaWorlds takes beside the kernel's own arguments (the robot rows, A and n), and where the frame table lies
struct LstmWorlds {
    const float* __restrict__ actions;     // [A][2]
    const float* __restrict__ next;        // [W][n][4 | 6]
    const float* __restrict__ cur;         // [W][n][5 | 7]
    float* __restrict__ rewards_out;       // [W][A] or null
    int frames;                            // floats from the start of the dynamic block to the table [JROWS][LA_FRAME_FLOATS]
    int headed;
};

__device__ __forceinline__ void lw_begin_job(const LaWorlds& s, float* frames, unsigned* key, float* J, int ld_j, long gbase, int ng, float dt)
{
    const int tid = threadIdx.x;
    la_job_table(s, frames, gbase, ng, dt);
    for (int i = tid; i < JROWS * ld_j; i += NT) J[i] = 0.0f;
    __syncthreads();                        // (uniform: every thread of the workgroup runs every job)
    for (int i = tid; i < ng * s.n; i += NT) {
        const int q = i / s.n, j = i - q * s.n;
        const long w = (unsigned)(gbase + q) / (unsigned)s.A;       // (W * A is below 2^30: check_decide_args)
        key[i] = lstm_key(la_world_quad<2>(s, frames + LA_FRAME_FLOATS * q, w, j).w);
    }
}

// the world of the sequence whose rows this lane generates, once a job: the division stays out of the step loop
__device__ __forceinline__ int lw_lane_world(long gbase, int ng, int A)
{
    const int q = threadIdx.x & 63;
    return q < ng ? (int)((unsigned)(gbase + q) / (unsigned)A) : 0;
}

// columns [4 Q, 4 Q + 4) of step t's rows: lane q of the wavefront writes those of sequence q, of world `world`
template <int Q>
__device__ __forceinline__ void lw_row_quad(const LaWorlds& s, const float* frames, float* X, int ld, const int* perm, int world, int ng, int t)
{
    const int q = threadIdx.x & 63;
    if (q >= TILE_M) return;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (q < ng) v = la_world_quad<Q>(s, frames + LA_FRAME_FLOATS * q, world, perm[q * s.n + t]);
    *reinterpret_cast<float4*>(X + q * ld + 4 * Q) = v;
}

__device__ __forceinline__ void lw_step_rows(const LaWorlds& s, const float* frames, float* X, int ld, const int* perm, int world, int ng, int t)
{
    la_wave_quad([&](auto Q) { lw_row_quad<Q()>(s, frames, X, ld, perm, world, ng, t); });
}

} // namespace

// the three seams: `world` (LstmWorlds) is the kernel's argument, `lds` the body's dynamic block
#undef LSTM_BEGIN_JOB
#undef LSTM_STEP_ROWS
#undef LSTM_STORE_VALUES
#define LSTM_BEGIN_JOB(KEY, J, LD_J, ROTATED, GBASE, NG, N, COLS)                                                            \
    const LaWorlds la_worlds{world.actions, world.next, world.cur, robot, world.rewards_out, rstride, world.headed, A, N};   \
    lw_begin_job(la_worlds, lds + world.frames, KEY, J, LD_J, GBASE, NG, dt);                                                \
    const int lane_world = lw_lane_world(GBASE, NG, A);
#define LSTM_STEP_ROWS(X, LD, T) lw_step_rows(la_worlds, lds + world.frames, X, LD, perm, lane_world, ng, T)
#define LSTM_STORE_VALUES(OUT, OUT_LD)                                                                                       \
    lstm_store_values<LA_FRAME_FLOATS>(OUT, OUT_LD, gbase, ng, A, lds + world.frames + LA_REWARD, robot, rstride, gamma, dt, values, tid)
