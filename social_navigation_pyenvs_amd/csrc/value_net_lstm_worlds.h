// value_net_lstm_worlds.h -- LSTM-RL's decision with its input rows generated inside the kernel, as value_net_worlds.hip does it for CADRL and
// SARL: what k_value_net_lstm_worlds (value_net_lstm_worlds.hip, float32) and k_value_net_lstm_worlds_bf16 (value_net_lstm_worlds_bf16.hip) share.
// The look-ahead tensor rotated [W][A][n][13|15] is never written, nor read back one sorted row at a time; the results are those of
// cs_lookahead followed by cs_value_net_decide_lstm[_bf16], bit for bit.
//
// The kernels are the two recurrent kernel texts (value_net_lstm_body.inc, value_net_lstm_bf16_body.inc, LSTM_OM 0) included once more with
// the three seams of a job's input (value_net_lstm_kernel.h) redefined at the end of this header:
//   LSTM_BEGIN_JOB     lane k of wavefront 0 computes the frame of the job's sequence k -- world g / A, action g % A: a job of 32 sequences
//                      crosses worlds -- and lane k of wavefront 1 its reward (the swept collision loop over the humans), into a table of
//                      JROWS x LA_FRAME_FLOATS floats behind the kernel's LDS map; d_rewards_out is written there.  A barrier, then the sort
//                      keys: lstm_key of column 11 as la_row_quad<2> computes it from the frame and the human's next row -- the function that
//                      wrote the tensor's column, so that ties fall as they do there.
//   LSTM_STEP_ROWS     one lane per (sequence, four columns): lane s of wavefront Q calls la_row_quad<Q> for human perm[s][t] and writes a
//                      float4 where lstm_gather writes the row, zeros beyond the columns and the sequences as it pads.  The human's next row
//                      and radius come from HBM / L2, the frame from LDS; the lane's world index is computed once a job (`lane_world`,
//                      declared by LSTM_BEGIN_JOB in the job's scope): the division stays out of the step loop.
//   LSTM_STORE_VALUES  lstm_store_values with the reward from the table.
// The arithmetic of frame, row and reward is lookahead_math.h's, shared with k_lookahead.  No atomics.  gfx950 only.
#pragma once
#include "lookahead_math.h"
#include "value_net_lstm_kernel.h"

namespace {

// the worlds' rows as cs_lookahead takes them (the robot rows, A and n are the kernel's own arguments), and where the frame table lies
struct LstmWorlds {
    const float* __restrict__ actions;     // [A][2]
    const float* __restrict__ next;        // [W][n][4 | 6]
    const float* __restrict__ cur;         // [W][n][5 | 7]
    float* __restrict__ rewards_out;       // [W][A] or null
    int frames;                            // floats from the start of the dynamic block to the table [JROWS][LA_FRAME_FLOATS]
    int headed;
};

__device__ __forceinline__ void lw_begin_job(const LstmWorlds& s, float* frames, unsigned* key, float* J, int ld_j, const float* __restrict__ robot,
                                             int rstride, long gbase, int ng, int A, int n, float dt)
{
    const int tid = threadIdx.x, wave = tid >> 6, k = tid & 63;
    if (wave < 2 && k < ng) {
        const long g = gbase + k, w = (unsigned)g / (unsigned)A;       // (W * A is below 2^30: check_decide_args)
        const int a = (int)(g - w * A);
        const float* rb = robot + w * rstride;
        const float ax = s.actions[2 * a], ay = s.actions[2 * a + 1];
        const LaStep st = la_step(rb, ax, ay, dt);
        float* f = frames + LA_FRAME_FLOATS * k;
        if (wave == 0) {
            f[0] = ax; f[1] = ay; f[2] = st.nrx; f[3] = st.nry; f[6] = st.dg;
            la_frame(st, f[4], f[5]);
        } else {
            const int cc = s.headed ? 7 : 5;
            const float rew = la_reward(s.cur + w * n * cc, n, cc, rb, ax, ay, dt, st.dg);
            f[7] = rew;
            if (s.rewards_out) s.rewards_out[g] = rew;
        }
    }
    for (int i = tid; i < JROWS * ld_j; i += NT) J[i] = 0.0f;
    __syncthreads();                        // (uniform: every thread of the workgroup runs every job)
    for (int i = tid; i < ng * n; i += NT) {
        const int q = i / n, j = i - q * n;
        const long w = (unsigned)(gbase + q) / (unsigned)A;
        const float* rb = robot + w * rstride;
        const float* nx = s.next + (w * n + j) * (s.headed ? 6 : 4);
        const float hr = s.cur[(w * n + j) * (s.headed ? 7 : 5) + 4];
        key[i] = lstm_key(la_row_quad<2>(frames + LA_FRAME_FLOATS * q, nx, hr, rb[7], rb[4], s.headed != 0).w);
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
__device__ __forceinline__ void lw_row_quad(const LstmWorlds& s, const float* frames, float* X, int ld, const int* perm, const float* __restrict__ robot,
                                            int rstride, int world, int ng, int n, int t)
{
    const int q = threadIdx.x & 63;
    if (q >= TILE_M) return;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (q < ng) {
        const int j = perm[q * n + t];
        const long w = world;
        const float* rb = robot + w * rstride;
        const float* nx = s.next + (w * n + j) * (s.headed ? 6 : 4);
        const float hr = s.cur[(w * n + j) * (s.headed ? 7 : 5) + 4];
        v = la_row_quad<Q>(frames + LA_FRAME_FLOATS * q, nx, hr, rb[7], rb[4], s.headed != 0);
    }
    *reinterpret_cast<float4*>(X + q * ld + 4 * Q) = v;
}

__device__ __forceinline__ void lw_step_rows(const LstmWorlds& s, const float* frames, float* X, int ld, const int* perm, const float* __restrict__ robot,
                                             int rstride, int world, int ng, int n, int t)
{
    switch (threadIdx.x >> 6) {
    case 0: lw_row_quad<0>(s, frames, X, ld, perm, robot, rstride, world, ng, n, t); break;
    case 1: lw_row_quad<1>(s, frames, X, ld, perm, robot, rstride, world, ng, n, t); break;
    case 2: lw_row_quad<2>(s, frames, X, ld, perm, robot, rstride, world, ng, n, t); break;
    default: lw_row_quad<3>(s, frames, X, ld, perm, robot, rstride, world, ng, n, t); break;
    }
}

} // namespace

// the three seams: `world` (LstmWorlds) is the kernel's argument, `lds` the body's dynamic block
#undef LSTM_BEGIN_JOB
#undef LSTM_STEP_ROWS
#undef LSTM_STORE_VALUES
#define LSTM_BEGIN_JOB(KEY, J, LD_J, ROTATED, GBASE, NG, N, COLS)                                                            \
    lw_begin_job(world, lds + world.frames, KEY, J, LD_J, robot, rstride, GBASE, NG, A, N, dt);                              \
    const int lane_world = lw_lane_world(GBASE, NG, A);
#define LSTM_STEP_ROWS(X, LD, T) lw_step_rows(world, lds + world.frames, X, LD, perm, robot, rstride, lane_world, ng, n, T)
#define LSTM_STORE_VALUES(OUT, OUT_LD)                                                                                       \
    lstm_store_values<LA_FRAME_FLOATS>(OUT, OUT_LD, gbase, ng, A, lds + world.frames + 7, robot, rstride, gamma, dt, values, tid)
