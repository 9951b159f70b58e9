// value_net_lstm_bf16.hip -- LSTM-RL's decision (value_net_lstm.hip: cs_value_net_decide_lstm) with the opt-in bf16 arithmetic
// (cs_value_net_decide_lstm_bf16; Python: LstmRL.set_recurrent_precision("bf16")).  The recurrent family without map columns only: networks 1
// and 2 on rows of 13 or 15 columns.  The tiling is k_value_net_lstm's -- a workgroup of 4 wavefronts owns 32 sequences, the order of a
// sequence's rows is ranked in LDS, the gates are the TRANSPOSED product (A = the gate weights, rows 8 * gate + unit of a block of 8 hidden
// units; B = the sequences' operand rows from LDS), wavefront w owns the blocks w, w + 4, ..., a lane holds i, f, g, o of four units of one
// sequence, c stays in registers for all n steps -- and so are the sort, sorted_by_distance, the value and the pick (value_net_pick.h).
// What the two kernels do alike is value_net_lstm_kernel.h's, stated once: the layer table, a job's start, the rank pass, the self state, h_n
// into J, the value store, the layer (lstm_layer, here with its in_bf16 / out_bf16 flags set per layer by lstm_chain<LC_BF16_*>) and the
// host's checks and (wreg, mlp1) choice; the bf16 pack of a Linear layer is value_net_bf16.h's.  What this arithmetic adds for both of its
// kernels (this one and k_value_net_lstm_om_bf16, value_net_lstm_om_bf16.hip) is value_net_lstm_bf16.h's: the plan's changes, the pack of the
// gates and of a blob, the slots of the gate product, the pointwise part.  This file keeps the LDS map, the step loop and the entries.
//
// The arithmetic:
//   float32 layers   network 1's W_ih on the raw row x_t, network 2's mlp1 layer 0, layer 0 of mlp (it reads the raw self state): full
//                    weights, unrounded inputs, v_mfma_f32_32x32x2_f32.  Columns reach 10 m, where one bf16 step is 3 cm.
//   bf16 layers      W_hh in both networks, network 2's W_ih (it reads mlp1's output), every mlp1 / mlp layer behind the first: weights
//                    rounded to bf16 (nearest even) at pack time, float32 biases, float32 accumulation, v_mfma_f32_32x32x16_bf16.
//   rounding points  each value once, nearest even, when it is stored as a bf16 operand: h_t after o * tanh(c) -- that one rounded value is
//                    the next step's operand and what mlp reads as h_n --; an mlp1 / mlp activation after the bias and the ReLU when a bf16
//                    layer reads it; mlp1's last output (no ReLU) as the gates' operand of network 2.
//   never rounded    c, the gate pre-activations, sigmoid and tanh (lstm_sigmoid, lstm_tanh), mlp's last output, rewards + gamma^(dt v_pref) V.
//   order            a gate pre-activation is one fixed chain: b_ih + b_hh (summed in float32 by the pack), the x part (network 1: the
//                    float32 k-groups ascending; network 2: W_ih's k-steps of 16 ascending), then W_hh's k-steps of 16 ascending.
// The x part does not depend on h: the register-resident build issues it before the barrier that publishes h_{t-1}, so that only W_hh's
// k-steps and the pointwise part lie between two barriers.  Hidden units beyond H are stored as exact 0.  A sequence's result depends on
// its own rows alone: the same bits for W = 1 as inside any batch, at any position of a tile.  No atomics.  gfx950 only.
//
// LDS image of a bf16 operand (value_net_bf16.hip's): row-major bfloat16, a row of 16 * odd bytes (a stride of 4 * odd floats); lane l reads
// the 8 k at 16 s + 8 (l >> 5) of row l & 31 with one ds_read_b128, conflict-free.  h: [2][32] rows of ceil(H / 16) * 16 bf16 (+ 8 bytes
// of pitch), double-buffered; network 2's gate input: [32] rows of mlp1's last width rounded up to 32.
#include <hip/hip_runtime.h>

#include "value_net_lstm_bf16.h"

namespace {

struct LstmHLds { int key, perm, G, HB, XB, P, Q, J, LT, total; };

inline LstmHLds lstm_bf16_lds_map(const LstmHPlan& s, int n)
{
    const VnPlan& p = s.q.v;
    LstmHLds m{};
    int o = 0;
    auto take = [&](int floats) { const int at = o; o += up(floats, 4); return at; };
    m.key = take(TILE_M * n);
    m.perm = take(TILE_M * n);
    m.G = take(2 * TILE_M * LDX);
    m.HB = take(2 * TILE_M * s.ld_h);
    m.XB = p.c0[1] > 0 ? take(TILE_M * s.ld_xb) : m.HB;
    m.P = take(TILE_M * p.ld_pq);
    m.Q = take(TILE_M * p.ld_pq);
    m.J = take(JROWS * p.ld_j);
    m.LT = take(VN_MAX_LAYERS * 8);
    m.total = o;
    return m;
}

template <bool WREG, bool MLP1>
__global__ __launch_bounds__(NT, 2) void k_value_net_lstm_bf16(LstmHPlan s, LstmHLds m, const float* __restrict__ wb, int NG, int A, int n, int sorted,
                                                            const float* __restrict__ rotated, const float* __restrict__ rewards,
                                                            const float* __restrict__ robot, int rstride, float gamma, float dt, float* __restrict__ values)
{
    extern __shared__ float lds[];
    constexpr int NB = WREG ? RB : GB;
    const LstmPlan& q = s.q;
    const VnPlan& p = q.v;
    float *P = lds + m.P, *Q = lds + m.Q, *J = lds + m.J, *G = lds + m.G, *HB = lds + m.HB, *XB = lds + m.XB;
    unsigned* key = reinterpret_cast<unsigned*>(lds + m.key);
    int* perm = reinterpret_cast<int*>(lds + m.perm);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), hh = lane >> 5, li = lane & 31;
    const int row8 = tid >> 3;
    const int cols = p.cols, H = q.H, ldh = s.ld_h, ksh = s.ksh, ksx = s.ksx, KT = q.g.kg_total;
    const int nbw = (q.g.ncb - wave + 3) >> 2;              // this wavefront's blocks: wave, wave + 4, ...
    constexpr int gbuf = TILE_M * LDX;
    const float4* gw = reinterpret_cast<const float4*>(wb + q.g.w_off) + lane;
    int out_ld;

    int* ltab = reinterpret_cast<int*>(lds + m.LT);
    LSTM_FILL_TABLE(ltab, p)

    float4 wh[RB][RKH], wx[RB][RKX];
    if constexpr (WREG) {
        const int slots = q.g.ncb * KT;
#pragma unroll
        for (int bi = 0; bi < RB; ++bi) {
            const int at = ((tid >> 6) + 4 * bi) * KT;             // (clamped: what lies beyond the wavefront's blocks and slots is never used)
#pragma unroll
            for (int k = 0; k < RKH; ++k) wh[bi][k] = gw[(at + k < slots ? at + k : 0) * 64];
#pragma unroll
            for (int j = 0; j < RKX; ++j) wx[bi][j] = gw[(at + ksh + j < slots ? at + ksh + j : 0) * 64];
        }
    }

    for (int job = blockIdx.x; job * JROWS < NG; job += gridDim.x) {
        const long gbase = (long)job * JROWS;
        const int ng = NG - gbase < JROWS ? (int)(NG - gbase) : JROWS;
        LSTM_BEGIN_JOB(key, J, p.ld_j, rotated, gbase, ng, n, cols)
        for (int i = tid; i < 2 * TILE_M * ldh; i += NT) HB[i] = 0.0f;           // h0 = 0, and the columns between H and the last k-step's end
        __syncthreads();
        LSTM_RANK(key, perm, n, ng, sorted)
        __syncthreads();
        lstm_gather(G, LDX, rotated, perm, gbase, ng, n, cols, 0);
        float c[NB][4];
#pragma unroll
        for (int bi = 0; bi < NB; ++bi)
#pragma unroll
            for (int u = 0; u < 4; ++u) c[bi][u] = 0.0f;
        __syncthreads();
        lstm_self_state(J, p.ld_j, G, LDX, ng, tid);

        for (int t = 0; t < n; ++t) {
            const float* hrow = HB + (t & 1) * TILE_M * ldh + li * ldh + 4 * hh;
            __bf16* hdst = reinterpret_cast<__bf16*>(HB + ((t + 1) & 1) * TILE_M * ldh + li * ldh);
            if (t + 1 < n) lstm_gather(G + ((t + 1) & 1) * gbuf, LDX, rotated, perm, gbase, ng, n, cols, t + 1);
            if constexpr (MLP1) lstm_chain<LC_BF16_MLP1>(ltab, p.ld_pq, wb, P, Q, p.c0[0], p.c0[1], G + (t & 1) * gbuf, LDX, XB, s.ld_xb, out_ld);
            const float* xrow = (MLP1 ? XB + li * s.ld_xb : G + (t & 1) * gbuf + li * LDX) + 4 * hh;
            if constexpr (WREG) {
                // the x part of every block of the wavefront, then the barrier that publishes h_{t-1}, then W_hh and the pointwise part
                f32x16 acc[RB];
#pragma unroll
                for (int bi = 0; bi < RB; ++bi) {
                    if (bi >= nbw) break;
                    const float* bias = wb + q.g.b_off + (wave + 4 * bi) * 32 + 4 * hh;
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[bi][r] = bias[(r & 3) + 8 * (r >> 2)];
#pragma unroll
                    for (int j = 0; j < RKX; ++j)
                        if (j < ksx) lh_x_slot<MLP1>(acc[bi], wx[bi][j], xrow + 8 * j);
                }
                __syncthreads();
#pragma unroll
                for (int bi = 0; bi < RB; ++bi) {
                    if (bi >= nbw) break;
#pragma unroll
                    for (int k = 0; k < RKH; ++k)
                        if (k < ksh) lh_h_slot(acc[bi], wh[bi][k], hrow + 8 * k);
                    lh_pointwise(acc[bi], c[bi], (wave + 4 * bi) * 8 + 4 * hh, H, hdst);
                }
            } else {
                // the same chain per block, its weights from the blob; the second barrier keeps the next step's gather and mlp1 off this step's rows
                __syncthreads();
#pragma unroll
                for (int bi = 0; bi < NB; ++bi) {
                    if (bi >= nbw) break;
                    const int blk = wave + 4 * bi;
                    const float* bias = wb + q.g.b_off + blk * 32 + 4 * hh;
                    f32x16 acc;
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[r] = bias[(r & 3) + 8 * (r >> 2)];
                    const float4* w = gw + (long)blk * KT * 64;
                    float4 nw = w[(long)ksh * 64];
                    for (int j = 0; j < ksx; ++j) {
                        const float4 wv = nw;
                        nw = w[(long)(j + 1 < ksx ? ksh + j + 1 : 0) * 64];
                        lh_x_slot<MLP1>(acc, wv, xrow + 8 * j);
                    }
                    for (int k = 0; k < ksh; ++k) {
                        const float4 wv = nw;
                        nw = w[(long)(k + 1 < ksh ? k + 1 : k) * 64];
                        lh_h_slot(acc, wv, hrow + 8 * k);
                    }
                    lh_pointwise(acc, c[bi], blk * 8 + 4 * hh, H, hdst);
                }
                __syncthreads();
            }
        }
        if constexpr (WREG) __syncthreads();          // (publishes h_n)

        lstm_hn_to_j(J, p.ld_j, reinterpret_cast<const __bf16*>(HB + (n & 1) * TILE_M * ldh), 2 * ldh, H, tid);
        __syncthreads();
        const float* out = lstm_chain<LC_BF16_MLP>(ltab, p.ld_pq, wb, P, Q, p.c0[1], p.c0[2], J, p.ld_j, nullptr, 0, out_ld);
        lstm_store_values(out, out_ld, gbase, ng, A, rewards, robot, rstride, gamma, dt, values, tid);
        __syncthreads();
    }
}

} // namespace

#include "value_net_pick.h"

extern "C" int cs_value_net_pack_lstm_bf16(const int32_t* dims, int n_dims, int cols, const float* const* params, void* blob, size_t* n_bytes)
{
    LstmHPlan s;
    const int rc = build_lstm_bf16_plan(dims, n_dims, cols, s);
    if (rc != CS_OK) return rc;
    return pack_lstm_bf16_blob(s, 0, params, blob, n_bytes);
}

extern "C" int cs_value_net_decide_lstm_bf16(const int32_t* dims, int n_dims, const void* d_weights, size_t n_weight_bytes, int W, int A, int n, int cols,
                                             int sorted_by_distance, const float* d_rotated, const float* d_rewards, const float* d_actions,
                                             const float* d_robot, int robot_stride, float gamma, float dt, const int32_t* d_override, float* d_values,
                                             int32_t* d_choice, float* d_action_out, void* stream)
{
    LstmHPlan s;
    const int rc = build_lstm_bf16_plan(dims, n_dims, cols, s);
    if (rc != CS_OK) return rc;
    const LstmPlan& q = s.q;
    // (a length that is no whole number of floats is no blob of any network: it fails the size check as SIZE_MAX floats)
    const size_t n_floats = n_weight_bytes % sizeof(float) ? (size_t)-1 : n_weight_bytes / sizeof(float);
    const int rc2 = lstm_check_decide("cs_value_net_decide_lstm_bf16", q.v, d_weights, n_floats, W, A, n, sorted_by_distance, d_rotated, d_rewards, d_actions,
                                      d_robot, robot_stride, d_values, d_action_out);
    if (rc2 != CS_OK) return rc2;
    const LstmHLds m = lstm_bf16_lds_map(s, n);
    const bool wreg = q.g.ncb <= 4 * RB && s.ksh <= RKH && s.ksx <= RKX, mlp1 = q.v.c0[1] > 0;
    const float* wb = static_cast<const float*>(d_weights);
    const int rc3 = lstm_launch(m.total, W, A, wreg, mlp1, [&](auto WR, auto M1, size_t shmem, int NG, int grid) {
        constexpr auto kernel = k_value_net_lstm_bf16<decltype(WR)::value, decltype(M1)::value>;
        const int rc4 = grant_lds<kernel>(shmem);
        if (rc4 != CS_OK) return rc4;
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(NT), shmem, (hipStream_t)stream, s, m, wb, NG, A, n, sorted_by_distance, d_rotated, d_rewards, d_robot,
                           robot_stride, gamma, dt, d_values);
        return (int)CS_OK;
    });
    if (rc3 != CS_OK) return rc3;
    return launch_pick(W, A, d_values, d_actions, d_robot, robot_stride, d_override, d_choice, d_action_out, stream);
}
