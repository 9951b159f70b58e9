// value_net_lstm_bf16.hip -- LSTM-RL's decision (value_net_lstm.hip: cs_value_net_decide_lstm) with the opt-in bf16 arithmetic
// (cs_value_net_decide_lstm_bf16; Python: LstmRL.set_recurrent_precision("bf16")).  The recurrent family without map columns only: networks 1
// and 2 on rows of 13 or 15 columns.  The tiling is k_value_net_lstm's -- a workgroup of 4 wavefronts owns 32 sequences, the order of a
// sequence's rows is ranked in LDS, the gates are the TRANSPOSED product (A = the gate weights, rows 8 * gate + unit of a block of 8 hidden
// units; B = the sequences' operand rows from LDS), wavefront w owns the blocks w, w + 4, ..., a lane holds i, f, g, o of four units of one
// sequence, c stays in registers for all n steps -- and so are the sort, sorted_by_distance, the value and the pick (value_net_pick.h).
// What the two kernels do alike is value_net_lstm_kernel.h's, stated once: the layer table, a job's start, the rank pass, the self state, h_n
// into J, the value store, the layer (lstm_layer, here with its in_bf16 / out_bf16 flags set per layer by lstm_chain<LC_BF16_*>) and the
// host's checks and (wreg, mlp1) choice; the bf16 pack of a Linear layer is value_net_bf16.h's.  This file keeps the plan's changes, the LDS
// map, the pack of the gates, the slots of the gate product, the pointwise part, the step loop and the entries.
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

#include "value_net_lstm_kernel.h"

namespace {

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

constexpr int RKH = 4, RKX = 4;            // register-resident gate weights: 16-byte lane slots of W_hh and of the x part a block (RB blocks a wavefront)

// the float32 plan and what this arithmetic changes: ksh k-steps of 16 of W_hh; ksx slots of the x part (network 1: float32 k-groups of 8 of
// W_ih, network 2: k-steps of 16); the strides (floats) of the h rows and of network 2's gate input rows
struct LstmHPlan { LstmPlan q; int ksh, ksx, ld_h, ld_xb; };

__host__ __device__ inline bool lh_f32_layer(const VnPlan& p, int l) { return l == p.c0[0] || l == p.c0[1]; }
// a layer whose output is the operand of a bf16 layer: all of mlp1 (its last output is the gates' operand), mlp but its last layer
inline bool lh_out_bf16(const VnPlan& p, int l) { return l < p.c0[1] || l != p.c0[2] - 1; }

// build_lstm_plan's table with the bf16 layers and the gates counted in 16-byte lane slots, the blob offsets that follow (in floats: a
// lane's 8 bf16 are 4 floats wide, so a piece keeps the size formula ncb * slots * 64 * 4 + ncb * 32) and the strides of bf16 rows
inline int build_lstm_bf16_plan(const int32_t* dims, int n_dims, int cols, LstmHPlan& s)
{
    const int rc = build_lstm_plan(dims, n_dims, cols, s.q);
    if (rc != CS_OK) return rc;
    VnPlan& p = s.q.v;
    VnLayer& g = s.q.g;
    int off = 0, widest = 36;
    for (int l = 0; l < p.n_layers; ++l) {
        if (l == p.c0[1]) {             // the gates lie between the two chains in the blob
            s.ksh = up(s.q.H, 16) / 16;
            s.ksx = p.c0[1] > 0 ? up(s.q.xin, 16) / 16 : up(cols, 8) / 8;
            g.kg_split = s.ksh;
            g.kg_total = s.ksh + s.ksx;
            place_layer(g, off);
        }
        VnLayer& L = p.L[l];
        if (!lh_f32_layer(p, l)) L.kg_split = L.kg_total = up(L.K1, 16) / 16;
        place_layer(L, off);
        const int ld = lh_out_bf16(p, l) ? L.ncb * 16 + 4 : L.ncb * 32 + 4;
        widest = ld > widest ? ld : widest;
    }
    p.ld_pq = widest;
    p.total_floats = off;
    s.ld_h = up(s.q.H, 16) / 2 + 4;
    s.ld_xb = up(s.q.xin, 32) / 2 + 4;
    return CS_OK;
}

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

// (bf16_bits and pack_layer_bf16 -- a bf16 layer's weights where the lanes of lstm_layer read them, cs_value_net_pack_bf16's layout -- are
// value_net_bf16.h's)

// the gate rows where the lanes of the transposed product read them: slot s of block b, lane l, gate row j = l & 31 = 8 * gate + u, torch's
// row gate * H + 8 b + u.  Slots below ksh: 8 bf16 of weight_hh at k = 16 s + 8 (l >> 5) + e.  Behind them the x part: network 2, 8 bf16 of
// weight_ih at k = 16 (s - ksh) + 8 (l >> 5) + e; network 1, 4 floats of weight_ih at k = 8 (s - ksh) + 4 (l >> 5) + e.  bias = b_ih + b_hh
// in float32.  blob zeroed before
inline void pack_gates_bf16(const LstmHPlan& s, const float* wih, const float* whh, const float* bih, const float* bhh, float* fb)
{
    const VnLayer& g = s.q.g;
    const int H = s.q.H, xin = s.q.xin;
    const bool net2 = s.q.v.c0[1] > 0;
    for (int cb = 0; cb < g.ncb; ++cb)
        for (int lane = 0; lane < 64; ++lane) {
            const int j = lane & 31, hh = lane >> 5, unit = cb * 8 + (j & 7), row = (j >> 3) * H + unit;
            if (unit >= H) continue;
            if (hh == 0) fb[g.b_off + cb * 32 + j] = bih[row] + bhh[row];
            for (int sl = 0; sl < g.kg_total; ++sl) {
                float* slot = fb + g.w_off + ((size_t)(cb * g.kg_total + sl) * 64 + lane) * 4;
                uint16_t* hs = reinterpret_cast<uint16_t*>(slot);
                if (sl < s.ksh) {
                    for (int e = 0; e < 8; ++e) {
                        const int k = 16 * sl + 8 * hh + e;
                        if (k < H) hs[e] = bf16_bits(whh[(size_t)row * H + k]);
                    }
                } else if (net2) {
                    for (int e = 0; e < 8; ++e) {
                        const int k = 16 * (sl - s.ksh) + 8 * hh + e;
                        if (k < xin) hs[e] = bf16_bits(wih[(size_t)row * xin + k]);
                    }
                } else {
                    for (int e = 0; e < 4; ++e) {
                        const int k = 8 * (sl - s.ksh) + 4 * hh + e;
                        if (k < xin) slot[e] = wih[(size_t)row * xin + k];
                    }
                }
            }
        }
}

// one 16-byte slot of the x part (network 1: a float32 k-group of W_ih on the raw row; network 2: a bf16 k-step of W_ih on mlp1's rounded
// output) and one of W_hh on the rounded h; `row`: the lane's operand row in LDS at the slot (its sequence, its half of the k range)
template <bool MLP1>
__device__ __forceinline__ void lh_x_slot(f32x16& acc, const float4 w, const float* row)
{
    if constexpr (MLP1) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, w), *reinterpret_cast<const bf16x8*>(row), acc, 0, 0, 0);
    } else {
        const float4 xv = *reinterpret_cast<const float4*>(row);
        LSTM_MFMA4(acc, w, xv)
    }
}

__device__ __forceinline__ void lh_h_slot(f32x16& acc, const float4 w, const float* row)
{
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, w), *reinterpret_cast<const bf16x8*>(row), acc, 0, 0, 0);
}

// the pointwise part of a block: the lane's i, f, g, o of four hidden units of its sequence -> c (float32, in place) and h, rounded once and
// stored as 4 bf16 (units beyond H as 0: the zero weights give 0 for finite inputs only)
__device__ __forceinline__ void lh_pointwise(const f32x16& acc, float (&c)[4], int unit0, int H, __bf16* hdst)
{
    bf16x4 hv;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const float ig = lstm_sigmoid(acc[u]), fg = lstm_sigmoid(acc[4 + u]), gg = lstm_tanh(acc[8 + u]), og = lstm_sigmoid(acc[12 + u]);
        const float cn = fg * c[u] + ig * gg;
        c[u] = cn;
        hv[u] = static_cast<__bf16>(unit0 + u < H ? og * lstm_tanh(cn) : 0.0f);
    }
    *reinterpret_cast<bf16x4*>(hdst + unit0) = hv;
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
    const VnPlan& p = s.q.v;
    if (!n_bytes) return fail(CS_ERR_ARG, "null argument");
    *n_bytes = (size_t)p.total_floats * sizeof(float);
    if (!blob) return CS_OK;
    if (!params) return fail(CS_ERR_ARG, "null argument");
    const int n1 = p.c0[1], n_params = 2 * p.n_layers + 4;
    for (int i = 0; i < n_params; ++i)
        if (!params[i]) return fail(CS_ERR_ARG, "null weight or bias array");
    float* fb = static_cast<float*>(blob);
    memset(fb, 0, (size_t)p.total_floats * sizeof(float));
    for (int l = 0; l < p.n_layers; ++l) {
        const int at = l < n1 ? 2 * l : 2 * l + 4;          // (the LSTM's four arrays lie between mlp1's and mlp's)
        if (lh_f32_layer(p, l)) pack_layer_f32(p.L[l], params[at], params[at + 1], fb);
        else pack_layer_bf16(p.L[l], params[at], params[at + 1], fb);
    }
    pack_gates_bf16(s, params[2 * n1], params[2 * n1 + 1], params[2 * n1 + 2], params[2 * n1 + 3], fb);
    return CS_OK;
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
