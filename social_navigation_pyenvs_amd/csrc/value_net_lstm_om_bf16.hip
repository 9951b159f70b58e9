// value_net_lstm_om_bf16.hip -- OM-LSTM-RL's decision (value_net_lstm.hip: cs_value_net_decide_lstm_om) with the opt-in bf16 arithmetic
// (cs_value_net_decide_lstm_om_bf16; Python: OMLstmRL.set_mapped_precision("bf16")): the recurrent network on rows of 13 | 15 rotated columns
// followed by om_cols occupancy-map columns.  From k_value_net_lstm_bf16 (value_net_lstm_bf16.hip) it has the tiling, the rank pass,
// sorted_by_distance, the h / c handling and the pick, through value_net_lstm_kernel.h and value_net_lstm_bf16.h; from k_value_net_lstm_om the
// map pairing: one map row per (world, human) read in place from d_maps [W][n][om_cols], a step's row beside its own map (CS_VN_MAPS_OWN) or
// beside the map at that place of the order of the world's action 0 (CS_VN_MAPS_FIRST_ACTION), which every workgroup ranks itself from
// that pair's own rows of d_rotated, whichever tile they lie in.  This file keeps the LDS map, the gather of the map columns, network 2's
// first layer, the step loop and the entries.
//
// The arithmetic.  The first layer that reads a row -- network 1's W_ih, network 2's mlp1 layer 0 -- is split by column:
//   float32          its 13 | 15 rotated columns: full weights, unrounded inputs, v_mfma_f32_32x32x2_f32 (they reach 10 m, where one bf16 step
//                    is 3 cm); and layer 0 of mlp, which reads the raw self state, as in the narrow bf16 kernel.
//   bf16             its map columns: the weights [:, cols:] rounded to bf16 (nearest even) at pack time, a map value rounded once, nearest
//                    even, when the gather stages it as an operand (an occupancy is 0 or 1, a mean velocity a few m/s), zeros up to a
//                    multiple of 16 columns, float32 accumulation, v_mfma_f32_32x32x16_bf16; and everything the narrow bf16 kernel runs in
//                    bf16: W_hh, network 2's W_ih, the layers behind each chain's first.
//   rounding points  and what is never rounded are value_net_lstm_bf16.hip's: h_t once a step; c, the pre-activations, sigmoid and tanh,
//                    mlp's last output and rewards + gamma^(dt v_pref) V stay float32.
//   order            a first-layer pre-activation is one fixed chain: the bias (the gates': b_ih + b_hh, summed in float32 by the pack),
//                    the two float32 k-groups of the rotated columns ascending, the map k-steps of 16 ascending, and for network 1's gates
//                    then W_hh's k-steps of 16 ascending.  With all-zero map weights and finite maps the map k-steps add exact zeros: the
//                    values are cs_value_net_decide_lstm_bf16's on the narrow network, bit for bit.
// The order of a sequence's rows is worked out on the float32 distances before any rounding: keys, permutations, ties and NaN distances
// are k_value_net_lstm_om's.  A sequence's value depends on its own rows and the map rows it reads: the same bits for W = 1 as inside any
// batch, at any position of a tile.  No atomics, no inline assembly.  gfx950 only.
//
// Register-resident weights (network 1, <true, false>): beside W_hh's RKH slots a block holds the x part's KGF float32 slots and RKM = 3 map
// k-steps (om_cols <= 48, the reference's 4 x 4 x 3 maps), 9 slots x 2 blocks = 72 VGPRs; they stay resident because the x part is what this
// arithmetic shortens, and reading the slots from the blob would put a global load in front of every map k-step of every step.  A fourth
// resident k-step fills the 256 VGPRs of two workgroups a CU and spills (8 bytes of scratch): wider maps read the gates from the blob.
// Network 2's map weights belong to mlp1's first layer, which reads its weights from the blob as every layer does (lstm_layer's one-deep
// prefetch); its gates are the narrow kernel's.  DESIGN.md 4.5 has the compiler's figures.
//
// LDS: the narrow bf16 kernel's map, and the map columns as bf16 rows MB [2][32][ceil(om_cols / 16) * 16 (+ 8 bytes of pitch)], double-
// buffered beside the gather tile G of the rotated columns; the keys and the order of action 0 behind everything else.
#include <hip/hip_runtime.h>

#include "value_net_lstm_bf16.h"

namespace {

constexpr int RKM = 3;                      // register-resident map k-steps of 16 a block (network 1): the reference's 48 map columns

// what the map columns add to a launch: the maps [W][n][om_cols], which map a step pairs with its row, ksm k-steps of 16 and the stride
// (floats) of a bf16 map row in LDS
struct LstmOmH { const float* maps; int om_cols, map_order, ksm, ld_m; };

struct LstmOmHLds { int key, perm, G, MB, HB, XB, P, Q, J, LT, key0, perm0, total; };

inline LstmOmHLds lstm_om_bf16_lds_map(const LstmHPlan& s, int n, int ld_m)
{
    const VnPlan& p = s.q.v;
    LstmOmHLds m{};
    int o = 0;
    auto take = [&](int floats) { const int at = o; o += up(floats, 4); return at; };
    m.key = take(TILE_M * n);
    m.perm = take(TILE_M * n);
    m.G = take(2 * TILE_M * LDX);
    m.MB = take(2 * TILE_M * ld_m);
    m.HB = take(2 * TILE_M * s.ld_h);
    m.XB = p.c0[1] > 0 ? take(TILE_M * s.ld_xb) : m.HB;
    m.P = take(TILE_M * p.ld_pq);
    m.Q = take(TILE_M * p.ld_pq);
    m.J = take(JROWS * p.ld_j);
    m.LT = take(VN_MAX_LAYERS * 8);
    m.key0 = take(TILE_M * n);
    m.perm0 = take(TILE_M * n);
    m.total = o;
    return m;
}

// the map columns of step t, eight lanes a sequence: maps[world of g][mperm[s][t]][0..om_cols), each value rounded once to bf16, zeros up to
// the last k-step's end and for the sequences beyond ng
__device__ __forceinline__ void lom_gather_maps(__bf16* MB, int ldb, const LstmOmH& om, const int* mperm, long gbase, int ng, int A, int n, int t)
{
    const int s = threadIdx.x >> 3;
    const bool live = s < ng;
    const long mrow = live ? (((gbase + s) / A) * n + mperm[s * n + t]) * om.om_cols : 0;
    for (int c = threadIdx.x & 7; c < 16 * om.ksm; c += 8) MB[s * ldb + c] = static_cast<__bf16>(live && c < om.om_cols ? om.maps[mrow + c] : 0.0f);
}

// network 2's mlp1 layer 0 on the tile's 32 rows: lstm_layer's float32 k-groups on the rotated columns (xf, stride ldf), then bf16 k-steps
// on the staged map columns (xm, stride ldm floats) -- the same blob walk and one-deep prefetch, the slots in the pack's order --, the
// output the operand of a bf16 layer (or of the gates): bfloat16 rows of 2 * ldd elements, rounded after the bias and the ReLU
__device__ __forceinline__ void lom_first_layer(const int* lt, const float* __restrict__ wb, const float* xf, int ldf, const float* xm, int ldm, float* dst, int ldd)
{
    const auto field = [&](int k) { return __builtin_amdgcn_readfirstlane(lt[k]); };
    const struct { int N, kg_total, ncb, relu, w_off, b_off; } L{field(LT_N), field(LT_KG), field(LT_NCB), field(LT_RELU), field(LT_W), field(LT_B)};
    const int lane = threadIdx.x & 63, h = lane >> 5, li = lane & 31, KG = L.kg_total;
    const float* a1 = xf + li * ldf + 4 * h;
    const float* am = xm + li * ldm + 4 * h;
    for (int cb = threadIdx.x >> 6; cb < L.ncb; cb += 4) {
        const float4* bw = reinterpret_cast<const float4*>(wb + L.w_off) + cb * KG * 64 + lane;
        const float bias = wb[L.b_off + cb * 32 + li];
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = bias;
        float4 nw = bw[0];
#pragma unroll
        for (int kg = 0; kg < KGF; ++kg) {
            const float4 w = nw;
            nw = bw[(kg + 1) * 64];                        // (KG > KGF: om_cols >= 1)
            const float4 a = *reinterpret_cast<const float4*>(a1 + kg * 8);
            LSTM_MFMA4(acc, a, w)
        }
        for (int kg = KGF; kg < KG; ++kg) {
            const float4 w = nw;
            nw = bw[(kg + 1 < KG ? kg + 1 : kg) * 64];
            const float4 a = *reinterpret_cast<const float4*>(am + (kg - KGF) * 8);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, w), acc, 0, 0, 0);
        }
        const bool pad = cb * 32 + li >= L.N;              // (the zero weights give 0 * inf = NaN there when an input is infinite)
        __bf16* dh = reinterpret_cast<__bf16*>(dst) + 4 * h * 2 * ldd + (cb * 32 + li);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = acc[r];
            if (L.relu) v = v < 0.0f ? 0.0f : v;          // (a NaN stays a NaN, as torch's ReLU leaves it)
            dh[((r & 3) + 8 * (r >> 2)) * 2 * ldd] = static_cast<__bf16>(pad ? 0.0f : v);
        }
    }
}

// slot j of the x part of the gates: network 2, the narrow kernel's bf16 k-step on mlp1's rounded output; network 1, a float32 k-group of
// the rotated columns (j < KGF) or a bf16 k-step of the staged map columns behind them
template <bool MLP1>
__device__ __forceinline__ void lom_x_slot(f32x16& acc, const float4 w, int j, const float* xrow, const float* mrow)
{
    if constexpr (MLP1) {
        lh_x_slot<true>(acc, w, xrow + 8 * j);
    } else {
        if (j < KGF) lh_x_slot<false>(acc, w, xrow + 8 * j);
        else lh_h_slot(acc, w, mrow + 8 * (j - KGF));
    }
}

template <bool WREG, bool MLP1>
__global__ __launch_bounds__(NT, 2) void k_value_net_lstm_om_bf16(LstmHPlan s, LstmOmHLds m, const float* __restrict__ wb, int NG, int A, int n, int sorted,
                                                               const float* __restrict__ rotated, const float* __restrict__ rewards,
                                                               const float* __restrict__ robot, int rstride, float gamma, float dt,
                                                               float* __restrict__ values, LstmOmH om)
{
    extern __shared__ float lds[];
    constexpr int NB = WREG ? RB : GB;
    constexpr int NX = MLP1 ? RKX : KGF + RKM;              // register-resident slots of the x part a block
    const LstmPlan& q = s.q;
    const VnPlan& p = q.v;
    float *P = lds + m.P, *Q = lds + m.Q, *J = lds + m.J, *G = lds + m.G, *HB = lds + m.HB, *XB = lds + m.XB, *MB = lds + m.MB;
    unsigned* key = reinterpret_cast<unsigned*>(lds + m.key);
    int* perm = reinterpret_cast<int*>(lds + m.perm);
    unsigned* key0 = reinterpret_cast<unsigned*>(lds + m.key0);
    int* perm0 = reinterpret_cast<int*>(lds + m.perm0);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), hh = lane >> 5, li = lane & 31;
    const int row8 = tid >> 3;
    const int cols = p.cols, H = q.H, ldh = s.ld_h, ldm = om.ld_m, ksh = s.ksh, ksx = s.ksx, KT = q.g.kg_total;
    const int nbw = (q.g.ncb - wave + 3) >> 2;              // this wavefront's blocks: wave, wave + 4, ...
    constexpr int gbuf = TILE_M * LDX;
    const int mbuf = TILE_M * ldm;
    const float4* gw = reinterpret_cast<const float4*>(wb + q.g.w_off) + lane;
    int out_ld;

    int* ltab = reinterpret_cast<int*>(lds + m.LT);
    LSTM_FILL_TABLE(ltab, p)

    float4 wh[RB][RKH], wx[RB][NX];
    if constexpr (WREG) {
        const int slots = q.g.ncb * KT;
#pragma unroll
        for (int bi = 0; bi < RB; ++bi) {
            const int at = ((tid >> 6) + 4 * bi) * KT;             // (clamped: what lies beyond the wavefront's blocks and slots is never used)
#pragma unroll
            for (int k = 0; k < RKH; ++k) wh[bi][k] = gw[(at + k < slots ? at + k : 0) * 64];
#pragma unroll
            for (int j = 0; j < NX; ++j) wx[bi][j] = gw[(at + ksh + j < slots ? at + ksh + j : 0) * 64];
        }
    }

    for (int job = blockIdx.x; job * JROWS < NG; job += gridDim.x) {
        const long gbase = (long)job * JROWS;
        const int ng = NG - gbase < JROWS ? (int)(NG - gbase) : JROWS;
        LSTM_BEGIN_JOB(key, J, p.ld_j, rotated, gbase, ng, n, cols)
        for (int i = tid; i < 2 * TILE_M * ldh; i += NT) HB[i] = 0.0f;           // h0 = 0, and the columns between H and the last k-step's end
        // which map a step takes: its row's own (mperm = perm), or the one at that place in the order of the world's action 0, which is worked
        // out from that pair's own rows of `rotated`, whichever tile they lie in (uniform over the workgroup: every barrier is reached by all)
        const bool first_order = om.map_order == CS_VN_MAPS_FIRST_ACTION && sorted;
        const int* mperm = first_order ? perm0 : perm;
        if (first_order) {
            const long pair0 = (gbase + (row8 < ng ? row8 : 0)) / A * A;
            for (int j = tid & 7; j < n && row8 < ng; j += 8) key0[row8 * n + j] = lstm_key(rotated[(pair0 * n + j) * cols + 11]);
        }
        __syncthreads();
        if (first_order) LSTM_RANK(key0, perm0, n, ng, true)
        LSTM_RANK(key, perm, n, ng, sorted)
        __syncthreads();
        lstm_gather(G, LDX, rotated, perm, gbase, ng, n, cols, 0);
        lom_gather_maps(reinterpret_cast<__bf16*>(MB), 2 * ldm, om, mperm, gbase, ng, A, n, 0);
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
            if (t + 1 < n) {
                lstm_gather(G + ((t + 1) & 1) * gbuf, LDX, rotated, perm, gbase, ng, n, cols, t + 1);
                lom_gather_maps(reinterpret_cast<__bf16*>(MB + ((t + 1) & 1) * mbuf), 2 * ldm, om, mperm, gbase, ng, A, n, t + 1);
            }
            if constexpr (MLP1) {
                // mlp1: its first layer here (into Q, or straight into the gates' operand rows when it is the only one), the others as the narrow kernel's
                const bool only = p.c0[1] - p.c0[0] == 1;
                lom_first_layer(ltab + p.c0[0] * LT_STRIDE, wb, G + (t & 1) * gbuf, LDX, MB + (t & 1) * mbuf, ldm, only ? XB : Q, only ? s.ld_xb : p.ld_pq);
                __syncthreads();
                if (!only) lstm_chain<LC_BF16_MLP1_REST>(ltab, p.ld_pq, wb, P, Q, p.c0[0] + 1, p.c0[1], Q, p.ld_pq, XB, s.ld_xb, out_ld);
            }
            const float* xrow = (MLP1 ? XB + li * s.ld_xb : G + (t & 1) * gbuf + li * LDX) + 4 * hh;
            const float* mrow = MB + (t & 1) * mbuf + li * ldm + 4 * hh;
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
                    for (int j = 0; j < NX; ++j)
                        if (j < ksx) lom_x_slot<MLP1>(acc[bi], wx[bi][j], j, xrow, mrow);
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
                        lom_x_slot<MLP1>(acc, wv, j, xrow, mrow);
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

extern "C" int cs_value_net_pack_lstm_om_bf16(const int32_t* dims, int n_dims, int cols, int om_cols, const float* const* params, void* blob,
                                              size_t* n_bytes)
{
    LstmHPlan s;
    const int rc = build_lstm_bf16_plan(dims, n_dims, cols, s, true, om_cols);
    if (rc != CS_OK) return rc;
    return pack_lstm_bf16_blob(s, om_cols, params, blob, n_bytes);
}

extern "C" int cs_value_net_decide_lstm_om_bf16(const int32_t* dims, int n_dims, const void* d_weights, size_t n_weight_bytes, int W, int A, int n,
                                                int cols, int om_cols, int sorted_by_distance, int map_order, const float* d_rotated,
                                                const float* d_maps, const float* d_rewards, const float* d_actions, const float* d_robot,
                                                int robot_stride, float gamma, float dt, const int32_t* d_override, float* d_values,
                                                int32_t* d_choice, float* d_action_out, void* stream)
{
    LstmHPlan s;
    const int rc = build_lstm_bf16_plan(dims, n_dims, cols, s, true, om_cols);
    if (rc != CS_OK) return rc;
    const LstmPlan& q = s.q;
    // (a length that is no whole number of floats is no blob of any network: it fails the size check as SIZE_MAX floats)
    const size_t n_floats = n_weight_bytes % sizeof(float) ? (size_t)-1 : n_weight_bytes / sizeof(float);
    const int rc2 = lstm_check_decide("cs_value_net_decide_lstm_om_bf16", q.v, d_weights, n_floats, W, A, n, sorted_by_distance, d_rotated, d_rewards,
                                      d_actions, d_robot, robot_stride, d_values, d_action_out, true, d_maps, map_order);
    if (rc2 != CS_OK) return rc2;
    LstmOmH om{d_maps, om_cols, map_order, up(om_cols, 16) / 16, up(om_cols, 16) / 2 + 4};
    const LstmOmHLds m = lstm_om_bf16_lds_map(s, n, om.ld_m);
    const bool mlp1 = q.v.c0[1] > 0;
    const bool wreg = q.g.ncb <= 4 * RB && s.ksh <= RKH && s.ksx <= (mlp1 ? RKX : KGF + RKM);
    const float* wb = static_cast<const float*>(d_weights);
    const int rc3 = lstm_launch(m.total, W, A, wreg, mlp1, [&](auto WR, auto M1, size_t shmem, int NG, int grid) {
        constexpr auto kernel = k_value_net_lstm_om_bf16<decltype(WR)::value, decltype(M1)::value>;
        const int rc4 = grant_lds<kernel>(shmem);
        if (rc4 != CS_OK) return rc4;
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(NT), shmem, (hipStream_t)stream, s, m, wb, NG, A, n, sorted_by_distance, d_rotated, d_rewards, d_robot,
                           robot_stride, gamma, dt, d_values, om);
        return (int)CS_OK;
    });
    if (rc3 != CS_OK) return rc3;
    return launch_pick(W, A, d_values, d_actions, d_robot, robot_stride, d_override, d_choice, d_action_out, stream);
}
