// value_net_lstm_bf16.h -- the opt-in bf16 arithmetic of the recurrent decision, beside value_net_lstm_kernel.h: what k_value_net_lstm_bf16
// (value_net_lstm_bf16.hip, rows of 13 | 15 columns; LstmRL.set_recurrent_precision("bf16")) and k_value_net_lstm_om_bf16
// (value_net_lstm_om_bf16.hip, the rows widened by om_cols occupancy-map columns; OMLstmRL.set_mapped_precision("bf16")) have in common.  The
// kernel text is value_net_lstm_bf16_body.inc, included by each file; here are the host's side -- the plan's changes, the pack of the gates
// and of a whole blob, the LDS map, a decide entry behind its name -- and the device's small pieces: one slot of W_hh on the rounded h, one
// of the narrow x part, the pointwise part.  om_cols = 0 everywhere below is the narrow network, whose plan and blob are what they were before
// there were map columns here.  Unnamed namespace: each translation unit gets its own copy.
//
// The tiling is k_value_net_lstm's (value_net_lstm.hip) -- a workgroup of 4 wavefronts owns 32 sequences, the order of a sequence's rows is
// ranked in LDS on the float32 distances before any rounding, the gates are the TRANSPOSED product (A = the gate weights, rows 8 * gate + unit
// of a block of 8 hidden units; B = the sequences' operand rows from LDS), wavefront w owns the blocks w, w + 4, ..., a lane holds i, f, g, o
// of four units of one sequence, c stays in registers for all n steps -- and so are the sort, sorted_by_distance, the map pairing, the value
// and the pick (value_net_pick.h).
//
// The arithmetic, said here for both kernels:
//   float32 layers   the 13 | 15 rotated columns of the first layer that reads a row -- network 1's W_ih, network 2's mlp1 layer 0 -- and layer 0
//                    of mlp (it reads the raw self state): full weights, unrounded inputs, v_mfma_f32_32x32x2_f32.  Columns reach 10 m, where
//                    one bf16 step is 3 cm.
//   bf16 layers      W_hh in both networks, network 2's W_ih (it reads mlp1's output), every mlp1 / mlp layer behind the first, and the map
//                    columns [:, cols:] of the first layer that reads a row: weights rounded to bf16 (nearest even) at pack time, float32
//                    biases, float32 accumulation, v_mfma_f32_32x32x16_bf16.
//   rounding points  each value once, nearest even, when it is stored as a bf16 operand: h_t after o * tanh(c) -- that one rounded value is
//                    the next step's operand and what mlp reads as h_n --; an mlp1 / mlp activation after the bias and the ReLU when a bf16
//                    layer reads it; mlp1's last output (no ReLU) as the gates' operand of network 2; a map value when the gather stages it
//                    (an occupancy is 0 or 1, a mean velocity a few m/s), zeros up to a multiple of 16 columns.
//   never rounded    c, the gate pre-activations, sigmoid and tanh (lstm_sigmoid, lstm_tanh), mlp's last output, rewards + gamma^(dt v_pref) V.
//   order            a gate pre-activation is one fixed chain: b_ih + b_hh (summed in float32 by the pack), the x part (network 1: the
//                    float32 k-groups of the rotated columns ascending, then the map k-steps of 16 ascending; network 2: W_ih's k-steps of
//                    16 ascending), then W_hh's k-steps of 16 ascending.  Network 2's mlp1 layer 0 on rows with maps: the bias, the float32
//                    k-groups, the map k-steps.  With all-zero map weights and finite maps the map k-steps add exact zeros: the values are
//                    the narrow kernel's on the narrow network, bit for bit.
// The x part does not depend on h: the register-resident build issues it before the barrier that publishes h_{t-1}, so that only W_hh's
// k-steps and the pointwise part lie between two barriers.  Hidden units beyond H are stored as exact 0.  A sequence's value depends on its
// own rows and the map rows it reads: the same bits for W = 1 as inside any batch, at any position of a tile.  No atomics, no inline
// assembly.  gfx950 only.
//
// Register-resident weights (<true, .>): a block holds RKH slots of W_hh and RKX of the x part; network 1 with map columns holds the x part's
// KGF float32 slots and RKM = 3 map k-steps (om_cols <= 48, the reference's 4 x 4 x 3 maps), 9 slots x 2 blocks = 72 VGPRs -- they stay
// resident because the x part is what this arithmetic shortens, and reading the slots from the blob would put a global load in front of
// every map k-step of every step.  A fourth resident k-step fills the 256 VGPRs of two workgroups a CU and spills (8 bytes of scratch):
// wider maps read the gates from the blob.  Network 2's map weights belong to mlp1's first layer, which reads its weights from the blob as
// every layer does (lstm_layer's one-deep prefetch); its gates are the narrow kernel's.  DESIGN.md 4.5 has the compiler's figures.
//
// LDS image of a bf16 operand (value_net_bf16.hip's): row-major bfloat16, a row of 16 * odd bytes (a stride of 4 * odd floats); lane l reads
// the 8 k at 16 s + 8 (l >> 5) of row l & 31 with one ds_read_b128, conflict-free.  h: [2][32] rows of ceil(H / 16) * 16 bf16 (+ 8 bytes
// of pitch), double-buffered; network 2's gate input: [32] rows of mlp1's last width rounded up to 32; the map columns: MB [2][32] rows of
// ceil(om_cols / 16) * 16 bf16 (+ 8 bytes of pitch), double-buffered beside the gather tile G of the rotated columns.
#pragma once
#include "value_net_lstm_kernel.h"

namespace {

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

constexpr int RKH = 4, RKX = 4;            // register-resident gate weights: 16-byte lane slots of W_hh and of the x part a block (RB blocks a wavefront)
constexpr int KGF = 2;                     // float32 k-groups of 8 of a rotated row: 13 | 15 columns
constexpr int RKM = 3;                     // register-resident map k-steps of 16 a block (network 1): the reference's 48 map columns

// the float32 plan and what this arithmetic changes: ksh k-steps of 16 of W_hh; ksx slots of the x part (network 1: float32 k-groups of 8 of
// W_ih's rotated columns, then k-steps of 16 of its map columns; network 2: k-steps of 16); the strides (floats) of the h rows and of
// network 2's gate input rows
struct LstmHPlan { LstmPlan q; int ksh, ksx, ld_h, ld_xb; };

__host__ __device__ inline bool lh_f32_layer(const VnPlan& p, int l) { return l == p.c0[0] || l == p.c0[1]; }
// a layer whose output is the operand of a bf16 layer: all of mlp1 (its last output is the gates' operand), mlp but its last layer
inline bool lh_out_bf16(const VnPlan& p, int l) { return l < p.c0[1] || l != p.c0[2] - 1; }
// the one layer that reads map columns in network 2: mlp1's first, float32 k-groups of the rotated columns, then bf16 k-steps of the maps
inline bool lh_mixed_layer(const VnPlan& p, int l, int om_cols) { return om_cols > 0 && p.c0[1] > 0 && l == p.c0[0]; }

// build_lstm_plan's table with the bf16 layers and the gates counted in 16-byte lane slots, the blob offsets that follow (in floats: a
// lane's 8 bf16 are 4 floats wide, so a piece keeps the size formula ncb * slots * 64 * 4 + ncb * 32) and the strides of bf16 rows.
// om: the rows carry om_cols map columns, which the first layer that reads a row takes in k-steps of 16 behind its float32 k-groups
inline int build_lstm_bf16_plan(const int32_t* dims, int n_dims, int cols, LstmHPlan& s, bool om = false, int om_cols = 0)
{
    const int rc = build_lstm_plan(dims, n_dims, cols, s.q, om, om_cols);
    if (rc != CS_OK) return rc;
    VnPlan& p = s.q.v;
    VnLayer& g = s.q.g;
    const int ksm = up(om_cols, 16) / 16;
    int off = 0, widest = 36;
    for (int l = 0; l < p.n_layers; ++l) {
        if (l == p.c0[1]) {             // the gates lie between the two chains in the blob
            s.ksh = up(s.q.H, 16) / 16;
            s.ksx = p.c0[1] > 0 ? up(s.q.xin, 16) / 16 : up(cols, 8) / 8 + ksm;
            g.kg_split = s.ksh;
            g.kg_total = s.ksh + s.ksx;
            place_layer(g, off);
        }
        VnLayer& L = p.L[l];
        if (lh_mixed_layer(p, l, om_cols)) {
            L.kg_split = up(cols, 8) / 8;
            L.kg_total = L.kg_split + ksm;
        } else if (!lh_f32_layer(p, l)) {
            L.kg_split = L.kg_total = up(L.K1, 16) / 16;
        }
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

// (bf16_bits, pack_layer_bf16 -- a bf16 layer's weights where the lanes of lstm_layer read them, cs_value_net_pack_bf16's layout -- and
// pack_layer_mixed -- network 2's first layer on rows with map columns -- are value_net_bf16.h's)

// the gate rows where the lanes of the transposed product read them: slot s of block b, lane l, gate row j = l & 31 = 8 * gate + u, torch's
// row gate * H + 8 b + u.  Slots below ksh: 8 bf16 of weight_hh at k = 16 s + 8 (l >> 5) + e.  Behind them the x part: network 2, 8 bf16 of
// weight_ih at k = 16 (s - ksh) + 8 (l >> 5) + e; network 1, 4 floats of weight_ih at k = 8 (s - ksh) + 4 (l >> 5) + e below the rotated
// columns' k-groups, then 8 bf16 of its map columns at k = cols + 16 (s - ksh - k-groups) + 8 (l >> 5) + e.  bias = b_ih + b_hh in float32.
// blob zeroed before
inline void pack_gates_bf16(const LstmHPlan& s, const float* wih, const float* whh, const float* bih, const float* bhh, float* fb)
{
    const VnLayer& g = s.q.g;
    const int H = s.q.H, xin = s.q.xin, cols = s.q.v.cols, kgf = up(cols, 8) / 8;
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
                } else if (sl - s.ksh < kgf) {
                    for (int e = 0; e < 4; ++e) {
                        const int k = 8 * (sl - s.ksh) + 4 * hh + e;
                        if (k < cols) slot[e] = wih[(size_t)row * xin + k];
                    }
                } else {
                    for (int e = 0; e < 8; ++e) {
                        const int k = cols + 16 * (sl - s.ksh - kgf) + 8 * hh + e;
                        if (k < xin) hs[e] = bf16_bits(wih[(size_t)row * xin + k]);
                    }
                }
            }
        }
}

// what the two pack entries do behind their plan: the size in bytes, the null checks, the zeroed blob, every layer in its arithmetic, the gates
inline int pack_lstm_bf16_blob(const LstmHPlan& s, int om_cols, const float* const* params, void* blob, size_t* n_bytes)
{
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
        if (lh_mixed_layer(p, l, om_cols)) pack_layer_mixed(p.L[l], p.cols, params[at], params[at + 1], fb);
        else if (lh_f32_layer(p, l)) pack_layer_f32(p.L[l], params[at], params[at + 1], fb);
        else pack_layer_bf16(p.L[l], params[at], params[at + 1], fb);
    }
    pack_gates_bf16(s, params[2 * n1], params[2 * n1 + 1], params[2 * n1 + 2], params[2 * n1 + 3], fb);
    return CS_OK;
}

// one 16-byte slot of the narrow x part (network 1: a float32 k-group of W_ih on the raw row; network 2: a bf16 k-step of W_ih on mlp1's
// rounded output) and one of W_hh on the rounded h; `row`: the lane's operand row in LDS at the slot (its sequence, its half of the k range)
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

// The kernels' LDS maps (offsets in floats).  The narrow kernel's is its kernel argument and keeps its fields; the one of the rows with map
// columns adds the staged map rows MB and, behind everything else, the keys and the order of action 0.
struct LstmHLds { int key, perm, G, HB, XB, P, Q, J, LT, total; };
struct LstmOmHLds { int key, perm, G, MB, HB, XB, P, Q, J, LT, key0, perm0, total; };

// what the map columns add to a launch: the maps [W][n][om_cols], which map a step pairs with its row, ksm k-steps of 16 and the stride
// (floats) of a bf16 map row in LDS
struct LstmOmH { const float* maps; int om_cols, map_order, ksm, ld_m; };

template <class Lds>
inline Lds lstm_bf16_lds_map(const LstmHPlan& s, int n, int ld_m)
{
    constexpr bool om = std::is_same<Lds, LstmOmHLds>::value;
    const VnPlan& p = s.q.v;
    Lds m{};
    int o = 0;
    auto take = [&](int floats) { const int at = o; o += up(floats, 4); return at; };
    m.key = take(TILE_M * n);
    m.perm = take(TILE_M * n);
    m.G = take(2 * TILE_M * LDX);
    if constexpr (om) m.MB = take(2 * TILE_M * ld_m);
    m.HB = take(2 * TILE_M * s.ld_h);
    m.XB = p.c0[1] > 0 ? take(TILE_M * s.ld_xb) : m.HB;
    m.P = take(TILE_M * p.ld_pq);
    m.Q = take(TILE_M * p.ld_pq);
    m.J = take(JROWS * p.ld_j);
    m.LT = take(VN_MAX_LAYERS * 8);
    if constexpr (om) {
        m.key0 = take(TILE_M * n);
        m.perm0 = take(TILE_M * n);
    }
    m.total = o;
    return m;
}

inline int launch_pick(int W, int A, const float* d_values, const float* d_actions, const float* d_robot, int robot_stride, const int32_t* d_override,
                       int32_t* d_choice, float* d_action_out, void* stream);         // (value_net_pick.h, included behind the unit's kernel)

// A decide entry behind its name.  K is the entry's kernel: K::om, whether its rows carry map columns (the entry without passes om_cols = 0,
// d_maps = nullptr, map_order = CS_VN_MAPS_OWN), K::Lds, its LDS map, and K::kernel<WREG, MLP1>, its four builds.
template <class K>
inline int lstm_bf16_decide(const char* entry, const int32_t* dims, int n_dims, const void* d_weights, size_t n_weight_bytes, int W, int A, int n, int cols,
                            int om_cols, int sorted_by_distance, int map_order, const float* d_rotated, const float* d_maps, const float* d_rewards,
                            const float* d_actions, const float* d_robot, int robot_stride, float gamma, float dt, const int32_t* d_override,
                            float* d_values, int32_t* d_choice, float* d_action_out, void* stream)
{
    LstmHPlan s;
    const int rc = build_lstm_bf16_plan(dims, n_dims, cols, s, K::om, om_cols);
    if (rc != CS_OK) return rc;
    const LstmPlan& q = s.q;
    // (a length that is no whole number of floats is no blob of any network: it fails the size check as SIZE_MAX floats)
    const size_t n_floats = n_weight_bytes % sizeof(float) ? (size_t)-1 : n_weight_bytes / sizeof(float);
    const int rc2 = lstm_check_decide(entry, q.v, d_weights, n_floats, W, A, n, sorted_by_distance, d_rotated, d_rewards, d_actions, d_robot, robot_stride,
                                      d_values, d_action_out, K::om, d_maps, map_order);
    if (rc2 != CS_OK) return rc2;
    const LstmOmH om{d_maps, om_cols, map_order, up(om_cols, 16) / 16, up(om_cols, 16) / 2 + 4};
    const auto m = lstm_bf16_lds_map<typename K::Lds>(s, n, om.ld_m);
    const bool mlp1 = q.v.c0[1] > 0;
    const bool wreg = q.g.ncb <= 4 * RB && s.ksh <= RKH && s.ksx <= (K::om && !mlp1 ? KGF + RKM : RKX);
    const float* wb = static_cast<const float*>(d_weights);
    const int rc3 = lstm_launch(m.total, W, A, wreg, mlp1, [&](auto WR, auto M1, size_t shmem, int NG, int grid) {
        constexpr auto kernel = K::template kernel<decltype(WR)::value, decltype(M1)::value>;
        const int rc4 = grant_lds<kernel>(shmem);
        if (rc4 != CS_OK) return rc4;
        const auto launch = [&](auto... behind) {       // (the kernel with map columns takes `om` behind the narrow kernel's arguments)
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(NT), shmem, (hipStream_t)stream, s, m, wb, NG, A, n, sorted_by_distance, d_rotated, d_rewards, d_robot,
                               robot_stride, gamma, dt, d_values, behind...);
        };
        if constexpr (K::om) launch(om);
        else launch();
        return (int)CS_OK;
    });
    if (rc3 != CS_OK) return rc3;
    return launch_pick(W, A, d_values, d_actions, d_robot, robot_stride, d_override, d_choice, d_action_out, stream);
}

} // namespace
