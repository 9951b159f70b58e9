// value_net_lstm_bf16.h -- what the two recurrent decision kernels with the opt-in bf16 arithmetic share beside value_net_lstm_kernel.h:
// k_value_net_lstm_bf16 (value_net_lstm_bf16.hip, rows of 13 | 15 columns) and k_value_net_lstm_om_bf16 (value_net_lstm_om_bf16.hip, the
// rows widened by occupancy-map columns).  Host: the plan's changes, the pack of the gates and of a whole blob.  Device: one slot of W_hh
// on the rounded h, one of the narrow x part, the pointwise part.  Each kernel keeps its LDS map, its step loop and its entries.
// om_cols = 0 everywhere below is the narrow network, whose plan and blob are what they were before there were map columns here.
// Unnamed namespace: each translation unit gets its own copy.
#pragma once
#include "value_net_lstm_kernel.h"

namespace {

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

constexpr int RKH = 4, RKX = 4;            // register-resident gate weights: 16-byte lane slots of W_hh and of the x part a block (RB blocks a wavefront)
constexpr int KGF = 2;                     // float32 k-groups of 8 of a rotated row: 13 | 15 columns

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

// (bf16_bits and pack_layer_bf16 -- a bf16 layer's weights where the lanes of lstm_layer read them, cs_value_net_pack_bf16's layout -- are
// value_net_bf16.h's)

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

// network 2's first layer on rows with map columns, where the lanes of its layer read it: [ncb][k-groups + k-steps][64 lanes] slots of 16
// bytes -- the float32 layer's k-groups of the rotated columns (pack_layer_f32's), then the bf16 layer's k-steps of the map columns
// (pack_layer_bf16's, k counted from `cols`); float32 biases.  blob zeroed before
inline void pack_layer_mixed(const VnLayer& L, int cols, const float* wgt, const float* bias, float* fb)
{
    const int K = L.K1;
    for (int cb = 0; cb < L.ncb; ++cb)
        for (int sl = 0; sl < L.kg_total; ++sl)
            for (int lane = 0; lane < 64; ++lane) {
                const int j = cb * 32 + (lane & 31), hh = lane >> 5;
                if (j >= L.N) continue;
                float* slot = fb + L.w_off + ((size_t)(cb * L.kg_total + sl) * 64 + lane) * 4;
                if (sl < L.kg_split) {
                    for (int e = 0; e < 4; ++e) {
                        const int k = 8 * sl + 4 * hh + e;
                        if (k < cols) slot[e] = wgt[(size_t)j * K + k];
                    }
                } else {
                    uint16_t* hs = reinterpret_cast<uint16_t*>(slot);
                    for (int e = 0; e < 8; ++e) {
                        const int k = cols + 16 * (sl - L.kg_split) + 8 * hh + e;
                        if (k < K) hs[e] = bf16_bits(wgt[(size_t)j * K + k]);
                    }
                }
            }
    for (int j = 0; j < L.N; ++j) fb[L.b_off + j] = bias[j];
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

} // namespace
