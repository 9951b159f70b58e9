// value_net_bf16.h -- bf16 as the opt-in arithmetics (value_net_bf16_layers.h, value_net_lstm_bf16.h) share it: the operand vector of
// v_mfma_f32_32x32x16_bf16, the host's rounding, the pack of a bf16 layer and of a first layer split between float32 rotated columns and
// bf16 map columns.  Unnamed namespace, as value_net_plan.h.
#pragma once
#include "value_net_plan.h"

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

inline uint16_t bf16_bits(float f)       // round to nearest even; a NaN becomes the quiet NaN 0x7fc0 (what torch's .bfloat16() gives)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// one bf16 layer's weights where the lanes of a bf16 layer read them, [ncb][k-steps][64 lanes][8 bf16]: lane l holds
// Wt[k = 16 s + 8 (l >> 5) + e][column 32 cb + (l & 31)], e = 0..7, of k-step s (the k-steps below kg_split from the first source, the others
// from the second); float32 biases.  wgt = torch.nn.Linear.weight [N][K1 + K2], blob zeroed before
inline void pack_layer_bf16(const VnLayer& L, const float* wgt, const float* bias, float* fb)
{
    uint16_t* hb = reinterpret_cast<uint16_t*>(fb + L.w_off);
    const int K = L.K1 + L.K2;
    for (int cb = 0; cb < L.ncb; ++cb)
        for (int ks = 0; ks < L.kg_total; ++ks)
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 8; ++e) {
                    const int j = cb * 32 + (lane & 31);
                    const int kk = ks * 16 + 8 * (lane >> 5) + e;
                    int k = -1;
                    if (ks < L.kg_split) { if (kk < L.K1) k = kk; }
                    else if (kk - L.kg_split * 16 < L.K2) k = L.K1 + kk - L.kg_split * 16;
                    if (j < L.N && k >= 0) hb[((size_t)(cb * L.kg_total + ks) * 64 + lane) * 8 + e] = bf16_bits(wgt[(size_t)j * K + k]);
                }
    for (int j = 0; j < L.N; ++j) fb[L.b_off + j] = bias[j];
}

// a first layer on rows with map columns (OM-SARL's mlp1 layer 0, OM-LSTM-RL network 2's), where the lanes of its layer read it:
// [ncb][k-groups + k-steps][64 lanes] slots of 16 bytes -- the float32 layer's k-groups of the rotated columns (pack_layer_f32's), then
// the bf16 layer's k-steps of the map columns (pack_layer_bf16's, k counted from `cols`); float32 biases.  blob zeroed before
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

} // namespace
