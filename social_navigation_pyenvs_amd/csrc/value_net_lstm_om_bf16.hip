// value_net_lstm_om_bf16.hip -- OM-LSTM-RL's decision (value_net_lstm.hip: cs_value_net_decide_lstm_om) with the opt-in bf16 arithmetic
// (cs_value_net_decide_lstm_om_bf16; Python: OMLstmRL.set_mapped_precision("bf16")): the recurrent network on rows of 13 | 15 rotated columns
// followed by om_cols occupancy-map columns.  The kernel is value_net_lstm_bf16_body.inc under LSTM_OM 1: k_value_net_lstm_bf16's text
// (value_net_lstm_bf16.hip) with the map pairing of k_value_net_lstm_om -- one map row per (world, human) read in place from d_maps
// [W][n][om_cols], a step's row beside its own map (CS_VN_MAPS_OWN) or beside the map at that place of the order of the world's action 0
// (CS_VN_MAPS_FIRST_ACTION), which every workgroup ranks itself from that pair's own rows of d_rotated, whichever tile they lie in; keys,
// permutations, ties and NaN distances are k_value_net_lstm_om's.  The arithmetic, its rounding points and the order of a chain, the
// register-resident slots, the LDS images, the plan, the pack and what a decide entry does are value_net_lstm_bf16.h's.  This file keeps what
// is the map columns' own on the device -- their gather, network 2's first layer, a slot of the x part -- the kernel's name and the two entries.
#include <hip/hip_runtime.h>

#include "value_net_lstm_bf16.h"

namespace {

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
#define LSTM_OM 1
#include "value_net_lstm_bf16_body.inc"
#undef LSTM_OM
}

struct Mapped {
    static constexpr bool om = true;
    using Lds = LstmOmHLds;
    template <bool WREG, bool MLP1> static constexpr auto kernel = k_value_net_lstm_om_bf16<WREG, MLP1>;
};

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
    return lstm_bf16_decide<Mapped>("cs_value_net_decide_lstm_om_bf16", dims, n_dims, d_weights, n_weight_bytes, W, A, n, cols, om_cols, sorted_by_distance,
                                    map_order, d_rotated, d_maps, d_rewards, d_actions, d_robot, robot_stride, gamma, dt, d_override, d_values, d_choice,
                                    d_action_out, stream);
}
