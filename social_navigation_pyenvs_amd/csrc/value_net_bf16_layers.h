// value_net_bf16_layers.h -- the opt-in bf16 arithmetic of the value-network decision as value_net_body.inc asks for an arithmetic (its
// header comment lists the names), stated once for its two kernels: k_value_net_bf16 (value_net_bf16.hip: CADRL / SARL on the narrow rows)
// and k_value_net_om_bf16 (value_net_om_bf16.hip: OM-SARL on rows with map columns).  The contract and the LDS image of a bf16 operand are
// value_net_bf16.hip's header comment; the host's rounding and the packs are value_net_bf16.h's.  Here: which layers are float32, the plan
// change, the bf16 layer of a tile, the chain of layers and the handful of functions the body asks for.
//
// mlp1's layer 0 is the one layer the two kernels run differently: it reads the input tile.  VN_MLP1_LAYER0 names the function that
// runs it, with layer_fwd's arguments and a bfloat16 output; the default is the float32 layer on the narrow rows, a kernel with columns
// of its own behind the rotated ones declares its function and defines the name before it includes this header.
// Unnamed namespace, as value_net_plan.h.
#pragma once
#include "value_net_bf16.h"

#ifndef VN_MLP1_LAYER0
#define VN_MLP1_LAYER0 layer_fwd<true>
#endif

namespace {

__host__ __device__ inline bool vn_mlp3(const VnPlan& p, int l) { return p.kind == CS_VN_SARL && l >= p.c0[3]; }
// a float32 layer: its input holds raw rotated-state columns
__host__ __device__ inline bool vn_f32_layer(const VnPlan& p, int l) { return l == p.c0[0] || vn_mlp3(p, l); }
// a layer whose output is the operand of a bf16 layer (a chain's last output goes to a reduction, except mlp1's)
inline bool vn_out_bf16(const VnPlan& p, int l)
{
    if (vn_mlp3(p, l)) return false;
    for (int c = 1; c <= 4; ++c)
        if (l == p.c0[c] - 1) return p.kind == CS_VN_SARL && c == 1;
    return true;
}

// build_plan's table with the bf16 layers counted in k-steps of 16 (kg_split, kg_total), the blob offsets that follow (still in floats:
// a lane's 8 bf16 are 4 floats wide, so a layer keeps the size formula ncb * kg_total * 64 * 4 + ncb * 32) and the LDS strides of
// bf16 rows (floats; header comment)
void replan_bf16(VnPlan& p)
{
    int off = 0, widest = 36;
    for (int l = 0; l < p.n_layers; ++l) {
        VnLayer& L = p.L[l];
        if (!vn_f32_layer(p, l)) {
            L.kg_split = up(L.K1, 16) / 16;
            L.kg_total = L.kg_split + up(L.K2, 16) / 16;
        }
        place_layer(L, off);
        const int ld = vn_out_bf16(p, l) ? L.ncb * 16 + 4 : L.ncb * 32 + 4;
        widest = ld > widest ? ld : widest;
    }
    p.ld_pq = widest;
    p.ld_m1 = up(p.m1w > 0 ? p.m1w : 1, 32) / 2 + 4;
    p.total_floats = off;
}

__device__ __forceinline__ void f2h(float* buf, int ld, int r, int c, float v) { reinterpret_cast<__bf16*>(buf)[r * 2 * ld + c] = static_cast<__bf16>(v); }

// what value_net_body.inc asks of an arithmetic beside run_chain (below): M1 and G hold bfloat16 rows, the attention's k-steps of 16 read
// m1pad columns of the mean, the running sum of a chunked mean is the float32 tail behind the LDS map, needed only with the global state
__device__ __forceinline__ float vn_m1(const float* buf, int ld, int r, int c) { return static_cast<float>(reinterpret_cast<const __bf16*>(buf)[r * 2 * ld + c]); }
__device__ __forceinline__ void vn_mean_store(float* buf, int ld, int k, int c, float v) { f2h(buf, ld, k, c, v); }
__device__ __forceinline__ int vn_m1pad(const VnPlan& p) { return (p.m1w + 15) & ~15; }
__device__ __forceinline__ int vn_sum_cols(const VnPlan&, int m1pad) { return m1pad; }
__device__ __forceinline__ bool vn_mean_pass(const VnPlan& p) { return p.with_global != 0; }

// One bf16 layer of a tile: layer_fwd's contract with bfloat16 rows in src / src2 (strides in floats) and the weights as
// [ncb][k-steps][64 lanes][8 bf16]: lane l holds Wt[k = 16 s + 8 (l >> 5) + j][column 32 cb + (l & 31)], j = 0..7, of k-step s.
template <bool OUT_BF16>
__device__ __forceinline__ void layer_fwd_h(const VnLayer& L, const float* __restrict__ wb, const float* src, int lds_, const float* src2, int lds2,
                                            const int* grp, int rbs, float* dst, int ldd, int rot)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, li = lane & 31;
    const int items = rbs * L.ncb;
    const int KS = L.kg_total, split = L.kg_split;
    for (int it = (wave + rot) & 3; it < items; it += 4) {
        const int rb = it % rbs, cb = it / rbs;
        const int row = rb * 32 + li;
        const bf16x8* a1 = reinterpret_cast<const bf16x8*>(src + row * lds_) + h;
        const bf16x8* a2 = src2 ? reinterpret_cast<const bf16x8*>(src2 + grp[row] * lds2) + h : a1;
        const bf16x8* bw = reinterpret_cast<const bf16x8*>(wb + L.w_off) + (long)cb * KS * 64 + lane;
        const float bias = wb[L.b_off + cb * 32 + li];
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = bias;
        bf16x8 nb0 = bw[0], nb1 = bw[(1 < KS ? 1 : KS - 1) * 64], nb2 = bw[(2 < KS ? 2 : KS - 1) * 64], nb3 = bw[(3 < KS ? 3 : KS - 1) * 64];
        for (int ks0 = 0; ks0 < KS; ks0 += 4) {
            const bf16x8 b0 = nb0, b1 = nb1, b2 = nb2, b3 = nb3;
            {   // the next four k-steps' weights are on their way while these four multiply (clamped: a tail re-reads the last step)
                const int q0 = ks0 + 4, q1 = ks0 + 5, q2 = ks0 + 6, q3 = ks0 + 7, last = KS - 1;
                nb0 = bw[(q0 < KS ? q0 : last) * 64];
                nb1 = bw[(q1 < KS ? q1 : last) * 64];
                nb2 = bw[(q2 < KS ? q2 : last) * 64];
                nb3 = bw[(q3 < KS ? q3 : last) * 64];
            }
#define VN_STEP(U, B)                                                                            \
    if (ks0 + U < KS) {                                                                          \
        const int ks = ks0 + U;                                                                  \
        const bf16x8 a = ks < split ? a1[2 * ks] : a2[2 * (ks - split)];                         \
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, B, acc, 0, 0, 0);                       \
    }
            VN_STEP(0, b0)
            VN_STEP(1, b1)
            VN_STEP(2, b2)
            VN_STEP(3, b3)
#undef VN_STEP
        }
        // C/D map of the 32x32 forms: column = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
        const bool pad = cb * 32 + li >= L.N;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = acc[r];
            if (L.relu) v = v < 0.0f ? 0.0f : v;
            v = pad ? 0.0f : v;
            const int orow = rb * 32 + 4 * h + (r & 3) + 8 * (r >> 2), ocol = cb * 32 + li;
            if constexpr (OUT_BF16) f2h(dst, ldd, orow, ocol, v);
            else dst[orow * ldd + ocol] = v;
        }
    }
}

// layers [first, last) from `src`; outputs alternate P, Q; the last one goes to final_dst when given.  Returns where the result is.
// The chain's kind fixes which arithmetic a layer may take, so that a call site carries only those.
template <int CH>
__device__ __forceinline__ const float* run_chain(const VnPlan& p, const float* __restrict__ wb, const VnBufs& b, int first, int last, const float* src,
                                                  int lds_, const float* src2, int lds2, int rbs, float* final_dst, int final_ld, int& out_ld)
{
    const float* cur = src;
    int cur_ld = lds_;
    for (int l = first; l < last; ++l) {
        const bool fin = l == last - 1;
        float* dst = fin && final_dst ? final_dst : (((l - first) & 1) ? b.Q : b.P);
        const int ldd = fin && final_dst ? final_ld : p.ld_pq;
        const float* s2 = l == first ? src2 : nullptr;
        const int rot = l + (int)blockIdx.x;
        if constexpr (CH == CH_MLP3) layer_fwd<false>(p.L[l], wb, cur, cur_ld, s2, lds2, b.grp, rbs, dst, ldd, rot);
        else if constexpr (CH == CH_MLP1) {
            if (l == first) VN_MLP1_LAYER0(p.L[l], wb, cur, cur_ld, s2, lds2, b.grp, rbs, dst, ldd, rot);
            else layer_fwd_h<true>(p.L[l], wb, cur, cur_ld, s2, lds2, b.grp, rbs, dst, ldd, rot);
        } else if constexpr (CH == CH_REDUCED) {
            if (fin) layer_fwd_h<false>(p.L[l], wb, cur, cur_ld, s2, lds2, b.grp, rbs, dst, ldd, rot);
            else layer_fwd_h<true>(p.L[l], wb, cur, cur_ld, s2, lds2, b.grp, rbs, dst, ldd, rot);
        } else {
            if (l == first && fin) layer_fwd<false>(p.L[l], wb, cur, cur_ld, s2, lds2, b.grp, rbs, dst, ldd, rot);
            else if (l == first) layer_fwd<true>(p.L[l], wb, cur, cur_ld, s2, lds2, b.grp, rbs, dst, ldd, rot);
            else if (fin) layer_fwd_h<false>(p.L[l], wb, cur, cur_ld, s2, lds2, b.grp, rbs, dst, ldd, rot);
            else layer_fwd_h<true>(p.L[l], wb, cur, cur_ld, s2, lds2, b.grp, rbs, dst, ldd, rot);
        }
        __syncthreads();
        cur = dst;
        cur_ld = ldd;
    }
    out_ld = cur_ld;
    return cur;
}

} // namespace
