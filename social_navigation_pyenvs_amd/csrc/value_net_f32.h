// value_net_f32.h -- the float32 arithmetic of the value-network decision, as value_net_body.inc asks for an arithmetic (its header comment
// lists the names): every layer of every chain is value_net_plan.h's layer_fwd, mlp1's output and the crowd mean are float rows.  Included
// by the two float32 kernels (value_net.hip: rows from cs_lookahead's tensor; value_net_worlds.hip: rows generated from the worlds); the
// bf16 arithmetic is stated in value_net_bf16.hip.  Unnamed namespace, as value_net_plan.h.
#pragma once
#include "value_net_plan.h"

namespace {

// layers [first, last) from `src`; outputs alternate P, Q; the last one goes to final_dst when given.  Returns where the result is.
// (the chain's tag changes nothing here: one arithmetic for every layer)
template <int>
__device__ __forceinline__ const float* run_chain(const VnPlan& p, const float* __restrict__ wb, const VnBufs& b, int first, int last, const float* src,
                                                  int lds_, const float* src2, int lds2, int rbs, float* final_dst, int final_ld, int& out_ld)
{
    const float* cur = src;
    int cur_ld = lds_;
    for (int l = first; l < last; ++l) {
        const bool fin = l == last - 1 && final_dst;
        float* dst = fin ? final_dst : (((l - first) & 1) ? b.Q : b.P);
        const int ldd = fin ? final_ld : p.ld_pq;
        layer_fwd<false>(p.L[l], wb, cur, cur_ld, l == first ? src2 : nullptr, lds2, b.grp, rbs, dst, ldd, l + (int)blockIdx.x);
        __syncthreads();
        cur = dst;
        cur_ld = ldd;
    }
    out_ld = cur_ld;
    return cur;
}

__device__ __forceinline__ float vn_m1(const float* buf, int ld, int r, int c) { return buf[r * ld + c]; }
__device__ __forceinline__ void vn_mean_store(float* buf, int ld, int k, int c, float v) { buf[k * ld + c] = v; }
__device__ __forceinline__ int vn_m1pad(const VnPlan& p) { return (p.m1w + 7) & ~7; }
// the running sum of a chunked mean is G's first row itself (the kernels' gsum = m.G), zeroed over the whole row
__device__ __forceinline__ int vn_sum_cols(const VnPlan& p, int) { return p.ld_m1; }
// A quirk, kept because removing it changes the float32 instruction stream: the pre-pass also runs without the global state, where
// nothing reads the mean it leaves in G.
__device__ __forceinline__ bool vn_mean_pass(const VnPlan&) { return true; }

} // namespace
