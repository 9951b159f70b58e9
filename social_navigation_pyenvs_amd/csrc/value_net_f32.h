// value_net_f32.h -- what the two float32 kernels of the value-network decision share beside their body (value_net_body.inc): the LDS
// buffers of a launch, a chain of layers and the loader that copies rows (value_net.hip: rows from cs_lookahead's tensor;
// value_net_worlds.hip: rows generated from the worlds).  Unnamed namespace, as value_net_plan.h.
#pragma once
#include "value_net_plan.h"

namespace {

struct VnBufs { float *X0, *M1, *P, *Q, *G, *J, *sc, *den, *val; int* grp; };

// layers [first, last) from `src`; outputs alternate P, Q; the last one goes to final_dst when given.  Returns where the result is.
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

// rows of the rotated array into the input tile, zero beyond the rows and the columns; grp[r] = the tile-local group of row r
__device__ __forceinline__ void load_tile(const VnBufs& b, const float* __restrict__ rows_src, int rows, int cols, int per_group, int M)
{
    for (int i = threadIdx.x; i < M * 16; i += NT) {
        const int r = i >> 4, c = i & 15;
        b.X0[r * LDX + c] = (r < rows && c < cols) ? rows_src[(long)r * cols + c] : 0.0f;
    }
    for (int r = threadIdx.x; r < M; r += NT) b.grp[r] = r < rows ? r / per_group : 0;
}

} // namespace
