// value_net_grad.h -- what the gradient kernels (value_net_grad.hip: CADRL / SARL; value_net_lstm_grad.hip: LSTM-RL) share: the flat
// parameter offsets, the layer-indexed part of the LDS map, the forward layer of a 32-row tile, the three backward products on
// v_mfma_f32_32x32x2_f32 (dX = dZ W, dWt = dZt X, db), the chains over them, the kernel that sums the workgroups' regions and the one that
// sums them, takes the SGD-momentum step and rewrites the blob (k_vn_sgd, the train-step entries).  Unnamed namespace: each translation
// unit gets its own copy.
#pragma once
#include "value_net_plan.h"

namespace {

constexpr int GRAD_MAX_GROUPS = 256;          // workgroups = scratch regions at most: one per CU

struct GradOffsets { int w[VN_MAX_LAYERS], b[VN_MAX_LAYERS], total; };      // floats into the flat parameters: weight [N][K], bias [N] per layer

// LDS map of the gradient kernel (floats).  act[l]: the output of layer l, 32 rows of up(N, 8) + 4 floats; mlp3's layers share the floats of
// the tile's (mlp1, mlp2, attention) layers.  ldx: the input tile's row stride, the first layer's K rounded up to 8, plus 4 (value_net_om.hip's:
// 20 for rows of 13 | 15 columns, 68 at 61 | 63, which is 4 mod 32).
struct GradLds { int X0, ldx, act[VN_MAX_LAYERS], ld[VN_MAX_LAYERS], D0, D1, dH, G, dG, J, dJ, sc, dw, den, val, grp, total; };

inline int ld8(int w) { return up(w, 8) + 4; }

// The input tile's stride as the device code reads it: in a vector register (a lane's count of the set bits of an empty mask below it is 0).
// Both gradient kernels sit at the limit of their scalar registers, which the arguments fill; one more scalar alive over the whole job makes
// the compiler reserve a private segment (36 bytes a lane in the resource report, with this 0).
__device__ __forceinline__ int tile_ldx(const GradLds& m) { return m.ldx + (int)__builtin_amdgcn_mbcnt_lo(0u, 0u); }

// One forward layer of a 32-row tile: value_net_plan.h's layer_fwd (the same k-order per output element: the accumulator starts from the
// bias, k-groups of 8 in order, within a group k = s, 4 + s for s = 0..3) with a destination stride of up(N, 8) + 4: columns N .. up(N, 8)
// are stored as 0, nothing beyond.
__device__ __forceinline__ void layer_fwd32(const VnLayer& L, const float* __restrict__ wb, const float* src, int lds_, const float* src2, int lds2,
                                            const int* grp, float* dst, int ldd)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, li = lane & 31;
    const int KG = L.kg_total, split = L.kg_split;
    for (int cb = wave; cb < L.ncb; cb += 4) {
        const float* a1 = src + li * lds_ + 4 * h;
        const float* a2 = src2 ? src2 + grp[li] * lds2 + 4 * h : a1;
        const float4* bw = reinterpret_cast<const float4*>(wb + L.w_off) + (long)cb * KG * 64 + lane;
        const float bias = wb[L.b_off + cb * 32 + li];
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = bias;
        float4 nb0 = bw[0], nb1 = bw[(1 < KG ? 1 : KG - 1) * 64], nb2 = bw[(2 < KG ? 2 : KG - 1) * 64], nb3 = bw[(3 < KG ? 3 : KG - 1) * 64];
        for (int kg0 = 0; kg0 < KG; kg0 += 4) {
            const float4 b0 = nb0, b1 = nb1, b2 = nb2, b3 = nb3;
            {   // the next four k-groups' weights are on their way while these four multiply (clamped: a tail re-reads the last group)
                const int q0 = kg0 + 4, q1 = kg0 + 5, q2 = kg0 + 6, q3 = kg0 + 7, last = KG - 1;
                nb0 = bw[(q0 < KG ? q0 : last) * 64];
                nb1 = bw[(q1 < KG ? q1 : last) * 64];
                nb2 = bw[(q2 < KG ? q2 : last) * 64];
                nb3 = bw[(q3 < KG ? q3 : last) * 64];
            }
#define VG_STEP(U, B)                                                                                                        \
    if (kg0 + U < KG) {                                                                                                      \
        const int kg = kg0 + U;                                                                                              \
        const float4 a = *reinterpret_cast<const float4*>(kg < split ? a1 + kg * 8 : a2 + (kg - split) * 8);                 \
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, B.x, acc, 0, 0, 0);                                                  \
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, B.y, acc, 0, 0, 0);                                                  \
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, B.z, acc, 0, 0, 0);                                                  \
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, B.w, acc, 0, 0, 0);                                                  \
    }
            VG_STEP(0, b0)
            VG_STEP(1, b1)
            VG_STEP(2, b2)
            VG_STEP(3, b3)
#undef VG_STEP
        }
        const int col = cb * 32 + li;
        if (col < ldd - 4) {
            float* d = dst + 4 * h * ldd + col;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = acc[r];
                if (L.relu) v = v < 0.0f ? 0.0f : v;
                d[((r & 3) + 8 * (r >> 2)) * ldd] = col >= L.N ? 0.0f : v;
            }
        }
    }
}

// dX [32][Kc] = dZ [32][N] x W [N][koff .. koff + Kc) (W rows of Kw floats, global): into dst (stride ldd >= up(Kc, 8) + 4), columns Kc ..
// up(Kc, 8) as 0; `add`: onto what dst holds; `mask` (stride ldd): the ReLU'd output this is the gradient of -- zero where it is not positive.
// dZ's columns N .. up(N, 8) hold zeros (finite): the weights beyond N read as 0.
__device__ __forceinline__ void bwd_dx(const float* __restrict__ W, int Kw, int koff, int Kc, int N, const float* dZ, int ldz, float* dst, int ldd,
                                       bool add, const float* mask)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, li = lane & 31;
    const int items = (Kc + 31) / 32, KG = (N + 7) / 8;
    for (int it = wave; it < items; it += 4) {
        const int col = it * 32 + li;
        const bool live = col < Kc;
        const float* a1 = dZ + li * ldz + 4 * h;
        const float* w = W + koff + (live ? col : 0);
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        // (the weights of k-group kg + 2 are on their way while k-group kg multiplies)
        auto wrow = [&](int kg) {
            const int n0 = kg * 8 + 4 * h;
            return make_float4(live && n0 + 0 < N ? w[(long)(n0 + 0) * Kw] : 0.0f, live && n0 + 1 < N ? w[(long)(n0 + 1) * Kw] : 0.0f,
                               live && n0 + 2 < N ? w[(long)(n0 + 2) * Kw] : 0.0f, live && n0 + 3 < N ? w[(long)(n0 + 3) * Kw] : 0.0f);
        };
        float4 n0b = wrow(0), n1b = wrow(1);
        for (int kg = 0; kg < KG; kg += 2) {
            const float4 b0 = n0b, b1 = n1b;
            n0b = wrow(kg + 2);
            n1b = wrow(kg + 3);
            {
                const float4 a = *reinterpret_cast<const float4*>(a1 + kg * 8);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b0.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b0.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b0.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b0.w, acc, 0, 0, 0);
            }
            if (kg + 1 < KG) {
                const float4 a = *reinterpret_cast<const float4*>(a1 + (kg + 1) * 8);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b1.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b1.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b1.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b1.w, acc, 0, 0, 0);
            }
        }
        if (col < ((Kc + 7) & ~7)) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int at = ((r & 3) + 8 * (r >> 2) + 4 * h) * ldd + col;
                float v = acc[r];
                if (mask && !(mask[at] > 0.0f)) v = 0.0f;
                dst[at] = add ? dst[at] + v : v;
            }
        }
    }
}

// gW [N][koff .. koff + Kc) += dZt [N][32] x X [32][Kc] (gW rows of Kw floats, the workgroup's scratch region); X's row r is X + r * ldx_, or
// X + grp[r] * ldx_ with `grp` (the crowd mean of the row's group).  Block (n-block, k-block) is always the same wavefront's: its lanes add to
// the same floats tile after tile.
__device__ __forceinline__ void bwd_dw(float* gW, int Kw, int koff, int Kc, int N, const float* dZ, int ldz, const float* X, int ldx_, const int* grp)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, li = lane & 31;
    const int kbs = (Kc + 31) / 32, items = ((N + 31) / 32) * kbs;
    for (int it = wave; it < items; it += 4) {
        const int jb = it / kbs, ib = it - jb * kbs;
        const int nn = jb * 32 + li, kk = ib * 32 + li;
        const bool kv = kk < Kc, nv = nn < N;
        f32x16 acc, old;                // (what the region holds loads while the block multiplies)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = jb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            old[r] = kv && row < N ? gW[(long)row * Kw + koff + kk] : 0.0f;
            acc[r] = 0.0f;
        }
#pragma unroll 4
        for (int r0 = 0; r0 < 32; r0 += 2) {
            const int r = r0 + h;
            const float a = nv ? dZ[r * ldz + nn] : 0.0f;
            const float b = kv ? X[(grp ? grp[r] : r) * ldx_ + kk] : 0.0f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = jb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (kv && row < N) gW[(long)row * Kw + koff + kk] = old[r] + acc[r];
        }
    }
}

// gb [N] += the column sums of dZ, rows in order
__device__ __forceinline__ void bwd_db(float* gb, int N, const float* dZ, int ldz)
{
    for (int c = threadIdx.x; c < N; c += NT) {
        float s = 0.0f;
        for (int r = 0; r < 32; ++r) s += dZ[r * ldz + c];
        gb[c] += s;
    }
}

// (a layer's output is lds + m.act[l]: an array of pointers indexed by a run-time layer would live in scratch memory)
struct GradBufs { float *lds, *X0, *D0, *D1, *dH, *G, *dG, *J, *dJ, *sc, *dw, *den, *val; int* grp; };

// layers [first, last) forward from src (and src2 per group behind it), every output kept in its act buffer
__device__ __forceinline__ void chain_fwd(const VnPlan& p, const GradLds& m, const GradBufs& b, const float* __restrict__ wb, int first, int last,
                                          const float* src, int lds_, const float* src2, int lds2)
{
    for (int l = first; l < last; ++l) {
        layer_fwd32(p.L[l], wb, src, lds_, l == first ? src2 : nullptr, lds2, b.grp, (b.lds + m.act[l]), m.ld[l]);
        __syncthreads();
        src = (b.lds + m.act[l]);
        lds_ = m.ld[l];
    }
}

// layers [first, last) backward.  dz: the gradient of the last layer's output (stride m.ld[last - 1], ReLU already applied), in one of D0 /
// D1 or a buffer of its own; the layers' intermediate gradients alternate between D0 and D1.  src / src2: what chain_fwd read.  in1 / in2:
// where the gradient of the chain's input goes (strides ld1 / ld2; null: not wanted), add1: onto what in1 holds.
__device__ __forceinline__ void chain_bwd(const VnPlan& p, const GradLds& m, const GradBufs& b, const float* __restrict__ params, const GradOffsets& o,
                                          float* g, int first, int last, const float* dz, const float* src, int lds_, const float* src2, int lds2,
                                          float* in1, int ld1, bool add1, float* in2, int ld2)
{
    for (int l = last - 1; l >= first; --l) {
        const VnLayer& L = p.L[l];
        const int Kw = L.K1 + L.K2, ldz = m.ld[l];
        const float* x = l == first ? src : (b.lds + m.act[l - 1]);
        const int ldx_ = l == first ? lds_ : m.ld[l - 1];
        bwd_dw(g + o.w[l], Kw, 0, L.K1, L.N, dz, ldz, x, ldx_, nullptr);
        if (L.K2) bwd_dw(g + o.w[l], Kw, L.K1, L.K2, L.N, dz, ldz, src2, lds2, b.grp);
        bwd_db(g + o.b[l], L.N, dz, ldz);
        float* next = dz == b.D0 ? b.D1 : b.D0;
        if (l > first) bwd_dx(params + o.w[l], Kw, 0, L.K1, L.N, dz, ldz, next, m.ld[l - 1], false, (b.lds + m.act[l - 1]));
        else {
            if (in1) bwd_dx(params + o.w[l], Kw, 0, L.K1, L.N, dz, ldz, in1, ld1, add1, nullptr);
            if (in2 && L.K2) bwd_dx(params + o.w[l], Kw, L.K1, L.K2, L.N, dz, ldz, in2, ld2, false, nullptr);
        }
        __syncthreads();
        dz = next;
    }
}

// d_grad[i] = the regions' floats i in region order; the loss = the regions' terms in order / B
__global__ void k_vn_grad_sum(const float* __restrict__ scratch, int region, int regions, int P, int B, float* __restrict__ grad, float* __restrict__ loss)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > P) return;
    float s = 0.0f;
    for (int r = 0; r < regions; ++r) s += scratch[(long)r * region + i];
    if (i < P) grad[i] = s;
    else *loss = s / (float)B;
}

// ---------------------------------------------------------------------------------------------------------------- the fused optimiser step
// The blob float that holds column kk (counted in the blob's k-groups: the second source's columns start at 8 * kg_split) of output `col` of
// 32-column block cb of a layer: pack_layer_f32's map, read forwards.
__host__ __device__ __forceinline__ int blob_weight_at(const VnLayer& L, int cb, int col, int kk)
{
    return L.w_off + (((cb * L.kg_total + (kk >> 3)) * 64 + col + 32 * ((kk >> 2) & 1)) << 2) + (kk & 3);
}

// the blob float of element e of a Linear layer's flat (weight [N][K1 + K2], bias [N]) pair
__host__ __device__ __forceinline__ int blob_layer_at(const VnLayer& L, int e)
{
    const int K = L.K1 + L.K2;
    if (e >= L.N * K) return L.b_off + e - L.N * K;
    const int j = e / K, k = e - j * K;
    return blob_weight_at(L, j >> 5, j & 31, k < L.K1 ? k : L.kg_split * 8 + k - L.K1);
}

// k_vn_grad_sum's sum for k_vn_sgd: the regions' floats i, added in region order -- the same adds, the same bytes --, with eight regions'
// loads in flight at a time (one load a trip waits a memory latency per region: 228 of them at 4096 x 5)
__device__ __forceinline__ float region_sum(const float* __restrict__ scratch, int region, int regions, int i)
{
    const float* at = scratch + i;
    float s = 0.0f;
    int r = 0;
    for (; r + 8 <= regions; r += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = at[(long)(r + u) * region];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; r < regions; ++r) s += at[(long)r * region];
    return s;
}

// k_vn_grad_sum, torch's SGD with momentum (dampening 0, no Nesterov, no weight decay) and the pack kernel in one launch, a thread per
// parameter i of the flat layout: g = the regions' floats i in region order (d_grad's bytes as k_vn_grad_sum writes them), buf = mu buf + g,
// p = p - lr buf, each one fmaf, and the blob float that reads p rewritten from the new value.  `Map`: map(i, twin) is that blob float; a
// parameter that shares its blob float with another (the LSTM's bias_ih and bias_hh) is updated by its partner's thread -- the partner gets
// twin = the other's index and writes the float32 sum of the two new values in the pack kernel's order, the other gets -1.  Every parameter
// is read by exactly one blob float (tests/test_value_step_cpu.py), so the padding floats, zero since the blob was packed, stay zero and
// no two threads write one float: no atomics, the same bytes twice.  The thread behind the last parameter owns the loss: the regions' terms
// / B, and that added in float64 to *loss_sum (may be null), as the trainer's loops add loss.item() on the host.
template <class Map>
__global__ __launch_bounds__(256) void k_vn_sgd(Map map, const float* __restrict__ scratch, int region, int regions, int P, int B, float lr, float mu,
                                                float* __restrict__ params, float* __restrict__ momentum, float* __restrict__ grad,
                                                float* __restrict__ blob, float* __restrict__ loss, double* __restrict__ loss_sum)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > P) return;
    if (i == P) {
        const float l = region_sum(scratch, region, regions, i) / (float)B;
        *loss = l;
        if (loss_sum) *loss_sum += (double)l;
        return;
    }
    int twin;
    const int at = map(i, twin);
    if (at < 0) return;
    auto step = [&](int k) {
        const float buf0 = momentum[k], p0 = params[k];
        const float g = region_sum(scratch, region, regions, k);
        const float buf = fmaf(mu, buf0, g);
        const float p = fmaf(-lr, buf, p0);
        grad[k] = g;
        momentum[k] = buf;
        params[k] = p;
        return p;
    };
    float v = step(i);
    if (twin >= 0) v = v + step(twin);
    blob[at] = v;
}

// what the train-step entries check beyond their loss-and-gradient entry's checks
inline int check_sgd_args(const float* d_momentum, size_t n_momentum_floats, size_t n_param_floats, float lr, float momentum)
{
    if (!d_momentum) return fail(CS_ERR_ARG, "null argument");
    if (n_momentum_floats != n_param_floats) return fail(CS_ERR_ARG, "the momentum buffer does not have the size of the flat parameters");
    if (!std::isfinite(lr) || lr < 0.0f) return fail(CS_ERR_ARG, "lr must be finite and at least 0");
    if (!std::isfinite(momentum) || momentum < 0.0f) return fail(CS_ERR_ARG, "momentum must be finite and at least 0");
    return CS_OK;
}

} // namespace
