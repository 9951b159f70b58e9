// value_net_grad.h -- what the training entries of the four value-network families (value_net_grad.hip: CADRL / SARL / OM-SARL;
// value_net_lstm_grad.hip: LSTM-RL / OM-LSTM-RL) share.  Device: the flat parameter offsets, the layer-indexed part of the LDS map, the forward
// layer of a 32-row tile, the three backward products on v_mfma_f32_32x32x2_f32 (dX = dZ W, dWt = dZt X, db), the chains over them, the value
// head of a job (VG_LOSS_HEAD), the kernel that sums the workgroups' regions, the one that sums them, takes the SGD-momentum step and rewrites
// the blob (k_vn_sgd, the train-step entries), and pack_layer_f32's map read forwards (blob_layer_at) and backwards (unpack_layer_at, the
// device-pack kernels).  Host: one call of an entry as a struct (GradCall) and the host functions behind the entries -- plan_grad, check_grad_args
// and one per kind of entry: grad_sizes, loss_grad, train_step, blob_index, pack_device --, templates over the family type each .hip file defines.  Unnamed
// namespace: each translation unit gets its own copy.
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

// The value head of a job behind its last layer: the values of its ng groups from gbase, the loss terms and dV = 2 (V - target) / B as the
// top gradient [32][12] in D0; thread 0 adds the job's loss terms, in group order, to its `loss`.  Reads the kernel's p, b, tid, gbase, ng,
// B, targets, values and loss; M: its GradLds; UNROLL: what stands before the loop (the recurrent kernels' `unroll 1`, or nothing).  A
// macro: as an inline function it left both recurrent builds at their registers but moved their schedule (DESIGN.md 4.5 "where the training side's pieces live").
#define VG_LOSS_HEAD(M, UNROLL)                                                                                              \
    {                                                                                                                        \
        const int last = p.n_layers - 1;                                                                                     \
        const float* out = b.lds + M.act[last];                                                                              \
        const int ldo = M.ld[last];                                                                                          \
        UNROLL                                                                                                               \
        for (int i = tid; i < 32 * ldo; i += NT) {                                                                           \
            const int k = i / ldo, c = i - k * ldo;                                                                          \
            float d = 0.0f;                                                                                                  \
            if (c == 0 && k < ng) {                                                                                          \
                const float v = out[k * ldo];                                                                                \
                if (values) values[gbase + k] = 0.0f + v;                                                                    \
                d = v - targets[gbase + k];                                                                                  \
                b.val[k] = d * d;                                                                                            \
                d = 2.0f * d / (float)B;                                                                                     \
            }                                                                                                                \
            b.D0[i] = d;                                                                                                     \
        }                                                                                                                    \
        __syncthreads();                                                                                                     \
        if (tid == 0) {                                                                                                      \
            float s = 0.0f;                                                                                                  \
            for (int k = 0; k < ng; ++k) s += b.val[k];                                                                      \
            loss += s;                                                                                                       \
        }                                                                                                                    \
    }

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

// pack_layer_f32's loop variables of float e of a layer's weights in the blob: the 32-column block, the column in it, the k-group and the
// column kk counted in the blob's k-groups
__device__ __forceinline__ void blob_weight_of(const VnLayer& L, int e, int& cb, int& col, int& kg, int& kk)
{
    const int s = e & 3, lane = (e >> 2) & 63, q = e >> 8;
    kg = q % L.kg_total;
    cb = q / L.kg_total;
    col = lane & 31;
    kk = kg * 8 + 4 * (lane >> 5) + s;
}

// blob float i of a Linear layer from its flat (weight [N][K1 + K2], bias [N]) pair: pack_layer_f32's map, read backwards (blob_layer_at
// reads it forwards); the padding is 0
__device__ __forceinline__ float unpack_layer_at(const VnLayer& L, int i, const float* __restrict__ weight, const float* __restrict__ bias)
{
    if (i >= L.b_off) return i - L.b_off < L.N ? bias[i - L.b_off] : 0.0f;
    int cb, col, kg, kk;
    blob_weight_of(L, i - L.w_off, cb, col, kg, kk);
    const int j = cb * 32 + col;
    int k = -1;
    if (kg < L.kg_split) { if (kk < L.K1) k = kk; }
    else if (kk - L.kg_split * 8 < L.K2) k = L.K1 + kk - L.kg_split * 8;
    return j < L.N && k >= 0 ? weight[(long)j * (L.K1 + L.K2) + k] : 0.0f;
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

// ---------------------------------------------------------------------------------------------------------------- the entries' host side
// One call of a training entry, whichever of the twenty: an extern "C" function fills the fields its arguments name (the rest stay null / 0)
// and hands it to one of the templates below.  `kind` is the feed-forward entries' alone; `om`: an *_om entry, whose rows carry om_cols
// map columns behind the cols rotated ones.  d_weights is the float32 blob: read by the job kernel, rewritten by the train-step and the
// device-pack entries.
struct GradCall {
    int kind; const int32_t* dims; int n_dims, cols; bool om; int om_cols;                      // the description
    int B, n; const float *d_rows, *d_targets;                                                  // the minibatch
    float* d_weights; size_t n_weight_floats; float* d_params; size_t n_param_floats; float* d_momentum; size_t n_momentum_floats;
    float *d_grad, *d_loss; double* d_loss_sum; float *d_values, *d_scratch; size_t n_scratch_floats;
    float lr, momentum;
    void* stream;
};

inline GradCall describe_call(int kind, const int32_t* dims, int n_dims, int cols, bool om, int om_cols, int B = 0, int n = 0)
{
    GradCall c{};
    c.kind = kind; c.dims = dims; c.n_dims = n_dims; c.cols = cols; c.om = om; c.om_cols = om_cols; c.B = B; c.n = n;
    return c;
}

// the arguments of a loss-and-gradient entry behind the description
inline void set_minibatch(GradCall& c, const float* d_weights, size_t n_weight_floats, const float* d_params, size_t n_param_floats,
                          const float* d_rows, const float* d_targets, float* d_grad, float* d_loss, float* d_values, float* d_scratch,
                          size_t n_scratch_floats, void* stream)
{
    c.d_weights = const_cast<float*>(d_weights); c.n_weight_floats = n_weight_floats; c.d_params = const_cast<float*>(d_params); c.n_param_floats = n_param_floats;
    c.d_rows = d_rows; c.d_targets = d_targets; c.d_grad = d_grad; c.d_loss = d_loss; c.d_values = d_values;
    c.d_scratch = d_scratch; c.n_scratch_floats = n_scratch_floats; c.stream = stream;
}

// what a train-step entry takes beyond them
inline void set_sgd(GradCall& c, float* d_momentum, size_t n_momentum_floats, float lr, float momentum, double* d_loss_sum)
{
    c.d_momentum = d_momentum; c.n_momentum_floats = n_momentum_floats; c.lr = lr; c.momentum = momentum; c.d_loss_sum = d_loss_sum;
}

// the arguments of a device-pack entry behind the description
inline void set_pack(GradCall& c, const float* d_params, size_t n_param_floats, float* d_blob, size_t n_blob_floats, void* stream)
{
    c.d_params = const_cast<float*>(d_params); c.n_param_floats = n_param_floats; c.d_weights = d_blob; c.n_weight_floats = n_blob_floats; c.stream = stream;
}

// The host functions below exist once, over a family type F (FeedForwardGrad in value_net_grad.hip, LstmGrad in value_net_lstm_grad.hip):
//   F::Launch          the launch record: the plan, the offsets `o`, the LDS map, grid, region, shmem; blob_floats()
//   F::describe(c, q)  the plan of the description and the flat offsets
//   F::check_n(c)      the family's own check of n, made between "n < 1" and "B * n"
//   F::plan(c, q)      the LDS map -- refused in the family's words when it does not fit --, the grid and the region (P + 1 rounded up to 4,
//                      plus the tape for the recurrent family)
//   F::launch_jobs(q, c), F::sgd_map(q), F::launch_pack(q, c)
//   F::pack_entry, F::sizes_entry   the entry names the messages quote
template <class F>
inline int plan_grad(const GradCall& c, typename F::Launch& q)
{
    const int rc = F::describe(c, q);
    if (rc != CS_OK) return rc;
    if (c.B < 1) return fail(CS_ERR_ARG, "B must be positive");
    if (c.n < 1) return fail(CS_ERR_ARG, "n must be at least 1: a value network needs a human to look at");
    const int rc1 = F::check_n(c);
    if (rc1 != CS_OK) return rc1;
    if ((long)c.B * c.n > INT_MAX / 16) return fail(CS_ERR_ARG, "B * n is too large");
    return F::plan(c, q);
}

// a size that is not this network's: `what`, and in brackets the entry that tells the right one
inline int size_refusal(const char* what, const char* entry) { return fail(CS_ERR_ARG, std::string(what) + " (" + entry + ")"); }

// cs_value_net_grad_sizes[_lstm][_om]
template <class F>
inline int grad_sizes(const GradCall& c, size_t* n_param_floats, size_t* n_scratch_floats)
{
    typename F::Launch q;
    const int rc = plan_grad<F>(c, q);
    if (rc != CS_OK) return rc;
    if (!n_param_floats || !n_scratch_floats) return fail(CS_ERR_ARG, "null argument");
    *n_param_floats = (size_t)q.o.total;
    *n_scratch_floats = (size_t)q.grid * q.region;
    return CS_OK;
}

// the argument checks of the loss-and-gradient entries, which the train-step entries make first
template <class F>
inline int check_grad_args(const GradCall& c, typename F::Launch& q)
{
    const int rc = plan_grad<F>(c, q);
    if (rc != CS_OK) return rc;
    if (!c.d_weights || !c.d_params || !c.d_rows || !c.d_targets || !c.d_grad || !c.d_loss || !c.d_scratch) return fail(CS_ERR_ARG, "null argument");
    if (c.n_weight_floats != q.blob_floats()) return size_refusal("the weight blob does not have the size of this network", F::pack_entry);
    if (c.n_param_floats != (size_t)q.o.total) return size_refusal("the flat parameters do not have the size of this network", F::sizes_entry);
    if (c.n_scratch_floats < (size_t)q.grid * q.region) return size_refusal("the scratch is too small for this minibatch", F::sizes_entry);
    return CS_OK;
}

// cs_value_net_loss_grad[_lstm][_om]: the job kernel, then the regions summed
template <class F>
inline int loss_grad(const GradCall& c)
{
    typename F::Launch q;
    const int rc = check_grad_args<F>(c, q);
    if (rc != CS_OK) return rc;
    const int rc2 = F::launch_jobs(q, c);
    if (rc2 != CS_OK) return rc2;
    hipLaunchKernelGGL(k_vn_grad_sum, dim3((q.o.total + 1 + 255) / 256), dim3(256), 0, (hipStream_t)c.stream, c.d_scratch, q.region, q.grid, q.o.total, c.B,
                       c.d_grad, c.d_loss);
    HIP_TRY(hipGetLastError());
    return CS_OK;
}

// cs_value_net_train_step[_lstm][_om]: the job kernel, then k_vn_sgd on the family's map of its blob
template <class F>
inline int train_step(const GradCall& c)
{
    typename F::Launch q;
    const int rc = check_grad_args<F>(c, q);
    if (rc != CS_OK) return rc;
    if (!c.d_momentum) return fail(CS_ERR_ARG, "null argument");
    if (c.n_momentum_floats != c.n_param_floats) return fail(CS_ERR_ARG, "the momentum buffer does not have the size of the flat parameters");
    if (!std::isfinite(c.lr) || c.lr < 0.0f) return fail(CS_ERR_ARG, "lr must be finite and at least 0");
    if (!std::isfinite(c.momentum) || c.momentum < 0.0f) return fail(CS_ERR_ARG, "momentum must be finite and at least 0");
    const int rc2 = F::launch_jobs(q, c);
    if (rc2 != CS_OK) return rc2;
    hipLaunchKernelGGL(k_vn_sgd<decltype(F::sgd_map(q))>, dim3((q.o.total + 1 + 255) / 256), dim3(256), 0, (hipStream_t)c.stream, F::sgd_map(q), c.d_scratch,
                       q.region, q.grid, q.o.total, c.B, c.lr, c.momentum, c.d_params, c.d_momentum, c.d_grad, c.d_weights, c.d_loss, c.d_loss_sum);
    HIP_TRY(hipGetLastError());
    return CS_OK;
}

// cs_value_net_blob_index[_lstm][_om]: a parameter whose map answers no float of its own (the LSTM's bias_hh) is written by its partner,
// which names it as its twin; the feed-forward map has no twins
template <class F>
inline int blob_index(const GradCall& c, int32_t* index, size_t n_param_floats)
{
    typename F::Launch q;
    const int rc = F::describe(c, q);
    if (rc != CS_OK) return rc;
    if (!index) return fail(CS_ERR_ARG, "null argument");
    if (n_param_floats != (size_t)q.o.total) return size_refusal("the flat parameters do not have the size of this network", F::sizes_entry);
    const auto map = F::sgd_map(q);
    for (int i = 0; i < q.o.total; ++i) {
        int twin;
        const int at = map(i, twin);
        if (at >= 0) index[i] = at;
        if (twin >= 0) index[twin] = at;
    }
    return CS_OK;
}

// cs_value_net_pack[_lstm][_om]_device: the blob (c.d_weights) from the flat parameters
template <class F>
inline int pack_device(const GradCall& c)
{
    typename F::Launch q;
    const int rc = F::describe(c, q);
    if (rc != CS_OK) return rc;
    if (!c.d_params || !c.d_weights) return fail(CS_ERR_ARG, "null argument");
    if (c.n_param_floats != (size_t)q.o.total) return size_refusal("the flat parameters do not have the size of this network", F::sizes_entry);
    if (c.n_weight_floats != q.blob_floats()) return size_refusal("the weight blob does not have the size of this network", F::pack_entry);
    F::launch_pack(q, c);
    HIP_TRY(hipGetLastError());
    return CS_OK;
}

} // namespace
