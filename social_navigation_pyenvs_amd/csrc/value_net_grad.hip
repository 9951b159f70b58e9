// value_net_grad.hip -- the training side of the feed-forward value networks (CADRL, SARL), fused: for a minibatch of B stored states the
// forward pass, the mean-squared-error loss against B targets and the gradient of that loss with respect to every parameter
// (cs_value_net_loss_grad), and the packing of the flat parameters into the decision kernels' blob on the device (cs_value_net_pack_device).
// Replaces, per optimiser step, crowd_nav/utils/trainer.py:50-71 (zero_grad, model(inputs), MSELoss, backward) for the networks of
// crowd_nav/policy/sarl.py:28-65 and crowd_nav/policy/cadrl.py:116-123; the optimiser stays torch's.
//
// Shape of the work.  A "group" is one sample: n rows [cols], one value.  As in value_net.hip a workgroup (4 wavefronts) takes jobs of 32
// groups and walks a job in tiles of 32 rows: whole groups while n <= 32, otherwise one group in chunks of 32 humans.  Every product of a tile --
// Z = X Wt, dX = dZ W, dWt = dZt X -- is a run of v_mfma_f32_32x32x2_f32 on 32 x 32 output blocks, one wavefront a block at a time.  The
// forward layers read the packed blob exactly as value_net_plan.h's layer_fwd does (the same fmaf chain per output element) and the
// reductions are value_net_body.inc's, so the values are the decision kernels' bits.  The backward products read the flat parameters in
// torch's own layout: W [N][K] row-major is the B operand of dX as it lies (lane = k).
//
// A job runs in three steps.  (1) forward over its tiles: the softmax weights and the joint rows J (self state, weighted feature).
// (2) mlp3 forward on the 32 joint rows, the loss terms, dV = 2 (V - target) / B, mlp3 backward: dJ.  (3) the tiles again: the forward is
// recomputed with every layer's output kept in LDS, then mlp2, the softmax, the attention chain and the mean, and mlp1 run backward.
// Recomputing the tile's forward is what lets mlp3's activations and the tile's share one LDS region (DESIGN.md 4.5 has the map).  A group
// in chunks needs three sums over ALL its humans before a chunk can go backward -- the crowd mean, the softmax denominator and
// sum_k w_k dw_k -- and hands the mean's gradient back only after its last chunk: each is a pass over the chunks of its own, and mlp1's
// backward (linear in its top gradient) takes the mean's share in a last pass.
//
// Sums.  A workgroup owns one region of d_scratch ([P parameters + 1 loss term]); it zeroes it, and every dW block and db column is added to
// it by the same lane in tile order (plain loads and stores, no atomics).  k_vn_grad_sum then adds the regions in index order into d_grad.
// The bits depend on B (the number of workgroups), never on timing.  gfx950 only.
#include <hip/hip_runtime.h>

#include "value_net_plan.h"

namespace {

constexpr int GRAD_MAX_GROUPS = 256;          // workgroups = scratch regions at most: one per CU

struct GradOffsets { int w[VN_MAX_LAYERS], b[VN_MAX_LAYERS], total; };      // floats into the flat parameters: weight [N][K], bias [N] per layer

inline GradOffsets param_offsets(const VnPlan& p)
{
    GradOffsets o{};
    int at = 0;
    for (int l = 0; l < p.n_layers; ++l) {
        o.w[l] = at; at += p.L[l].N * (p.L[l].K1 + p.L[l].K2);
        o.b[l] = at; at += p.L[l].N;
    }
    o.total = at;
    return o;
}

// LDS map of the gradient kernel (floats).  act[l]: the output of layer l, 32 rows of up(N, 8) + 4 floats; mlp3's layers share the floats of
// the tile's (mlp1, mlp2, attention) layers.
struct GradLds { int X0, act[VN_MAX_LAYERS], ld[VN_MAX_LAYERS], D0, D1, dH, G, dG, J, dJ, sc, dw, den, val, grp, total; };

inline int ld8(int w) { return up(w, 8) + 4; }

inline GradLds grad_lds_map(const VnPlan& p, int n)
{
    GradLds m{};
    int o = 0, widest = 8;
    auto take = [&](int floats) { const int at = o; o += up(floats, 4); return at; };
    m.X0 = take(32 * LDX);
    const int tile_layers = p.kind == CS_VN_SARL ? p.c0[3] : p.n_layers;
    const int base = o;
    for (int l = 0; l < p.n_layers; ++l) {
        if (l == tile_layers) o = base;                  // mlp3 over the tile's activations
        m.ld[l] = ld8(p.L[l].N);
        m.act[l] = take(32 * m.ld[l]);
        widest = p.L[l].N > widest ? p.L[l].N : widest;
        widest = p.L[l].K1 > widest ? p.L[l].K1 : widest;
    }
    int end = o;
    o = base;
    for (int l = 0; l < tile_layers; ++l) take(32 * m.ld[l]);
    o = o > end ? o : end;
    m.D0 = take(32 * ld8(widest));
    m.D1 = take(32 * ld8(widest));
    if (p.kind == CS_VN_SARL) {
        const int ld_m1 = ld8(p.m1w);
        m.dH = take(32 * ld_m1);
        m.G = n == 1 ? m.act[p.c0[1] - 1] : take((n <= 32 ? 32 / n : 1) * ld_m1);      // one human: the mean of mlp1 over the group IS its row
        m.dG = take(ld_m1);                              // the mean's gradient of a group in chunks, summed over its chunks
        m.J = take(32 * p.ld_j);
        m.dJ = take(32 * p.ld_j);
    }
    m.sc = take(32); m.dw = take(32); m.den = take(32); m.val = take(32); m.grp = take(32);
    m.total = o;
    return m;
}

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

// what a visit of a tile does beside the layers: the self state into J; the crowd mean of whole groups into G; the softmax denominator
// summed into den; stop behind the denominator (a group in chunks needs it whole before its first weight, sarl.py:52-53); the weighted
// feature summed into J
enum { T_SELF = 1, T_MEAN = 2, T_DEN = 4, T_STOP = 8, T_J = 16 };

// The forward of one tile of a SARL job, value_net_body.inc's arithmetic: `tg` groups from group t0 of the job, `per` humans of each in
// this tile (all n of them, or one chunk of a group walked in chunks), rows = tg * per.  Leaves every layer's output and the softmax
// weights in sc (the terms exp(s) (s != 0) with T_STOP).
__device__ __forceinline__ void sarl_tile_fwd(const VnPlan& p, const GradLds& m, const GradBufs& b, const float* __restrict__ wb, int t0, int tg,
                                              int per, int rows, int n, int what)
{
    const int tid = threadIdx.x;
    const int ld_m1 = m.ld[p.c0[1] - 1], m1pad = (p.m1w + 7) & ~7;
    float* M1 = (b.lds + m.act[p.c0[1] - 1]);
    if (what & T_SELF)      // sarl.py:36: the self state is read from the first human's row
        for (int i = tid; i < tg * SELF_DIM; i += NT) b.J[(t0 + i / SELF_DIM) * p.ld_j + i % SELF_DIM] = b.X0[(i / SELF_DIM) * per * LDX + i % SELF_DIM];
    chain_fwd(p, m, b, wb, p.c0[0], p.c0[1], b.X0, LDX, nullptr, 0);
    if (what & T_MEAN) {
        for (int i = tid; i < tg * m1pad; i += NT) {
            const int k = i / m1pad, c = i - k * m1pad;
            float s = 0.0f;
            for (int j = 0; j < n; ++j) s += M1[(k * n + j) * ld_m1 + c];
            b.G[k * ld_m1 + c] = s / (float)n;
        }
        __syncthreads();
    }
    chain_fwd(p, m, b, wb, p.c0[2], p.c0[3], M1, ld_m1, p.with_global ? b.G : nullptr, ld_m1);
    {   // the masked softmax's terms exp(s) * (s != 0) (sarl.py:48-52)
        const float* out = (b.lds + m.act[p.c0[3] - 1]);
        const int ldo = m.ld[p.c0[3] - 1];
        for (int r = tid; r < 32; r += NT) {
            const float s = out[r * ldo];
            b.sc[r] = (r < rows && s != 0.0f) ? expf(s) : 0.0f;
        }
        __syncthreads();
    }
    if (what & T_DEN) {     // the denominator, in human order
        if (tid < tg) {
            float s = b.den[t0 + tid];
            for (int j = 0; j < per; ++j) s += b.sc[tid * per + j];
            b.den[t0 + tid] = s;
        }
        __syncthreads();
    }
    if (what & T_STOP) return;
    for (int r = tid; r < rows; r += NT) b.sc[r] = b.sc[r] / b.den[t0 + r / per];
    __syncthreads();
    chain_fwd(p, m, b, wb, p.c0[1], p.c0[2], M1, ld_m1, nullptr, 0);
    if (what & T_J) {       // the weighted sum of mlp2's rows (sarl.py:57-60)
        const float* f = (b.lds + m.act[p.c0[2] - 1]);
        const int ldf = m.ld[p.c0[2] - 1], fw = p.feat;
        for (int i = tid; i < tg * fw; i += NT) {
            const int k = i / fw, c = i - k * fw;
            float s = b.J[(t0 + k) * p.ld_j + SELF_DIM + c];
            for (int j = 0; j < per; ++j) s = fmaf(b.sc[k * per + j], f[(k * per + j) * ldf + c], s);
            b.J[(t0 + k) * p.ld_j + SELF_DIM + c] = s;
        }
        __syncthreads();
    }
}

// dw_j = f_j . dF of the tile's rows (0 beyond them), behind a forward that left mlp2's output
__device__ __forceinline__ void sarl_tile_dw(const VnPlan& p, const GradLds& m, const GradBufs& b, int t0, int per, int rows)
{
    const float* f = (b.lds + m.act[p.c0[2] - 1]);
    const int ldf = m.ld[p.c0[2] - 1], tid = threadIdx.x;
    if (tid < 32) {
        float s = 0.0f;
        if (tid < rows)
            for (int c = 0; c < p.feat; ++c) s = fmaf(f[tid * ldf + c], b.dJ[(t0 + tid / per) * p.ld_j + SELF_DIM + c], s);
        b.dw[tid] = s;
    }
    __syncthreads();
}

// The backward of one tile behind sarl_tile_fwd and sarl_tile_dw: mlp2, the softmax, the attention chain, the mean, mlp1.  `whole`: the
// tile holds its groups whole -- sum_k w_k dw_k is formed here (into val) and the mean's gradient goes back to the tile's rows; else val[0]
// holds that sum over all the group's chunks, the mean's gradient is added to dG and goes back in a pass of its own (mlp1_mean_bwd).
__device__ __forceinline__ void sarl_tile_bwd(const VnPlan& p, const GradLds& m, const GradBufs& b, const float* __restrict__ params, const GradOffsets& o,
                                              float* g, int t0, int tg, int per, int rows, int n, bool whole)
{
    const int tid = threadIdx.x;
    const int l_m1 = p.c0[1] - 1, l_f = p.c0[2] - 1, l_a = p.c0[3] - 1;
    const int ld_m1 = m.ld[l_m1], ldf = m.ld[l_f], lda = m.ld[l_a];
    float* M1 = (b.lds + m.act[l_m1]);
    for (int i = tid; i < 32 * ldf; i += NT) {      // F = sum_j w_j f_j: df_j = w_j dF
        const int r = i / ldf, c = i - r * ldf;
        b.D0[i] = (r < rows && c < p.feat) ? b.sc[r] * b.dJ[(t0 + r / per) * p.ld_j + SELF_DIM + c] : 0.0f;
    }
    __syncthreads();
    chain_bwd(p, m, b, params, o, g, p.c0[1], p.c0[2], b.D0, M1, ld_m1, nullptr, 0, b.dH, ld_m1, false, nullptr, 0);
    if (whole) {
        if (tid < tg) {
            float s = 0.0f;
            for (int j = 0; j < per; ++j) s = fmaf(b.sc[tid * per + j], b.dw[tid * per + j], s);
            b.val[tid] = s;
        }
        __syncthreads();
    }
    for (int i = tid; i < 32 * lda; i += NT) {      // w = e / sum e with the mask a constant: ds_j = w_j (dw_j - sum_k w_k dw_k)
        const int r = i / lda, c = i - r * lda;
        b.D0[i] = (r < rows && c == 0) ? b.sc[r] * (b.dw[r] - b.val[r / per]) : 0.0f;
    }
    __syncthreads();
    // the attention chain; its input (mlp1, crowd mean): the first part adds to dH, the second goes to the free one of D0 / D1
    float* T = ((p.c0[3] - p.c0[2]) & 1) ? b.D1 : b.D0;
    chain_bwd(p, m, b, params, o, g, p.c0[2], p.c0[3], b.D0, M1, ld_m1, p.with_global ? b.G : nullptr, ld_m1, b.dH, ld_m1, true,
              p.with_global ? T : nullptr, ld_m1);
    if (p.with_global) {        // the mean hands 1 / n of its gradient to every human of the group
        if (whole) {
            for (int i = tid; i < tg * p.m1w; i += NT) {
                const int k = i / p.m1w, c = i - k * p.m1w;
                float s = 0.0f;
                for (int j = 0; j < n; ++j) s += T[(k * n + j) * ld_m1 + c];
                s = s / (float)n;
                for (int j = 0; j < n; ++j) b.dH[(k * n + j) * ld_m1 + c] += s;
            }
        } else {
            for (int c = tid; c < p.m1w; c += NT) {
                float s = b.dG[c];
                for (int r = 0; r < rows; ++r) s += T[r * ld_m1 + c];
                b.dG[c] = s;
            }
        }
        __syncthreads();
    }
    for (int i = tid; i < 32 * ld_m1; i += NT)      // mlp1 ends in a ReLU (last_relu)
        if (!(M1[i] > 0.0f)) b.dH[i] = 0.0f;
    __syncthreads();
    chain_bwd(p, m, b, params, o, g, p.c0[0], p.c0[1], b.dH, b.X0, LDX, nullptr, 0, nullptr, 0, false, nullptr, 0);
}

__global__ __launch_bounds__(NT) void k_vn_grad(VnPlan p, GradLds m, GradOffsets o, const float* __restrict__ wb, const float* __restrict__ params,
                                                int B, int n, int jrows, const float* __restrict__ rows_in, const float* __restrict__ targets,
                                                float* __restrict__ scratch, int region, float* __restrict__ values)
{
    extern __shared__ float lds[];
    GradBufs b;
    b.X0 = lds + m.X0; b.D0 = lds + m.D0; b.D1 = lds + m.D1; b.dH = lds + m.dH; b.G = lds + m.G; b.dG = lds + m.dG; b.J = lds + m.J; b.dJ = lds + m.dJ;
    b.sc = lds + m.sc; b.dw = lds + m.dw; b.den = lds + m.den; b.val = lds + m.val; b.grp = reinterpret_cast<int*>(lds + m.grp);
    b.lds = lds;
    const int tid = threadIdx.x, cols = p.cols;
    const bool sarl = p.kind == CS_VN_SARL;
    float* g = scratch + (long)blockIdx.x * region;
    VnBufs lb{};
    lb.X0 = b.X0; lb.grp = b.grp;

    for (int i = tid; i < region; i += NT) g[i] = 0.0f;
    float loss = 0.0f;                  // thread 0's: the job sums, in job order
    __syncthreads();

    const int chunks = n <= 32 ? 1 : (n + 31) / 32;
    const int gpt = n <= 32 ? 32 / n : 1;
    const int l_m1 = sarl ? p.c0[1] - 1 : 0, ld_m1 = m.ld[l_m1], m1pad = (p.m1w + 7) & ~7;
    float* M1 = (b.lds + m.act[l_m1]);

    for (int job = blockIdx.x; (long)job * jrows < B; job += gridDim.x) {
        const int gbase = job * jrows;
        const int ng = B - gbase < jrows ? B - gbase : jrows;
        // chunk ch of the tile whose first group is the job's t0: `per` humans of each of its tg groups
        auto load = [&](int t0, int tg, int ch, int per) {
            load_tile(lb, rows_in + ((long)(gbase + t0) * n + ch * 32) * cols, tg * per, cols, per, 32);
            __syncthreads();
        };
        auto chunk_rows = [&](int ch) { return n - ch * 32 < 32 ? n - ch * 32 : 32; };
        // more humans than a tile holds: a pass over the chunks for the mean of mlp1 (sarl.py:42), a running sum in G's row
        auto mean_pass = [&](int t0) {
            for (int c = tid; c < ld_m1; c += NT) b.G[c] = 0.0f;
            for (int ch = 0; ch < chunks; ++ch) {
                const int per = chunk_rows(ch);
                load(t0, 1, ch, per);
                chain_fwd(p, m, b, wb, p.c0[0], p.c0[1], b.X0, LDX, nullptr, 0);
                for (int c = tid; c < m1pad; c += NT) {
                    float s = b.G[c];
                    for (int r = 0; r < per; ++r) s += M1[r * ld_m1 + c];
                    b.G[c] = s;
                }
                __syncthreads();
            }
            for (int c = tid; c < m1pad; c += NT) b.G[c] = b.G[c] / (float)n;
            __syncthreads();
        };
        if (sarl) {
            for (int i = tid; i < JROWS * p.ld_j; i += NT) b.J[i] = 0.0f;
            if (tid < JROWS) b.den[tid] = 0.0f;
            __syncthreads();
            for (int t0 = 0; t0 < ng; t0 += gpt) {
                const int tg = ng - t0 < gpt ? ng - t0 : gpt;
                if (chunks == 1) {
                    load(t0, tg, 0, n);
                    sarl_tile_fwd(p, m, b, wb, t0, tg, n, tg * n, n, T_SELF | (p.with_global && n > 1 ? T_MEAN : 0) | T_DEN | T_J);
                    continue;
                }
                if (p.with_global) mean_pass(t0);
                for (int ch = 0; ch < chunks; ++ch) {
                    load(t0, 1, ch, chunk_rows(ch));
                    sarl_tile_fwd(p, m, b, wb, t0, 1, chunk_rows(ch), chunk_rows(ch), n, T_DEN | T_STOP);
                }
                for (int ch = 0; ch < chunks; ++ch) {
                    load(t0, 1, ch, chunk_rows(ch));
                    sarl_tile_fwd(p, m, b, wb, t0, 1, chunk_rows(ch), chunk_rows(ch), n, (ch == 0 ? T_SELF : 0) | T_J);
                }
            }
            chain_fwd(p, m, b, wb, p.c0[3], p.c0[4], b.J, p.ld_j, nullptr, 0);
        } else {
            load(0, ng, 0, 1);
            chain_fwd(p, m, b, wb, p.c0[0], p.c0[1], b.X0, LDX, nullptr, 0);
        }
        {   // the values, the loss terms and dV = 2 (V - target) / B as the top gradient [32][12] in D0
            const int last = p.n_layers - 1;
            const float* out = (b.lds + m.act[last]);
            const int ldo = m.ld[last];
            for (int i = tid; i < 32 * ldo; i += NT) {
                const int k = i / ldo, c = i - k * ldo;
                float d = 0.0f;
                if (c == 0 && k < ng) {
                    const float v = out[k * ldo];
                    if (values) values[gbase + k] = 0.0f + v;
                    d = v - targets[gbase + k];
                    b.val[k] = d * d;
                    d = 2.0f * d / (float)B;
                }
                b.D0[i] = d;
            }
            __syncthreads();
            if (tid == 0) {
                float s = 0.0f;
                for (int k = 0; k < ng; ++k) s += b.val[k];
                loss += s;
            }
        }
        if (!sarl) {
            chain_bwd(p, m, b, params, o, g, p.c0[0], p.c0[1], b.D0, b.X0, LDX, nullptr, 0, nullptr, 0, false, nullptr, 0);
            continue;
        }
        chain_bwd(p, m, b, params, o, g, p.c0[3], p.c0[4], b.D0, b.J, p.ld_j, nullptr, 0, b.dJ, p.ld_j, false, nullptr, 0);

        for (int t0 = 0; t0 < ng; t0 += gpt) {
            const int tg = ng - t0 < gpt ? ng - t0 : gpt;
            if (chunks == 1) {
                load(t0, tg, 0, n);
                sarl_tile_fwd(p, m, b, wb, t0, tg, n, tg * n, n, p.with_global && n > 1 ? T_MEAN : 0);
                sarl_tile_dw(p, m, b, t0, n, tg * n);
                sarl_tile_bwd(p, m, b, params, o, g, t0, tg, n, tg * n, n, true);
                continue;
            }
            // a group in chunks: its mean again; sum_k w_k dw_k over all its chunks; the chunks' backward; the mean's gradient to mlp1
            if (p.with_global) mean_pass(t0);
            if (tid == 0) b.val[0] = 0.0f;
            for (int c = tid; c < ld_m1; c += NT) b.dG[c] = 0.0f;
            for (int ch = 0; ch < chunks; ++ch) {
                const int per = chunk_rows(ch);
                load(t0, 1, ch, per);
                sarl_tile_fwd(p, m, b, wb, t0, 1, per, per, n, 0);
                sarl_tile_dw(p, m, b, t0, per, per);
                if (tid == 0) {
                    float s = b.val[0];
                    for (int j = 0; j < per; ++j) s = fmaf(b.sc[j], b.dw[j], s);
                    b.val[0] = s;
                }
                __syncthreads();
            }
            for (int ch = 0; ch < chunks; ++ch) {
                const int per = chunk_rows(ch);
                load(t0, 1, ch, per);
                sarl_tile_fwd(p, m, b, wb, t0, 1, per, per, n, 0);
                sarl_tile_dw(p, m, b, t0, per, per);
                sarl_tile_bwd(p, m, b, params, o, g, t0, 1, per, per, n, false);
            }
            if (p.with_global)
                for (int ch = 0; ch < chunks; ++ch) {
                    const int per = chunk_rows(ch);
                    load(t0, 1, ch, per);
                    chain_fwd(p, m, b, wb, p.c0[0], p.c0[1], b.X0, LDX, nullptr, 0);
                    for (int i = tid; i < 32 * ld_m1; i += NT) {
                        const int r = i / ld_m1, c = i - r * ld_m1;
                        b.dH[i] = (r < per && c < p.m1w && M1[i] > 0.0f) ? b.dG[c] / (float)n : 0.0f;
                    }
                    __syncthreads();
                    chain_bwd(p, m, b, params, o, g, p.c0[0], p.c0[1], b.dH, b.X0, LDX, nullptr, 0, nullptr, 0, false, nullptr, 0);
                }
        }
    }
    if (tid == 0) g[o.total] = loss;
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

// blob float i from the flat parameters: pack_layer_f32's map, read backwards
__global__ void k_vn_pack(VnPlan p, GradOffsets o, const float* __restrict__ params, float* __restrict__ blob)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.total_floats) return;
    int l = 0;
    while (l + 1 < p.n_layers && i >= p.L[l + 1].w_off) ++l;
    const VnLayer& L = p.L[l];
    float v = 0.0f;
    if (i >= L.b_off) {
        const int j = i - L.b_off;
        if (j < L.N) v = params[o.b[l] + j];
    } else {
        const int e = i - L.w_off;
        const int s = e & 3, lane = (e >> 2) & 63, q = e >> 8;
        const int kg = q % L.kg_total, cb = q / L.kg_total;
        const int j = cb * 32 + (lane & 31);
        const int kk = kg * 8 + 4 * (lane >> 5) + s;
        int k = -1;
        if (kg < L.kg_split) { if (kk < L.K1) k = kk; }
        else if (kk - L.kg_split * 8 < L.K2) k = L.K1 + kk - L.kg_split * 8;
        if (j < L.N && k >= 0) v = params[o.w[l] + (long)j * (L.K1 + L.K2) + k];
    }
    blob[i] = v;
}

// what the entries of this file check alike: the description, the shape of the minibatch; leaves the plan, the offsets, the map, the grid
struct GradLaunch { VnPlan p; GradOffsets o; GradLds m; int grid, region, jrows; size_t shmem; };

inline int plan_grad(int kind, const int32_t* dims, int n_dims, int cols, int B, int n, GradLaunch& q)
{
    const int rc = build_plan(kind, dims, n_dims, cols, 0, q.p);
    if (rc != CS_OK) return rc;
    if (B < 1) return fail(CS_ERR_ARG, "B must be positive");
    if (n < 1) return fail(CS_ERR_ARG, "n must be at least 1: a value network needs a human to look at");
    if (kind == CS_VN_CADRL && n != 1) return fail(CS_ERR_ARG, "CADRL's trainer stores one human's row per sample: n must be 1");
    if ((long)B * n > INT_MAX / 16) return fail(CS_ERR_ARG, "B * n is too large");
    q.o = param_offsets(q.p);
    q.m = grad_lds_map(q.p, n);
    q.shmem = (size_t)q.m.total * sizeof(float);
    if (q.shmem > 160 * 1024) return fail(CS_ERR_ARG, "the activations and gradients of a tile of this network do not fit the 160 KiB of LDS");
    // groups per job: whole tiles, as few as spread the minibatch over the workgroups, at most mlp3's block of 32 rows
    const int gpt = n <= 32 ? 32 / n : 1;
    const int want = up((B + GRAD_MAX_GROUPS - 1) / GRAD_MAX_GROUPS, gpt);
    q.jrows = want < JROWS ? want : JROWS;
    const int jobs = (B + q.jrows - 1) / q.jrows;
    q.grid = jobs < GRAD_MAX_GROUPS ? jobs : GRAD_MAX_GROUPS;
    q.region = up(q.o.total + 1, 4);
    return CS_OK;
}

} // namespace

extern "C" int cs_value_net_grad_sizes(int kind, const int32_t* dims, int n_dims, int cols, int B, int n, size_t* n_param_floats,
                                       size_t* n_scratch_floats)
{
    GradLaunch q;
    const int rc = plan_grad(kind, dims, n_dims, cols, B, n, q);
    if (rc != CS_OK) return rc;
    if (!n_param_floats || !n_scratch_floats) return fail(CS_ERR_ARG, "null argument");
    *n_param_floats = (size_t)q.o.total;
    *n_scratch_floats = (size_t)q.grid * q.region;
    return CS_OK;
}

extern "C" int cs_value_net_loss_grad(int kind, const int32_t* dims, int n_dims, const float* d_weights, size_t n_weight_floats, const float* d_params,
                                      size_t n_param_floats, int B, int n, int cols, const float* d_rows, const float* d_targets, float* d_grad,
                                      float* d_loss, float* d_values, float* d_scratch, size_t n_scratch_floats, void* stream)
{
    GradLaunch q;
    const int rc = plan_grad(kind, dims, n_dims, cols, B, n, q);
    if (rc != CS_OK) return rc;
    if (!d_weights || !d_params || !d_rows || !d_targets || !d_grad || !d_loss || !d_scratch) return fail(CS_ERR_ARG, "null argument");
    if (n_weight_floats != (size_t)q.p.total_floats) return fail(CS_ERR_ARG, "the weight blob does not have the size of this network (cs_value_net_pack)");
    if (n_param_floats != (size_t)q.o.total) return fail(CS_ERR_ARG, "the flat parameters do not have the size of this network (cs_value_net_grad_sizes)");
    if (n_scratch_floats < (size_t)q.grid * q.region) return fail(CS_ERR_ARG, "the scratch is too small for this minibatch (cs_value_net_grad_sizes)");
    const int rc2 = grant_lds<k_vn_grad>(q.shmem);
    if (rc2 != CS_OK) return rc2;
    hipLaunchKernelGGL(k_vn_grad, dim3(q.grid), dim3(NT), q.shmem, (hipStream_t)stream, q.p, q.m, q.o, d_weights, d_params, B, n, q.jrows, d_rows, d_targets,
                       d_scratch, q.region, d_values);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_vn_grad_sum, dim3((q.o.total + 1 + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_scratch, q.region, q.grid, q.o.total, B,
                       d_grad, d_loss);
    HIP_TRY(hipGetLastError());
    return CS_OK;
}

extern "C" int cs_value_net_pack_device(int kind, const int32_t* dims, int n_dims, int cols, const float* d_params, size_t n_param_floats,
                                        float* d_blob, size_t n_blob_floats, void* stream)
{
    VnPlan p;
    const int rc = build_plan(kind, dims, n_dims, cols, 0, p);
    if (rc != CS_OK) return rc;
    const GradOffsets o = param_offsets(p);
    if (!d_params || !d_blob) return fail(CS_ERR_ARG, "null argument");
    if (n_param_floats != (size_t)o.total) return fail(CS_ERR_ARG, "the flat parameters do not have the size of this network (cs_value_net_grad_sizes)");
    if (n_blob_floats != (size_t)p.total_floats) return fail(CS_ERR_ARG, "the weight blob does not have the size of this network (cs_value_net_pack)");
    hipLaunchKernelGGL(k_vn_pack, dim3((p.total_floats + 255) / 256), dim3(256), 0, (hipStream_t)stream, p, o, d_params, d_blob);
    HIP_TRY(hipGetLastError());
    return CS_OK;
}
