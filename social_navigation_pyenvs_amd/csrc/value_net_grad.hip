// value_net_grad.hip -- the training side of the feed-forward value networks (CADRL, SARL), fused: for a minibatch of B stored states the
// forward pass, the mean-squared-error loss against B targets and the gradient of that loss with respect to every parameter
// (cs_value_net_loss_grad), and the packing of the flat parameters into the decision kernels' blob on the device (cs_value_net_pack_device).
// The entries' host side is value_net_grad.h's templates over this file's FeedForwardGrad.
// Replaces, per optimiser step, crowd_nav/utils/trainer.py:50-71 (zero_grad, model(inputs), MSELoss, backward) for the networks of
// crowd_nav/policy/sarl.py:28-65 and crowd_nav/policy/cadrl.py:116-123; the optimiser stays torch's -- or, for SGD with momentum, runs in
// the launch that sums the gradient and rewrites the blob there (cs_value_net_train_step: value_net_grad.h k_vn_sgd).
//
// Shape of the work.  A "group" is one sample: n rows [cols], one value; for OM-SARL (the *_om entries) a row carries its human's om_cols map
// columns behind the cols rotated ones, and the input tile's stride follows (GradLds.ldx).  As in value_net.hip a workgroup (4 wavefronts) takes jobs of 32
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

#include "value_net_grad.h"

namespace {

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

inline GradLds grad_lds_map(const VnPlan& p, int n)
{
    GradLds m{};
    int o = 0, widest = 8;
    auto take = [&](int floats) { const int at = o; o += up(floats, 4); return at; };
    m.ldx = p.L[0].kg_split * 8 + 4;
    m.X0 = take(32 * m.ldx);
    const int tile_layers = p.kind == CS_VN_SARL ? p.c0[3] : p.n_layers;
    const int base = o;
    for (int l = 0; l < p.n_layers; ++l) {
        if (l == tile_layers) o = base;                  // mlp3 over the tile's activations
        m.ld[l] = ld8(p.L[l].N);
        m.act[l] = take(32 * m.ld[l]);
        widest = p.L[l].N > widest ? p.L[l].N : widest;
        if (l > 0) widest = p.L[l].K1 > widest ? p.L[l].K1 : widest;      // (the input layer's K is no buffer's width: no dX is formed for it)
    }
    int end = o;
    o = base;
    for (int l = 0; l < tile_layers; ++l) take(32 * m.ld[l]);
    o = o > end ? o : end;
    m.D0 = take(32 * ld8(widest));
    m.D1 = take(32 * ld8(widest));
    if (p.kind == CS_VN_SARL) {
        const int ld_m1 = ld8(p.m1w);
        // dH and J share their floats: J lives in steps (1) and (2) -- mlp3's backward is its last reader --, dH in step (3), whose tile
        // visits touch neither the self state nor the weighted feature; the next job zeroes J again.  (The 7.5 KiB are what lets the
        // reference's widths with a 68-float input tile fit the 160 KiB.)
        m.dH = take(32 * (ld_m1 > p.ld_j ? ld_m1 : p.ld_j));
        m.J = m.dH;
        m.G = n == 1 ? m.act[p.c0[1] - 1] : take((n <= 32 ? 32 / n : 1) * ld_m1);      // one human: the mean of mlp1 over the group IS its row
        m.dG = take(ld_m1);                              // the mean's gradient of a group in chunks, summed over its chunks
        m.dJ = take(32 * p.ld_j);
    }
    m.sc = take(32); m.dw = take(32); m.den = take(32); m.val = take(32); m.grp = take(32);
    m.total = o;
    return m;
}

// 32 rows of a minibatch into the input tile X0 (stride ldx): row r is the K consecutive floats at src + r * pitch -- the rotated columns and
// behind them the map columns, as policy.transform stores a row --, zeros up to kpad (K rounded up to 8) and in the rows from `rows` on.  A
// row's loads are consecutive floats: 16 lanes a row for the rows of 13 | 15 columns, a wavefront a row for the wide ones.
__device__ __forceinline__ void load_rows32(float* X0, int ldx, int kpad, const float* __restrict__ src, long pitch, int rows, int K)
{
    const int sh = kpad <= 16 ? 4 : 6, c0 = threadIdx.x & ((1 << sh) - 1);
#pragma unroll 1
    for (int r = threadIdx.x >> sh; r < 32; r += NT >> sh) {
        const bool live = r < rows;
        const float* from = src + (long)r * pitch;
        float* to = X0 + r * ldx;
#pragma unroll 1
        for (int c = c0; c < kpad; c += 1 << sh) to[c] = (live && c < K) ? from[c] : 0.0f;
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
        for (int i = tid; i < tg * SELF_DIM; i += NT) b.J[(t0 + i / SELF_DIM) * p.ld_j + i % SELF_DIM] = b.X0[(i / SELF_DIM) * per * tile_ldx(m) + i % SELF_DIM];
    chain_fwd(p, m, b, wb, p.c0[0], p.c0[1], b.X0, tile_ldx(m), nullptr, 0);
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
    chain_bwd(p, m, b, params, o, g, p.c0[0], p.c0[1], b.dH, b.X0, tile_ldx(m), nullptr, 0, nullptr, 0, false, nullptr, 0);
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
    const int tid = threadIdx.x;
    const bool sarl = p.kind == CS_VN_SARL;
    float* g = scratch + (long)blockIdx.x * region;

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
            const int K = p.L[0].K1;        // a row: the rotated columns, then the map columns
            load_rows32(b.X0, tile_ldx(m), tile_ldx(m) - 4, rows_in + ((long)(gbase + t0) * n + ch * 32) * K, K, tg * per, K);
            for (int r = tid; r < 32; r += NT) b.grp[r] = r < tg * per ? r / per : 0;
            __syncthreads();
        };
        auto chunk_rows = [&](int ch) { return n - ch * 32 < 32 ? n - ch * 32 : 32; };
        // more humans than a tile holds: a pass over the chunks for the mean of mlp1 (sarl.py:42), a running sum in G's row
        auto mean_pass = [&](int t0) {
            for (int c = tid; c < ld_m1; c += NT) b.G[c] = 0.0f;
            for (int ch = 0; ch < chunks; ++ch) {
                const int per = chunk_rows(ch);
                load(t0, 1, ch, per);
                chain_fwd(p, m, b, wb, p.c0[0], p.c0[1], b.X0, tile_ldx(m), nullptr, 0);
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
            chain_fwd(p, m, b, wb, p.c0[0], p.c0[1], b.X0, tile_ldx(m), nullptr, 0);
        }
        VG_LOSS_HEAD(m, )
        if (!sarl) {
            chain_bwd(p, m, b, params, o, g, p.c0[0], p.c0[1], b.D0, b.X0, tile_ldx(m), nullptr, 0, nullptr, 0, false, nullptr, 0);
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
                    chain_fwd(p, m, b, wb, p.c0[0], p.c0[1], b.X0, tile_ldx(m), nullptr, 0);
                    for (int i = tid; i < 32 * ld_m1; i += NT) {
                        const int r = i / ld_m1, c = i - r * ld_m1;
                        b.dH[i] = (r < per && c < p.m1w && M1[i] > 0.0f) ? b.dG[c] / (float)n : 0.0f;
                    }
                    __syncthreads();
                    chain_bwd(p, m, b, params, o, g, p.c0[0], p.c0[1], b.dH, b.X0, tile_ldx(m), nullptr, 0, nullptr, 0, false, nullptr, 0);
                }
        }
    }
    if (tid == 0) g[o.total] = loss;
}

// blob float i from the flat parameters: pack_layer_f32's map, read backwards
__global__ void k_vn_pack(VnPlan p, GradOffsets o, const float* __restrict__ params, float* __restrict__ blob)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.total_floats) return;
    int l = 0;
    while (l + 1 < p.n_layers && i >= p.L[l + 1].w_off) ++l;
    blob[i] = unpack_layer_at(p.L[l], i, params + o.w[l], params + o.b[l]);
}

// The feed-forward family as value_net_grad.h's host templates ask it (GradCall: the call; om_cols: the map columns behind the rotated ones in
// a stored row, 0 for the rows of 13 | 15 columns)
struct FeedForwardGrad {
    struct Launch {
        VnPlan p; GradOffsets o; GradLds m; int grid, region, jrows; size_t shmem;
        size_t blob_floats() const { return (size_t)p.total_floats; }
    };
    static constexpr const char *pack_entry = "cs_value_net_pack", *sizes_entry = "cs_value_net_grad_sizes";

    static int describe(const GradCall& c, Launch& q)
    {
        if (c.om && c.om_cols < 1) return fail(CS_ERR_ARG, "om_cols must be at least 1");      // the *_om entries' own check, made first
        const int rc = build_plan(c.kind, c.dims, c.n_dims, c.cols, c.om_cols, q.p);
        if (rc == CS_OK) q.o = param_offsets(q.p);
        return rc;
    }

    static int check_n(const GradCall& c)
    {
        return c.kind == CS_VN_CADRL && c.n != 1 ? fail(CS_ERR_ARG, "CADRL's trainer stores one human's row per sample: n must be 1") : CS_OK;
    }

    static int plan(const GradCall& c, Launch& q)
    {
        q.m = grad_lds_map(q.p, c.n);
        q.shmem = (size_t)q.m.total * sizeof(float);
        if (q.shmem > 160 * 1024)
            return fail(CS_ERR_ARG, "the activations and gradients of a tile of this network (rows of " + std::to_string(c.cols) + " + " +
                                        std::to_string(c.om_cols) + " columns: " + std::to_string(q.shmem) + " bytes) do not fit the 160 KiB of LDS");
        // groups per job: whole tiles, as few as spread the minibatch over the workgroups, at most mlp3's block of 32 rows
        const int gpt = c.n <= 32 ? 32 / c.n : 1;
        const int want = up((c.B + GRAD_MAX_GROUPS - 1) / GRAD_MAX_GROUPS, gpt);
        q.jrows = want < JROWS ? want : JROWS;
        const int jobs = (c.B + q.jrows - 1) / q.jrows;
        q.grid = jobs < GRAD_MAX_GROUPS ? jobs : GRAD_MAX_GROUPS;
        q.region = up(q.o.total + 1, 4);
        return CS_OK;
    }

    // the job kernel: every workgroup's partial gradient and loss term into its region of the scratch
    static int launch_jobs(const Launch& q, const GradCall& c)
    {
        const int rc = grant_lds<k_vn_grad>(q.shmem);
        if (rc != CS_OK) return rc;
        hipLaunchKernelGGL(k_vn_grad, dim3(q.grid), dim3(NT), q.shmem, (hipStream_t)c.stream, q.p, q.m, q.o, c.d_weights, c.d_params, c.B, c.n, q.jrows,
                           c.d_rows, c.d_targets, c.d_scratch, q.region, c.d_values);
        HIP_TRY(hipGetLastError());
        return CS_OK;
    }

    // k_vn_sgd's map of the feed-forward blob: every parameter has a blob float of its own
    struct SgdMap {
        VnPlan p;
        GradOffsets o;
        __host__ __device__ int operator()(int i, int& twin) const
        {
            twin = -1;
            int l = 0;
            while (l + 1 < p.n_layers && i >= o.w[l + 1]) ++l;
            return blob_layer_at(p.L[l], i - o.w[l]);
        }
    };
    static SgdMap sgd_map(const Launch& q) { return SgdMap{q.p, q.o}; }

    static void launch_pack(const Launch& q, const GradCall& c)
    {
        hipLaunchKernelGGL(k_vn_pack, dim3((q.p.total_floats + 255) / 256), dim3(256), 0, (hipStream_t)c.stream, q.p, q.o, c.d_params, c.d_weights);
    }
};

} // namespace

// ---- the rows of 13 | 15 columns: no map columns
extern "C" int cs_value_net_grad_sizes(int kind, const int32_t* dims, int n_dims, int cols, int B, int n, size_t* n_param_floats,
                                       size_t* n_scratch_floats)
{
    const GradCall c = describe_call(kind, dims, n_dims, cols, false, 0, B, n);
    return grad_sizes<FeedForwardGrad>(c, n_param_floats, n_scratch_floats);
}

extern "C" int cs_value_net_loss_grad(int kind, const int32_t* dims, int n_dims, const float* d_weights, size_t n_weight_floats, const float* d_params,
                                      size_t n_param_floats, int B, int n, int cols, const float* d_rows, const float* d_targets, float* d_grad,
                                      float* d_loss, float* d_values, float* d_scratch, size_t n_scratch_floats, void* stream)
{
    GradCall c = describe_call(kind, dims, n_dims, cols, false, 0, B, n);
    set_minibatch(c, d_weights, n_weight_floats, d_params, n_param_floats, d_rows, d_targets, d_grad, d_loss, d_values, d_scratch, n_scratch_floats, stream);
    return loss_grad<FeedForwardGrad>(c);
}

extern "C" int cs_value_net_train_step(int kind, const int32_t* dims, int n_dims, float* d_weights, size_t n_weight_floats, float* d_params,
                                       size_t n_param_floats, float* d_momentum, size_t n_momentum_floats, float lr, float momentum, int B, int n,
                                       int cols, const float* d_rows, const float* d_targets, float* d_grad, float* d_loss, double* d_loss_sum,
                                       float* d_values, float* d_scratch, size_t n_scratch_floats, void* stream)
{
    GradCall c = describe_call(kind, dims, n_dims, cols, false, 0, B, n);
    set_minibatch(c, d_weights, n_weight_floats, d_params, n_param_floats, d_rows, d_targets, d_grad, d_loss, d_values, d_scratch, n_scratch_floats, stream);
    set_sgd(c, d_momentum, n_momentum_floats, lr, momentum, d_loss_sum);
    return train_step<FeedForwardGrad>(c);
}

extern "C" int cs_value_net_blob_index(int kind, const int32_t* dims, int n_dims, int cols, int32_t* index, size_t n_param_floats)
{
    return blob_index<FeedForwardGrad>(describe_call(kind, dims, n_dims, cols, false, 0), index, n_param_floats);
}

extern "C" int cs_value_net_pack_device(int kind, const int32_t* dims, int n_dims, int cols, const float* d_params, size_t n_param_floats,
                                        float* d_blob, size_t n_blob_floats, void* stream)
{
    GradCall c = describe_call(kind, dims, n_dims, cols, false, 0);
    set_pack(c, d_params, n_param_floats, d_blob, n_blob_floats, stream);
    return pack_device<FeedForwardGrad>(c);
}

// ---- OM-SARL: rows of cols + om_cols columns (FeedForwardGrad::describe refuses om_cols < 1 before anything else)
extern "C" int cs_value_net_grad_sizes_om(int kind, const int32_t* dims, int n_dims, int cols, int om_cols, int B, int n, size_t* n_param_floats,
                                          size_t* n_scratch_floats)
{
    const GradCall c = describe_call(kind, dims, n_dims, cols, true, om_cols, B, n);
    return grad_sizes<FeedForwardGrad>(c, n_param_floats, n_scratch_floats);
}

extern "C" int cs_value_net_loss_grad_om(int kind, const int32_t* dims, int n_dims, const float* d_weights, size_t n_weight_floats,
                                         const float* d_params, size_t n_param_floats, int B, int n, int cols, int om_cols, const float* d_rows,
                                         const float* d_targets, float* d_grad, float* d_loss, float* d_values, float* d_scratch,
                                         size_t n_scratch_floats, void* stream)
{
    GradCall c = describe_call(kind, dims, n_dims, cols, true, om_cols, B, n);
    set_minibatch(c, d_weights, n_weight_floats, d_params, n_param_floats, d_rows, d_targets, d_grad, d_loss, d_values, d_scratch, n_scratch_floats, stream);
    return loss_grad<FeedForwardGrad>(c);
}

extern "C" int cs_value_net_train_step_om(int kind, const int32_t* dims, int n_dims, float* d_weights, size_t n_weight_floats, float* d_params,
                                          size_t n_param_floats, float* d_momentum, size_t n_momentum_floats, float lr, float momentum, int B, int n,
                                          int cols, int om_cols, const float* d_rows, const float* d_targets, float* d_grad, float* d_loss,
                                          double* d_loss_sum, float* d_values, float* d_scratch, size_t n_scratch_floats, void* stream)
{
    GradCall c = describe_call(kind, dims, n_dims, cols, true, om_cols, B, n);
    set_minibatch(c, d_weights, n_weight_floats, d_params, n_param_floats, d_rows, d_targets, d_grad, d_loss, d_values, d_scratch, n_scratch_floats, stream);
    set_sgd(c, d_momentum, n_momentum_floats, lr, momentum, d_loss_sum);
    return train_step<FeedForwardGrad>(c);
}

extern "C" int cs_value_net_blob_index_om(int kind, const int32_t* dims, int n_dims, int cols, int om_cols, int32_t* index, size_t n_param_floats)
{
    return blob_index<FeedForwardGrad>(describe_call(kind, dims, n_dims, cols, true, om_cols), index, n_param_floats);
}

extern "C" int cs_value_net_pack_om_device(int kind, const int32_t* dims, int n_dims, int cols, int om_cols, const float* d_params,
                                           size_t n_param_floats, float* d_blob, size_t n_blob_floats, void* stream)
{
    GradCall c = describe_call(kind, dims, n_dims, cols, true, om_cols);
    set_pack(c, d_params, n_param_floats, d_blob, n_blob_floats, stream);
    return pack_device<FeedForwardGrad>(c);
}
