// value_net.hip -- the value-network decision of the trained CrowdNav robots, batched and fused: CADRL and SARL decide for W worlds.
// Replaces the per-action model() loop, compute_action_value and the arg-max of
//   crowd_nav/policy/cadrl.py:264-273 (value_network MLP on every (action, human) row, minimum over the humans),
//   crowd_nav/policy/multi_human_rl.py:52-63 with crowd_nav/policy/sarl.py:28-65 (mlp1 -> mlp2, attention, masked softmax, mlp3)
// and reach_destination (cadrl.py:244), reading cs_lookahead's output (rotated [W][A][n][13|15], rewards [W][A]).
//
// Shape of the work.  A "group" is one (world, action): n rows of the rotated array, one scalar value.  A workgroup (4 wavefronts) takes
// 32 consecutive groups.  It walks them in tiles of M = 32 rows (whole groups while n <= M, otherwise one group in chunks of
// M humans), and every layer of a tile is a [M x K] x [K x N] product on v_mfma_f32_32x32x2_f32: the activations of the tile sit in LDS
// (row-major, row stride = width + 4 floats: 16-byte aligned rows whose ds_read_b128 of 8 consecutive rows cover the 32 banks), one
// wavefront owns one 32 x 32 output block at a time, its A operand comes from LDS and its B operand straight from the packed weight
// blob (read-only, shared by every workgroup: L2).  No activation leaves the CU: the tile's input rows come in, one float per group
// goes out.  SARL's mlp3 runs once per workgroup on the 32 joint rows (self state, attention-weighted feature) of its groups, as a
// full 32-row block.  A second, tiny kernel takes the arg-max of the A values of every world (first maximum, as np.argmax), applies the
// caller's override column and the goal test, and writes the ActionXY row.
//
// Numerics: float32 throughout.  One MFMA sums k = {kg*8 + s, kg*8 + 4 + s} (s = 0..3) for the k-group kg, the groups follow in order,
// the accumulator starts from the bias: every output element is one fixed fmaf chain that depends on the layer's widths alone.  The
// reductions over the humans of a group (minimum; mean; softmax denominator; weighted sum) are sequential in human order by one lane
// per (group, column).  So a (world, action) gives the same bits alone (W = 1) and inside a batch of 4096, wherever its rows fall in a
// tile.  No atomics.  gfx950 only.
#include <hip/hip_runtime.h>

#include <atomic>
#include <climits>
#include <cmath>
#include <cstring>

#include "common.h"

namespace {

using csimpl::fail;

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int NT = 256;            // 4 wavefronts
constexpr int TILE_M = 32;         // rows of a tile: one 32-row MFMA block (a 64-row tile measured 15 - 40 % slower: one workgroup per CU)
constexpr int JROWS = 32;          // groups per workgroup = rows of the mlp3 block
constexpr int VN_MAX_LAYERS = 16;
constexpr int VN_MAX_WIDTH = 256;
constexpr int SELF_DIM = 6;        // sarl.py self_state_dim: dg, v_pref, theta, radius, vx, vy
constexpr int LDX = 20;            // row stride of the input tile (13 or 15 columns padded to 16)

struct VnLayer {
    int K1, K2, N;                 // input columns from the first / second source, output columns
    int kg_split, kg_total;        // k-groups of 8 from the first source; in all
    int ncb;                       // 32-column output blocks
    int relu;
    int w_off, b_off;              // floats into the blob: [ncb][kg_total][64 lanes][4], then [ncb * 32] biases
};

struct VnPlan {
    int kind, cols, with_global, n_layers;
    int c0[5];                     // CADRL: c0[0..1] = value_network; SARL: mlp1, mlp2, attention, mlp3 = [c0[i], c0[i + 1])
    VnLayer L[VN_MAX_LAYERS];
    int feat;                      // width of mlp2's output
    int m1w;                       // width of mlp1's output
    int ld_m1, ld_pq, ld_j;        // LDS row strides
    int total_floats;
};

inline int up(int x, int m) { return (x + m - 1) / m * m; }

// the layer table of a network description (include/crowdstep.h cs_value_net_decide: `dims`); CS_OK or the fail() status
int build_plan(int kind, const int32_t* dims, int n_dims, int cols, VnPlan& p)
{
    memset(&p, 0, sizeof p);
    if (kind != CS_VN_CADRL && kind != CS_VN_SARL) return fail(CS_ERR_ARG, "unknown value network kind (CS_VN_CADRL, CS_VN_SARL)");
    if (cols != 13 && cols != 15) return fail(CS_ERR_ARG, "rotated rows have 13 or 15 columns");
    if (!dims || n_dims < 2) return fail(CS_ERR_ARG, "null or empty layer description");
    p.kind = kind;
    p.cols = cols;
    int at = 0;
    const int n_chains = kind == CS_VN_CADRL ? 1 : 4;
    if (kind == CS_VN_SARL) p.with_global = dims[at++] ? 1 : 0;
    int off = 0;
    for (int c = 0; c < n_chains; ++c) {
        if (at >= n_dims) return fail(CS_ERR_ARG, "layer description ends early");
        const int nl = dims[at++];
        if (nl < 1 || at + nl > n_dims) return fail(CS_ERR_ARG, "a chain needs at least one layer and its widths");
        if (p.n_layers + nl > VN_MAX_LAYERS) return fail(CS_ERR_ARG, "at most 16 layers in all");
        p.c0[c] = p.n_layers;
        // what the chain reads (sarl.py:15-25): mlp1 the rotated row; mlp2 mlp1's output; attention (mlp1, mean of mlp1) or mlp1; mlp3 (self state, feature)
        int k1 = cols, k2 = 0;
        if (c == 1) k1 = p.m1w;
        if (c == 2) { k1 = p.m1w; k2 = p.with_global ? p.m1w : 0; }
        if (c == 3) k1 = SELF_DIM + p.feat;
        for (int i = 0; i < nl; ++i) {
            const int wdt = dims[at++];
            if (wdt < 1 || wdt > VN_MAX_WIDTH) return fail(CS_ERR_ARG, "layer widths must be between 1 and 256");
            VnLayer& l = p.L[p.n_layers++];
            l.K1 = k1; l.K2 = k2; l.N = wdt;
            l.kg_split = up(k1, 8) / 8;
            l.kg_total = l.kg_split + up(k2, 8) / 8;
            l.ncb = up(wdt, 32) / 32;
            l.relu = (i != nl - 1 || (kind == CS_VN_SARL && c == 0)) ? 1 : 0;     // cadrl.py mlp(): last_relu only for mlp1
            l.w_off = off;
            off += l.ncb * l.kg_total * 64 * 4;
            l.b_off = off;
            off += l.ncb * 32;
            k1 = wdt; k2 = 0;
        }
        const int last = p.L[p.n_layers - 1].N;
        if (c == 0 && kind == CS_VN_SARL) p.m1w = last;
        if (c == 1) p.feat = last;
        if ((kind == CS_VN_CADRL || c >= 2) && last != 1) return fail(CS_ERR_ARG, "value_network, attention and mlp3 end in one output");
    }
    p.c0[n_chains] = p.n_layers;
    if (at != n_dims) return fail(CS_ERR_ARG, "layer description has trailing entries");
    int widest = 32;
    for (int i = 0; i < p.n_layers; ++i) widest = p.L[i].ncb * 32 > widest ? p.L[i].ncb * 32 : widest;
    p.ld_pq = widest + 4;
    p.ld_m1 = up(p.m1w > 0 ? p.m1w : 1, 32) + 4;
    p.ld_j = up(SELF_DIM + p.feat, 8) + 4;
    p.total_floats = off;
    return CS_OK;
}

// LDS map of a launch (floats from the start of the dynamic block)
struct VnLds { int X0, M1, P, Q, G, J, sc, den, val, self, grp, total; };

VnLds lds_map(const VnPlan& p, int M, int n)
{
    VnLds m{};
    int o = 0;
    auto take = [&](int floats) { const int at = o; o += up(floats, 4); return at; };
    m.X0 = take(M * LDX);
    m.P = take(M * p.ld_pq);
    m.Q = take(M * p.ld_pq);
    if (p.kind == CS_VN_SARL) {
        const int gpt = n <= M ? M / n : 1;
        m.M1 = take(M * p.ld_m1);
        m.G = n == 1 ? m.M1 : take(gpt * p.ld_m1);     // one human: the mean of mlp1 over the group IS its row (x / 1, exactly)
        m.J = take(JROWS * p.ld_j);
    }
    m.sc = take(M);
    m.den = take(JROWS);
    m.val = take(JROWS);
    m.grp = take(M);
    m.total = o;
    return m;
}

// One layer of a tile: dst[rows][ncb * 32] = act(src[rows][K] x Wt + b) for `rbs` row blocks of 32.  The A operand of row r comes from
// src (k-groups below kg_split) and then from src2[grp[r]] (the per-group second source: SARL's mean of mlp1); columns beyond N are
// stored as 0 whatever the inputs (their zero weights and bias give 0 only for finite inputs: 0 * inf is a NaN, which the next layer's
// zero weights would hand on where torch returns +-inf), so the next layer may read its K rounded up to 8.
__device__ __forceinline__ void layer_fwd(const VnLayer& L, const float* __restrict__ wb, const float* src, int lds_, const float* src2, int lds2,
                                          const int* grp, int rbs, float* dst, int ldd, int rot)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, li = lane & 31;
    const int items = rbs * L.ncb;
    const int KG = L.kg_total, split = L.kg_split;
    for (int it = (wave + rot) & 3; it < items; it += 4) {
        const int rb = it % rbs, cb = it / rbs;
        const int row = rb * 32 + li;
        const float* a1 = src + row * lds_ + 4 * h;
        const float* a2 = src2 ? src2 + grp[row] * lds2 + 4 * h : a1;
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
#define VN_STEP(U, B)                                                                                                        \
    if (kg0 + U < KG) {                                                                                                      \
        const int kg = kg0 + U;                                                                                              \
        const float4 a = *reinterpret_cast<const float4*>(kg < split ? a1 + kg * 8 : a2 + (kg - split) * 8);                 \
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, B.x, acc, 0, 0, 0);                                                  \
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, B.y, acc, 0, 0, 0);                                                  \
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, B.z, acc, 0, 0, 0);                                                  \
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, B.w, acc, 0, 0, 0);                                                  \
    }
            VN_STEP(0, b0)
            VN_STEP(1, b1)
            VN_STEP(2, b2)
            VN_STEP(3, b3)
#undef VN_STEP
        }
        // C/D map of the 32x32 forms: column = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
        float* d = dst + (rb * 32 + 4 * h) * ldd + cb * 32 + li;
        const bool pad = cb * 32 + li >= L.N;          // (the zero weights give 0 * inf = NaN there when an input is infinite)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = acc[r];
            if (L.relu) v = v < 0.0f ? 0.0f : v;      // (a NaN stays a NaN, as torch's ReLU leaves it)
            d[((r & 3) + 8 * (r >> 2)) * ldd] = pad ? 0.0f : v;
        }
    }
}

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
        layer_fwd(p.L[l], wb, cur, cur_ld, l == first ? src2 : nullptr, lds2, b.grp, rbs, dst, ldd, l + (int)blockIdx.x);
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

__global__ __launch_bounds__(NT) void k_value_net(VnPlan p, VnLds m, int M, const float* __restrict__ wb, int NG, int A, int n,
                                                  const float* __restrict__ rotated, const float* __restrict__ rewards,
                                                  const float* __restrict__ robot, int rstride, float gamma, float dt, float* __restrict__ values)
{
    extern __shared__ float lds[];
    VnBufs b;
    b.X0 = lds + m.X0; b.M1 = lds + m.M1; b.P = lds + m.P; b.Q = lds + m.Q; b.G = lds + m.G; b.J = lds + m.J;
    b.sc = lds + m.sc; b.den = lds + m.den; b.val = lds + m.val; b.grp = reinterpret_cast<int*>(lds + m.grp);
    const int tid = threadIdx.x;
    const int rbs = M / 32, cols = p.cols;
    const bool sarl = p.kind == CS_VN_SARL;
    const int chunks = n <= M ? 1 : (n + M - 1) / M;
    const int gpt = n <= M ? M / n : 1;
    const int m1pad = (p.m1w + 7) & ~7;
    int out_ld;

    for (int job = blockIdx.x; job * JROWS < NG; job += gridDim.x) {
        const int gbase = job * JROWS;
        const int ng = NG - gbase < JROWS ? NG - gbase : JROWS;
        if (sarl) {
            for (int i = tid; i < JROWS * p.ld_j; i += NT) b.J[i] = 0.0f;
            if (tid < JROWS) b.den[tid] = 0.0f;
        } else if (tid < JROWS) b.val[tid] = INFINITY;
        __syncthreads();

        for (int t0 = 0; t0 < ng; t0 += gpt) {
            const int tg = ng - t0 < gpt ? ng - t0 : gpt;
            const float* grows = rotated + (long)(gbase + t0) * n * cols;
            if (sarl && chunks > 1) {
                // more humans than a tile holds: a first pass over the chunks for the mean of mlp1 (sarl.py:42), kept as a running sum in G
                for (int c = tid; c < p.ld_m1; c += NT) b.G[c] = 0.0f;
                for (int ch = 0; ch < chunks; ++ch) {
                    const int rows = n - ch * M < M ? n - ch * M : M;
                    load_tile(b, grows + (long)ch * M * cols, rows, cols, n, M);
                    __syncthreads();
                    run_chain(p, wb, b, p.c0[0], p.c0[1], b.X0, LDX, nullptr, 0, rbs, b.M1, p.ld_m1, out_ld);
                    for (int c = tid; c < m1pad; c += NT) {
                        float s = b.G[c];
                        for (int r = 0; r < rows; ++r) s += b.M1[r * p.ld_m1 + c];
                        b.G[c] = s;
                    }
                    __syncthreads();
                }
                for (int c = tid; c < m1pad; c += NT) b.G[c] = b.G[c] / (float)n;
                __syncthreads();
            }
            // phase 0: a tile holds its groups whole -- denominator, weights and weighted sum in one visit.  A group in chunks needs the
            // softmax denominator of ALL its humans before the first weight (sarl.py:52-53): phase 1 sums it, phase 2 recomputes and weighs.
            for (int phase = chunks > 1 ? 1 : 0; phase <= (chunks > 1 ? 2 : 0); ++phase)
            for (int ch = 0; ch < chunks; ++ch) {
                const int per = chunks > 1 ? (n - ch * M < M ? n - ch * M : M) : n;      // humans of each group in this tile
                const int rows = chunks > 1 ? per : tg * n;
                load_tile(b, grows + (long)ch * M * cols, rows, cols, per, M);
                __syncthreads();
                if (!sarl) {
                    if (phase == 1) continue;
                    const float* out = run_chain(p, wb, b, p.c0[0], p.c0[1], b.X0, LDX, nullptr, 0, rbs, nullptr, 0, out_ld);
                    if (tid < tg) {         // cadrl.py:269: the minimum over the humans
                        float v = b.val[t0 + tid];
                        for (int j = 0; j < per; ++j) {      // (torch.min's order: a NaN stays)
                            const float x = out[(tid * per + j) * out_ld];
                            v = (x < v || x != x) ? x : v;
                        }
                        b.val[t0 + tid] = v;
                    }
                    __syncthreads();
                    continue;
                }
                if (ch == 0)                // sarl.py:36: the self state is read from the first human's row
                    for (int i = tid; i < tg * SELF_DIM; i += NT) b.J[(t0 + i / SELF_DIM) * p.ld_j + i % SELF_DIM] = b.X0[(i / SELF_DIM) * per * LDX + i % SELF_DIM];
                run_chain(p, wb, b, p.c0[0], p.c0[1], b.X0, LDX, nullptr, 0, rbs, b.M1, p.ld_m1, out_ld);
                if (p.with_global && chunks == 1 && n > 1) {
                    for (int i = tid; i < tg * m1pad; i += NT) {
                        const int k = i / m1pad, c = i - k * m1pad;
                        float s = 0.0f;
                        for (int j = 0; j < n; ++j) s += b.M1[(k * n + j) * p.ld_m1 + c];
                        b.G[k * p.ld_m1 + c] = s / (float)n;
                    }
                    __syncthreads();
                }
                {   // attention scores and the masked softmax's terms exp(s) * (s != 0) (sarl.py:48-52)
                    const float* out = run_chain(p, wb, b, p.c0[2], p.c0[3], b.M1, p.ld_m1, p.with_global ? b.G : nullptr, p.ld_m1, rbs, nullptr, 0, out_ld);
                    for (int r = tid; r < M; r += NT) {
                        const float s = out[r * out_ld];
                        b.sc[r] = (r < rows && s != 0.0f) ? expf(s) : 0.0f;
                    }
                    __syncthreads();
                }
                if (phase != 2) {           // the denominator, in human order
                    if (tid < tg) {
                        float s = b.den[t0 + tid];
                        for (int j = 0; j < per; ++j) s += b.sc[tid * per + j];
                        b.den[t0 + tid] = s;
                    }
                    __syncthreads();
                    if (phase == 1) continue;
                }
                for (int r = tid; r < rows; r += NT) b.sc[r] = b.sc[r] / b.den[t0 + r / per];
                __syncthreads();
                {   // mlp2 and the weighted sum of its rows (sarl.py:57-60)
                    const float* f = run_chain(p, wb, b, p.c0[1], p.c0[2], b.M1, p.ld_m1, nullptr, 0, rbs, nullptr, 0, out_ld);
                    const int fw = p.feat;
                    for (int i = tid; i < tg * fw; i += NT) {
                        const int k = i / fw, c = i - k * fw;
                        float s = b.J[(t0 + k) * p.ld_j + SELF_DIM + c];
                        for (int j = 0; j < per; ++j) s = fmaf(b.sc[k * per + j], f[(k * per + j) * out_ld + c], s);
                        b.J[(t0 + k) * p.ld_j + SELF_DIM + c] = s;
                    }
                    __syncthreads();
                }
            }
        }

        if (sarl) {
            const float* out = run_chain(p, wb, b, p.c0[3], p.c0[4], b.J, p.ld_j, nullptr, 0, 1, nullptr, 0, out_ld);
            if (tid < ng) b.val[tid] = out[tid * out_ld];
            __syncthreads();
        }
        if (tid < ng) {                     // cadrl.py:85-90 compute_action_value
            const int g = gbase + tid;
            const float vpref = robot[(long)(g / A) * rstride + 7];
            values[g] = rewards[g] + powf(gamma, dt * vpref) * b.val[tid];
        }
        __syncthreads();
    }
}

// one wavefront per world: first maximum of its A values (np.argmax), the override column, the goal test (cadrl.py:244), the ActionXY row
__global__ __launch_bounds__(256) void k_value_pick(int W, int A, const float* __restrict__ values, const float* __restrict__ actions,
                                                    const float* __restrict__ robot, int rstride, const int32_t* __restrict__ override_,
                                                    int32_t* __restrict__ choice, float* __restrict__ action_out)
{
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= W) return;
    // np.argmax's order: a NaN (a network that overflowed) counts as the maximum, the first one wins; otherwise the first largest value
    auto better = [](float v, int i, float bv, int bi) {
        if (v != v) return !(bv != bv) || i < bi;
        if (bv != bv) return false;
        return v > bv || (v == bv && i < bi);
    };
    float bv = -INFINITY;
    int bi = INT_MAX;
    for (int a = lane; a < A; a += 64) {
        const float v = values[(long)w * A + a];
        if (better(v, a, bv, bi)) { bv = v; bi = a; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane != 0) return;
    if (bi == INT_MAX) bi = 0;
    if (override_) {
        const int o = override_[w];
        if (o >= 0 && o < A) bi = o;
    }
    const float* rb = robot + (long)w * rstride;
    const float dx = rb[0] - rb[5], dy = rb[1] - rb[6];
    const bool there = sqrtf(dy * dy + dx * dx) < rb[4];
    if (choice) choice[w] = bi;
    action_out[2 * w] = there ? 0.0f : actions[2 * bi];
    action_out[2 * w + 1] = there ? 0.0f : actions[2 * bi + 1];
}

} // namespace

extern "C" int cs_value_net_pack(int kind, const int32_t* dims, int n_dims, int cols, const float* const* params, float* blob, size_t* n_floats)
{
    VnPlan p;
    const int rc = build_plan(kind, dims, n_dims, cols, p);
    if (rc != CS_OK) return rc;
    if (!n_floats) return fail(CS_ERR_ARG, "null argument");
    *n_floats = (size_t)p.total_floats;
    if (!blob) return CS_OK;
    if (!params) return fail(CS_ERR_ARG, "null argument");
    for (int l = 0; l < p.n_layers; ++l)
        if (!params[2 * l] || !params[2 * l + 1]) return fail(CS_ERR_ARG, "null weight or bias array");
    memset(blob, 0, (size_t)p.total_floats * sizeof(float));
    for (int l = 0; l < p.n_layers; ++l) {
        const VnLayer& L = p.L[l];
        const float* wgt = params[2 * l];       // torch.nn.Linear.weight: [N][K1 + K2]
        const float* bias = params[2 * l + 1];
        const int K = L.K1 + L.K2;
        for (int cb = 0; cb < L.ncb; ++cb)
            for (int kg = 0; kg < L.kg_total; ++kg)
                for (int lane = 0; lane < 64; ++lane)
                    for (int s = 0; s < 4; ++s) {
                        const int j = cb * 32 + (lane & 31);
                        const int kk = kg * 8 + 4 * (lane >> 5) + s;
                        int k = -1;
                        if (kg < L.kg_split) { if (kk < L.K1) k = kk; }
                        else if (kk - L.kg_split * 8 < L.K2) k = L.K1 + kk - L.kg_split * 8;
                        if (j < L.N && k >= 0) blob[L.w_off + ((cb * L.kg_total + kg) * 64 + lane) * 4 + s] = wgt[(size_t)j * K + k];
                    }
        for (int j = 0; j < L.N; ++j) blob[L.b_off + j] = bias[j];
    }
    return CS_OK;
}

extern "C" int cs_value_net_decide(int kind, const int32_t* dims, int n_dims, const float* d_weights, size_t n_weight_floats, int W, int A, int n,
                                   int cols, const float* d_rotated, const float* d_rewards, const float* d_actions, const float* d_robot,
                                   int robot_stride, float gamma, float dt, const int32_t* d_override, float* d_values, int32_t* d_choice,
                                   float* d_action_out, void* stream)
{
    VnPlan p;
    const int rc = build_plan(kind, dims, n_dims, cols, p);
    if (rc != CS_OK) return rc;
    if (W < 1 || A < 1) return fail(CS_ERR_ARG, "W and A must be positive");
    if (n < 1) return fail(CS_ERR_ARG, "n must be at least 1: a value network needs a human to look at");
    if ((long)W * A > INT_MAX / 2 || (long)W * A * n > (1L << 40)) return fail(CS_ERR_ARG, "W * A * n is too large");
    if (!d_weights || !d_rotated || !d_rewards || !d_actions || !d_robot || !d_values || !d_action_out) return fail(CS_ERR_ARG, "null argument");
    if (n_weight_floats != (size_t)p.total_floats) return fail(CS_ERR_ARG, "the weight blob does not have the size of this network (cs_value_net_pack)");
    if (robot_stride < 8) return fail(CS_ERR_ARG, "robot rows need at least 8 columns: px,py,vx,vy,r,gx,gy,v_pref");
    const size_t lds_limit = 160 * 1024;
    const int M = TILE_M;
    const VnLds m = lds_map(p, M, n);
    const size_t shmem = (size_t)m.total * sizeof(float);
    // (cannot happen within the limits above -- 16 layers of up to 256 columns need about 150 KiB at most, at n = 2 -- kept as the guard of the launch)
    if (shmem > lds_limit) return fail(CS_ERR_ARG, "the tile buffers of this network do not fit the 160 KiB of LDS");
    if (shmem > 64 * 1024) {                 // beyond the default dynamic LDS of a kernel: raised per device to the largest size asked for so far
        static std::atomic<int> granted[64];
        int dev = 0;
        HIP_TRY(hipGetDevice(&dev));
        const bool slot = dev >= 0 && dev < 64;
        if (!slot || granted[dev].load(std::memory_order_acquire) < (int)shmem) {
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_value_net), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
            if (slot) granted[dev].store((int)shmem, std::memory_order_release);
        }
    }
    const int NG = W * A;
    const int jobs = (NG + JROWS - 1) / JROWS;
    const int grid = jobs < 4096 ? jobs : 4096;
    hipLaunchKernelGGL(k_value_net, dim3(grid), dim3(NT), shmem, (hipStream_t)stream, p, m, M, d_weights, NG, A, n, d_rotated, d_rewards, d_robot,
                       robot_stride, gamma, dt, d_values);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_value_pick, dim3((W + 3) / 4), dim3(256), 0, (hipStream_t)stream, W, A, d_values, d_actions, d_robot, robot_stride,
                       d_override, d_choice, d_action_out);
    HIP_TRY(hipGetLastError());
    return CS_OK;
}
