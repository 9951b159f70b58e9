// value_net_plan.h -- what the three kernels of the value-network decision share beside their body (value_net_body.inc) and their
// arithmetic (value_net_f32.h: float32, for value_net.hip and value_net_worlds.hip; value_net_bf16_layers.h: the opt-in bf16 layers, whose host pieces are value_net_bf16.h).  Host: the
// layer table of a network description, the argument checks, the LDS map, what the decide entries do before their launch and the pack
// entries before they fill.  Device: the LDS buffers, the chain tags, the tile loader that copies rows and the float32 layer of a tile.
// Everything sits in an unnamed namespace: each translation unit gets its own copy, the kernels keep their names.  The per-world pick and
// its launch are value_net_pick.h.
#pragma once
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
constexpr int LDX = 20;            // row stride of the input tile (13 or 15 columns padded to 16); k_value_net_om has its own

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

// a layer's place in the blob, from its ncb and kg_total: the weights [ncb][kg_total][64 lanes][4 floats] at float `off` (a lane's 8 bf16 of
// a k-step of 16 are as wide), then [ncb * 32] biases; `off` moves behind them
inline void place_layer(VnLayer& l, int& off)
{
    l.w_off = off;
    off += l.ncb * l.kg_total * 64 * 4;
    l.b_off = off;
    off += l.ncb * 32;
}

// one Linear layer of `wdt` outputs behind the table's last: k1 (+ k2) inputs, its weights and biases at float `off` of the blob, which
// moves behind them; CS_OK or the fail() status
inline int add_layer(VnPlan& p, int k1, int k2, int wdt, int relu, int& off)
{
    if (wdt < 1 || wdt > VN_MAX_WIDTH) return fail(CS_ERR_ARG, "layer widths must be between 1 and 256");
    VnLayer& l = p.L[p.n_layers++];
    l.K1 = k1; l.K2 = k2; l.N = wdt;
    l.kg_split = up(k1, 8) / 8;
    l.kg_total = l.kg_split + up(k2, 8) / 8;
    l.ncb = up(wdt, 32) / 32;
    l.relu = relu;
    place_layer(l, off);
    return CS_OK;
}

// the row stride of the P / Q buffers: the widest layer's whole 32-column blocks
inline void set_ld_pq(VnPlan& p)
{
    int widest = 32;
    for (int i = 0; i < p.n_layers; ++i) widest = p.L[i].ncb * 32 > widest ? p.L[i].ncb * 32 : widest;
    p.ld_pq = widest + 4;
}

// the layer table of a network description (include/crowdstep.h cs_value_net_decide: `dims`); CS_OK or the fail() status
// om_cols: the occupancy-map columns behind the rotated ones in the first layer's input (cs_value_net_decide_om; 0: none)
inline int build_plan(int kind, const int32_t* dims, int n_dims, int cols, int om_cols, VnPlan& p)
{
    memset(&p, 0, sizeof p);
    if (kind != CS_VN_CADRL && kind != CS_VN_SARL) return fail(CS_ERR_ARG, "unknown value network kind (CS_VN_CADRL, CS_VN_SARL)");
    if (cols != 13 && cols != 15) return fail(CS_ERR_ARG, "rotated rows have 13 or 15 columns");
    if (om_cols && kind != CS_VN_SARL) return fail(CS_ERR_ARG, "occupancy maps belong to SARL's network");
    if (om_cols < 0) return fail(CS_ERR_ARG, "om_cols must be at least 1");
    if (cols + om_cols > VN_MAX_WIDTH) return fail(CS_ERR_ARG, "rotated and map columns together exceed a layer's 256 inputs");
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
        int k1 = cols + om_cols, k2 = 0;
        if (c == 1) k1 = p.m1w;
        if (c == 2) { k1 = p.m1w; k2 = p.with_global ? p.m1w : 0; }
        if (c == 3) k1 = SELF_DIM + p.feat;
        for (int i = 0; i < nl; ++i) {
            const int wdt = dims[at++];
            const int rc = add_layer(p, k1, k2, wdt, (i != nl - 1 || (kind == CS_VN_SARL && c == 0)) ? 1 : 0, off);     // cadrl.py mlp(): last_relu only for mlp1
            if (rc != CS_OK) return rc;
            k1 = wdt; k2 = 0;
        }
        const int last = p.L[p.n_layers - 1].N;
        if (c == 0 && kind == CS_VN_SARL) p.m1w = last;
        if (c == 1) p.feat = last;
        if ((kind == CS_VN_CADRL || c >= 2) && last != 1) return fail(CS_ERR_ARG, "value_network, attention and mlp3 end in one output");
    }
    p.c0[n_chains] = p.n_layers;
    if (at != n_dims) return fail(CS_ERR_ARG, "layer description has trailing entries");
    set_ld_pq(p);
    p.ld_m1 = up(p.m1w > 0 ? p.m1w : 1, 32) + 4;
    p.ld_j = up(SELF_DIM + p.feat, 8) + 4;
    p.total_floats = off;
    return CS_OK;
}

// the checks of a decision's arguments that follow the layer table, in the order cs_value_net_decide gives them; n_weight_floats is
// the length of the caller's blob in floats
inline int check_decide_args(const VnPlan& p, const void* d_weights, size_t n_weight_floats, int W, int A, int n, const void* d_rotated,
                             const void* d_rewards, const void* d_actions, const void* d_robot, int robot_stride, const void* d_values,
                             const void* d_action_out)
{
    if (W < 1 || A < 1) return fail(CS_ERR_ARG, "W and A must be positive");
    if (n < 1) return fail(CS_ERR_ARG, "n must be at least 1: a value network needs a human to look at");
    if ((long)W * A > INT_MAX / 2 || (long)W * A * n > (1L << 40)) return fail(CS_ERR_ARG, "W * A * n is too large");
    if (!d_weights || !d_rotated || !d_rewards || !d_actions || !d_robot || !d_values || !d_action_out) return fail(CS_ERR_ARG, "null argument");
    if (n_weight_floats != (size_t)p.total_floats) return fail(CS_ERR_ARG, "the weight blob does not have the size of this network (cs_value_net_pack)");
    if (robot_stride < 8) return fail(CS_ERR_ARG, "robot rows need at least 8 columns: px,py,vx,vy,r,gx,gy,v_pref");
    return CS_OK;
}

// one layer's float32 weights and biases where the lanes of layer_fwd read them: wgt = torch.nn.Linear.weight [N][K1 + K2], blob zeroed before
inline void pack_layer_f32(const VnLayer& L, const float* wgt, const float* bias, float* blob)
{
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

// LDS map of a launch (floats from the start of the dynamic block)
struct VnLds { int X0, M1, P, Q, G, J, sc, den, val, self, grp, total; };

// ldx: the input tile's row stride
inline VnLds lds_map(const VnPlan& p, int M, int n, int ldx)
{
    VnLds m{};
    int o = 0;
    auto take = [&](int floats) { const int at = o; o += up(floats, 4); return at; };
    m.X0 = take(M * ldx);
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

// A dynamic LDS block beyond a kernel's default 64 KiB is granted per device, raised to the largest size asked for so far.
template <auto Kernel>
inline int grant_lds(size_t shmem)
{
    if (shmem <= 64 * 1024) return CS_OK;
    static std::atomic<int> granted[64];
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    const bool slot = dev >= 0 && dev < 64;
    if (!slot || granted[dev].load(std::memory_order_acquire) < (int)shmem) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
        if (slot) granted[dev].store((int)shmem, std::memory_order_release);
    }
    return CS_OK;
}

// the groups of a decision and the workgroups of its launch: JROWS groups a job, the jobs strided over at most 4096 workgroups
inline void job_grid(int W, int A, int& NG, int& grid)
{
    NG = W * A;
    const int jobs = (NG + JROWS - 1) / JROWS;
    grid = jobs < 4096 ? jobs : 4096;
}

// What the decide entries do alike before their kernel's launch.  The dynamic block is the map plus `tail_floats` of the kernel's own
// (at float `tail`), granted by grant_lds.
struct VnLaunch { VnLds m; int tail; size_t shmem; int NG, grid; };

template <auto Kernel>
inline int prepare_launch(const VnPlan& p, int n, int tail_floats, int W, int A, VnLaunch& q, int ldx = LDX)
{
    q.m = lds_map(p, TILE_M, n, ldx);
    q.tail = q.m.total;
    q.shmem = (size_t)(q.m.total + tail_floats) * sizeof(float);
    // (the float32 tensor path cannot get here within build_plan's limits -- 16 layers of up to 256 columns need about 150 KiB at most, at n = 2)
    if (q.shmem > 160 * 1024) return fail(CS_ERR_ARG, "the tile buffers of this network do not fit the 160 KiB of LDS");
    const int rc = grant_lds<Kernel>(q.shmem);
    if (rc != CS_OK) return rc;
    job_grid(W, A, q.NG, q.grid);
    return CS_OK;
}

// What the pack entries do alike before they fill the blob: the plan (`replan`: the arithmetic's changes to it, or null), the size query
// through n_units (`units_per_float`: 1 for a blob counted in floats, 4 in bytes), the null checks, the zeroed blob.  `fill` tells whether
// there is a blob to fill.
inline int begin_pack(int kind, const int32_t* dims, int n_dims, int cols, int om_cols, void (*replan)(VnPlan&), int units_per_float, const float* const* params,
                      void* blob, size_t* n_units, VnPlan& p, bool& fill)
{
    fill = false;
    const int rc = build_plan(kind, dims, n_dims, cols, om_cols, p);
    if (rc != CS_OK) return rc;
    if (replan) replan(p);
    if (!n_units) return fail(CS_ERR_ARG, "null argument");
    *n_units = (size_t)p.total_floats * units_per_float;
    if (!blob) return CS_OK;
    if (!params) return fail(CS_ERR_ARG, "null argument");
    for (int l = 0; l < p.n_layers; ++l)
        if (!params[2 * l] || !params[2 * l + 1]) return fail(CS_ERR_ARG, "null weight or bias array");
    memset(blob, 0, (size_t)p.total_floats * sizeof(float));
    fill = true;
    return CS_OK;
}

// the LDS buffers of a launch; Gsum: the float32 running sum of the crowd mean of a group in chunks
struct VnBufs { float *X0, *M1, *P, *Q, *G, *Gsum, *J, *sc, *den, *val; int* grp; };

// the chains of value_net_body.inc: mlp1 (ends in M1); mlp2 / attention (their output goes to a reduction); mlp3; CADRL's value_network
enum { CH_MLP1, CH_REDUCED, CH_MLP3, CH_CADRL };

// rows of the rotated array into the input tile, zero beyond the rows and the columns; grp[r] = the tile-local group of row r
__device__ __forceinline__ void load_tile(const VnBufs& b, const float* __restrict__ rows_src, int rows, int cols, int per_group, int M)
{
    for (int i = threadIdx.x; i < M * 16; i += NT) {
        const int r = i >> 4, c = i & 15;
        b.X0[r * LDX + c] = (r < rows && c < cols) ? rows_src[(long)r * cols + c] : 0.0f;
    }
    for (int r = threadIdx.x; r < M; r += NT) b.grp[r] = r < rows ? r / per_group : 0;
}

// One float32 layer of a tile: dst[rows][ncb * 32] = act(src[rows][K] x Wt + b) for `rbs` row blocks of 32.  The A operand of row r comes
// from src (k-groups below kg_split) and then from src2[grp[r]] (the per-group second source: SARL's mean of mlp1); columns beyond N are
// stored as 0 whatever the inputs (their zero weights and bias give 0 only for finite inputs: 0 * inf is a NaN, which the next layer's
// zero weights would hand on where torch returns +-inf), so the next layer may read its K rounded up to 8.
// OUT_BF16 (value_net_bf16.hip): the output is the operand of a bf16 layer -- dst holds bfloat16 rows of 2 * ldd elements, each value
// rounded to nearest even after the bias and the ReLU.
template <bool OUT_BF16>
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
        if constexpr (OUT_BF16) {
            __bf16* d = reinterpret_cast<__bf16*>(dst) + (rb * 32 + 4 * h) * (2 * ldd) + cb * 32 + li;
            const bool pad = cb * 32 + li >= L.N;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = acc[r];
                if (L.relu) v = v < 0.0f ? 0.0f : v;
                d[((r & 3) + 8 * (r >> 2)) * (2 * ldd)] = static_cast<__bf16>(pad ? 0.0f : v);
            }
        } else {
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
}

} // namespace
