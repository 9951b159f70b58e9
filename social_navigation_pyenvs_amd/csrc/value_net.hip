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

} // namespace

#include "value_net_pick.h"

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
    for (int l = 0; l < p.n_layers; ++l)
        pack_layer_f32(p.L[l], params[2 * l], params[2 * l + 1], blob);
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
    const int rc2 = check_decide_args(p, d_weights, n_weight_floats, W, A, n, d_rotated, d_rewards, d_actions, d_robot, robot_stride, d_values, d_action_out);
    if (rc2 != CS_OK) return rc2;
    const size_t lds_limit = 160 * 1024;
    const int M = TILE_M;
    const VnLds m = lds_map(p, M, n);
    const size_t shmem = (size_t)m.total * sizeof(float);
    // (cannot happen within the limits above -- 16 layers of up to 256 columns need about 150 KiB at most, at n = 2 -- kept as the guard of the launch)
    if (shmem > lds_limit) return fail(CS_ERR_ARG, "the tile buffers of this network do not fit the 160 KiB of LDS");
    if (shmem > 64 * 1024) VN_GRANT_LDS(k_value_net, shmem);
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
