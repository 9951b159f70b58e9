// value_net_bf16.hip -- the value-network decision of value_net.hip with the opt-in bf16 arithmetic (cs_value_net_decide_bf16; Python:
// policy.set_decision_precision("bf16")).  The kernel is value_net.hip's: the same body (value_net_body.inc: groups, tiles, workgroups, phases,
// reductions) with the same copying loader; this file states the arithmetic the body runs on -- the bf16 layer, the chain of layers and the
// handful of functions the body asks an arithmetic for -- the pack entry of its blob and the decide entry.  The pick kernel follows.
// The host's rounding (bf16_bits), the pack of one bf16 layer and the operand vector bf16x8 are value_net_bf16.h's, which
// value_net_lstm_bf16.hip shares.
//
// The arithmetic:
//   float32 layers   a layer whose input holds raw rotated-state columns: CADRL value_network layer 0, SARL mlp1 layer 0, all of mlp3.
//                    They are value_net.hip's layer (value_net_plan.h layer_fwd) on v_mfma_f32_32x32x2_f32.  dg, px1, da reach 10 m, where
//                    one bf16 step is 3 cm; layer 0 has K = 13 / 15, about 1/10 of the next layer's work; mlp3 runs once per group.
//   bf16 layers      every other layer, on v_mfma_f32_32x32x16_bf16.  Weights rounded to bf16 (nearest even) at pack time; biases
//                    float32, they start the accumulator; float32 accumulation, the k-steps of 16 in order: one fixed order per
//                    output element that depends on the layer's widths alone.
//   rounding points  an activation is rounded to bf16 (nearest even) exactly once: when the epilogue stores it to LDS as the operand of a
//                    bf16 layer, after the bias and the ReLU.  An output that a reduction consumes is NOT rounded: the attention
//                    scores, mlp2's features, CADRL's per-human value.  with_global_state: the crowd mean is summed in float32, in
//                    human order, from the bf16-rounded mlp1 outputs, divided by n, and rounded once as the attention operand.
//   float32 as before  the masked softmax exp(s) * (s != 0) without maximum subtraction, the minimum, the weighted sum,
//                    rewards + gamma^(dt v_pref) out, k_value_pick.
//   NaN / +-inf      follow IEEE through the conversion; padding columns are stored as 0 (0 * inf, as in the float32 kernel).
// A (world, action) gives the same bits alone (W = 1) and anywhere inside a batch.  No atomics.  gfx950 only.
//
// LDS image of a bf16 operand: row-major bfloat16, row stride S = 2 * ld elements where ld = 4 * odd floats, so a row is 16 * odd bytes.
// Lane l of a wavefront reads the 16 bytes (8 k) of row l & 31 at k = 16 s + 8 (l >> 5) with one ds_read_b128; that instruction is served
// in the 16-lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same two + 32: each group holds 16 rows that are distinct
// modulo 16 at one column offset, and row * (16 * odd) bytes puts them on the 16 different 16-byte slots of the 256-byte bank row:
// conflict-free (the float32 file's width + 4 floats does the same for 8 rows of its 32-byte k-groups).
#include <hip/hip_runtime.h>

#include "value_net_bf16.h"

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
            if (l == first) layer_fwd<true>(p.L[l], wb, cur, cur_ld, s2, lds2, b.grp, rbs, dst, ldd, rot);
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

// value_net.hip's k_value_net with this file's arithmetic; `gsum`: floats from the start of the dynamic block to the float32 running
// sum of the crowd mean of a group in chunks, behind the map m
__global__ __launch_bounds__(NT) void k_value_net_bf16(VnPlan p, VnLds m, int gsum, int M, const float* __restrict__ wb, int NG, int A, int n,
                                                       const float* __restrict__ rotated, const float* __restrict__ rewards,
                                                       const float* __restrict__ robot, int rstride, float gamma, float dt, float* __restrict__ values)
{
    extern __shared__ float lds[];
#define VN_BEGIN_JOB(gbase, ng)
#define VN_TILE_SOURCE(g0) const float* grows = rotated + (long)(g0) * n * cols
#define VN_LOAD_TILE(ch, rows, per) load_tile(b, grows + (long)(ch) * M * cols, rows, cols, per, M)
#define VN_REWARD(g, k) rewards[g]
#include "value_net_body.inc"
#undef VN_BEGIN_JOB
#undef VN_TILE_SOURCE
#undef VN_LOAD_TILE
#undef VN_REWARD
}

} // namespace

#include "value_net_pick.h"

extern "C" int cs_value_net_pack_bf16(int kind, const int32_t* dims, int n_dims, int cols, const float* const* params, void* blob, size_t* n_bytes)
{
    VnPlan p;
    bool fill;
    const int rc = begin_pack(kind, dims, n_dims, cols, 0, replan_bf16, sizeof(float), params, blob, n_bytes, p, fill);
    if (rc != CS_OK || !fill) return rc;
    float* fb = static_cast<float*>(blob);
    for (int l = 0; l < p.n_layers; ++l) {       // params: torch.nn.Linear.weight [N][K1 + K2] and bias of every layer
        if (vn_f32_layer(p, l)) pack_layer_f32(p.L[l], params[2 * l], params[2 * l + 1], fb);
        else pack_layer_bf16(p.L[l], params[2 * l], params[2 * l + 1], fb);
    }
    return CS_OK;
}

extern "C" int cs_value_net_decide_bf16(int kind, const int32_t* dims, int n_dims, const void* d_weights, size_t n_weight_bytes, int W, int A, int n,
                                        int cols, const float* d_rotated, const float* d_rewards, const float* d_actions, const float* d_robot,
                                        int robot_stride, float gamma, float dt, const int32_t* d_override, float* d_values, int32_t* d_choice,
                                        float* d_action_out, void* stream)
{
    VnPlan p;
    const int rc = build_plan(kind, dims, n_dims, cols, 0, p);
    if (rc != CS_OK) return rc;
    replan_bf16(p);
    // (a length that is no whole number of floats is no blob of any network: it fails the size check as SIZE_MAX floats)
    const size_t n_floats = n_weight_bytes % sizeof(float) ? (size_t)-1 : n_weight_bytes / sizeof(float);
    const int rc2 = check_decide_args(p, d_weights, n_floats, W, A, n, d_rotated, d_rewards, d_actions, d_robot, robot_stride, d_values, d_action_out);
    if (rc2 != CS_OK) return rc2;
    // (the tail: the float32 running sum of a chunked crowd mean, where the kernel keeps one)
    const int tail = p.kind == CS_VN_SARL && p.with_global && n > TILE_M ? up(p.m1w, 16) : 0;
    VnLaunch q;
    const int rc3 = prepare_launch<k_value_net_bf16>(p, n, tail, W, A, q);
    if (rc3 != CS_OK) return rc3;
    hipLaunchKernelGGL(k_value_net_bf16, dim3(q.grid), dim3(NT), q.shmem, (hipStream_t)stream, p, q.m, q.tail, TILE_M, static_cast<const float*>(d_weights),
                       q.NG, A, n, d_rotated, d_rewards, d_robot, robot_stride, gamma, dt, d_values);
    return launch_pick(W, A, d_values, d_actions, d_robot, robot_stride, d_override, d_choice, d_action_out, stream);
}
