// value_net_om_bf16.hip -- OM-SARL's decision (value_net_om.hip: cs_value_net_decide_om) with the opt-in bf16 arithmetic
// (cs_value_net_decide_om_bf16; Python: OMSARL.set_wide_precision("bf16")): SARL's network on rows of 13 | 15 rotated columns followed by
// om_cols occupancy-map columns, from the same inputs -- cs_lookahead's rows and rewards, the maps [W][n][om_cols] of cs_occupancy_maps
// read in place, one map row for all A actions of its world.  The kernel is value_net_body.inc on the arithmetic of
// value_net_bf16_layers.h (value_net_bf16.hip states the contract) with one layer of its own: mlp1's layer 0, split by column as
// value_net_lstm_om_bf16.hip splits its first layer.  This file keeps what is the map columns' own: the loader, that layer, the plan
// change and the two entries.
//
// mlp1 layer 0: the rotated columns take full-precision weights [:, :cols] and unrounded inputs on
// v_mfma_f32_32x32x2_f32 (they reach 10 m, where one bf16 step is 3 cm); the map columns take weights [:, cols:] rounded to bf16 (nearest
// even) by the pack and values rounded once, nearest even, when the loader stages them (an occupancy is 0 or 1 exactly, a mean velocity a
// few m/s), zeros up to a multiple of 16 columns, on v_mfma_f32_32x32x16_bf16.  A pre-activation is one chain: the bias, the two float32
// k-groups ascending, the ksm = ceil(om_cols / 16) map k-steps ascending; then the ReLU; then it is rounded once as the operand of the
// next layer.  With all-zero map weights the map k-steps add +0 to a finite sum: the values are cs_value_net_decide_bf16's on the narrow
// network.
//
// The input tile: the rotated columns as value_net_bf16.hip's kernel holds them (float32 rows at the narrow stride LDX), and behind the
// tile's M rows the map columns as bfloat16 rows of 16 ksm elements at a pitch of 16 * odd bytes (8 ksm + 4 floats), the pitch of every
// bf16 operand here.  Both lie in the LDS map's X0, which is asked for M rows of LDX + 8 ksm + 4 floats.  A group in chunks (n > 32)
// reads human ch * 32 + r.  SARL only, no atomics, gfx950 only.
#include <hip/hip_runtime.h>

#include "value_net_bf16.h"

namespace {

__device__ __forceinline__ void om_first_layer(const VnLayer& L, const float* __restrict__ wb, const float* src, int lds_, const float* src2, int lds2,
                                               const int* grp, int rbs, float* dst, int ldd, int rot);

} // namespace

#define VN_MLP1_LAYER0 om_first_layer
#include "value_net_bf16_layers.h"

namespace {

constexpr int OM_KGF = 2;              // float32 k-groups of 8 of a rotated row: 13 | 15 columns (build_plan admits no other)

// the pitch (floats) of a staged map row of ksm k-steps
__host__ __device__ inline int om_pitch(int ksm) { return 8 * ksm + 4; }

// replan_bf16 for rows with map columns: mlp1's layer 0 counts the float32 k-groups of its rotated columns, then the k-steps of 16 of its
// map columns -- [ncb][2 + ksm][64 lanes] slots of 16 bytes in the blob (pack_layer_mixed)
void replan_om_bf16(VnPlan& p)
{
    VnLayer& L = p.L[p.c0[0]];
    L.kg_split = OM_KGF;
    L.kg_total = OM_KGF + up(L.K1 - p.cols, 16) / 16;
    replan_bf16(p);
}

struct OmMaps {
    const float* __restrict__ maps;        // [W][n][om]
    int A, n, om, ksm;
};

// chunk ch of the tile whose first group is g0: the rotated columns as load_tile leaves them (grp too); behind the tile's M float32 rows
// the map columns of every row's (world, human), each value rounded once to bf16, zeros up to the last k-step's end and in the rows
// beyond the tile's.  One wavefront stages a row at a time, a lane per column: the world and the human are uniform over the wavefront.
__device__ __forceinline__ void load_tile_om_h(const OmMaps& s, const VnBufs& b, const float* __restrict__ grows, int g0, int ch, int rows, int cols,
                                               int per, int M)
{
    load_tile(b, grows + (long)ch * M * cols, rows, cols, per, M);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __bf16* mb = reinterpret_cast<__bf16*>(b.X0 + M * LDX);
    const int pitch = 2 * om_pitch(s.ksm);
    for (int r = wave; r < M; r += NT / 64) {
        const bool live = r < rows;
        const int k = live ? r / per : 0, j = live ? ch * M + r - k * per : 0;
        const float* map = s.maps + ((long)((g0 + k) / s.A) * s.n + j) * s.om;
        for (int c = lane; c < 16 * s.ksm; c += 64) mb[r * pitch + c] = static_cast<__bf16>(live && c < s.om ? map[c] : 0.0f);
    }
}

// mlp1's layer 0 on a tile: layer_fwd's arguments (src the input tile at the narrow stride, the staged map rows behind its rbs * 32
// rows; no second source).  The float32 k-groups of the rotated columns, then the bf16 k-steps of the map columns, into one accumulator
// -- the blob walk and the one-deep prefetch of value_net_lstm_om_bf16.hip's first layer --; the output is the operand of a bf16 layer.
__device__ __forceinline__ void om_first_layer(const VnLayer& L, const float* __restrict__ wb, const float* src, int lds_, const float*, int, const int*,
                                               int rbs, float* dst, int ldd, int rot)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, li = lane & 31;
    const int items = rbs * L.ncb;
    const int KG = L.kg_total, ldm = om_pitch(KG - OM_KGF);
    const float* xm = src + rbs * 32 * lds_;
    for (int it = (wave + rot) & 3; it < items; it += 4) {
        const int rb = it % rbs, cb = it / rbs;
        const int row = rb * 32 + li;
        const float* a1 = src + row * lds_ + 4 * h;
        const float* am = xm + row * ldm + 4 * h;
        const float4* bw = reinterpret_cast<const float4*>(wb + L.w_off) + (long)cb * KG * 64 + lane;
        const float bias = wb[L.b_off + cb * 32 + li];
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = bias;
        float4 nw = bw[0];
#pragma unroll
        for (int kg = 0; kg < OM_KGF; ++kg) {
            const float4 w = nw;
            nw = bw[(kg + 1) * 64];                        // (KG > OM_KGF: om_cols >= 1)
            const float4 a = *reinterpret_cast<const float4*>(a1 + kg * 8);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, w.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, w.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, w.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, w.w, acc, 0, 0, 0);
        }
        for (int kg = OM_KGF; kg < KG; ++kg) {
            const float4 w = nw;
            nw = bw[(kg + 1 < KG ? kg + 1 : kg) * 64];
            const float4 a = *reinterpret_cast<const float4*>(am + (kg - OM_KGF) * 8);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, w), acc, 0, 0, 0);
        }
        // C/D map of the 32x32 forms: column = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
        __bf16* d = reinterpret_cast<__bf16*>(dst) + (rb * 32 + 4 * h) * (2 * ldd) + cb * 32 + li;
        const bool pad = cb * 32 + li >= L.N;              // (the zero weights give 0 * inf = NaN there when an input is infinite)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = acc[r];
            if (L.relu) v = v < 0.0f ? 0.0f : v;          // (a NaN stays a NaN, as torch's ReLU leaves it)
            d[((r & 3) + 8 * (r >> 2)) * (2 * ldd)] = static_cast<__bf16>(pad ? 0.0f : v);
        }
    }
}

// k_value_net_bf16 with the wide loader; `gsum` as there
__global__ __launch_bounds__(NT) void k_value_net_om_bf16(VnPlan p, VnLds m, int gsum, int M, const float* __restrict__ wb, int NG, int A, int n,
                                                          const float* __restrict__ rotated, const float* __restrict__ maps,
                                                          const float* __restrict__ rewards, const float* __restrict__ robot, int rstride,
                                                          float gamma, float dt, float* __restrict__ values)
{
    extern __shared__ float lds[];
    const VnLayer& first = p.L[p.c0[0]];
    const OmMaps wide{maps, A, n, first.K1 - p.cols, first.kg_total - OM_KGF};
#define VN_BEGIN_JOB(gbase, ng)
#define VN_TILE_SOURCE(g0) const int tile_g0 = (g0); const float* grows = rotated + (long)tile_g0 * n * cols
#define VN_LOAD_TILE(ch, rows, per) load_tile_om_h(wide, b, grows, tile_g0, ch, rows, cols, per, M)
#define VN_REWARD(g, k) rewards[g]
#include "value_net_body.inc"
#undef VN_BEGIN_JOB
#undef VN_TILE_SOURCE
#undef VN_LOAD_TILE
#undef VN_REWARD
}

} // namespace

#include "value_net_pick.h"

extern "C" int cs_value_net_pack_om_bf16(int kind, const int32_t* dims, int n_dims, int cols, int om_cols, const float* const* params, void* blob,
                                         size_t* n_bytes)
{
    if (om_cols < 1) return fail(CS_ERR_ARG, "om_cols must be at least 1");
    VnPlan p;
    bool fill;
    const int rc = begin_pack(kind, dims, n_dims, cols, om_cols, replan_om_bf16, sizeof(float), params, blob, n_bytes, p, fill);
    if (rc != CS_OK || !fill) return rc;
    float* fb = static_cast<float*>(blob);
    for (int l = 0; l < p.n_layers; ++l) {
        if (l == p.c0[0]) pack_layer_mixed(p.L[l], cols, params[2 * l], params[2 * l + 1], fb);
        else if (vn_f32_layer(p, l)) pack_layer_f32(p.L[l], params[2 * l], params[2 * l + 1], fb);
        else pack_layer_bf16(p.L[l], params[2 * l], params[2 * l + 1], fb);
    }
    return CS_OK;
}

extern "C" int cs_value_net_decide_om_bf16(int kind, const int32_t* dims, int n_dims, const void* d_weights, size_t n_weight_bytes, int W, int A, int n,
                                           int cols, int om_cols, const float* d_rotated, const float* d_maps, const float* d_rewards,
                                           const float* d_actions, const float* d_robot, int robot_stride, float gamma, float dt,
                                           const int32_t* d_override, float* d_values, int32_t* d_choice, float* d_action_out, void* stream)
{
    if (om_cols < 1) return fail(CS_ERR_ARG, "om_cols must be at least 1");
    VnPlan p;
    const int rc = build_plan(kind, dims, n_dims, cols, om_cols, p);
    if (rc != CS_OK) return rc;
    replan_om_bf16(p);
    // (a length that is no whole number of floats is no blob of any network: it fails the size check as SIZE_MAX floats)
    const size_t n_floats = n_weight_bytes % sizeof(float) ? (size_t)-1 : n_weight_bytes / sizeof(float);
    const int rc2 = check_decide_args(p, d_weights, n_floats, W, A, n, d_rotated, d_rewards, d_actions, d_robot, robot_stride, d_values, d_action_out);
    if (rc2 != CS_OK) return rc2;
    if (!d_maps) return fail(CS_ERR_ARG, "null argument");
    // (the tail: the float32 running sum of a chunked crowd mean, where the kernel keeps one)
    const int tail = p.with_global && n > TILE_M ? up(p.m1w, 16) : 0;
    VnLaunch q;
    const int rc3 = prepare_launch<k_value_net_om_bf16>(p, n, tail, W, A, q, LDX + om_pitch(p.L[p.c0[0]].kg_total - OM_KGF));
    if (rc3 != CS_OK) return rc3;
    hipLaunchKernelGGL(k_value_net_om_bf16, dim3(q.grid), dim3(NT), q.shmem, (hipStream_t)stream, p, q.m, q.tail, TILE_M, static_cast<const float*>(d_weights),
                       q.NG, A, n, d_rotated, d_maps, d_rewards, d_robot, robot_stride, gamma, dt, d_values);
    return launch_pick(W, A, d_values, d_actions, d_robot, robot_stride, d_override, d_choice, d_action_out, stream);
}
