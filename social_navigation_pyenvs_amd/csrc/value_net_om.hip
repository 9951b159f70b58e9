// value_net_om.hip -- OM-SARL's decision (sarl.with_om = true: crowd_nav/policy/multi_human_rl.py:57-59 and 75-78): SARL's network on rows
// widened by every human's local occupancy map.  The kernel is value_net.hip's (value_net_body.inc, value_net_f32.h's arithmetic, the same
// tiles, workgroups, layers and reductions; cs_value_net_pack's blob layout with a wider first layer) with a fifth tile loader.  Row r of a
// tile is the 13 | 15 rotated columns of its (world, action, human) from cs_lookahead's tensor, then the C map columns of that (world,
// human) from d_maps [W][n][C] (cs_occupancy_maps) -- one map row serves all A actions of its world, the maps are never expanded A-fold in
// HBM --, then zeros up to the first layer's K rounded up to 8, and zero rows beyond the tile's, as load_tile pads.  A group in chunks
// (n > 32) reads human ch * 32 + r.
//
// The input tile's row stride is this kernel's own: K rounded up to 8, plus 4 floats (an argument; the other kernels keep LDX = 20).  Rows
// stay 16-byte aligned; at the reference's default widths (61 | 63 -> 64 + 4 = 68) the stride is 4 (mod 32), the bank spread of the
// other LDS buffers.  One wavefront copies a row at a time, a lane per column: the world, the human and the two source rows are uniform
// over the wavefront and the loads of a row are consecutive floats.  Float32, SARL only, no atomics.  gfx950 only.
#include <hip/hip_runtime.h>

#include "value_net_f32.h"

namespace {

struct OmRows {
    const float* __restrict__ rotated;     // [W][A][n][cols]
    const float* __restrict__ maps;        // [W][n][om]
    int A, n, om, kpad, ldx;               // kpad: the first layer's K rounded up to 8
};

// chunk ch of the tile whose first group is g0: `rows` rows of `per` humans a group
__device__ __forceinline__ void load_tile_om(const OmRows& s, const VnBufs& b, int g0, int ch, int rows, int cols, int per, int M)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* src = s.rotated + ((long)g0 * s.n + (long)ch * M) * cols;
    for (int r = wave; r < M; r += NT / 64) {
        const bool live = r < rows;
        const int k = live ? r / per : 0, j = ch * M + r - k * per;
        const float* rot = src + (long)r * cols;
        const float* map = s.maps + ((long)((g0 + k) / s.A) * s.n + j) * s.om;
        for (int c = lane; c < s.kpad; c += 64) {
            float v = 0.0f;
            if (live && c < cols) v = rot[c];
            else if (live && c < cols + s.om) v = map[c - cols];
            b.X0[r * s.ldx + c] = v;
        }
    }
    for (int r = threadIdx.x; r < M; r += NT) b.grp[r] = r < rows ? r / per : 0;
}

__global__ __launch_bounds__(NT) void k_value_net_om(VnPlan p, VnLds m, int ldx_in, int M, const float* __restrict__ wb, int NG, int A, int n,
                                                     const float* __restrict__ rotated, const float* __restrict__ maps,
                                                     const float* __restrict__ rewards, const float* __restrict__ robot, int rstride, float gamma,
                                                     float dt, float* __restrict__ values)
{
    extern __shared__ float lds[];
    const int gsum = m.G;
    const OmRows wide{rotated, maps, A, n, p.L[0].K1 - p.cols, p.L[0].kg_split * 8, ldx_in};
#define VN_INPUT_STRIDE ldx_in
#define VN_BEGIN_JOB(gbase, ng)
#define VN_TILE_SOURCE(g0) const int tile_g0 = (g0)
#define VN_LOAD_TILE(ch, rows, per) load_tile_om(wide, b, tile_g0, ch, rows, cols, per, M)
#define VN_REWARD(g, k) rewards[g]
#include "value_net_body.inc"
#undef VN_INPUT_STRIDE
#undef VN_BEGIN_JOB
#undef VN_TILE_SOURCE
#undef VN_LOAD_TILE
#undef VN_REWARD
}

} // namespace

#include "value_net_pick.h"

extern "C" int cs_value_net_pack_om(int kind, const int32_t* dims, int n_dims, int cols, int om_cols, const float* const* params, float* blob,
                                    size_t* n_floats)
{
    if (om_cols < 1) return fail(CS_ERR_ARG, "om_cols must be at least 1");
    VnPlan p;
    bool fill;
    const int rc = begin_pack(kind, dims, n_dims, cols, om_cols, nullptr, 1, params, blob, n_floats, p, fill);
    if (rc != CS_OK || !fill) return rc;
    for (int l = 0; l < p.n_layers; ++l)
        pack_layer_f32(p.L[l], params[2 * l], params[2 * l + 1], blob);
    return CS_OK;
}

extern "C" int cs_value_net_decide_om(int kind, const int32_t* dims, int n_dims, const float* d_weights, size_t n_weight_floats, int W, int A, int n,
                                      int cols, int om_cols, const float* d_rotated, const float* d_maps, const float* d_rewards,
                                      const float* d_actions, const float* d_robot, int robot_stride, float gamma, float dt,
                                      const int32_t* d_override, float* d_values, int32_t* d_choice, float* d_action_out, void* stream)
{
    if (om_cols < 1) return fail(CS_ERR_ARG, "om_cols must be at least 1");
    VnPlan p;
    const int rc = build_plan(kind, dims, n_dims, cols, om_cols, p);
    if (rc != CS_OK) return rc;
    const int rc2 = check_decide_args(p, d_weights, n_weight_floats, W, A, n, d_rotated, d_rewards, d_actions, d_robot, robot_stride, d_values, d_action_out);
    if (rc2 != CS_OK) return rc2;
    if (!d_maps) return fail(CS_ERR_ARG, "null argument");
    const int ldx = p.L[0].kg_split * 8 + 4;
    VnLaunch q;
    const int rc3 = prepare_launch<k_value_net_om>(p, n, 0, W, A, q, ldx);
    if (rc3 != CS_OK) return rc3;
    hipLaunchKernelGGL(k_value_net_om, dim3(q.grid), dim3(NT), q.shmem, (hipStream_t)stream, p, q.m, ldx, TILE_M, d_weights, q.NG, A, n, d_rotated,
                       d_maps, d_rewards, d_robot, robot_stride, gamma, dt, d_values);
    return launch_pick(W, A, d_values, d_actions, d_robot, robot_stride, d_override, d_choice, d_action_out, stream);
}
