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

#include "value_net_f32.h"

namespace {

__global__ __launch_bounds__(NT) void k_value_net(VnPlan p, VnLds m, int M, const float* __restrict__ wb, int NG, int A, int n,
                                                  const float* __restrict__ rotated, const float* __restrict__ rewards,
                                                  const float* __restrict__ robot, int rstride, float gamma, float dt, float* __restrict__ values)
{
    extern __shared__ float lds[];
    const int gsum = m.G;
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

extern "C" int cs_value_net_pack(int kind, const int32_t* dims, int n_dims, int cols, const float* const* params, float* blob, size_t* n_floats)
{
    VnPlan p;
    bool fill;
    const int rc = begin_pack(kind, dims, n_dims, cols, 0, nullptr, 1, params, blob, n_floats, p, fill);
    if (rc != CS_OK || !fill) return rc;
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
    const int rc = build_plan(kind, dims, n_dims, cols, 0, p);
    if (rc != CS_OK) return rc;
    const int rc2 = check_decide_args(p, d_weights, n_weight_floats, W, A, n, d_rotated, d_rewards, d_actions, d_robot, robot_stride, d_values, d_action_out);
    if (rc2 != CS_OK) return rc2;
    VnLaunch q;
    const int rc3 = prepare_launch<k_value_net>(p, n, 0, W, A, q);
    if (rc3 != CS_OK) return rc3;
    hipLaunchKernelGGL(k_value_net, dim3(q.grid), dim3(NT), q.shmem, (hipStream_t)stream, p, q.m, TILE_M, d_weights, q.NG, A, n, d_rotated, d_rewards,
                       d_robot, robot_stride, gamma, dt, d_values);
    return launch_pick(W, A, d_values, d_actions, d_robot, robot_stride, d_override, d_choice, d_action_out, stream);
}
