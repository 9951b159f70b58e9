// value_net_bf16.hip -- the value-network decision of value_net.hip with the opt-in bf16 arithmetic (cs_value_net_decide_bf16; Python:
// policy.set_decision_precision("bf16")).  The kernel is value_net.hip's: the same body (value_net_body.inc: groups, tiles, workgroups, phases,
// reductions) with the same copying loader, on the arithmetic of value_net_bf16_layers.h -- the bf16 layer, the chain of layers and the
// handful of functions the body asks an arithmetic for, which value_net_om_bf16.hip (OM-SARL) shares; this file states the contract, the
// kernel, the pack entry of its blob and the decide entry.  The pick kernel follows.  The host's rounding (bf16_bits), the pack of one
// bf16 layer and the operand vector bf16x8 are value_net_bf16.h's, which value_net_lstm_bf16.hip shares.
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

#include "value_net_bf16_layers.h"

namespace {

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
