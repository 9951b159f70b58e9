// value_net_pick.h -- the per-world pick that follows the network kernel of every decide entry (value_net.hip, value_net_worlds.hip,
// value_net_bf16.hip), and its launch.  Included behind the translation unit's network kernel; unnamed namespace, as value_net_plan.h.
#pragma once
#include "value_net_plan.h"

namespace {

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

// what the decide entries do alike after their kernel's launch: its launch status, then the pick on the same stream
inline int launch_pick(int W, int A, const float* d_values, const float* d_actions, const float* d_robot, int robot_stride, const int32_t* d_override,
                       int32_t* d_choice, float* d_action_out, void* stream)
{
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_value_pick, dim3((W + 3) / 4), dim3(256), 0, (hipStream_t)stream, W, A, d_values, d_actions, d_robot, robot_stride,
                       d_override, d_choice, d_action_out);
    HIP_TRY(hipGetLastError());
    return CS_OK;
}

} // namespace
