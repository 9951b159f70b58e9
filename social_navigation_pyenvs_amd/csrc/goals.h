// goals.h -- a human's goal list [G][2]: the goals in use are the prefix before the first NaN x coordinate.  update_goals
// (motion_model_manager.py:66-70) moves the reached head behind the last goal in use; cs_peek commits nothing and only needs the
// head the rotated list would have.  Loads, stores and isnan only: the same in every translation unit whatever its contraction.
#pragma once
#include <hip/hip_runtime.h>

namespace csimpl {

// number of goals in use
__device__ __forceinline__ int goal_count(const float* gi, int G)
{
    int k = G;
    for (int g = 0; g < G; ++g) if (isnan(gi[2 * g])) { k = g; break; }
    return k;
}

// update_goals commits: the first k goals rotate in place (the head becomes the last); (g0x, g0y) = the new head
__device__ __forceinline__ void goal_rotate(float* gi, int k, float& g0x, float& g0y)
{
    const float r0 = gi[0], r1 = gi[1];
    for (int g = 0; g + 1 < k; ++g) { gi[2 * g] = gi[2 * g + 2]; gi[2 * g + 1] = gi[2 * g + 3]; }
    if (k > 0) { gi[2 * (k - 1)] = r0; gi[2 * (k - 1) + 1] = r1; }
    g0x = gi[0]; g0y = gi[1];
}

// cs_peek commits nothing: (g0x, g0y) = the head the rotated list would have
__device__ __forceinline__ void goal_peek_head(const float* gi, int k, float& g0x, float& g0y)
{
    if (k > 1) { g0x = gi[2]; g0y = gi[3]; }
}

} // namespace csimpl
