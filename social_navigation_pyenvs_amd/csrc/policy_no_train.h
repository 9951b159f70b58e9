// policy_no_train.h -- the decision of the CrowdNav baseline robot policies that need no training, the arithmetic shared by its two homes:
//   policy_no_train.hip  k_policy_no_train: one wavefront per world, lanes over humans (cs_policy_no_train, a launch of its own)
//   sfmstep_kernel.h     k_sfm_step<..., LEAN = 8 + 1 | 3>: the decision inside the Gym step's launch (cs_gym_step_policy), taken in the
//                        prologue from the rows the launch has loaded, before the Gym head consumes the action
// One statement of each policy: BlindPlanner / SimpleSocialPlanner / SFMHelbing / SFMGuo / SFMMoussaid .predict
//   crowd_nav/policy_no_train/blind_planner.py:16-23, simple_social_planner.py:18-33, sfm_helbing.py:34-55 (sfm_guo.py, sfm_moussaid.py),
//   forces.py:11-100.
// Both homes must give the SAME bits (tests/test_gpu_policy_step.py compares the two paths with array_equal), so every function here runs
// with floating-point contraction OFF, the pair law is rmodel::pair_term, and the sum over humans is rmodel::wave_sum over 64 lanes that
// hold human j's term in lane j and an exact +0 elsewhere (world_sum below brings a world that lives anywhere in a wavefront into that
// shape).  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "crowdstep.h"
#include "robot_model.h"

namespace pnt {

// bp (and ssp with nobody near): straight to the goal at v_pref
__device__ __forceinline__ void toward_goal(float px, float py, float gx, float gy, float vd, float& ox, float& oy)
{
#pragma clang fp contract(off)
    // theta = atan2(gy - py, gx - px); (cos, sin) * v_pref: at the goal atan2(0, 0) = 0 gives (v_pref, 0), never NaN
    const float th = atan2f(gy - py, gx - px);
    float s, c;
    sincosf(th, &s, &c);
    ox = c * vd;
    oy = s * vd;
}

// simple_social_planner.py:23-27: one human's surface distance to the robot is <= 0.2 (the robot stops as soon as one is)
__device__ __forceinline__ bool ssp_near(float hx, float hy, float hr, float px, float py, float rr)
{
#pragma clang fp contract(off)
    const float dx = hx - px, dy = hy - py;
    const float d = sqrtf(dx * dx + dy * dy) - hr - rr;
    return d <= 0.2f;
}

// what a lane adds to its running sum for one human: the running sum starts at +0, so a term of -0 goes in as +0 -- and no partial sum of
// the butterfly is ever -0, which is what makes an absent lane's +0 an exact identity
__device__ __forceinline__ void add_term(float& fx, float& fy, float tx, float ty)
{
#pragma clang fp contract(off)
    fx += tx;
    fy += ty;
}

// the social-force robots behind the sum over humans (fx, fy): desired force (forces.py:11-25: 0 within one radius of the goal), Euler
// over the policy's time step, speed clamped to v_pref (sfm_helbing.py:46-48).  relax_t = P[0] of the packed parameters.
__device__ __forceinline__ void sfm_decide(float relax_t, float mass, float time_step, float px, float py, float vx, float vy, float rr,
                                           float gx, float gy, float vd, float fx, float fy, float& ox, float& oy)
{
#pragma clang fp contract(off)
    const float ddx = gx - px, ddy = gy - py;
    const float dist = sqrtf(ddx * ddx + ddy * ddy);
    if (dist > rr) {
        fx = mass * (ddx / dist * vd - vx) / relax_t + fx;
        fy = mass * (ddy / dist * vd - vy) / relax_t + fy;
    }
    float nvx = vx + fx / mass * time_step, nvy = vy + fy / mass * time_step;
    const float sp = sqrtf(nvx * nvx + nvy * nvy);
    if (sp > vd) { nvx = nvx / sp * vd; nvy = nvy / sp * vd; }
    ox = nvx;
    oy = nvy;
}

// The sum of a world's per-human terms inside a wavefront that holds `wpb` worlds of `rows` lanes each (human j of world l in lane
// l * rows + j, j < n; v = the lane's term, +0 in a lane without a human), as k_policy_no_train sums them: for one world after the other,
// lane j < n fetches human j's term, every other lane takes +0, and rmodel::wave_sum runs over the 64 lanes.  Every lane of world `lw`
// returns its own world's total.  Wave-uniform control flow; the fetch is one ds_bpermute.
__device__ __forceinline__ float world_sum(float v, int tid, int lw, int rows, int n, int wpb)
{
    float mine = 0.0f;
    for (int l = 0; l < wpb; ++l) {
        const int got = __builtin_amdgcn_ds_bpermute(((l * rows + tid) & 63) << 2, __float_as_int(v));
        const float s = rmodel::wave_sum(tid < n ? __int_as_float(got) : 0.0f);
        if (lw == l) mine = s;
    }
    return mine;
}

} // namespace pnt
