// policy_no_train.hip -- the CrowdNav baseline robot policies that need no training, batched: one launch gives the ActionXY of the
// robots of W worlds.  Replaces BlindPlanner / SimpleSocialPlanner / SFMHelbing / SFMGuo / SFMMoussaid .predict
//   /root/reference/crowd_nav/policy_no_train/blind_planner.py:16-23, simple_social_planner.py:18-33, sfm_helbing.py:34-55 (and
//   sfm_guo.py / sfm_moussaid.py), forces.py:11-100
// reading the robot from its safe-state record (agent.py:256-258: x, y, yaw, Vx, Vy, BVx, BVy, Omega, radius, mass, gx, gy, v_pref)
// and the humans from the observation rows the Gym writes (cs_gym_observe: px, py, vx, vy, radius[, theta, omega]).
//
// One wavefront per world, lanes over humans (a loop of stride 64 beyond 64 humans), then a butterfly reduction: the per-human
// terms are summed in the same tree for every world, so a world gives the same bits in a batch of 4096 as alone (predict(), W = 1).
// The pair law is rmodel::pair_term (robot_model.h), the single-agent term of forces.py with r_ij = robot radius + human radius.
// Floating-point contraction is off, as in robot_model.h.  gfx950 only.
#include <hip/hip_runtime.h>

#include <cmath>

#include "common.h"
#include "robot_model.h"

namespace {

using csimpl::fail;

constexpr int WAVE = 64;
constexpr int WAVES_PER_BLOCK = 4;

struct PntParams { float p[CS_PNT_N_PARAMS]; };

using rmodel::wave_sum;

__device__ __forceinline__ void toward_goal(float px, float py, float gx, float gy, float vd, float* out)
{
    // theta = atan2(gy - py, gx - px); (cos, sin) * v_pref: at the goal atan2(0, 0) = 0 gives (v_pref, 0), never NaN
    const float th = atan2f(gy - py, gx - px);
    float s, c;
    sincosf(th, &s, &c);
    out[0] = c * vd;
    out[1] = s * vd;
}

__global__ __launch_bounds__(WAVE * WAVES_PER_BLOCK) void k_policy_no_train(int policy, int W, int n, const float* __restrict__ robot,
                                                                            const float* __restrict__ obs, int oc, float time_step,
                                                                            PntParams prm, float* __restrict__ action)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (WAVE - 1);
    const int w = blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6);
    if (w >= W) return;                       // whole wavefronts leave together: no lane of a live world is missing below
    const float* rb = robot + (long)w * 13;
    const float px = rb[0], py = rb[1], vx = rb[3], vy = rb[4], rr = rb[8], gx = rb[10], gy = rb[11], vd = rb[12];
    const float* ow = obs + (long)w * n * oc;
    float* out = action + (long)w * 2;

    if (policy == CS_PNT_BP) {
        if (lane == 0) toward_goal(px, py, gx, gy, vd, out);
        return;
    }
    if (policy == CS_PNT_SSP) {
        // simple_social_planner.py:23-27: stop as soon as one human's surface distance is <= 0.2
        bool near = false;
        for (int j = lane; j < n; j += WAVE) {
            const float* h = ow + (long)j * oc;
            const float dx = h[0] - px, dy = h[1] - py;
            const float d = sqrtf(dx * dx + dy * dy) - h[4] - rr;
            near = near || (d <= 0.2f);
        }
        const bool any = __any(near);
        if (lane == 0) {
            if (any) { out[0] = 0.0f; out[1] = 0.0f; }
            else toward_goal(px, py, gx, gy, vd, out);
        }
        return;
    }
    // the three social-force robots: soc = 0 Helbing, 1 Guo, 2 Moussaid (robot_model.h pair_term)
    const int soc = policy - CS_PNT_SFM_HELBING;
    const float* P = prm.p;
    float fx = 0.0f, fy = 0.0f;
    for (int j = lane; j < n; j += WAVE) {
        const float* h = ow + (long)j * oc;
        float tx, ty;
        rmodel::pair_term(soc, P, px, py, vx, vy, h[0], h[1], h[2], h[3], rr + h[4], tx, ty);
        fx += tx;
        fy += ty;
    }
    fx = wave_sum(fx);
    fy = wave_sum(fy);
    if (lane != 0) return;
    // forces.py:11-25: desired force, 0 within one radius of the goal
    const float mass = P[CS_PNT_MASS];
    const float ddx = gx - px, ddy = gy - py;
    const float dist = sqrtf(ddx * ddx + ddy * ddy);
    if (dist > rr) {
        fx = mass * (ddx / dist * vd - vx) / P[0] + fx;
        fy = mass * (ddy / dist * vd - vy) / P[0] + fy;
    }
    // sfm_helbing.py:46-48: Euler over the policy's time step, speed clamped to v_pref
    float nvx = vx + fx / mass * time_step, nvy = vy + fy / mass * time_step;
    const float sp = sqrtf(nvx * nvx + nvy * nvy);
    if (sp > vd) { nvx = nvx / sp * vd; nvy = nvy / sp * vd; }
    out[0] = nvx;
    out[1] = nvy;
}

} // namespace

extern "C" int cs_policy_no_train(int policy, int W, int n, const float* d_robot13, const float* d_obs, int obs_cols, float time_step,
                                  const float* params, float* d_action, void* stream)
{
    if (policy < CS_PNT_BP || policy > CS_PNT_SFM_MOUSSAID) return fail(CS_ERR_ARG, "unknown no-train policy id (CS_PNT_*)");
    if (W < 1 || n < 0) return fail(CS_ERR_ARG, "W must be >= 1 and n >= 0");
    if (obs_cols != 5 && obs_cols != 7) return fail(CS_ERR_ARG, "observation rows have 5 or 7 columns");
    if (!d_robot13 || !d_action || (n > 0 && !d_obs)) return fail(CS_ERR_ARG, "null argument");
    const bool sfm = policy >= CS_PNT_SFM_HELBING;
    if (sfm && !params) return fail(CS_ERR_ARG, "the social-force policies need their parameters");
    PntParams prm{};
    if (sfm) {
        for (int i = 0; i < CS_PNT_N_PARAMS; ++i) prm.p[i] = params[i];
        if (!(prm.p[CS_PNT_MASS] != 0.0f) || !(prm.p[0] != 0.0f)) return fail(CS_ERR_ARG, "mass and relaxation_time must be non-zero");
    }
    const int blocks = (W + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    hipLaunchKernelGGL(k_policy_no_train, dim3(blocks), dim3(WAVE * WAVES_PER_BLOCK), 0, (hipStream_t)stream, policy, W, n, d_robot13,
                       d_obs, obs_cols, time_step, prm, d_action);
    HIP_TRY(hipGetLastError());
    return CS_OK;
}
