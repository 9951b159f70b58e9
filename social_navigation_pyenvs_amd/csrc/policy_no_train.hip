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
// The policies themselves are stated once, in policy_no_train.h, which the Gym step's kernel includes too (cs_gym_step_policy).
// Floating-point contraction is off, as in robot_model.h.  gfx950 only.
#include <hip/hip_runtime.h>

#include <cmath>

#include "common.h"
#include "policy_no_train.h"
#include "robot_model.h"

namespace {

using csimpl::fail;

constexpr int WAVE = 64;
constexpr int WAVES_PER_BLOCK = 4;

struct PntParams { float p[CS_PNT_N_PARAMS]; };

using rmodel::wave_sum;

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
        if (lane == 0) pnt::toward_goal(px, py, gx, gy, vd, out[0], out[1]);
        return;
    }
    if (policy == CS_PNT_SSP) {
        // simple_social_planner.py:23-27: stop as soon as one human's surface distance is <= 0.2
        bool near = false;
        for (int j = lane; j < n; j += WAVE) {
            const float* h = ow + (long)j * oc;
            near = near || pnt::ssp_near(h[0], h[1], h[4], px, py, rr);
        }
        const bool any = __any(near);
        if (lane == 0) {
            if (any) { out[0] = 0.0f; out[1] = 0.0f; }
            else pnt::toward_goal(px, py, gx, gy, vd, out[0], out[1]);
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
        pnt::add_term(fx, fy, tx, ty);
    }
    fx = wave_sum(fx);
    fy = wave_sum(fy);
    if (lane != 0) return;
    // desired force, Euler over the policy's time step, the v_pref clamp (policy_no_train.h)
    pnt::sfm_decide(P[0], P[CS_PNT_MASS], time_step, px, py, vx, vy, rr, gx, gy, vd, fx, fy, out[0], out[1]);
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
