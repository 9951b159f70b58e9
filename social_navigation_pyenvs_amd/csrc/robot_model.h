// robot_model.h -- the robot under a HUMAN motion model (imitation learning), the arithmetic shared by its two homes:
//   robot_model.hip   k_robot_model_step: one wavefront per world (cs_robot_model_step, the robot half of an alternating loop, and
//                     the robot's substeps behind the crowd's snapshots of an invisible-robot imitation block)
//   sfmstep_kernel.h  k_sfm_step<..., LEAN = 4>: the robot as the last row of the crowd's own fused launch (a VISIBLE robot:
//                     robot and crowd act on each other in every substep, so the robot's update sits inside the substep loop)
// Restates MotionModelManager.update_robot(t, dt) for the nine SFM / HSFM titles with the SINGLE-AGENT force functions
//   /root/reference/social_gym/src/motion_model_manager.py:591-629, 72-86;  forces.py:9-16, 27-53, 153-218, 279-290.
// Both homes must give the SAME bits (tests/test_imitation.py compares the fused launch with the alternating launches), so every
// function here runs with floating-point contraction OFF: each operation is one IEEE operation (or one libm call) whatever code
// surrounds it, and the per-human terms are summed in index order by both.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "forces_ref.h"

namespace rmodel {

// sum over the 64 lanes of a wavefront, xor butterfly (every lane gets the total; robot_model.hip's DPP / readlane sum adds in another order)
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the robot's dynamic state and what its model remembers between substeps (agent.desired_force)
struct RState {
    float px, py, yaw, vx, vy, bvx, bvy, om;
    float radius, mass, gx, gy, vd;
    float fdx, fdy;
};

// The term human (hx, hy, hvx, hvy) adds to the robot's social force (forces.py:153-218, consider_robot = False).  P: the robot's
// 20 parameters (agent.py:269 slots); rij = robot radius + robot margin + human radius + human margin; soc = type % 3.
__device__ __forceinline__ void pair_term(int soc, const float* P, float px, float py, float vx, float vy, float hx, float hy, float hvx,
                                          float hvy, float rij, float& tx_out, float& ty_out)
{
    fref::strict::pair_force<fref::strict::FastF>(soc, P, px, py, vx, vy, hx, hy, hvx, hvy, rij, tx_out, ty_out);
}

// headed_agent_update_linear_velocity (motion_model_manager.py:143-145) at the head of compute_robot_forces: the heading's sine /
// cosine (kept for the body-frame projection) and, for a headed robot, the linear velocity from the body velocity
__device__ __forceinline__ void refresh_velocity(RState& r, bool headed, float& sn, float& cs)
{
#pragma clang fp contract(off)
    sincosf(r.yaw, &sn, &cs);
    if (headed) { r.vx = cs * r.bvx - sn * r.bvy; r.vy = sn * r.bvx + cs * r.bvy; }
}

// the right-hand side of the robot's RK45 solve (motion_model_manager.py:661-687) from the forces of compute_robot_forces: the
// desired force (kept within one radius of the goal), then ydot = [v, F / m] or [R bv, omega, F_body / m, torque / I]
template <int NS>
__device__ __forceinline__ void derivative(RState& r, int type, const float* P, float fsx, float fsy, float fox, float foy, float sn, float cs,
                                           float (&out)[NS])
{
#pragma clang fp contract(off)
    const bool torque_new = type >= 6;
    fref::strict::desired_force(r.gx, r.gy, r.px, r.py, r.vx, r.vy, r.radius, r.mass, r.vd, P[0], r.fdx, r.fdy);
    const float fdx = r.fdx, fdy = r.fdy;
    if constexpr (NS == 4) {
        out[0] = r.vx; out[1] = r.vy;
        out[2] = (fdx + fox + fsx) / r.mass; out[3] = (fdy + foy + fsy) / r.mass;
    } else {
        const float inertia = 0.5f * r.mass * r.radius * r.radius;
        float g0, g1, torque;
        fref::strict::headed_force(torque_new, P, inertia, fdx, fdy, fdx + fox + fsx, fdy + foy + fsy, fox + fsx, foy + fsy, r.yaw, r.om, r.bvy, sn, cs, g0, g1, torque);
        out[0] = cs * r.bvx - sn * r.bvy; out[1] = sn * r.bvx + cs * r.bvy; out[2] = r.om;
        out[3] = g0 / r.mass; out[4] = g1 / r.mass; out[5] = torque / inertia;
    }
}

// desired force (forces.py:9-16; within one radius of the goal the previous one is kept), total force, torque (forces.py:279-290)
// and the Euler update (motion_model_manager.py:72-86: position first, then velocity, speed clamp; headed: yaw, body velocity,
// angular velocity, linear velocity from the NEW yaw).  (fsx, fsy): the summed social force; (fox, foy): the obstacle force.
__device__ __forceinline__ void integrate(RState& r, int type, const float* P, float fsx, float fsy, float fox, float foy, float sn, float cs,
                                          float dt, int just_velocities)
{
#pragma clang fp contract(off)
    const bool headed = type >= 3, torque_new = type >= 6;
    fref::strict::desired_force(r.gx, r.gy, r.px, r.py, r.vx, r.vy, r.radius, r.mass, r.vd, P[0], r.fdx, r.fdy);
    const float fdx = r.fdx, fdy = r.fdy;
    float npx, npy, nyaw = r.yaw, nvx, nvy, nbx = r.bvx, nby = r.bvy, nom = r.om;
    if (!headed) {
        const float gfx = fdx + fox + fsx, gfy = fdy + foy + fsy;
        npx = just_velocities ? r.px : r.px + r.vx * dt; npy = just_velocities ? r.py : r.py + r.vy * dt;
        nvx = r.vx + gfx / r.mass * dt; nvy = r.vy + gfy / r.mass * dt;
        const float sp = sqrtf(nvx * nvx + nvy * nvy);
        if (sp > r.vd) { nvx = nvx / sp * r.vd; nvy = nvy / sp * r.vd; }
    } else {
        const float inertia = 0.5f * r.mass * r.radius * r.radius;
        float g0, g1, torque;
        fref::strict::headed_force(torque_new, P, inertia, fdx, fdy, fdx + fox + fsx, fdy + foy + fsy, fox + fsx, foy + fsy, r.yaw, r.om, r.bvy, sn, cs, g0, g1, torque);
        npx = just_velocities ? r.px : r.px + r.vx * dt; npy = just_velocities ? r.py : r.py + r.vy * dt;
        nyaw = just_velocities ? r.yaw : fref::bound_angle(r.yaw + r.om * dt);
        nbx = r.bvx + g0 / r.mass * dt; nby = r.bvy + g1 / r.mass * dt;
        nom = r.om + torque / inertia * dt;
        const float sp = sqrtf(nbx * nbx + nby * nby);
        if (sp > r.vd) { nbx = nbx / sp * r.vd; nby = nby / sp * r.vd; }
        float s2, c2;
        sincosf(nyaw, &s2, &c2);
        nvx = c2 * nbx - s2 * nby; nvy = s2 * nbx + c2 * nby;
    }
    r.px = npx; r.py = npy; r.yaw = nyaw; r.vx = nvx; r.vy = nvy; r.bvx = nbx; r.bvy = nby; r.om = nom;
}

} // namespace rmodel
