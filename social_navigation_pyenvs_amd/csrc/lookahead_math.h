// lookahead_math.h -- the arithmetic of the robot's one-step look-ahead, stated once for the two kernels that evaluate it: k_lookahead
// (lookahead.hip), which writes the rows to HBM, and k_value_net_worlds (value_net.hip), whose tile loader generates them in LDS -- and, at
// the end of this header, for k_value_net_state (value_net_state.hip), whose rows are the look-ahead's of a step of no length.
// Replaces compute_rotated_states_and_reward + transform_state_to_agent_centric (crowd_nav/policy/cadrl.py:42-83, :13-39).
//
// The two kernels must agree to the last bit, and hipcc contracts a * b + c * d by context.  Every function therefore switches the
// contraction off and writes the fused operations out: a * b + c * d is fmaf(a, b, c * d) and a + b * c is fmaf(b, c, a) -- the
// operations k_lookahead compiled to before this header existed (first product fused, second one rounded), so its output keeps its bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace {

constexpr int LA_FRAME_FLOATS = 8;     // a frame in LDS: ax, ay, nrx, nry, cos, sin, dg, reward

// a * b + c * d and a * b - c * d as the look-ahead rounds them
__device__ __forceinline__ float la_dot(float a, float b, float c, float d)
{
#pragma clang fp contract(off)
    return fmaf(a, b, c * d);
}

__device__ __forceinline__ float la_cross(float a, float b, float c, float d)
{
#pragma clang fp contract(off)
    return fmaf(a, b, -(c * d));
}

// the robot one step along action (ax, ay): its next position, the vector to its goal and that vector's length dg (cadrl.py:22-24)
struct LaStep { float nrx, nry, gdx, gdy, dg; };

__device__ __forceinline__ LaStep la_step(const float* __restrict__ rb, float ax, float ay, float dt)
{
#pragma clang fp contract(off)
    LaStep s;
    s.nrx = fmaf(ax, dt, rb[0]);
    s.nry = fmaf(ay, dt, rb[1]);
    s.gdx = rb[5] - s.nrx;
    s.gdy = rb[6] - s.nry;
    s.dg = sqrtf(la_dot(s.gdx, s.gdx, s.gdy, s.gdy));
    return s;
}

// the agent-centric frame: x axis from the next robot position to the goal (cadrl.py:22)
__device__ __forceinline__ void la_frame(const LaStep& s, float& cr, float& sr)
{
    const float rot = atan2f(s.gdy, s.gdx);
    cr = cosf(rot);
    sr = sinf(rot);
}

// the reward of the step (cadrl.py:56-72, utils.py:22-36): the swept collision test over the n current humans `curw` [n][cc], sequential
// with the reference's early break, then the three literals
__device__ __forceinline__ float la_reward(const float* __restrict__ curw, int n, int cc, const float* __restrict__ rb, float ax, float ay, float dt,
                                           float dg)
{
#pragma clang fp contract(off)
    const float rpx = rb[0], rpy = rb[1], rr = rb[4];
    float dmin = 9223372036854775807.0f;
    bool collision = false;
    for (int j = 0; j < n; ++j) {
        const float* c = curw + (long)j * cc;
        const float x1 = c[0] - rpx, y1 = c[1] - rpy;
        const float x2 = fmaf(c[2] - ax, dt, x1), y2 = fmaf(c[3] - ay, dt, y1);
        const float px = x2 - x1, py = y2 - y1;
        float d;
        if (px == 0.0f && py == 0.0f) d = sqrtf(la_dot(x1, x1, y1, y1));
        else {
            float u = la_dot(0.0f - x1, px, 0.0f - y1, py) / la_dot(px, px, py, py);
            u = u > 1.0f ? 1.0f : (u < 0.0f ? 0.0f : u);
            const float qx = fmaf(u, px, x1), qy = fmaf(u, py, y1);
            d = sqrtf(la_dot(qx, qx, qy, qy));
        }
        const float dist = d - c[4] - rr;
        if (dist < 0.0f) { collision = true; break; }
        else if (dist < dmin) dmin = dist;
    }
    float rew = 0.0f;
    if (collision) rew = -0.25f;
    else if (dg < rr) rew = 1.0f;
    else if (dmin < 0.2f) rew = (dmin - 0.2f) * 0.5f * dt;
    return rew;
}

// Columns [4 Q, 4 Q + 4) of the network's input row of one (action, human): `f` the action's frame (LA_FRAME_FLOATS), `q` the human's
// next row (px, py, vx, vy | x, y, yaw, Vx, Vy, Omega), hr its radius, rvd / rr the robot's v_pref and radius.  Columns:
// dg, v_pref, theta (0: holonomic), radius, vx, vy, px1, py1, vx1, vy1, radius1, da, radius + radius1 [, theta1, omega1]; zero beyond.
template <int Q>
__device__ __forceinline__ float4 la_row_quad(const float* f, const float* __restrict__ q, float hr, float rvd, float rr, bool headed)
{
#pragma clang fp contract(off)
    const float ax = f[0], ay = f[1], cr = f[4], sr = f[5];
    if constexpr (Q == 0) return make_float4(f[6], rvd, 0.0f, rr);
    else if constexpr (Q == 1) {
        const float hx = q[0] - f[2], hy = q[1] - f[3];
        return make_float4(la_dot(ax, cr, ay, sr), la_cross(ay, cr, ax, sr), la_dot(hx, cr, hy, sr), la_cross(hy, cr, hx, sr));
    } else if constexpr (Q == 2) {
        const float hx = q[0] - f[2], hy = q[1] - f[3];
        const float hvx = headed ? q[3] : q[2], hvy = headed ? q[4] : q[3];
        return make_float4(la_dot(hvx, cr, hvy, sr), la_cross(hvy, cr, hvx, sr), hr, sqrtf(la_dot(hx, hx, hy, hy)));
    } else
        return make_float4(rr + hr, headed ? q[2] - 0.0f : 0.0f, headed ? q[5] : 0.0f, 0.0f);
}

// The network's row of a world's CURRENT state (what a trainer stores: CADRL.transform / MultiHumanRL.transform, cadrl.py:305-345) is, by
// definition, the look-ahead row above for the action (robot vx, vy), a step of dt = 0 -- fmaf(ax, 0, px) is px exactly -- and the humans'
// current rows as their next ones.  The frame of that row (f[0..6] of LA_FRAME_FLOATS; f[7], the reward, is the caller's), for
// k_value_net_state (value_net_state.hip); la_row_quad then takes the human's current (px, py, vx, vy | x, y, yaw, Vx, Vy, Omega).
__device__ __forceinline__ void la_state_frame(const float* __restrict__ rb, float* f)
{
    const float ax = rb[2], ay = rb[3];
    const LaStep st = la_step(rb, ax, ay, 0.0f);
    f[0] = ax; f[1] = ay; f[2] = st.nrx; f[3] = st.nry; f[6] = st.dg;
    la_frame(st, f[4], f[5]);
}

} // namespace
