// lookahead_math.h -- the robot's one-step look-ahead, stated once for the five kernels that turn the robot row, an action and a human's rows
// into the network's input row: k_lookahead (lookahead.hip), which writes the rows to HBM; k_value_net_worlds (value_net_worlds.hip),
// k_value_net_lstm_worlds and k_value_net_lstm_worlds_bf16 (value_net_lstm_worlds.h), whose loaders generate them in LDS from the worlds'
// rows; and k_value_net_state (value_net_state.hip), whose rows are the look-ahead's of a step of no length.  First the arithmetic (la_step,
// la_frame, la_reward, la_row_quad), then what the generating loaders share around it: the frame and its slots, the worlds' rows
// (LaWorlds), the frame-and-reward table of a job (la_job_table), the row of a world's human (la_world_quad) and the hand-out of a row's
// four column quads to the four wavefronts (la_wave_quad).
// Replaces compute_rotated_states_and_reward + transform_state_to_agent_centric (crowd_nav/policy/cadrl.py:42-83, :13-39).
//
// The kernels must agree to the last bit, and hipcc contracts a * b + c * d by context.  Every function therefore switches the
// contraction off and writes the fused operations out: a * b + c * d is fmaf(a, b, c * d) and a + b * c is fmaf(b, c, a) -- the
// operations k_lookahead compiled to before this header existed (first product fused, second one rounded), so its output keeps its bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <type_traits>

namespace {

// a frame in LDS: the action, the robot's next position, the rotation into the agent-centric frame, the distance to the goal, the reward
constexpr int LA_FRAME_FLOATS = 8;
enum { LA_AX, LA_AY, LA_NRX, LA_NRY, LA_COS, LA_SIN, LA_DG, LA_REWARD };

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

// the frame of the step along (ax, ay) into f: every slot but LA_REWARD
__device__ __forceinline__ void la_store_frame(float* f, const LaStep& st, float ax, float ay)
{
    f[LA_AX] = ax; f[LA_AY] = ay; f[LA_NRX] = st.nrx; f[LA_NRY] = st.nry; f[LA_DG] = st.dg;
    la_frame(st, f[LA_COS], f[LA_SIN]);
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
    const float ax = f[LA_AX], ay = f[LA_AY], cr = f[LA_COS], sr = f[LA_SIN];
    if constexpr (Q == 0) return make_float4(f[LA_DG], rvd, 0.0f, rr);
    else if constexpr (Q == 1) {
        const float hx = q[0] - f[LA_NRX], hy = q[1] - f[LA_NRY];
        return make_float4(la_dot(ax, cr, ay, sr), la_cross(ay, cr, ax, sr), la_dot(hx, cr, hy, sr), la_cross(hy, cr, hx, sr));
    } else if constexpr (Q == 2) {
        const float hx = q[0] - f[LA_NRX], hy = q[1] - f[LA_NRY];
        const float hvx = headed ? q[3] : q[2], hvy = headed ? q[4] : q[3];
        return make_float4(la_dot(hvx, cr, hvy, sr), la_cross(hvy, cr, hvx, sr), hr, sqrtf(la_dot(hx, hx, hy, hy)));
    } else
        return make_float4(rr + hr, headed ? q[2] - 0.0f : 0.0f, headed ? q[5] : 0.0f, 0.0f);
}

// The network's row of a world's CURRENT state (what a trainer stores: CADRL.transform / MultiHumanRL.transform, cadrl.py:305-345) is, by
// definition, the look-ahead row above for the action (robot vx, vy), a step of dt = 0 -- fmaf(ax, 0, px) is px exactly -- and the humans'
// current rows as their next ones.  The frame of that row (LA_REWARD is the caller's), for
// k_value_net_state (value_net_state.hip); la_row_quad then takes the human's current (px, py, vx, vy | x, y, yaw, Vx, Vy, Omega).
__device__ __forceinline__ void la_state_frame(const float* __restrict__ rb, float* f)
{
    const float ax = rb[2], ay = rb[3];
    la_store_frame(f, la_step(rb, ax, ay, 0.0f), ax, ay);
}

// Wavefront Q of the workgroup's four writes columns [4 Q, 4 Q + 4) of a loader's rows: f(std::integral_constant<int, Q>) on wavefront Q.
template <class F>
__device__ __forceinline__ void la_wave_quad(F&& f)
{
    switch (threadIdx.x >> 6) {
    case 0: f(std::integral_constant<int, 0>{}); break;
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    default: f(std::integral_constant<int, 3>{}); break;
    }
}

// The worlds' rows as cs_lookahead takes them, for the kernels that generate a job's rows in LDS instead of reading its tensor.
struct LaWorlds {
    const float* __restrict__ actions;     // [A][2]
    const float* __restrict__ next;        // [W][n][4 | 6]
    const float* __restrict__ cur;         // [W][n][5 | 7]
    const float* __restrict__ robot;       // [W][rstride]
    float* __restrict__ rewards_out;       // [W][A] or null
    int rstride, headed, A, n;
};

// The frame-and-reward table of a job: its ng <= 64 groups from gbase on, group g being action g % A of world g / A (a job crosses worlds, so
// both are per group).  Lane k of wavefront 0 computes the frame of group gbase + k into frames[k], lane k of wavefront 1 its reward (the
// swept collision loop over the humans) into that frame's LA_REWARD and into rewards_out.  The caller's next barrier publishes both.
// I: the integer type in which the kernel counts its groups (int in value_net_body.inc, long in the recurrent bodies); the division is
// unsigned and 32 bits wide in both (W * A is below 2^30: check_decide_args) -- with I = long in k_value_net_worlds it cost 36 bytes of
// scratch a lane, and with a signed division in int the recurrent float32 kernels ran 0.3 - 0.5 % slower (HISTORY.md).
template <class I>
__device__ __forceinline__ void la_job_table(const LaWorlds& s, float* frames, I gbase, int ng, float dt)
{
    const int wave = threadIdx.x >> 6, k = threadIdx.x & 63;
    if (wave < 2 && k < ng) {
        const I g = gbase + k, w = (unsigned)g / (unsigned)s.A;
        const int a = (int)(g - w * s.A);
        const float* rb = s.robot + (long)w * s.rstride;
        const float ax = s.actions[2 * a], ay = s.actions[2 * a + 1];
        const LaStep st = la_step(rb, ax, ay, dt);
        float* f = frames + LA_FRAME_FLOATS * k;
        if (wave == 0) la_store_frame(f, st, ax, ay);
        else {
            const int cc = s.headed ? 7 : 5;
            const float rew = la_reward(s.cur + (long)w * s.n * cc, s.n, cc, rb, ax, ay, dt, st.dg);
            f[LA_REWARD] = rew;
            if (s.rewards_out) s.rewards_out[g] = rew;
        }
    }
}

// columns [4 Q, 4 Q + 4) of the row of human j of world w under the action of `frame`: the human's next row, its radius from the current one
template <int Q>
__device__ __forceinline__ float4 la_world_quad(const LaWorlds& s, const float* frame, long w, int j)
{
    const float* rb = s.robot + w * s.rstride;
    const float* q = s.next + (w * s.n + j) * (s.headed ? 6 : 4);
    const float hr = s.cur[(w * s.n + j) * (s.headed ? 7 : 5) + 4];
    return la_row_quad<Q>(frame, q, hr, rb[7], rb[4], s.headed != 0);
}

} // namespace
