// orca_solve.h -- the pieces of the RVO2 restatement that every ORCA translation unit needs, stated once: the exact arithmetic
// (ieee_div / ieee_sqrt and the FM-templated operators), det2, the agent-agent half-plane (orca_line), the per-lane LDS column
// accessor (Lines) and the generic linearProgram1 / 2 / 3.  Included by orca.hip (crowd, robot-model and big-world kernels) and by
// policy_orca.hip (the robot's ORCA policy).  Floating-point contraction is off from here to the end of the including file:
// the restatement follows oracle/orca_oracle.c operation for operation.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr float RVO_EPSILON = 0.00001f;

__device__ __forceinline__ float det2(float ax, float ay, float bx, float by) { return ax * by - ay * bx; }
// IEEE divide / sqrt are kept on purpose: with v_rcp_f32 / v_sqrt_f32 the kernel ran 1.3x faster but left the
// 1e-5 band around the C restatement (the LP's branch decisions amplify ulp-level differences).
//
// ieee_div / ieee_sqrt: the correctly rounded quotient / root by the very FMA sequences hipcc emits for `a / b` and
// sqrtf(x) on gfx950 -- v_rcp_f32, one Newton step on the reciprocal, the quotient refined twice (the last refinement is
// what v_div_fmas_f32 does); v_sqrt_f32 corrected by the two one-ulp residual tests -- WITHOUT the range handling around
// them (v_div_scale_f32 x2 + v_div_fixup_f32; the 2^32 pre-scale of sqrt), which only acts on operands whose exponents lie
// outside [-96, 96] or so: the linear programmes work on velocities, unit directions and their determinants (|x| in
// 1e-30 .. 1e8; quotients of parallel lines, the one place a denominator can vanish, are discarded by a select).  8 VALU
// instructions instead of 11, 9 instead of 13.  tests/test_gpu_orca.py::test_ieee_div_sqrt_sequences_are_correctly_rounded
// compares both with the compiler's operators on 2^31 operand pairs drawn from that range, bit for bit.
__device__ __forceinline__ float ieee_div(float a, float b)
{
    float r = __builtin_amdgcn_rcpf(b);
    const float e0 = fmaf(-b, r, 1.0f);
    r = fmaf(e0, r, r);
    float q = a * r;
    const float e1 = fmaf(-b, q, a);
    q = fmaf(e1, r, q);
    const float e2 = fmaf(-b, q, a);
    return fmaf(e2, r, q);
}
__device__ __forceinline__ float ieee_sqrt(float x)
{
    const float s = __builtin_amdgcn_sqrtf(x);
    const float dn = __uint_as_float(__float_as_uint(s) - 1u), up = __uint_as_float(__float_as_uint(s) + 1u);
    const float rd = fmaf(-dn, s, x);
    const float t = (rd <= 0.0f) ? dn : s;      // (0 >= residual): the root was rounded up, step down
    const float ru = fmaf(-up, s, x);
    const float res = (ru > 0.0f) ? up : t;     // the root was rounded down, step up
    return (x == 0.0f) ? x : res;               // +-0 stay (s - 1 ulp of 0 is not a number to step to)
}

// ---- the arithmetic the register-resident build is instantiated with (template parameter FM of everything below) -------------
// FM = 0: "exact": IEEE divide / square root, no FMA contraction -- the restatement's operations on the restatement's operands,
//         bit-identical to oracle/orca_oracle.c (the bit-identity reference; cs_worlds.orca_math = CS_ORCA_MATH_EXACT, the default).
// FM = 1: "fast": v_rcp_f32 / v_sqrt_f32 / v_rsq_f32 (1 ulp each) instead of the 8- and 9-instruction correctly rounded sequences.
// FM = 2: "fast + fma": and the 2 x 2 determinants, dot products and point + t * direction as mul + fma (one rounding less).
// north_star asks for 1e-5 on positions / velocities per step, not for bits, and the restatement cannot be pinned on rvo2 anyway;
// tests/test_gpu_orca_fast.py measures the fast builds per substep from re-synchronised state against the exact restatement and
// accounts for every agent-substep beyond 1e-5.
template <int FM> __device__ __forceinline__ float odiv(float a, float b)
{
    if constexpr (FM != 0) return a * __builtin_amdgcn_rcpf(b); else return ieee_div(a, b);
}
template <int FM> __device__ __forceinline__ float orcp(float b)
{
    if constexpr (FM != 0) return __builtin_amdgcn_rcpf(b); else return ieee_div(1.0f, b);
}
template <int FM> __device__ __forceinline__ float osqrt(float x)
{
    if constexpr (FM != 0) return __builtin_amdgcn_sqrtf(x); else return ieee_sqrt(x);
}
// 1 / sqrt(x): RVO2 normalises a vector by the reciprocal of its length (Vector2 / float)
template <int FM> __device__ __forceinline__ float orsqrt(float x)
{
    if constexpr (FM != 0) return __builtin_amdgcn_rsqf(x); else return ieee_div(1.0f, ieee_sqrt(x));
}
// a.x * b.y - a.y * b.x
template <int FM> __device__ __forceinline__ float odet(float ax, float ay, float bx, float by)
{
    if constexpr (FM >= 2) return fmaf(ax, by, -(ay * bx)); else return ax * by - ay * bx;
}
// a.x * b.x + a.y * b.y
template <int FM> __device__ __forceinline__ float odot(float ax, float ay, float bx, float by)
{
    if constexpr (FM >= 2) return fmaf(ax, bx, ay * by); else return ax * bx + ay * by;
}
// p + t * d
template <int FM> __device__ __forceinline__ float omad(float t, float d, float p)
{
    if constexpr (FM >= 2) return fmaf(t, d, p); else return p + t * d;
}

// per-lane column views into LDS: element i of lane tid lives at base[i * T + tid]
struct Lines {
    float4* p;
    int T, tid;
    __device__ __forceinline__ float4 get(int i) const { return p[i * T + tid]; }
    __device__ __forceinline__ void set(int i, float4 v) const { p[i * T + tid] = v; }
};

// RVO2 linearProgram1
__device__ bool lp1(const Lines& L, int lineNo, float radius, float ox, float oy, bool dirOpt, float& rx, float& ry)
{
    const float4 ln = L.get(lineNo); // x,y = point ; z,w = direction
    const float dot = ln.x * ln.z + ln.y * ln.w;
    const float disc = dot * dot + radius * radius - (ln.x * ln.x + ln.y * ln.y);
    if (disc < 0.0f) return false;
    const float sq = sqrtf(disc);
    float tL = -dot - sq, tR = -dot + sq;
    for (int i = 0; i < lineNo; ++i) {
        const float4 li = L.get(i);
        const float den = det2(ln.z, ln.w, li.z, li.w);
        const float num = det2(li.z, li.w, ln.x - li.x, ln.y - li.y);
        if (fabsf(den) <= RVO_EPSILON) {
            if (num < 0.0f) return false;
            continue;
        }
        const float t = num / den;
        if (den >= 0.0f) tR = fminf(tR, t); else tL = fmaxf(tL, t);
        if (tL > tR) return false;
    }
    float t;
    if (dirOpt) {
        t = (ox * ln.z + oy * ln.w > 0.0f) ? tR : tL;
    } else {
        t = ln.z * (ox - ln.x) + ln.w * (oy - ln.y);
        if (t < tL) t = tL; else if (t > tR) t = tR;
    }
    rx = ln.x + t * ln.z;
    ry = ln.y + t * ln.w;
    return true;
}

// RVO2 linearProgram2
__device__ int lp2(const Lines& L, int nl, float radius, float ox, float oy, bool dirOpt, float& rx, float& ry)
{
    if (dirOpt) { rx = ox * radius; ry = oy * radius; }
    else if (ox * ox + oy * oy > radius * radius) {
        const float nrm = sqrtf(ox * ox + oy * oy);
        const float inv = 1.0f / nrm;             // RVO2's Vector2 / float multiplies by the reciprocal (Vector2.h)
        rx = ox * inv * radius; ry = oy * inv * radius;
    } else { rx = ox; ry = oy; }
    for (int i = 0; i < nl; ++i) {
        const float4 li = L.get(i);
        if (det2(li.z, li.w, li.x - rx, li.y - ry) > 0.0f) {
            const float tx = rx, ty = ry;
            if (!lp1(L, i, radius, ox, oy, dirOpt, rx, ry)) { rx = tx; ry = ty; return i; }
        }
    }
    return nl;
}

// RVO2 linearProgram3: the first numObst lines (static obstacles) are hard constraints, copied unprojected
__device__ void lp3(const Lines& L, const Lines& P, int nl, int numObst, int begin, float radius, float& rx, float& ry)
{
    float distance = 0.0f;
    for (int i = begin; i < nl; ++i) {
        const float4 li = L.get(i);
        if (det2(li.z, li.w, li.x - rx, li.y - ry) > distance) {
            int np = 0;
            for (int j = 0; j < numObst; ++j) P.set(np++, L.get(j));
            for (int j = numObst; j < i; ++j) {
                const float4 lj = L.get(j);
                float4 ln;
                const float d = det2(li.z, li.w, lj.z, lj.w);
                if (fabsf(d) <= RVO_EPSILON) {
                    if (li.z * lj.z + li.w * lj.w > 0.0f) continue;
                    ln.x = 0.5f * (li.x + lj.x); ln.y = 0.5f * (li.y + lj.y);
                } else {
                    const float s = det2(lj.z, lj.w, li.x - lj.x, li.y - lj.y) / d;
                    ln.x = li.x + s * li.z; ln.y = li.y + s * li.w;
                }
                const float ex = lj.z - li.z, ey = lj.w - li.w;
                const float en = sqrtf(ex * ex + ey * ey);
                const float inv = 1.0f / en;
                ln.z = ex * inv; ln.w = ey * inv;
                P.set(np++, ln);
            }
            const float tx = rx, ty = ry;
            if (lp2(P, np, radius, -li.w, li.z, true, rx, ry) < np) { rx = tx; ry = ty; }
            distance = det2(li.z, li.w, li.x - rx, li.y - ry);
        }
    }
}

// One ORCA half-plane (RVO2 Agent::computeNewVelocity, agent part): q = (x, y, vx, vy) of the neighbour,
// R = combined radius.  Returns (point.x, point.y, direction.x, direction.y).
// One agent-agent ORCA half-plane (RVO2 Agent::computeNewVelocity).  RVO2's three cases -- projection on the cut-off circle,
// on a leg, and the collision case (cut-off circle of the time step) -- each take one square root and one reciprocal of
// different arguments; the arguments are selected first, so a lane pays one IEEE sqrt and one IEEE divide whatever cases the
// wavefront mixes, with the very same operations on the very same operands as the case it is in.  invDt = 1 / timeStep.
// (FM: the decisions -- collision, cut-off circle or leg, which leg -- are taken on the same uncontracted quantities in every build;
//  only the root and the reciprocal differ.)
template <int FM = 0>
__device__ __forceinline__ float4 orca_line(float px, float py, float vx, float vy, const float4 q, float R, float invT, float invDt)
{
    const float rpx = q.x - px, rpy = q.y - py;
    const float rvx = vx - q.z, rvy = vy - q.w;
    const float distSq = rpx * rpx + rpy * rpy;
    const float RSq = R * R;
    const bool coll = !(distSq > RSq);
    const float kT = coll ? invDt : invT;
    const float wx = rvx - kT * rpx, wy = rvy - kT * rpy;
    const float wLenSq = wx * wx + wy * wy;
    const float dot1 = wx * rpx + wy * rpy;
    const bool circ = coll | ((dot1 < 0.0f) & (dot1 * dot1 > RSq * wLenSq));   // (no short circuit: three compares, no branch per line)
    const float root = osqrt<FM>(circ ? wLenSq : distSq - RSq);   // |w|  or  the leg length
    const float den = circ ? root : distSq;
    float inv;
    if constexpr (FM != 0) inv = __builtin_amdgcn_rcpf(den);           // (v_rcp_f32(+0) = +inf)
    else inv = (den == 0.0f) ? INFINITY : ieee_div(1.0f, den);          // (w == 0 exactly: 1 / +0 as the operator gives it)
    // cut-off circle (of the time horizon, or of the time step when the discs overlap)
    const float uwx = wx * inv, uwy = wy * inv;
    const float sc = R * kT - root;
    // legs
    const bool left = det2(rpx, rpy, wx, wy) > 0.0f;
    // RVO2: left leg (rp.x * leg - rp.y * R, rp.x * R + rp.y * leg) / distSq, right leg -(rp.x * leg + rp.y * R, -rp.x * R + rp.y * leg) / distSq:
    // the right leg is the left one with -leg for leg, bit for bit (negation commutes with every rounding here)
    const float sroot = left ? root : -root;
    const float lx = (rpx * sroot - rpy * R) * inv;
    const float ly = (rpx * R + rpy * sroot) * inv;
    const float dot2 = rvx * lx + rvy * ly;
    const float dx = circ ? uwy : lx, dy = circ ? -uwx : ly;
    const float ux = circ ? sc * uwx : dot2 * lx - rvx, uy = circ ? sc * uwy : dot2 * ly - rvy;
    return make_float4(vx + 0.5f * ux, vy + 0.5f * uy, dx, dy);
}

} // namespace
