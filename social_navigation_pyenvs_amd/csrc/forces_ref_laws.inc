// forces_ref_laws.inc -- the policies and the four laws of forces_ref.h, which includes this text once per contraction mode
// (FREF_MODE: the namespace, fused or strict; FREF_FP: nothing, or the pragma that turns contraction off in a function body).
namespace fref { namespace FREF_MODE {

// unit(): distance dn, unit vector n and the distance dov the body overlap is taken from.  Plain sqrt and divide, the library's exp:
template <class S> struct Libm {
    using T = S;
    static __device__ __forceinline__ void unit(T dx, T dy, T& dn, T& nx, T& ny, T& dov)
    {
        FREF_FP
        dn = sqrt(dx * dx + dy * dy);
        nx = dx / dn; ny = dy / dn; dov = dn;
    }
    static __device__ __forceinline__ T exp_rep(T x) { return exp(x); }
    static __device__ __forceinline__ T atan2_th(T y, T x) { return atan2(y, x); }
};
// float64: the two atan2 of Moussaid's theta_ij correctly rounded (atan2_cr.h: their last bit decides sign(theta_ij) in a crowd at
// rest; the reference's C library rounds them correctly, the device library's atan2 is an ulp off now and then)
struct CrD : Libm<double> {
    static __device__ __forceinline__ double atan2_th(double y, double x) { return crmath::atan2_cr(y, x); }
};
// single-instruction rsq / exp in the repulsion terms as in the crowd kernel (<= 1 ulp each, two orders of magnitude inside the parity
// bar), coincident agents finite, the overlap from a Newton-refined distance: one ulp of dn is 1.4e-5 of the k1 / k2 force
// (stepcommon.h dist_refined)
struct FastF {
    using T = float;
    static __device__ __forceinline__ void unit(float dx, float dy, float& dn, float& nx, float& ny, float& dov)
    {
        FREF_FP
        const float d2h = fmaxf(dx * dx + dy * dy, 1e-30f);
        const float dinv = __builtin_amdgcn_rsqf(d2h);
        dn = d2h * dinv;
        nx = dx * dinv; ny = dy * dinv;
        dov = fmaf(fmaf(-dn, dn, d2h), 0.5f * dinv, dn);
    }
    static __device__ __forceinline__ float exp_rep(float x) { return __expf(x); }
    static __device__ __forceinline__ float atan2_th(float y, float x) { return atan2f(y, x); }
};

// Pairwise social force (forces.py:63-128, 153-218; forces_parallel.py:60-83, 109-130): the force ON agent 1 (p1, v1) FROM agent 2;
// rij = both radii + both safety spaces
template <class M, class T = typename M::T>
__device__ __forceinline__ void pair_force(int soc, const T* P, T p1x, T p1y, T v1x, T v1y, T p2x, T p2y, T v2x, T v2y, T rij, T& fx, T& fy)
{
    FREF_FP
    T dn, nx, ny, dov;
    M::unit(p1x - p2x, p1y - p2y, dn, nx, ny, dov);
    const T rd = rij - dn;
    const T comp = pos(rij - dov);
    if (soc == 2) {
        const T ivx = P[12] * (v1x - v2x) - nx, ivy = P[12] * (v1y - v2y) - ny;
        const T inorm = sqrt(ivx * ivx + ivy * ivy);
        const T ix = ivx / inorm, iy = ivy / inorm;
        const T th = bound_angle(M::atan2_th(ny, nx) - M::atan2_th(iy, ix) + T(M_PI));
        const T k = (th > 0) ? T(1) : ((th < 0) ? T(-1) : T(0));
        const T hx = -iy, hy = ix;
        const T F = P[13] * inorm;
        const T dvh = (v2x - v1x) * hx + (v2y - v1y) * hy;
        const T e0 = P[9] * exp(-dn / F);
        const T t1 = P[15] * F * th, t2 = P[14] * F * th;
        const T e1 = exp(-(t1 * t1)), e2 = k * exp(-(t2 * t2));
        fx = -(e0 * (e1 * ix + e2 * hx) + P[10] * comp * ix + P[11] * comp * dvh * hx);
        fy = -(e0 * (e1 * iy + e2 * hy) + P[10] * comp * iy + P[11] * comp * dvh * hy);
    } else {
        const T tx = -ny, ty = nx;
        const T dv = (v2x - v1x) * tx + (v2y - v1y) * ty;
        const T fn = P[1] * M::exp_rep(rd / P[3]) + P[10] * comp;
        T ft = P[11] * comp * dv;
        if (soc == 1) ft += P[5] * M::exp_rep(rd / P[7]);
        fx = fn * nx + ft * tx;
        fy = fn * ny + ft * ty;
    }
}

// One wall's term of the obstacle force (forces.py:27-53, forces_parallel.py:136-162), added to (fox, foy): n the unit vector from the
// wall's closest point to the agent, rd = radius + safety space - distance, v the agent's velocity.  Guo adds the tangential wall law.
template <class T>
__device__ __forceinline__ void wall_term(int soc, const T* P, T nx, T ny, T rd, T vx, T vy, T& fox, T& foy)
{
    FREF_FP
    const T tx = -ny, ty = nx;
    const T dv = -(vx * tx + vy * ty);
    const T comp = pos(rd);
    const T fn = P[2] * exp(rd / P[4]) + P[10] * comp;
    const T ft = (soc == 1) ? (-P[6] * exp(rd / P[8]) - P[11] * comp) * dv : -P[11] * comp * dv;
    fox += fn * nx + ft * tx;
    foy += fn * ny + ft * ty;
}

// Obstacle force of the single-agent functions (forces.py:27-53): one closest point per polygon (the LAST nearest segment point, `<=`,
// obstacle.py:53-66), Helbing averaged over the polygons, Guo a plain sum.  ob: [O][Smax][2][2] NaN-padded; not read when O <= 0 (the entry points refuse O > 0 without a table: check_obstacles).
__device__ __forceinline__ void obstacle_force(const float* ob, int O, int Smax, int soc, const float* P, float px, float py, float vx, float vy,
                                               float reach, float& fox, float& foy)
{
    FREF_FP
    fox = 0.0f; foy = 0.0f;
    for (int o = 0; o < O; ++o) {
        float bx = 0.0f, by = 0.0f, bd = 10000.0f;
        for (int sg = 0; sg < Smax; ++sg) {
            const float* q = ob + ((long)o * Smax + sg) * 4;
            const float ax = q[0], ay = q[1], ex = q[2], ey = q[3];
            if (isnan(ax) || isnan(ay) || isnan(ex) || isnan(ey)) continue;
            const float sx = ex - ax, sy = ey - ay;
            const float len = sqrtf(sx * sx + sy * sy);
            float t = ((px - ax) * sx + (py - ay) * sy) / (len * len);
            t = fminf(fmaxf(0.0f, t), 1.0f);
            const float hx = ax + t * sx, hy = ay + t * sy;
            const float d = sqrtf((hx - px) * (hx - px) + (hy - py) * (hy - py));
            if (d <= bd) { bx = hx; by = hy; bd = d; }
        }
        const float dx = px - bx, dy = py - by;
        const float dn = sqrtf(dx * dx + dy * dy);
        wall_term(soc, P, dx / dn, dy / dn, reach - dn, vx, vy, fox, foy);
    }
    if (O > 0 && soc != 1) { fox /= (float)O; foy /= (float)O; }
}

// Desired force (forces.py:9-16, forces_parallel.py:23-40).  Within one radius of the goal (fdx, fdy) stays what it was: the
// single-agent functions keep the previous substep's force there, the parallel ones hand in zero.
template <class T>
__device__ __forceinline__ void desired_force(T gx, T gy, T px, T py, T vx, T vy, T radius, T mass, T vd, T relaxation_time, T& fdx, T& fdy)
{
    FREF_FP
    const T ddx = gx - px, ddy = gy - py;
    const T dist = sqrt(ddx * ddx + ddy * ddy);
    if (dist > radius) {
        fdx = mass * (ddx / dist * vd - vx) / relaxation_time;
        fdy = mass * (ddy / dist * vd - vy) / relaxation_time;
    }
}

// The headed models: torque (forces.py:279-290) towards the desired force (Farina) or the total force ("new"), and the force in the
// body frame (sn, cs of the heading): g0 = f . R[:,0],  g1 = ko * o . R[:,1] - kd * body_velocity[1], with the caller's sums
// f = (fd + fo) + fs and o = fo + fs
template <class T>
__device__ __forceinline__ void headed_force(bool torque_new, const T* P, T inertia, T fdx, T fdy, T fx, T fy, T ox, T oy, T yaw, T om, T bvy,
                                             T sn, T cs, T& g0, T& g1, T& torque)
{
    FREF_FP
    const T tx = torque_new ? fx : fdx, ty = torque_new ? fy : fdy;
    const T tn = sqrt(tx * tx + ty * ty);
    const T k_theta = inertia * P[19] * tn;
    const T k_omega = inertia * (T(1) + P[18]) * sqrt(P[19] * tn / P[18]);
    torque = -k_theta * bound_angle(yaw - atan2(ty, tx)) - k_omega * om;
    g0 = fx * cs + fy * sn;
    g1 = P[16] * (ox * -sn + oy * cs) - P[17] * bvy;
}

}} // namespace fref::FREF_MODE
