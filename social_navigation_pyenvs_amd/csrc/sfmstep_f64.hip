// sfmstep_f64.hip -- the SFM / HSFM substep in FLOAT64 (the reference's PRECISION = np.float64): cs_step_f64,
// cs_update_humans_parallel_f64, cs_peek_f64 of include/crowdstep.h.  An opt-in arithmetic beside the float32 step kernels
// (DESIGN.md 4.6): a float32 world leaves the reference's trajectory by centimetres to metres over an episode, this one by ~1e-10 m.
//
// Semantics: update_humans_parallel (social_gym/src/forces_parallel.py:185-284) with the substep loop of SocialNavGym.step and the
// respawn rule (motion_model_manager.py:354-367, 407-422), operation for operation as oracle/sfm_step.inc states them -- the same
// products, sums and quotients in the same order, so that the only differences from the CPU restatement are those of the device
// library's exp / atan2 / sin / cos.
//
// Mapping: one wavefront per world (up to 64 rows), lane = row, four worlds per workgroup.  The columns the pair forces read
// (px, py, vx, vy, r, safety and the refreshed linear velocity) are published per substep in LDS, column-major per world: the
// partner loop reads ONE address per iteration across the wavefront (a broadcast, no bank conflict).  Every lane walks all its
// partners; under all_params_equal the lower-indexed row of a pair is the first argument and the higher one takes the negated
// force, as the reference fills F[i][j] = f, F[j][i] = -f.  The row stays in registers between the fused substeps.
//
// Arithmetic: IEEE division and sqrt, the device library's double exp / atan2 / sin / cos / fmod -- except the two atan2 of Moussaid's
// theta_ij, which are correctly rounded (atan2_cr.h: their last bit decides sign(theta_ij) in a crowd at rest) --, no contraction (the
// pragma below: the oracle is built with -ffp-contract=off), no float32 intermediate anywhere.  gfx950 only.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "common.h"
#include "crowdstep.h"
#include "forces_ref.h"

namespace {

constexpr int F64_WPB = 4;     // one-wavefront worlds per workgroup
constexpr int F64_COLS = 8;    // LDS columns per world: px, py, vx, vy, r, safety, refreshed vx, refreshed vy
enum { M64_COMMIT_GOALS = 1, M64_MUTATE_INPUT = 2, M64_PEEK = 4, M64_ROBOT_FROM_ARRAY = 8 };

// the compiler must not move a lane's LDS load above another lane's store (the hardware runs a wavefront's LDS operations in order)
#define F64_LDS_FENCE() do { asm volatile("" ::: "memory"); __builtin_amdgcn_wave_barrier(); } while (0)

struct Args64 {
    int W, n, rows, G, O, Smax, type, flags, mode, n_substeps;
    double* state;            // [W][rows][13]
    double* out;              // where the stepped rows go (== state for the in-place entries)
    double* goals;            // [W][n][G][2]
    const double* params;     // [W][n][20] or [n][20]
    const double* safety;     // [W][rows]
    const double* obstacles;  // [W][O][Smax][2][2] or shared
    double* robot;            // [W][13] or null
    const int32_t* world_flags;
    const double* action;     // [W][2] or null
    double* peek;             // [W][n][8]
    double dt, bx, by;
};

__device__ inline double norm2(double x, double y) { return sqrt(x * x + y * y); }

using fref::bound_angle;
namespace laws = fref::strict;   // the four laws with Libm<double> + correctly rounded theta_ij (forces_ref.h), no contraction

struct Body { double px, py, vx, vy, r, s; };

// forces_parallel.py:109-130 (= :60-83): force ON a FROM b with the 20 parameters P
template <int SOC>
__device__ inline void pair_force(const Body& A, const Body& B, const double (&P)[20], double& fx, double& fy)
{
    laws::pair_force<laws::CrD>(SOC, P, A.px, A.py, A.vx, A.vy, B.px, B.py, B.vx, B.vy, A.r + B.r + A.s + B.s, fx, fy);
}

template <int SOC, bool PEQ>
__global__ __launch_bounds__(64 * F64_WPB) void k_sfm_step_f64(const Args64 a)
{
    __shared__ double lds_all[F64_WPB][F64_COLS][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int w = blockIdx.x * F64_WPB + wave;
    if (w >= a.W) return;   // (no workgroup barrier anywhere: a wavefront owns its world and its LDS columns)
    double (*lds)[64] = lds_all[wave];

    const int n = a.n, rows = a.rows, G = a.G;
    const bool robot_row = rows > n;
    const bool valid = lane < rows, human = lane < n, is_robot = robot_row && lane == n;
    const int headed = a.type / 3;
    const double dt = a.dt;
    const bool robot_from_array = (a.mode & M64_ROBOT_FROM_ARRAY) != 0;

    // ---- the lane's row, its parameters, its goal list
    double px = 0, py = 0, th = 0, vx = 0, vy = 0, bvx = 0, bvy = 0, om = 0, r = 0, m = 1, gx = 0, gy = 0, vd = 0, sf = 0;
    if (valid) {
        const double* S = (is_robot && robot_from_array) ? a.robot + (long)w * 13 : a.state + ((long)w * rows + lane) * 13;
        px = S[0]; py = S[1]; th = S[2]; vx = S[3]; vy = S[4]; bvx = S[5]; bvy = S[6]; om = S[7];
        r = S[8]; m = S[9]; gx = S[10]; gy = S[11]; vd = S[12];
        sf = a.safety[(long)w * rows + lane];
    }
    const double* Pw = a.params + ((a.flags & CS_PARAMS_SHARED) ? 0 : (long)w * n * 20);
    double Pi[20], PP[20];   // the lane's own parameters; those of the pair forces (row 0's when all are equal: the reference's choice)
#pragma unroll
    for (int k = 0; k < 20; ++k) Pi[k] = human ? Pw[lane * 20 + k] : 1.0;
#pragma unroll
    for (int k = 0; k < 20; ++k) PP[k] = PEQ ? Pw[k] : Pi[k];
    double* gi = a.goals + ((long)w * n + (human ? lane : 0)) * G * 2;
    double g0x = 0, g0y = 0;
    if (human) { g0x = gi[0]; g0y = gi[1]; }
    const double* ob = a.O > 0 ? a.obstacles + ((a.flags & CS_OBSTACLES_SHARED) ? 0 : (long)w * a.O * a.Smax * 4) : nullptr;
    const bool respawn_here = (a.flags & CS_RESPAWN) && (a.world_flags == nullptr || (a.world_flags[w] & 1));
    // the robot under a held holonomic action (robot_agent.py:114-118), tracked by every lane (uniform values)
    const bool robot_moves = a.action != nullptr && a.robot != nullptr;
    double rbx = 0, rby = 0, ax = 0, ay = 0;
    if (robot_moves) { rbx = a.robot[(long)w * 13]; rby = a.robot[(long)w * 13 + 1]; ax = a.action[(long)w * 2]; ay = a.action[(long)w * 2 + 1]; }

    for (int sub = 0; sub < a.n_substeps; ++sub) {
        // -- robot.step(action, dt), then states[-1] = robot row (social_nav_gym.py:240-243, motion_model_manager.py:359)
        if (robot_moves) {
            rbx += ax * dt; rby += ay * dt;
            if (is_robot && robot_from_array) { px = rbx; py = rby; vx = ax; vy = ay; }
        }
        // -- the incoming rows, for everybody's pair forces
        if (valid) { lds[0][lane] = px; lds[1][lane] = py; lds[2][lane] = vx; lds[3][lane] = vy; lds[4][lane] = r; lds[5][lane] = sf; }
        F64_LDS_FENCE();
        const Body me_in{px, py, vx, vy, r, sf};
        double fsx = 0, fsy = 0;
        if constexpr (PEQ) {
            // compute_all_social_force_parallel :87-133: from the incoming rows, the pair evaluated as (lower, higher)
            if (human) {
                for (int j = 0; j < rows; ++j) {
                    if (j == lane) continue;
                    const Body q{lds[0][j], lds[1][j], lds[2][j], lds[3][j], lds[4][j], lds[5][j]};
                    const bool lower = lane < j;
                    const Body A = lower ? me_in : q, B = lower ? q : me_in;
                    double fx, fy;
                    pair_force<SOC>(A, B, PP, fx, fy);
                    fsx += lower ? fx : -fx;
                    fsy += lower ? fy : -fy;
                }
            }
        }
        // -- goal switch :226-234 (on the incoming position; <=)
        if (human && norm2(g0x - px, g0y - py) <= r) {
            int k = G;
            for (int g = 0; g < G; ++g) if (isnan(gi[2 * g]) || isnan(gi[2 * g + 1])) { k = g; break; }
            if (a.mode & M64_COMMIT_GOALS) {
                const double r0 = gi[0], r1 = gi[1];
                for (int g = 0; g + 1 < k; ++g) { gi[2 * g] = gi[2 * g + 2]; gi[2 * g + 1] = gi[2 * g + 3]; }
                if (k > 0) { gi[2 * (k - 1)] = r0; gi[2 * (k - 1) + 1] = r1; }
                g0x = gi[0]; g0y = gi[1];
            } else if (k > 1) {
                g0x = gi[2]; g0y = gi[3];
            }
            gx = g0x; gy = g0y;
        }
        // -- rotation matrix and the refresh of the linear velocity :254-256 (the humans; never the robot row)
        double c = 1, s = 0, svx = vx, svy = vy;
        if (headed > 0 && human) {
            c = cos(th); s = sin(th);
            svx = c * bvx + (-s) * bvy;
            svy = s * bvx + c * bvy;
        }
        if constexpr (!PEQ) {
            // compute_social_force_parallel :43-84 with the lane's parameters: rows below see their refreshed velocity, rows above
            // the incoming one (the order the reference executes in, oracle/sfm_step.inc)
            if (valid) { lds[6][lane] = svx; lds[7][lane] = svy; }
            F64_LDS_FENCE();
            if (human) {
                const Body me{px, py, svx, svy, r, sf};
                for (int j = 0; j < rows; ++j) {
                    if (j == lane) continue;
                    const bool below = j < lane;
                    const Body q{lds[0][j], lds[1][j], below ? lds[6][j] : lds[2][j], below ? lds[7][j] : lds[3][j], lds[4][j], lds[5][j]};
                    double fx, fy;
                    pair_force<SOC>(me, q, PP, fx, fy);
                    fsx += fx; fsy += fy;
                }
            }
        }
        F64_LDS_FENCE();   // (the next substep, and the respawn below, overwrite the columns read above)
        if (human) {
            // -- desired force :23-40
            double fdx = 0, fdy = 0;
            laws::desired_force(gx, gy, px, py, svx, svy, r, m, vd, Pi[0], fdx, fdy);
            // -- closest point per polygon :236-252 (first argmin, a NaN segment = huge distance) and the obstacle force :136-162
            double fox = 0, foy = 0;
            if (ob != nullptr) {
                for (int o = 0; o < a.O; ++o) {
                    double best = 0, cx = 0, cy = 0;
                    bool have = false;
                    for (int sg = 0; sg < a.Smax; ++sg) {
                        const double* seg = ob + ((long)o * a.Smax + sg) * 4;
                        const double s0 = seg[0], s1 = seg[1], s2 = seg[2], s3 = seg[3];
                        double d, hx = 0, hy = 0;
                        if (isnan(s0)) {
                            d = 9223372036854775807.0;
                        } else {
                            const double ex = s2 - s0, ey = s3 - s1;
                            const double len = norm2(ex, ey);
                            const double t = ((px - s0) * ex + (py - s1) * ey) / (len * len);
                            double ts = t > 0 ? t : 0.0;
                            ts = ts < 1 ? ts : 1.0;
                            hx = s0 + ts * ex; hy = s1 + ts * ey;
                            d = norm2(hx - px, hy - py);
                        }
                        if (!have || d < best) { best = d; cx = hx; cy = hy; have = true; }
                    }
                    const double dx = px - cx, dy = py - cy;
                    const double dist = norm2(dx, dy);
                    laws::wall_term(SOC, Pi, dx / dist, dy / dist, r - dist + sf, svx, svy, fox, foy);
                }
                fox /= (double)a.O; foy /= (double)a.O;
            }
            const double fix = fdx + fox + fsx, fiy = fdy + foy + fsy;
            double gfx, gfy, torque = 0, inertia = 1;
            if (headed == 0) { gfx = fix; gfy = fiy; }
            else {
                inertia = 0.5 * m * r * r;
                laws::headed_force(headed == 2, Pi, inertia, fdx, fdy, fix, fiy, fox + fsx, foy + fsy, th, om, bvy, s, c, gfx, gfy, torque);
            }
            // -- update_humans_parallel(...) out of place: the input array keeps the reference's in-place mutations
            if (a.mode & M64_MUTATE_INPUT) {
                double* S = a.state + ((long)w * rows + lane) * 13;
                if (headed > 0) { S[3] = svx; S[4] = svy; }
                S[10] = gx; S[11] = gy;
            }
            // -- Euler :273-283 (the position moves with the incoming linear velocity)
            px += vx * dt;
            py += vy * dt;
            if (headed > 0) {
                th = bound_angle(th + om * dt);
                bvx += (gfx / m) * dt;
                bvy += (gfy / m) * dt;
                const double nb = norm2(bvx, bvy);
                if (nb > vd) { bvx = (bvx / nb) * vd; bvy = (bvy / nb) * vd; }
                om += (torque / inertia) * dt;
                const double c2 = cos(th), s2 = sin(th);
                vx = c2 * bvx + (-s2) * bvy;
                vy = s2 * bvx + c2 * bvy;
            } else {
                vx += (gfx / m) * dt;
                vy += (gfy / m) * dt;
                const double nb = norm2(vx, vy);
                if (nb > vd) { vx = (vx / nb) * vd; vy = (vy / nb) * vd; }
            }
        }
        // -- parallel-traffic respawn, motion_model_manager.py:407-422: the flagged humans in index order, each behind everybody else
        if (respawn_here) {
            const bool flag = human && norm2(px - g0x, py - g0y) < 3;
            const unsigned long long fm = __builtin_amdgcn_ballot_w64(flag);
            if (fm != 0ull) {
                // the maxima of the world as the first respawned human finds it: the stepped humans, the robot where it stands
                if (valid) { lds[0][lane] = px; lds[4][lane] = r + sf; }
                F64_LDS_FENCE();
                if (flag) {
                    double mx = lds[0][0], mr = lds[4][0];
                    for (int j = 1; j < rows; ++j) {
                        const double xj = lds[0][j], rj = lds[4][j];
                        if (xj > mx) mx = xj;
                        if (rj > mr) mr = rj;
                    }
                    const int cnt = __builtin_popcountll(fm & ((1ull << lane) - 1ull));
                    double x0 = mx + mr * 2.0;
                    if (!(x0 > a.bx)) x0 = a.bx;
                    px = x0 + (double)cnt * (mr * 2.0);
                    if (py >= 0) py = py < a.by ? py : a.by;
                    else py = py > -a.by ? py : -a.by;
                    g0y = py;
                    bvy = g0x; om = g0y;   // the reference writes the new goal into columns 6:8 of the row (:421)
                    if (a.mode & M64_COMMIT_GOALS)
                        for (int g = 0; g < G; ++g) { gi[2 * g] = g0x; gi[2 * g + 1] = g0y; }
                }
                F64_LDS_FENCE();
            }
        }
    }

    if (a.mode & M64_PEEK) {
        if (human) {
            double* o = a.peek + ((long)w * n + lane) * 8;
            o[0] = px; o[1] = py; o[2] = th; o[3] = vx; o[4] = vy; o[5] = om; o[6] = g0x; o[7] = g0y;
        }
        return;
    }
    if (valid) {
        double* o = a.out + ((long)w * rows + lane) * 13;
        o[0] = px; o[1] = py; o[2] = th; o[3] = vx; o[4] = vy; o[5] = bvx; o[6] = bvy; o[7] = om;
        o[8] = r; o[9] = m; o[10] = gx; o[11] = gy; o[12] = vd;
    }
    if (robot_moves && lane == 0) {
        double* rb = a.robot + (long)w * 13;
        rb[0] = rbx; rb[1] = rby; rb[3] = ax; rb[4] = ay;
    }
}

using csimpl::fail;

inline int rows_of64(const cs_worlds_f64* w) { return w->n + ((w->flags & CS_ROBOT_ROW) ? 1 : 0); }

// every argument check of the three entries, before the first HIP call
int check_worlds64(const cs_worlds_f64* w)
{
    if (!w) return fail(CS_ERR_ARG, "null cs_worlds_f64");
    if (w->type < 0 || w->type > 8) return fail(CS_ERR_ARG, "Type " + std::to_string(w->type) + " does not exist for this implementation");
    if (w->W <= 0 || w->n <= 0 || w->G <= 0) return fail(CS_ERR_ARG, "W, n, G must be positive");
    if (rows_of64(w) > 64) return fail(CS_ERR_ARG, "float64 worlds hold up to 64 rows (one wavefront per world), got " + std::to_string(rows_of64(w)));
    if (!w->d_state || !w->d_goals || !w->d_params || !w->d_safety) return fail(CS_ERR_ARG, "null device buffer in cs_worlds_f64");
    if (w->layout != CS_LAYOUT_AOS) return fail(CS_ERR_ARG, "float64 worlds are CS_LAYOUT_AOS only");
    if (w->flags & CS_ROBOT_UNICYCLE) return fail(CS_ERR_ARG, "float64 worlds do not cover the unicycle robot (CS_ROBOT_UNICYCLE)");
    if (!(w->O == 0 || (w->O > 0 && w->d_obstacles && w->Smax > 0))) return fail(CS_ERR_ARG, "bad obstacle description");
    return CS_OK;
}

int launch64(const cs_worlds_f64* w, double dt, int n_substeps, int mode, double* d_out, const double* d_action, double* d_peek, int flags,
             double* d_robot, hipStream_t stream)
{
    Args64 a{};
    a.W = w->W; a.n = w->n; a.rows = rows_of64(w); a.G = w->G; a.O = w->O; a.Smax = w->Smax; a.type = w->type; a.flags = flags;
    a.mode = mode; a.n_substeps = n_substeps;
    a.state = w->d_state; a.out = d_out; a.goals = w->d_goals; a.params = w->d_params; a.safety = w->d_safety;
    a.obstacles = w->O > 0 ? w->d_obstacles : nullptr; a.robot = d_robot; a.world_flags = w->d_world_flags; a.action = d_action; a.peek = d_peek;
    a.dt = dt; a.bx = w->respawn_bound_x; a.by = w->respawn_bound_y;
    const dim3 grid((unsigned)((w->W + F64_WPB - 1) / F64_WPB)), block(64 * F64_WPB);
    const bool peq = (flags & CS_ALL_PARAMS_EQUAL) != 0;
    switch ((w->type % 3) * 2 + (peq ? 1 : 0)) {
    case 0: hipLaunchKernelGGL((k_sfm_step_f64<0, false>), grid, block, 0, stream, a); break;
    case 1: hipLaunchKernelGGL((k_sfm_step_f64<0, true>), grid, block, 0, stream, a); break;
    case 2: hipLaunchKernelGGL((k_sfm_step_f64<1, false>), grid, block, 0, stream, a); break;
    case 3: hipLaunchKernelGGL((k_sfm_step_f64<1, true>), grid, block, 0, stream, a); break;
    case 4: hipLaunchKernelGGL((k_sfm_step_f64<2, false>), grid, block, 0, stream, a); break;
    default: hipLaunchKernelGGL((k_sfm_step_f64<2, true>), grid, block, 0, stream, a); break;
    }
    HIP_TRY(hipGetLastError());
    return CS_OK;
}

} // namespace

extern "C" {

int cs_step_f64(const cs_worlds_f64* w, double dt, int n_substeps, const double* d_action, void* stream)
{
    if (const int rc = check_worlds64(w)) return rc;
    if (n_substeps < 1) return fail(CS_ERR_ARG, "n_substeps must be positive");
    if (d_action && !w->d_robot) return fail(CS_ERR_ARG, "robot action given but cs_worlds_f64.d_robot is null");
    const int mode = M64_COMMIT_GOALS | (((w->flags & CS_ROBOT_ROW) && w->d_robot) ? (int)M64_ROBOT_FROM_ARRAY : 0);
    return launch64(w, dt, n_substeps, mode, w->d_state, d_action, nullptr, w->flags, w->d_robot, (hipStream_t)stream);
}

int cs_update_humans_parallel_f64(const cs_worlds_f64* w, double dt, double* d_out, void* stream)
{
    if (const int rc = check_worlds64(w)) return rc;
    if (!d_out) return fail(CS_ERR_ARG, "null argument");
    int mode = M64_COMMIT_GOALS;
    if (d_out != w->d_state) mode |= M64_MUTATE_INPUT;
    // one substep of the function itself: no respawn, the last row of d_state IS the robot row
    return launch64(w, dt, 1, mode, d_out, nullptr, nullptr, w->flags & ~CS_RESPAWN, nullptr, (hipStream_t)stream);
}

int cs_peek_f64(const cs_worlds_f64* w, double dt, double* d_next, void* stream)
{
    if (const int rc = check_worlds64(w)) return rc;
    if (!d_next) return fail(CS_ERR_ARG, "null argument");
    int mode = M64_PEEK;
    if ((w->flags & CS_ROBOT_ROW) && w->d_robot) mode |= M64_ROBOT_FROM_ARRAY;
    // update_humans(0, dt, post_update=False), motion_model_manager.py:705: no respawn
    return launch64(w, dt, 1, mode, nullptr, nullptr, d_next, w->flags & ~CS_RESPAWN, w->d_robot, (hipStream_t)stream);
}

} // extern "C"
