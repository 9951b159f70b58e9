// generate.hip -- device-side scenario generators: reset() of W worlds without W serial host
// rejection-sampling loops.
//
// Restates, one GPU lane per world, what SocialNavGym.reset does per world on the host:
//   np.random.seed(offset[phase] + case)                         /root/reference/social_gym/social_nav_gym.py:135-137
//   hybrid_scenario: np.random.choice([...]) then re-seed         social_nav_gym.py:156-157, 185-186
//   generate_circular_crossing_setting                            /root/reference/social_gym/social_nav_sim.py:200-299
//   generate_parallel_traffic_scenario                            social_nav_sim.py:301-362
//   generate_circular_crossing_with_static_obstacles              social_nav_sim.py:364-431
//   HumanAgent rows built by reset_sim                            social_nav_sim.py:97-198 (mass 75, zero velocities)
// The reference draws from numpy's legacy global stream: MT19937 seeded by init_genrand (integer seed),
// random_sample() = (a >> 5, b >> 6) 53-bit doubles, uniform(lo, hi) = lo + (hi - lo) * random_sample(),
// choice of two = next_uint32 & 1.  All of it is restated here in integer / f64 arithmetic, so the draw ORDER and the
// accept / reject decisions are the reference's; rows are rounded to f32 only when they are stored.
//
// MT19937 state: 624 words per world, kept in a caller-provided scratch [624][W] (word-major: the seeding and twist
// loops of the 64 lanes of a wavefront touch consecutive addresses).
//
// gfx950 only; not a hot path (one launch per reset), written for clarity.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>

#include "common.h"
#include "crowdstep.h"
#include "gymhead.h"
#include "worldcopy.h"

#pragma clang fp contract(off) // the reference's numpy expressions are not fused

namespace {

using csimpl::fail;
using namespace csimpl;

constexpr int GEN_MAXN = 128; // humans per world the per-lane placement arrays hold
constexpr double PI = 3.141592653589793;

// where a generated world goes (the batch being reset, a staging batch, or the live batch of cs_consume_staged_worlds)
struct GenOut {
    float* S; long as, fs; float* goals; float* robot; int* world_flags; int rows, G, robot_row;
    int orca;     // the batch is an ORCA crowd: columns 5:7 carry RVO2's preferred velocity (orca_pref below)
};

struct GArgs {
    cs_generator g;
    int W;        // (in front of `out`: behind it the wavefront kernel spilled 3x the scalar registers and lost 2-5 us a world, HISTORY.md)
    GenOut out;
    const uint32_t* seeds;
    const int32_t* mask;
    int32_t* status;
    int32_t* scenario_out;
    uint32_t* mt; // [624][W]: the states of the lane-per-world kernel
};

// ---- MT19937 as numpy's legacy stream runs it (numpy/random/src/mt19937/mt19937.c): the pieces both storages below are made of ----
// one step of mt19937_seed (init_genrand): word i from word i - 1
__device__ __forceinline__ uint32_t mt_seed_step(uint32_t prev, int i) { return 1812433253u * (prev ^ (prev >> 30)) + (uint32_t)i; }

// word k of the next block (genrand's block update) from old[k], old[k + 1] and the far word: old[k + 397], or new[k - 227] from k = 227 on
__device__ __forceinline__ uint32_t mt_twist_word(uint32_t w0, uint32_t w1, uint32_t far)
{
    constexpr uint32_t UPPER = 0x80000000u, LOWER = 0x7fffffffu, MATRIX_A = 0x9908b0dfu;
    const uint32_t y = (w0 & UPPER) | (w1 & LOWER);
    return far ^ (y >> 1) ^ ((y & 1u) ? MATRIX_A : 0u);
}

__device__ __forceinline__ uint32_t mt_temper(uint32_t y)
{
    y ^= (y >> 11);
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= (y >> 18);
    return y;
}

// legacy random_sample(): the 53-bit double in [0, 1) of two consecutive tempered words
__device__ __forceinline__ double mt_double(uint32_t ta, uint32_t tb)
{
    const uint32_t a = ta >> 5, b = tb >> 6;
    return (a * 67108864.0 + b) / 9007199254740992.0;
}

// storage 1, one LANE per world: 624 words in a strided global array, twisted in place
struct MT {
    uint32_t* s;
    long stride;
    int pos;
    __device__ uint32_t& at(int k) { return s[(long)k * stride]; }
};

__device__ void mt_seed(MT& m, uint32_t seed)
{
    uint32_t prev = seed;
    m.at(0) = prev;
    for (int i = 1; i < 624; ++i) m.at(i) = prev = mt_seed_step(prev, i);
    m.pos = 624;
}

__device__ void mt_twist(MT& m)
{
    for (int kk = 0; kk < 624 - 397; ++kk) m.at(kk) = mt_twist_word(m.at(kk), m.at(kk + 1), m.at(kk + 397));
    for (int kk = 624 - 397; kk < 623; ++kk) m.at(kk) = mt_twist_word(m.at(kk), m.at(kk + 1), m.at(kk - 227));
    m.at(623) = mt_twist_word(m.at(623), m.at(0), m.at(396));
    m.pos = 0;
}

__device__ uint32_t mt_next(MT& m)
{
    if (m.pos >= 624) mt_twist(m);
    return mt_temper(m.at(m.pos++));
}

__device__ double rnd(MT& m)
{
    const uint32_t a = mt_next(m), b = mt_next(m);
    return mt_double(a, b);
}

// storage 2, one WAVEFRONT per world: the block the stream is in and its successor in LDS, twisted cooperatively and out of place
struct WMT {
    uint32_t* cur; // [624] in LDS: the block the stream is in
    uint32_t* nxt; // [624] in LDS: twist(cur), kept ready so that speculative attempts can read across the block boundary
    int pos;       // wave-uniform index into cur; 624 <= pos < 1248 means "in nxt" until the next advance
};

// nw = twist(old), cooperatively: chunks of 64 in increasing order -- element kk reads old[kk], old[kk + 1] and either old[kk + 397]
// (kk < 227) or nw[kk - 227], written at least three chunks earlier
__device__ void wmt_twist_from(const uint32_t* old, uint32_t* nw, int lane)
{
    for (int k0 = 0; k0 < 623; k0 += 64) {
        const int kk = k0 + lane;
        if (kk < 623) nw[kk] = mt_twist_word(old[kk], old[kk + 1], kk < 227 ? old[kk + 397] : nw[kk - 227]);
        __syncthreads();
    }
    if (lane == 0) nw[623] = mt_twist_word(old[623], nw[0], nw[396]);
    __syncthreads();
}

__device__ void wmt_seed(WMT& m, uint32_t seed, int lane)
{
    __syncthreads();
    if (lane == 0) { // the init_genrand recurrence is serial
        uint32_t prev = seed;
        m.cur[0] = prev;
        for (int i = 1; i < 624; ++i) m.cur[i] = prev = mt_seed_step(prev, i);
    }
    __syncthreads();
    wmt_twist_from(m.cur, m.nxt, lane);
    m.pos = 624;   // numpy leaves the seeded block exhausted: the first draw comes from its twist
}

__device__ void wmt_advance(WMT& m, int lane)   // the stream has left `cur`: make `nxt` current and prepare the block after it
{
    uint32_t* t = m.cur; m.cur = m.nxt; m.nxt = t;
    m.pos -= 624;
    __syncthreads();
    wmt_twist_from(m.cur, m.nxt, lane);
}

__device__ uint32_t wmt_next(WMT& m, int lane)
{
    if (m.pos >= 624) wmt_advance(m, lane);
    return mt_temper(m.cur[m.pos++]);
}

__device__ double wrnd(WMT& m, int lane)
{
    const uint32_t a = wmt_next(m, lane), b = wmt_next(m, lane);
    return mt_double(a, b);
}

// random_sample() number q of the stream counted from word index k0 (k0 < 624, read-ahead below 1248), without consuming it
__device__ __forceinline__ double wmt_peek_double(const WMT& m, int k0, int q)
{
    const int k = k0 + 2 * q;
    const uint32_t wa = (k < 624) ? m.cur[k] : m.nxt[k - 624];
    const uint32_t wb = (k + 1 < 624) ? m.cur[k + 1] : m.nxt[k + 1 - 624];
    return mt_double(mt_temper(wa), mt_temper(wb));
}

// ---- the reference's rules as functions of values: they read no stream and do not know which kernel calls them ----------------------
// social_gym/src/utils.py:7-13 (Python's sign-of-divisor modulo == fmod for the operand signs of each branch)
__device__ double bound_angle_d(double a)
{
    const double two_pi = 2.0 * PI;
    if (a >= two_pi) a = fmod(a, two_pi);
    if (a <= -two_pi) a = fmod(a, two_pi);
    if (a > PI) a -= two_pi;
    if (a < -PI) a += two_pi;
    return a;
}

__device__ double norm2d(double x, double y) { return sqrt(x * x + y * y); } // np.linalg.norm of a 2-vector

struct P2 { double x, y; };

// the scenario frame: where the robot starts, where it looks and where it goes (centre (0, 0): the reference's cx, cy)
struct Frame { double px, py, yaw, gx, gy; };

__device__ __forceinline__ Frame scenario_frame(int scenario, double R, double L)
{
    if (scenario == CS_SCN_PARALLEL_TRAFFIC) return Frame{-(L / 2.0) + 1.0, 0.0, 0.0, (L / 2.0) - 1.0, 0.0};
    return Frame{0.0, 0.0 - R, PI / 2.0, 0.0, 0.0 + R}; // the circular crossing, with and without static obstacles
}

// attributes of human i: the random_sample() draws they take, in order, and what the draws give
__device__ __forceinline__ int attribute_draws(const cs_generator& g, bool obstacles, int i)
{
    if (obstacles) return i < 3 ? 1 : 0;
    return g.randomize_attributes ? 2 : 0;
}

__device__ __forceinline__ void attributes(const cs_generator& g, bool obstacles, int i, double d0, double d1, double& spd, double& rad)
{
    spd = 1.0; rad = 0.3;
    if (obstacles) {                                              // the three "obstacles" are immobile humans with a drawn radius (:381-387)
        if (i < 3) { spd = 0.0; rad = 1.0 + (d0 - 1.0) * 0.4; }
    } else if (g.randomize_attributes) {                          // uniform(0.5, 1.5) speed then uniform(0.3, 0.5) radius (:217-220)
        spd = 0.5 + (1.5 - 0.5) * d0; rad = 0.3 + (0.5 - 0.3) * d1;
    }
}

// parallel traffic: ValueError in the reference when the humans cover more than 40 % of the box (:318-319)
__device__ __forceinline__ bool traffic_too_dense(const double* rad, int n, double L, double H)
{
    double area = 0.0;
    for (int i = 0; i < n; ++i) area += PI * (rad[i] * rad[i]);
    return area > L * H * 0.4;
}

// the candidate position of one attempt, from its draws in stream order (d0, d1, d2) and the caller's (cos, sin) of the attempt's angle
__device__ __forceinline__ double circle_angle(double d0) { return d0 * PI * 2.0; }

__device__ __forceinline__ P2 circle_candidate(double R, double spd, double d1, double d2, double ca, double sa)
{
    const double nx = (d1 - 0.5) * spd, ny = (d2 - 0.5) * spd;
    return P2{0.0 + R * ca + nx, 0.0 + R * sa + ny};
}

__device__ __forceinline__ P2 traffic_candidate(double L, double H, double rad, double d0, double d1)
{
    const double lo = -(L / 2.0) + rad, hi = L / 2.0 - rad;
    return P2{(hi - lo) * d0 + lo, (d1 - 0.5) * H};
}

__device__ __forceinline__ double static_angle(int n, int i, double d0) // obstacles in the even sectors, humans in the odd ones
{
    const double sector = PI / (double)(n / 2);
    return sector * ((i < 3 ? -0.5 : 0.5) + 2.0 * i + (d0 - 0.5) * 0.5);
}

__device__ __forceinline__ P2 static_candidate(double R, int i, double d1, double d2, double ca, double sa)
{
    const double noise = i < 3 ? 0.1 : 0.7, ring = i < 3 ? R - 3.0 : R; // obstacles stand on the inner circle
    const double nx = (d1 - 0.5) * noise, ny = (d2 - 0.5) * noise;
    return P2{0.0 + ring * ca + nx, 0.0 + ring * sa + ny};
}

// the spot a placed human keeps free besides its own: its goal as the rejection test states it -- (-x + 2 cx, -y + 2 cx), :280 uses
// the centre's x twice, cx = cy = 0 --, or, for a static obstacle, where it stands
__device__ __forceinline__ P2 kept_free(bool obstacle, double x, double y) { return obstacle ? P2{x, y} : P2{-x + 0.0, -y + 0.0}; }

// slot i of the evenly spaced circle (:231-251); the robot, when inserted, takes slot 0 at the bottom
__device__ __forceinline__ void fixed_circle_slot(double R, int n, bool insert_robot, int i, double& x, double& y, double& yaw)
{
    const int slots = n + (insert_robot ? 1 : 0);
    const double step = (2.0 * PI) / slots;
    const int k = insert_robot ? i + 1 : i;
    const double off = insert_robot ? -(PI / 2.0) : 0.0;
    x = 0.0 + R * cos(off + step * k); y = 0.0 + R * sin(off + step * k);
    yaw = insert_robot ? bound_angle_d((PI / 2.0) + step * k) : bound_angle_d(-PI + step * k);
}

// the goals of human i placed at (x, y): the far end of the corridor, its own spot twice (a static obstacle), or the opposite point and back
struct Goals { double x0, y0, x1, y1; int count; };

__device__ __forceinline__ Goals human_goals(int scenario, double L, int i, double x, double y)
{
    if (scenario == CS_SCN_PARALLEL_TRAFFIC) return Goals{-(L / 2.0) - 3.0, y, 0.0, 0.0, 1};
    if (scenario == CS_SCN_CIRCULAR_CROSSING_STATIC_OBSTACLES && i < 3) return Goals{x, y, x, y, 2};
    return Goals{0.0 * 2.0 - x, 0.0 * 2.0 - y, x, y, 2};
}

// ---- the row store -------------------------------------------------------------------------------------------------------------------
// An ORCA crowd keeps RVO2's preferred velocity in columns 5:7 of its rows (set_state_orca / update_goals_orca,
// motion_model_manager.py:105-133: (g - p) / |g - p| if |g - p| > desired_speed else (g - p)), set when the simulator is built -- so
// a world generated on the device must carry it from its first substep on.  float32 on the stored (rounded) columns, as the host
// form of the same reset computes it (BatchedSocialNavGym._reset_on_device).
__device__ __forceinline__ void orca_pref(float* s, long fs, float px, float py, float gx, float gy, float vd)
{
    const float dx = gx - px, dy = gy - py;
    const float dn = sqrtf(dx * dx + dy * dy);
    const float dd = dn > 1e-30f ? dn : 1e-30f;
    s[5 * fs] = dn > vd ? dx / dd : dx;
    s[6 * fs] = dn > vd ? dy / dd : dy;
}

// one agent at rest: [px,py,theta,vx,vy,bvx,bvy,omega,r,m,gx,gy,vd]  (agent.py:256-258), rounded to f32 here and nowhere earlier
__device__ __forceinline__ void store_row(float* o, long fs, double x, double y, double yaw, double rad, double mass, double gx, double gy, double vd)
{
    o[0] = (float)x; o[fs] = (float)y; o[2 * fs] = (float)yaw;
    for (int c = 3; c < 8; ++c) o[c * fs] = 0.0f;
    o[8 * fs] = (float)rad; o[9 * fs] = (float)mass; o[10 * fs] = (float)gx; o[11 * fs] = (float)gy;
    o[12 * fs] = (float)vd;
}

// human i of world w: its row, an ORCA crowd's preferred velocity, and its goal list [G][2], NaN-padded
__device__ __forceinline__ void store_human(const cs_generator& g, const GenOut& a, int scenario, int w, int i, double x, double y, double yaw,
                                            double rad, double spd)
{
    const Goals gl = human_goals(scenario, g.traffic_length, i, x, y);
    float* s = a.S + ((long)w * a.rows + i) * a.as;
    store_row(s, a.fs, x, y, yaw, rad, g.human_mass, gl.x0, gl.y0, spd);
    if (a.orca) orca_pref(s, a.fs, (float)x, (float)y, (float)gl.x0, (float)gl.y0, (float)spd);
    const float nanf_ = __builtin_nanf("");
    float* o = a.goals + ((long)w * g.n + i) * a.G * 2;
    for (int k = 0; k < a.G; ++k) {
        float gx = nanf_, gy = nanf_;
        if (k == 0) { gx = (float)gl.x0; gy = (float)gl.y0; }
        else if (k == 1 && gl.count == 2) { gx = (float)gl.x1; gy = (float)gl.y1; }
        o[2 * k] = gx; o[2 * k + 1] = gy;
    }
}

// the robot's safe-state row (social_nav_gym.py:211-213: robot.set(px, py, gx, gy, 0, 0, yaw, w=0)) in the robot buffer and, where the
// batch has one, in the state row behind the humans; the flag of the traffic's respawn rule (:359-360)
__device__ __forceinline__ void store_robot_and_flag(const cs_generator& g, const GenOut& a, int scenario, int w, const Frame& f)
{
    if (a.robot != nullptr) store_row(a.robot + (long)w * 13, 1, f.px, f.py, f.yaw, g.robot_radius, g.robot_mass, f.gx, f.gy, g.robot_desired_speed);
    if (a.robot_row)
        store_row(a.S + ((long)w * a.rows + g.n) * a.as, a.fs, f.px, f.py, f.yaw, g.robot_radius, g.robot_mass, f.gx, f.gy, g.robot_desired_speed);
    if (a.world_flags != nullptr) a.world_flags[w] = (scenario == CS_SCN_PARALLEL_TRAFFIC) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------
// One LANE per world (n <= 128): the plain sequential loops of the reference, its np.linalg.norm tests written as they stand.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_generate(const GArgs a)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= a.W) return;
    if (a.mask != nullptr && a.mask[w] == 0) return;
    const cs_generator& g = a.g;
    const int n = g.n;
    MT m{a.mt + w, (long)a.W, 624};
    const uint32_t seed = a.seeds[w];
    mt_seed(m, seed);
    int scenario = g.scenario;
    if (scenario == CS_SCN_HYBRID) { // np.random.choice(['circle_crossing', 'parallel_traffic']); np.random.seed(seed)
        scenario = (mt_next(m) & 1u) ? CS_SCN_PARALLEL_TRAFFIC : CS_SCN_CIRCULAR_CROSSING;
        mt_seed(m, seed);
    }
    double px[GEN_MAXN], py[GEN_MAXN], yaw[GEN_MAXN], rad[GEN_MAXN], spd[GEN_MAXN];
    int status = 0;
    const double R = g.circle_radius, L = g.traffic_length, H = g.traffic_height, rr = g.robot_radius;
    const bool insert_robot = g.insert_robot != 0;
    const Frame f = scenario_frame(scenario, R, L);
    const bool obstacles = scenario == CS_SCN_CIRCULAR_CROSSING_STATIC_OBSTACLES;

    for (int i = 0; i < n; ++i) {
        const int k = attribute_draws(g, obstacles, i);
        const double d0 = k > 0 ? rnd(m) : 0.0, d1 = k > 1 ? rnd(m) : 0.0;
        attributes(g, obstacles, i, d0, d1, spd[i], rad[i]);
    }
    if (scenario == CS_SCN_CIRCULAR_CROSSING && !g.randomize_positions) {
        for (int i = 0; i < n; ++i) fixed_circle_slot(R, n, insert_robot, i, px[i], py[i], yaw[i]);
    } else if (scenario == CS_SCN_PARALLEL_TRAFFIC) {
        if (traffic_too_dense(rad, n, L, H)) status = 2;
        for (int i = 0; i < n && status == 0; ++i) {
            bool placed = false;
            for (int t = 0; t < g.max_tries; ++t) {
                const double d0 = rnd(m), d1 = rnd(m);
                const P2 c = traffic_candidate(L, H, rad[i], d0, d1);
                bool collide = false;
                for (int j = 0; j < i; ++j)
                    if (norm2d(c.x - px[j], c.y - py[j]) - rad[i] - rad[j] - 0.1 < 0.0) { collide = true; break; }
                if (insert_robot && norm2d(c.x - f.px, c.y - f.py) - rad[i] - rr - 0.1 < 0.0) collide = true;
                if (!collide) {
                    px[i] = c.x; py[i] = c.y; yaw[i] = bound_angle_d(-PI);
                    placed = true;
                    break;
                }
            }
            if (!placed) status = 1;
        }
    } else { // the circular crossing and its form with static obstacles: one loop, each with its own candidate; the latter always keeps off the robot
        for (int i = 0; i < n && status == 0; ++i) {
            bool placed = false;
            for (int t = 0; t < g.max_tries; ++t) {
                const double d0 = rnd(m), d1 = rnd(m), d2 = rnd(m);
                const double angle = obstacles ? static_angle(n, i, d0) : circle_angle(d0);
                const double ca = cos(angle), sa = sin(angle);
                const P2 c = obstacles ? static_candidate(R, i, d1, d2, ca, sa) : circle_candidate(R, spd[i], d1, d2, ca, sa);
                bool collide = false;
                for (int j = 0; j < i; ++j) {
                    const double md = rad[i] + rad[j] + 0.2;
                    const P2 q = kept_free(obstacles && j < 3, px[j], py[j]);
                    if (norm2d(c.x - px[j], c.y - py[j]) < md || norm2d(c.x - q.x, c.y - q.y) < md) { collide = true; break; }
                }
                if ((obstacles || insert_robot) &&
                    (norm2d(c.x - f.px, c.y - f.py) < rad[i] + rr + 0.2 || norm2d(c.x - f.gx, c.y - f.gy) < rad[i] + rr + 0.2))
                    collide = true;
                if (!collide) {
                    px[i] = c.x; py[i] = c.y; yaw[i] = bound_angle_d(PI + angle);
                    placed = true;
                    break;
                }
            }
            if (!placed) status = 1;
        }
    }
    if (a.status != nullptr) a.status[w] = status;
    if (a.scenario_out != nullptr) a.scenario_out[w] = scenario;
    if (status != 0) return; // the rows of a world that could not be generated are left untouched

    for (int i = 0; i < n; ++i) store_human(g, a.out, scenario, w, i, px[i], py[i], yaw[i], rad[i], spd[i]);
    store_robot_and_flag(g, a.out, scenario, w, f);
}

// ------------------------------------------------------------------------------------------
// One WAVEFRONT per world (n <= 64): the latency form, used for the masked auto-reset inside a device-resident loop.
// MT19937 state in LDS (the current block and its successor, twisted cooperatively); attribute draws are read as wave-wide
// broadcasts.  The rejection loops of the circular crossing and of the parallel traffic are SPECULATIVE: eight attempts of
// the human being placed are evaluated at once, each from its own words of the stream by eight lanes that share the test
// against the placed humans (kept in LDS); the first accepted attempt wins and the stream position moves to just behind
// it, so a human mostly costs one round whatever its rejection count -- the slowest world of a batch no longer sets the
// latency of a masked reset.
// Same draws, same f64 expressions, same accept / reject decisions as k_generate above.
// ------------------------------------------------------------------------------------------
// np.linalg.norm((dx, dy)) < md, decided on the squares; the square root only inside the rounding band of the comparison
__device__ __forceinline__ bool closer_than(double dx, double dy, double md)
{
    const double d2 = dx * dx + dy * dy, md2 = md * md;
    bool c = d2 < md2;
    if (fabs(d2 - md2) <= 1e-14 * md2) c = sqrt(d2) < md;
    return c;
}

// the traffic's norm((dx, dy)) - ri - rj - 0.1 < 0, decided on the squares outside the rounding band of that expression
__device__ __forceinline__ bool traffic_closer(double dx, double dy, double ri, double rj)
{
    const double d2 = dx * dx + dy * dy, T = ri + rj + 0.1, T2 = T * T;
    bool c = d2 < T2;
    if (fabs(d2 - T2) <= 1e-12 * T2) c = norm2d(dx, dy) - ri - rj - 0.1 < 0.0;
    return c;
}

struct Attempt { double x, y, yaw; bool collide; }; // a candidate, its heading before bound_angle, and what THIS lane's share of the test found

// Speculative rejection sampling of one human: the wavefront evaluates 8 attempts at once, attempt lane / 8 from its own WORDS words of
// the stream (read ahead without consuming them) -- `attempt(k0)` is that evaluation for the attempt whose words start at k0 --, its 8
// lanes sharing the test against the placed humans (lane % 8 takes every eighth one).  The first attempt none of whose lanes found a
// collision wins, is stored to (px, py, yaw) and the stream moves to just behind it: the same draws and decisions as the sequential loop.
// Returns whether the human was placed within max_tries attempts.
template <int WORDS, class F>
__device__ __forceinline__ bool place_speculatively(WMT& m, int lane, int max_tries, double& px, double& py, double& yaw, F attempt)
{
    const int att = lane >> 3;
    bool placed = false;
    for (int t0 = 0; t0 < max_tries && !placed; t0 += 8) {
        if (m.pos >= 624) wmt_advance(m, lane);
        const int base = m.pos;
        const Attempt c = attempt(base + WORDS * att);
        const unsigned long long bad = __builtin_amdgcn_ballot_w64(c.collide || t0 + att >= max_tries);
        int win = -1;
        for (int q = 7; q >= 0; --q) if (((bad >> (8 * q)) & 0xFFull) == 0) win = q;
        if (win >= 0) {
            if (lane == 8 * win) { px = c.x; py = c.y; yaw = bound_angle_d(c.yaw); }
            m.pos = base + WORDS * (win + 1);
            placed = true;
        } else {
            m.pos = base + WORDS * 8;
        }
        __syncthreads();
    }
    return placed;
}

// One world by one wavefront (the block): the reference's generator for `seed`, rows written to `a` when it succeeds.  Returns the
// status (0 ok, 1 rejection sampling gave up, 2 traffic too dense); `scenario_out` = the scenario drawn (hybrid batches).
__device__ int generate_world_wave(const cs_generator& g, const GenOut& a, int w, int lane, uint32_t seed, int& scenario_out)
{
    __shared__ uint32_t s_mt[2][624];
    __shared__ double s_rad[64], s_spd[64], s_px[64], s_py[64], s_yaw[64];
    const int n = g.n;
    WMT m;
    m.cur = s_mt[0];
    m.nxt = s_mt[1];
    m.pos = 624;
    wmt_seed(m, seed, lane);
    int scenario = g.scenario;
    if (scenario == CS_SCN_HYBRID) {
        scenario = (wmt_next(m, lane) & 1u) ? CS_SCN_PARALLEL_TRAFFIC : CS_SCN_CIRCULAR_CROSSING;
        // np.random.seed(seed) again (:156-157): the stream restarts at its first word, which is word 0 of the block the
        // choice was just drawn from -- rewinding the position is the whole re-seeding
        m.pos = 0;
    }
    const double R = g.circle_radius, L = g.traffic_length, H = g.traffic_height, rr = g.robot_radius;
    const bool insert_robot = g.insert_robot != 0;
    // The robot's frame, the attribute draws and the static obstacles' candidate are restated in this function, not taken from
    // scenario_frame(), attribute_draws() and static_angle() / static_candidate(): each of the three moved a line of
    // tools/gen_latency.py out of the parent's spread (HISTORY.md, "Scenario generators"); k_generate uses the functions.
    double rpx = 0, rpy = 0, ryaw = 0, rgx = 0, rgy = 0;
    double mx = 0, my = 0, myaw = 0; // placed human `lane`
    int status = 0;

    // attributes: every lane sees every draw; slot i keeps its own in LDS for the uniform reads below
    if (scenario == CS_SCN_CIRCULAR_CROSSING_STATIC_OBSTACLES) {
        for (int i = 0; i < n; ++i) {
            double sp, ra;
            attributes(g, true, i, i < 3 ? wrnd(m, lane) : 0.0, 0.0, sp, ra);
            if (lane == i) { s_spd[i] = sp; s_rad[i] = ra; }
        }
    } else {
        for (int i = 0; i < n; ++i) {
            double d0 = 0.0, d1 = 0.0, sp, ra;
            if (g.randomize_attributes) { d0 = wrnd(m, lane); d1 = wrnd(m, lane); }
            attributes(g, false, i, d0, d1, sp, ra);
            if (lane == i) { s_spd[i] = sp; s_rad[i] = ra; }
        }
    }
    __syncthreads();
    const double myrad = lane < n ? s_rad[lane] : 0.0;

    if (scenario == CS_SCN_CIRCULAR_CROSSING) {
        rpx = 0.0; rpy = 0.0 - R; ryaw = PI / 2.0; rgx = 0.0; rgy = 0.0 + R;
        if (!g.randomize_positions) {
            fixed_circle_slot(R, n, insert_robot, lane, mx, my, myaw);
        } else {
            const int sub = lane & 7;                      // speculative, six words per attempt: this lane's share of an attempt's test
            for (int i = 0; i < n && status == 0; ++i) {
                const double ri = s_rad[i], si = s_spd[i];
                const bool placed = place_speculatively<6>(m, lane, g.max_tries, s_px[i], s_py[i], s_yaw[i], [&](int k0) {
                    const double angle = circle_angle(wmt_peek_double(m, k0, 0));
                    double sa, ca;
                    sincos(angle, &sa, &ca); // one range reduction for both (same values as cos() and sin(): G6 parity)
                    const P2 c = circle_candidate(R, si, wmt_peek_double(m, k0, 1), wmt_peek_double(m, k0, 2), ca, sa);
                    const double x = c.x, y = c.y;
                    bool collide = false;
                    for (int j = sub; j < i; j += 8) {
                        const double qx = s_px[j], qy = s_py[j], md = ri + s_rad[j] + 0.2;
                        const P2 q = kept_free(false, qx, qy);
                        collide |= closer_than(x - qx, y - qy, md) || closer_than(x - q.x, y - q.y, md);
                    }
                    if (insert_robot && sub == 0)
                        collide |= closer_than(x - rpx, y - rpy, ri + rr + 0.2) || closer_than(x - rgx, y - rgy, ri + rr + 0.2);
                    return Attempt{x, y, PI + angle, collide};
                });
                if (!placed) status = 1;
            }
            if (lane < n) { mx = s_px[lane]; my = s_py[lane]; myaw = s_yaw[lane]; }
        }
    } else if (scenario == CS_SCN_PARALLEL_TRAFFIC) {
        rpx = -(L / 2.0) + 1.0; rpy = 0.0; ryaw = 0.0; rgx = (L / 2.0) - 1.0; rgy = 0.0;
        if (traffic_too_dense(s_rad, n, L, H)) status = 2;
        const int sub = lane & 7;                          // speculative, four words per attempt
        for (int i = 0; i < n && status == 0; ++i) {
            const double ri = s_rad[i];
            const bool placed = place_speculatively<4>(m, lane, g.max_tries, s_px[i], s_py[i], s_yaw[i], [&](int k0) {
                const P2 c = traffic_candidate(L, H, ri, wmt_peek_double(m, k0, 0), wmt_peek_double(m, k0, 1));
                const double x = c.x, y = c.y;
                bool collide = false;
                for (int j = sub; j < i; j += 8) collide |= traffic_closer(x - s_px[j], y - s_py[j], ri, s_rad[j]);
                if (insert_robot && sub == 0) collide |= traffic_closer(x - rpx, y - rpy, ri, rr);
                return Attempt{x, y, -PI, collide};
            });
            if (!placed) status = 1;
        }
        if (lane < n) { mx = s_px[lane]; my = s_py[lane]; myaw = s_yaw[lane]; }
    } else { // static obstacles: sequential attempts, lane j holding placed human j in registers and testing the candidate against it
        rpx = 0.0; rpy = 0.0 - R; ryaw = PI / 2.0; rgx = 0.0; rgy = 0.0 + R;
        const double inner = R - 3.0;
        const double sector = PI / (double)(n / 2);
        for (int i = 0; i < n && status == 0; ++i) {
            const double ri = s_rad[i];
            bool placed = false;
            for (int t = 0; t < g.max_tries; ++t) {
                double angle, nx, ny, ring;
                if (i < 3) {
                    angle = sector * (-0.5 + 2.0 * i + (wrnd(m, lane) - 0.5) * 0.5);
                    nx = (wrnd(m, lane) - 0.5) * 0.1; ny = (wrnd(m, lane) - 0.5) * 0.1;
                    ring = inner;
                } else {
                    angle = sector * (0.5 + 2.0 * i + (wrnd(m, lane) - 0.5) * 0.5);
                    nx = (wrnd(m, lane) - 0.5) * 0.7; ny = (wrnd(m, lane) - 0.5) * 0.7;
                    ring = R;
                }
                double sa, ca;
                sincos(angle, &sa, &ca);
                const double x = 0.0 + ring * ca + nx, y = 0.0 + ring * sa + ny;
                const double md = ri + myrad + 0.2;
                const double gxj = (lane < 3) ? mx : (-mx + 0.0), gyj = (lane < 3) ? my : (-my + 0.0);
                const bool hit = lane < i && (norm2d(x - mx, y - my) < md || norm2d(x - gxj, y - gyj) < md);
                bool collide = __builtin_amdgcn_ballot_w64(hit) != 0;
                if (norm2d(x - rpx, y - rpy) < ri + rr + 0.2 || norm2d(x - rgx, y - rgy) < ri + rr + 0.2) collide = true;
                if (!collide) {
                    if (lane == i) { mx = x; my = y; myaw = bound_angle_d(PI + angle); }
                    placed = true;
                    break;
                }
            }
            if (!placed) status = 1;
        }
    }
    scenario_out = scenario;
    if (status != 0) return status;

    if (lane < n) store_human(g, a, scenario, w, lane, mx, my, myaw, myrad, s_spd[lane]);
    if (lane == 0) store_robot_and_flag(g, a, scenario, w, Frame{rpx, rpy, ryaw, rgx, rgy});
    return 0;
}

__global__ __launch_bounds__(64) void k_generate_wave(const GArgs a)
{
    const int w = blockIdx.x, lane = threadIdx.x;
    if (a.mask != nullptr && a.mask[w] == 0) return; // block-uniform
    int scenario = 0;
    const int status = generate_world_wave(a.g, a.out, w, lane, a.seeds[w], scenario);
    if (lane == 0) {
        if (a.status != nullptr) a.status[w] = status;
        if (a.scenario_out != nullptr) a.scenario_out[w] = scenario;
    }
}

// ---- pre-staged episodes (include/crowdstep.h cs_stage_book) -----------------------------------------------------------------
struct StageArgs {
    cs_generator g;
    GenOut staging, live;
    csimpl::CopyArgs copy;          // staging -> live (mask / status unused here)
    const uint32_t* seeds; const uint32_t* base_seed; uint32_t* epoch; uint32_t* staged_seed; int32_t* staged_status; int32_t* failed;
    const int32_t* mask;
    uint32_t stride;
    int W, depth;
};

__device__ __forceinline__ uint32_t load_relaxed(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void store_release(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT); }

// ---- the staging protocol: two kernels on two streams, no event, no acquire ----------------------------------------------------------
// Writer: k_refill_staged (side stream).  Readers: k_consume_staged (step stream) and the epilogue of k_sfm_step under cs_gym_step_staged
// (gymhead.h GymFold).  Shared words: the slot's rows / goal lists / robot row / flag / status, its TAG staged_seed[slot], and epoch[w].
// What makes it correct -- each line is an obligation of the code, checked by the tests named at the end:
//   W1  the writer regenerates a slot only when its tag differs from the seed of the episode that belongs in it NOW (a function of
//       epoch[w], base_seed[w], the slot index): a slot a reader may be copying -- tag == the world's next seed, epoch not yet moved --
//       is never written.
//   W2  the writer stores the tag LAST, with a device-scope RELEASE (store_release): a reader that sees the new tag sees every word
//       of the slot the writer stored before it, PROVIDED the reader's loads of those words cannot be served from a line cached before
//       the release -- R2.
//   R1  a reader loads the tag first (device-scope relaxed atomic load) and touches the slot only if tag == the world's next seed:
//       a CONTROL dependency.  No load of a slot word may be issued before the tag has returned and compared equal: the loads sit in the
//       taken branch and are `__hip_atomic_load`s, which the compiler may not hoist above the branch or merge with earlier loads.
//   R2  the slot's words are read with device-scope relaxed atomic loads (copy_world<COHERENT = true>: sc1 loads that miss this XCD's
//       L2 instead of hitting a line from before the refill).  A plain load here would be a silent bug.  Not an acquire on purpose: an
//       acquire fence at device scope invalidates the whole L2 of the XCD beside the running step kernels, each time a world ends.
//   R3  the reader stores epoch[w] (device-scope relaxed) only after EVERY load of the slot has returned: behind a barrier of the
//       block (k_consume_staged) / an s_waitcnt vmcnt(0) of the one wavefront (the step kernel's epilogue).  From that store on W1 lets
//       the writer take the slot.  It is the linearisation point of the take-over.
//   R4  only readers write epoch[w], and one world is read by one block per launch; launches of a reader are ordered on the step stream,
//       launches of the writer on the side stream.
// This is outside the HIP memory model's guarantees for coarse-grained memory between concurrent kernels (no happens-before without
// an acquire); it relies on gfx950's device-scope atomics going to the memory side of the L2s.  The net under it: every regenerated
// episode is compared bit for bit with the in-place generation of the same seed, under three refill cadences, at 96 and at 4096 worlds
// (tests/test_gpu_generators.py::test_step_device_is_the_same_whatever_the_refill_cadence, ::test_one_launch_gym_step_equals_the_two_launches,
// tools/device_loop_soak.py: 191k episodes).  A half-written world would differ from its seed's.
//
// side stream.  Slot s = j * W + w holds the episode of world w that belongs in ring position j now: the one e in (epoch, epoch + depth]
// with e = j mod depth; it is regenerated when its tag is not that episode's seed.  The grid is SMALL (<= 1024 blocks of one wavefront,
// every lane checking one slot per trip, two relaxed device-scope loads): a block per slot -- 65536 workgroups at depth 16 x 4096 worlds,
// nearly all of which leave at once -- kept the workgroup dispatcher busy for ~45 us per pass and the step stream's next launch waited
// behind it.  The slots a wavefront finds stale are generated one after the other by the whole wavefront; only those pay for a release
// (a cache-maintenance operation per checked slot would disturb the step kernel).
__global__ __launch_bounds__(64) void k_refill_staged(const StageArgs a)
{
    const int lane = threadIdx.x;
    const long total = (long)a.W * a.depth;
    for (long s0 = (long)blockIdx.x * 64; s0 < total; s0 += (long)gridDim.x * 64) {
        const long s = s0 + lane;
        uint32_t want = 0;
        bool stale = false;
        if (s < total) {
            const int w = (int)(s % a.W), j = (int)(s / a.W);
            const uint32_t epoch = load_relaxed(a.epoch + w);
            const uint32_t ahead = ((uint32_t)j - epoch - 1u) & (uint32_t)(a.depth - 1);      // 0 .. depth-1
            want = a.base_seed[w] + (epoch + 1u + ahead) * a.stride;
            stale = load_relaxed(a.staged_seed + s) != want;
        }
        unsigned long long todo = __builtin_amdgcn_ballot_w64(stale);                  // wave-uniform from here on
        while (todo != 0) {
            const int l = __builtin_ctzll(todo);
            todo &= todo - 1;
            const long slot = s0 + l;
            const uint32_t seed = (uint32_t)__builtin_amdgcn_readlane((int)want, l);
            int scenario = 0;
            const int status = generate_world_wave(a.g, a.staging, (int)slot, lane, seed, scenario);
            if (lane == 0) a.staged_status[slot] = status;
            __syncthreads();
            // the tag goes LAST: a consumer that reads `seed` in it (acquire) sees the rows, goal lists, robot row, flag and status above
            if (lane == 0) store_release(a.staged_seed + slot, seed);
            __syncthreads();                                                           // (the generator's LDS is reused by the next slot)
        }
    }
}

// the step's stream: a finished world takes over its staged episode -- or, if the refill has not got to it yet, is generated in place.
// One block per world (4096 workgroups, most of which read one integer and leave: 2.9 us when nobody ends; tools/consume_probe.py): the
// refill's small grid was tried here too -- 64 masks per wavefront, its finished worlds copied one after the other -- and cost 13 us more
// per Gym step (a wavefront with three ends copies serially).
// No acquire / release pair here: an acquire at device scope invalidates this XCD's L2 and a release writes all of it back, each time a
// world ends, beside the step kernels.  The slot is read with device-scope relaxed loads instead (they miss a stale L2 line by themselves),
// after the tag -- a control dependency --, and the epoch is stored after the loads have returned (the barrier waits for them): all the
// refill needs to know before it overwrites the slot is that nobody reads it any more.
__global__ __launch_bounds__(64) void k_consume_staged(const StageArgs a)
{
    const int w = blockIdx.x, lane = threadIdx.x;
    if (!a.mask[w]) return;                                                    // block-uniform (seed and epoch requested with the mask: +2 us for the 4000 blocks that leave here)
    const uint32_t want = a.seeds[w];                                          // the seed the bookkeeping moved this world to
    const uint32_t e = a.epoch[w] + 1u;                                        // (only this kernel writes the epochs)
    const long slot = (long)(e & (uint32_t)(a.depth - 1)) * a.W + w;
    int status;
    if (load_relaxed(a.staged_seed + slot) == want) {                          // written LAST by the refill, behind a release of the slot's words
        status = csimpl::copy_world<true>(a.copy, slot, w, lane, a.staged_status + slot);   // (the status word comes with the first batch)
    } else {
        int scenario = 0;
        status = generate_world_wave(a.g, a.live, w, lane, want, scenario);
        if (status == 0 && a.copy.obs != nullptr) {
            __syncthreads();                                                   // the rows this block just wrote
            for (int k = lane; k < a.copy.n * a.copy.C; k += 64) {
                const int i = k / a.copy.C, c = k - i * a.copy.C;
                a.copy.obs[((long)w * a.copy.n + i) * a.copy.C + c] = a.live.S[((long)w * a.live.rows + i) * a.live.as + csimpl::obs_state_column(c) * a.live.fs];
            }
        }
    }
    if (lane == 0) a.failed[w] = status != 0 ? 1 : 0;
    __syncthreads();                                                           // every lane's loads of the slot have returned
    // LAST: from here on the refill may overwrite the slot (it now belongs to episode e + depth)
    if (lane == 0) __hip_atomic_store(a.epoch + w, e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

int fill_gen_out(const cs_worlds* w, GenOut& o)
{
    o.rows = rows_of(w);
    o.robot_row = o.rows - w->n;
    o.orca = w->type == CS_ORCA ? 1 : 0;
    o.G = w->G;
    o.S = w->d_state;
    if (const int rc = check_layout(w)) return rc;
    state_strides(w, o.as, o.fs);
    o.goals = w->d_goals;
    o.robot = w->d_robot;
    o.world_flags = const_cast<int*>(w->d_world_flags);
    return CS_OK;
}

int check_generator(const cs_generator* gen, const cs_worlds* w)
{
    if (!w->d_state || !w->d_goals) return fail(CS_ERR_ARG, "null device buffer in cs_worlds");   // (the generators write rows and goals only)
    if (const int rc = check_shape(w)) return rc;
    if (gen->n != w->n) return fail(CS_ERR_ARG, "cs_generator.n differs from cs_worlds.n");
    if (gen->n > GEN_MAXN) return fail(CS_ERR_ARG, "the device generators place at most 128 humans per world");
    if (gen->scenario < CS_SCN_CIRCULAR_CROSSING || gen->scenario > CS_SCN_HYBRID) return fail(CS_ERR_ARG, "unknown scenario");
    if (gen->scenario != CS_SCN_PARALLEL_TRAFFIC && w->G < 2) return fail(CS_ERR_ARG, "circular scenarios need G >= 2 goal slots");
    if (gen->scenario == CS_SCN_CIRCULAR_CROSSING_STATIC_OBSTACLES) {
        if (!(gen->circle_radius > 5.0)) return fail(CS_ERR_ARG, "Radius must be greater than 5 for this scenario"); // :375
        if (gen->n < 2) return fail(CS_ERR_ARG, "static-obstacle scenario needs at least 2 humans (sector = pi / (n // 2))");
    }
    if (gen->max_tries <= 0) return fail(CS_ERR_ARG, "max_tries must be positive (the reference's loops are unbounded)");
    return CS_OK;
}

int stage_args(const cs_generator* gen, const cs_worlds* staging, const cs_worlds* live, const cs_stage_book* book, StageArgs& a)
{
    if (!gen || !staging || !book) return fail(CS_ERR_ARG, "null argument");
    if (const int rc = check_stage_book(book)) return rc;
    const int K = book->depth;
    if (K <= 0 || (K & (K - 1)) != 0) return fail(CS_ERR_ARG, "cs_stage_book.depth must be a power of two");
    if (staging->W % K != 0) return fail(CS_ERR_ARG, "the staging batch must hold depth * W worlds");
    int rc = check_generator(gen, staging);
    if (rc) return rc;
    if (gen->n > 64) return fail(CS_ERR_ARG, "pre-staged episodes are built for worlds of up to 64 humans (one wavefront per world)");
    std::memset(&a, 0, sizeof(a));
    a.g = *gen;
    if ((rc = fill_gen_out(staging, a.staging))) return rc;
    a.W = staging->W / K; a.depth = K;
    a.seeds = book->d_seeds; a.base_seed = book->d_base_seed; a.epoch = book->d_epoch; a.staged_seed = book->d_staged_seed;
    a.staged_status = book->d_staged_status; a.failed = book->d_failed;
    a.stride = book->seed_stride ? book->seed_stride : (uint32_t)a.W;
    if (live) {
        if (a.W != live->W || staging->n != live->n || staging->G != live->G || staging->layout != live->layout ||
            ((staging->flags ^ live->flags) & CS_ROBOT_ROW) || (!staging->d_robot) != (!live->d_robot) || (!staging->d_world_flags) != (!live->d_world_flags))
            return fail(CS_ERR_ARG, "staging and live worlds differ in shape");
        if ((rc = check_generator(gen, live))) return rc;
        if ((rc = fill_gen_out(live, a.live))) return rc;
        csimpl::CopyArgs& c = a.copy;
        c.W = live->W; c.n = live->n; c.rows = a.live.rows; c.G = live->G;
        c.Ss = staging->d_state; c.Sd = live->d_state; c.as = a.live.as; c.fs = a.live.fs; c.sas = a.staging.as; c.sfs = a.staging.fs;
        c.gs = staging->d_goals; c.gd = live->d_goals; c.rs = staging->d_robot; c.rd = live->d_robot;
        c.fsrc = staging->d_world_flags; c.fdst = const_cast<int*>(live->d_world_flags);
    }
    return CS_OK;
}

} // namespace

int csimpl::stage_fold(const cs_generator* gen, const cs_worlds* staging, const cs_worlds* live, const cs_stage_book* book, int obs_cols, float* d_obs,
                       cstep::GymFold& out)
{
    StageArgs a;
    const int rc = stage_args(gen, staging, live, book, a);
    if (rc) return rc;
    if (!live || !book->d_pending || !book->d_failed) return fail(CS_ERR_ARG, "null argument");
    out.on = 1; out.depth = a.depth; out.W = a.W;
    out.staged_seed = a.staged_seed; out.staged_status = a.staged_status; out.epoch = a.epoch; out.failed = a.failed; out.pending = book->d_pending;
    out.copy = a.copy;
    out.copy.obs = d_obs; out.copy.C = obs_cols;
    return CS_OK;
}

extern "C" {

size_t cs_generate_scratch_bytes(int W) { return W > 0 ? (size_t)624 * (size_t)W * sizeof(uint32_t) : 0; }

int cs_generate_worlds(const cs_generator* gen, const cs_worlds* w, const uint32_t* d_seeds, const int32_t* d_mask,
                       int32_t* d_status, int32_t* d_scenario, void* d_scratch, void* stream)
{
    if (!gen || !w || !d_seeds || !d_scratch) return fail(CS_ERR_ARG, "null argument");
    {
        const int rc = check_generator(gen, w);
        if (rc) return rc;
    }
    GArgs a;
    a.g = *gen;
    if (const int rc = fill_gen_out(w, a.out)) return rc;
    a.W = w->W;
    a.seeds = d_seeds;
    a.mask = d_mask;
    a.status = d_status;
    a.scenario_out = d_scenario;
    a.mt = (uint32_t*)d_scratch;
    if (gen->n <= 64) { // one wavefront per world: ~10x shorter latency per world, and faster for full batches too
        hipLaunchKernelGGL(k_generate_wave, dim3(w->W), dim3(64), 0, (hipStream_t)stream, a);
    } else {            // one lane per world, MT19937 state in the scratch buffer
        const int block = 64, grid = (w->W + block - 1) / block;
        hipLaunchKernelGGL(k_generate, dim3(grid), dim3(block), 0, (hipStream_t)stream, a);
    }
    HIP_TRY(hipGetLastError());
    return CS_OK;
}

int cs_refill_staged_worlds(const cs_generator* gen, const cs_worlds* staging, const cs_stage_book* book, void* stream)
{
    StageArgs a;
    const int rc = stage_args(gen, staging, nullptr, book, a);
    if (rc) return rc;
    const long slots = (long)a.W * a.depth;
    const int grid = (int)((slots + 63) / 64 < 1024 ? (slots + 63) / 64 : 1024);
    hipLaunchKernelGGL(k_refill_staged, dim3(grid), dim3(64), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return CS_OK;
}

int cs_consume_staged_worlds(const cs_generator* gen, const cs_worlds* staging, const cs_worlds* live, const int32_t* d_mask,
                             const cs_stage_book* book, int theta_and_omega_visible, float* d_obs, void* stream)
{
    if (!live || !d_mask || !book || !book->d_seeds || !book->d_failed) return fail(CS_ERR_ARG, "null argument");
    StageArgs a;
    const int rc = stage_args(gen, staging, live, book, a);
    if (rc) return rc;
    a.mask = d_mask;
    a.copy.obs = d_obs; a.copy.C = theta_and_omega_visible ? 7 : 5;
    hipLaunchKernelGGL(k_consume_staged, dim3(live->W), dim3(64), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return CS_OK;
}

} // extern "C"
