// policy_orca.hip -- the CrowdNav ORCA robot policy, batched: one launch gives the ActionXY of the robots of W worlds.  Replaces
// ORCA.predict (reference: crowd_nav/policy_no_train/orca.py:82-132), which builds a fresh RVO2 simulator per decision, adds the robot as
// agent 0 and the humans behind it, runs ONE doStep and reads agent 0's new velocity.  Only agent 0 is solved here.
//
// The decision, stated once:
//   inputs     the robot's 13-column safe-state row (px, py, ., vx, vy, ., ., ., radius, ., gx, gy, v_pref) and the n observation rows
//              [n][5|7] (px, py, vx, vy, radius[, theta, omega]) -- what cs_policy_no_train reads.
//   agents     the robot is agent 0: radius `radius + margin`, maxSpeed v_pref.  Human j is agent j + 1: radius `radius_j + margin`
//              (its preferred velocity (0, 0) and maxSpeed do not enter agent 0's solve).  margin = float32(0.01 + safety_space) comes from
//              the host and is added in float32, as the crowd kernels add theirs.
//   preferred  d = g - p, s = sqrt(d.x * d.x + d.y * d.y), pref = s > 1 ? d / s : d (orca.py:113-115): the test is strict, the operation
//   velocity   an IEEE division (no reciprocal multiply), the bound 1 and not v_pref.  linearProgram2 then clips pref to the maxSpeed circle.
//   neighbours the humans with distSq < neighbor_dist^2 (strict); the list is the first max_neighbors of them in ascending
//              (distSq, human index) order -- what RVO2's insertion keeps after a walk in index order (insert_neighbor in orca.hip: strict <,
//              ties keep the order, the range shrinks to the farthest kept neighbour once the list is full).
//   lines      one ORCA half-plane per neighbour in list order (orca_line; a colliding pair uses 1 / time_step), linearProgram2 on them,
//   and solve  linearProgram3 where that programme is infeasible.
//   arithmetic exact only: IEEE divide and square root, no contraction (FM = 0 of the crowd kernel) -- the restatement's operations on the
//              restatement's operands, so the result has the bits of oracle/orca_oracle.c's agent 0.
//   output     the robot's new velocity as the ActionXY row [vx, vy].  Nothing else is written, no position is advanced.
//
// Mapping: one wavefront per world, four per block, lanes over humans (a loop of stride 64 beyond 64 humans); whole wavefronts leave
// together for w >= W.  A lane holds the key (distSq, index) of its human; its place in the list is its RANK -- the number of keys before
// its own -- counted against every human's distSq, which a v_readlane with a wave-uniform lane index fetches from the lane that holds it:
// no sort, no dependent cross-lane chain, and a function of the key SET alone.  The lanes of rank < max_neighbors build their half-planes
// in parallel and store them in the wavefront's LDS lines at their rank.  The linear programme is the generic lp2 / lp3 of orca_solve.h on
// lane 0, reading those lines: the very code the robot's motion model (k_orca_robot_step) and the generic crowd path run per lane.
// No value depends on what the other wavefronts of the block hold: a world gives the same bits alone (predict(), W = 1) and in any batch.
// gfx950 only.
#include <hip/hip_runtime.h>

#include <cmath>

#include "common.h"
#include "orca_solve.h"

namespace {

using csimpl::fail;

constexpr int WAVE = 64;
constexpr int WAVES_PER_BLOCK = 4;
constexpr int KMAX = 10;             // neighbours (= ORCA lines) kept at most; the reference's max_neighbors

__global__ __launch_bounds__(WAVE * WAVES_PER_BLOCK) void k_policy_orca(int W, int n, const float* __restrict__ robot,
                                                                        const float* __restrict__ obs, int oc, float time_step,
                                                                        float neighbor_dist, int K, float time_horizon, float margin,
                                                                        float* __restrict__ action)
{
    // per wavefront: [0, KMAX) the ORCA lines in list order, [KMAX, 2 KMAX) linearProgram3's projected lines (at most KMAX - 1)
    __shared__ float4 lds_lines[WAVES_PER_BLOCK][2 * KMAX];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wv = threadIdx.x >> 6;
    const int w = blockIdx.x * WAVES_PER_BLOCK + wv;
    if (w >= W) return;                       // whole wavefronts leave together: no lane of a live world is missing below
    const float* rb = robot + (long)w * 13;
    const float px = rb[0], py = rb[1], vx = rb[3], vy = rb[4], gx = rb[10], gy = rb[11], vmax = rb[12];
    const float my_r = rb[8] + margin;
    const float* ow = obs + (long)w * n * oc;
    float4* Lw = lds_lines[wv];

    // preferred velocity (orca.py:113-115)
    const float gdx = gx - px, gdy = gy - py;
    const float gs = sqrtf(gdx * gdx + gdy * gdy);
    float pvx = gdx, pvy = gdy;
    if (gs > 1.0f) { pvx = gdx / gs; pvy = gdy / gs; }

    const float range2 = neighbor_dist * neighbor_dist;
    const float invT = 1.0f / time_horizon;
    const float invDt = 1.0f / time_step;
    int in_range = 0;
    for (int base = 0; base < n && K > 0; base += WAVE) {
        // my human of this chunk (a lane beyond n reads row 0: finite, never used)
        const int j = base + lane;
        const bool have = j < n;
        const float* h = ow + (long)(have ? j : 0) * oc;
        const float4 q = make_float4(h[0], h[1], h[2], h[3]);
        const float hr = h[4];
        const float ddx = px - q.x, ddy = py - q.y;
        const float dsq = ddx * ddx + ddy * ddy;
        const bool in = have && dsq < range2;
        const unsigned long long in_m = __builtin_amdgcn_ballot_w64(in);
        if (in_m == 0) continue;
        in_range += __builtin_popcountll(in_m);
        // rank of my key (distSq, j): the humans b with distSq_b < distSq, or the same distSq and b < j -- such a b is in range whenever I am
        int rank = 0;
        for (int cb = 0; cb < n; cb += WAVE) {
            float dc = dsq;                  // the chunk's distances, lane l holding human cb + l (my own chunk: what I have)
            if (cb != base) {
                const float* hc = ow + (long)(cb + lane < n ? cb + lane : 0) * oc;
                const float cx = px - hc[0], cy = py - hc[1];
                dc = cx * cx + cy * cy;
            }
            const int m = n - cb < WAVE ? n - cb : WAVE;
            for (int l = 0; l < m; ++l) {
                const float db = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dc), l));
                rank += (db < dsq || (db == dsq && cb + l < j)) ? 1 : 0;
            }
        }
        if (in && rank < K) Lw[rank] = orca_line(px, py, vx, vy, q, my_r + (hr + margin), invT, invDt);
    }
    const int cnt = in_range < K ? in_range : K;
    // the lines were stored by other lanes of this wavefront: LDS operations of one wavefront complete in order, the fence keeps the
    // compiler from moving lane 0's reads above the stores
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane != 0) return;
    const Lines L{Lw, 1, 0}, P{Lw + KMAX, 1, 0};
    float rx, ry;
    const int failed = lp2(L, cnt, vmax, pvx, pvy, false, rx, ry);
    if (failed < cnt) lp3(L, P, cnt, 0, failed, vmax, rx, ry);
    float* out = action + (long)w * 2;
    out[0] = rx;
    out[1] = ry;
}

} // namespace

extern "C" int cs_policy_orca(int W, int n, const float* d_robot13, const float* d_obs, int obs_cols, float time_step, float neighbor_dist,
                              int max_neighbors, float time_horizon, float margin, float* d_action, void* stream)
{
    if (W < 1) return fail(CS_ERR_ARG, "cs_policy_orca: W must be >= 1");
    if (n < 0) return fail(CS_ERR_ARG, "cs_policy_orca: n must be >= 0");
    if (obs_cols != 5 && obs_cols != 7) return fail(CS_ERR_ARG, "cs_policy_orca: observation rows have 5 or 7 columns");
    if (!d_robot13) return fail(CS_ERR_ARG, "cs_policy_orca: null robot rows");
    if (!d_action) return fail(CS_ERR_ARG, "cs_policy_orca: null action rows");
    if (n > 0 && !d_obs) return fail(CS_ERR_ARG, "cs_policy_orca: null observation rows with n > 0");
    if (!(time_step > 0.0f)) return fail(CS_ERR_ARG, "cs_policy_orca: time_step must be positive");
    if (!(time_horizon > 0.0f)) return fail(CS_ERR_ARG, "cs_policy_orca: time_horizon must be positive");
    if (!(neighbor_dist >= 0.0f)) return fail(CS_ERR_ARG, "cs_policy_orca: neighbor_dist must not be negative");
    if (max_neighbors < 0 || max_neighbors > KMAX) return fail(CS_ERR_ARG, "cs_policy_orca: max_neighbors must be in 0..10 (the kernel keeps at most ten neighbours)");
    const int blocks = (W + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    hipLaunchKernelGGL(k_policy_orca, dim3(blocks), dim3(WAVE * WAVES_PER_BLOCK), 0, (hipStream_t)stream, W, n, d_robot13, d_obs, obs_cols,
                       time_step, neighbor_dist, max_neighbors, time_horizon, margin, d_action);
    HIP_TRY(hipGetLastError());
    return CS_OK;
}
