// value_net_state.hip -- the value network on the worlds' CURRENT state: for W worlds, the rotated joint state the robot acts from (what a
// trainer stores: policy.transform, crowd_nav/policy/multi_human_rl.py:115-128, cadrl.py:305-345) and reward + gamma^(dt * v_pref) * V(s)
// (the trainer's target, crowd_nav/utils/explorer.py:120-153; plain V(s) with no rewards and dt = 0).  The decide kernels always evaluate
// (world, action) look-ahead groups; here a group is a world as it stands.
//
// The kernel is value_net.hip's (value_net_body.inc with A = 1: the same tiles, workgroups, layers and reductions, value_net_f32.h's
// arithmetic, cs_value_net_pack's blob) with a fourth tile loader, value_net_worlds.hip's on other rows (the frame, la_row_quad and
// la_wave_quad are lookahead_math.h's).  Once per job, lane k of wavefront 0 computes the frame of world gbase + k from its robot row
// (la_state_frame: the look-ahead frame for action = the robot's velocity and a step of 0) into a table of 32 x LA_FRAME_FLOATS floats
// behind the LDS map; the job's first barrier publishes it.  A tile is written as there, but la_row_quad reads the human's current row
// where the look-ahead has its next row -- the headed layout (px, py, vx, vy, radius, theta, omega) is mapped onto (x, y, yaw, Vx, Vy,
// Omega) here, which is why this loader stays its own.  A world in chunks (n > 32) regenerates a chunk at each of SARL's passes.  With
// d_rotated_out the tile's rows -- one dense run of rows * cols floats of [W][n][cols] -- are also stored from LDS, 16 bytes a lane between the run's first
// and last 16-byte boundary (a run starts at any float: cols is odd), the first time the tile holds them.  The rows are cs_lookahead's
// for (action = robot velocity, dt = 0, next = current) to the last bit.  No atomics.  gfx950 only.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "lookahead_math.h"
#include "value_net_f32.h"

namespace {

struct StateRows {
    const float* __restrict__ cur;         // [W][n][5 | 7]
    const float* __restrict__ robot;
    float* __restrict__ rotated_out;       // [W][n][13 | 15] or null
    float* frames;                         // LDS [JROWS][LA_FRAME_FLOATS]: the frames of the job's worlds (LA_REWARD unused)
    int rstride, headed, n;
};

__device__ __forceinline__ void begin_job(const StateRows& s, int gbase, int ng)
{
    const int k = threadIdx.x;
    if (k >= ng) return;                   // (ng <= JROWS: lanes of wavefront 0)
    la_state_frame(s.robot + (long)(gbase + k) * s.rstride, s.frames + LA_FRAME_FLOATS * k);
}

// columns [4 Q, 4 Q + 4) of the tile's rows: row r belongs to the tile's world r / per (the job's t0 + r / per, the launch's g0 + r / per) and
// is its human ch * M + r % per
template <int Q>
__device__ __forceinline__ void generate_quad(const StateRows& s, const VnBufs& b, int t0, int g0, int ch, int rows, int per, int M)
{
    const int r = threadIdx.x & 63;
    if (r >= M) return;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (r < rows) {
        const int k = r / per, j = ch * M + r - k * per;
        const long w = g0 + k;
        const bool h = s.headed != 0;
        const float* rb = s.robot + w * s.rstride;
        const float* c = s.cur + (w * s.n + j) * (h ? 7 : 5);
        // the current row where la_row_quad reads a next row: (px, py, vx, vy), or headed (x, y, yaw, Vx, Vy, Omega) -- theta and omega
        // stand behind the radius in a current row
        const float q[6] = {c[0], c[1], c[h ? 5 : 2], c[h ? 2 : 3], c[h ? 3 : 0], c[h ? 6 : 0]};
        v = la_row_quad<Q>(s.frames + LA_FRAME_FLOATS * (t0 + k), q, c[4], rb[7], rb[4], h);
    }
    *reinterpret_cast<float4*>(b.X0 + r * LDX + 4 * Q) = v;
    if (Q == 0) b.grp[r] = r < rows ? r / per : 0;
}

__device__ __forceinline__ void generate_tile(const StateRows& s, const VnBufs& b, int t0, int g0, int ch, int rows, int per, int M)
{
    la_wave_quad([&](auto Q) { generate_quad<Q()>(s, b, t0, g0, ch, rows, per, M); });
}

// The tile's rows to rotated_out: they are the `rows * cols` floats from float `first` of the dense output on.  Float4 stores between the
// run's first and last 16-byte boundary, the at most three floats before and after them one a lane.  After a barrier behind generate_tile.
__device__ __forceinline__ void store_tile(const StateRows& s, const VnBufs& b, long first, int rows, int cols)
{
    float* dst = s.rotated_out + first;
    const int total = rows * cols;
    const int lead = (int)((4 - ((reinterpret_cast<uintptr_t>(dst) >> 2) & 3)) & 3);
    const int head = lead < total ? lead : total;
    const int quads = (total - head) >> 2;
    const int tail0 = head + 4 * quads;
    auto at = [&](int i) { const int r = i / cols; return b.X0[r * LDX + i - r * cols]; };
    for (int i = threadIdx.x; i < quads; i += NT) {
        const int e = head + 4 * i;
        *reinterpret_cast<float4*>(dst + e) = make_float4(at(e), at(e + 1), at(e + 2), at(e + 3));
    }
    const int t = threadIdx.x;
    if (t < head + total - tail0) {
        const int e = t < head ? t : tail0 + t - head;
        dst[e] = at(e);
    }
}

// `frames`: floats from the start of the dynamic block to the frame table, behind the map m that the decide kernels share
__global__ __launch_bounds__(NT) void k_value_net_state(VnPlan p, VnLds m, int frames, int M, const float* __restrict__ wb, int NG, int n, int headed,
                                                        const float* __restrict__ cur, const float* __restrict__ robot, int rstride,
                                                        const float* __restrict__ rewards, float gamma, float dt, float* __restrict__ rotated_out,
                                                        float* __restrict__ values)
{
    extern __shared__ float lds[];
    constexpr int A = 1;                   // a group is a world
    const int gsum = m.G;
    const StateRows world{cur, robot, rotated_out, lds + frames, rstride, headed, n};
#define VN_BEGIN_JOB(gbase, ng) begin_job(world, gbase, ng)
    // (tile_visit: the first `chunks` loads of a tile are its chunks 0 .. chunks - 1, whichever of the body's passes comes first)
#define VN_TILE_SOURCE(g0) const int tile_g0 = (g0); int tile_visit = 0
#define VN_LOAD_TILE(ch, rows, per)                                                                                   \
    do {                                                                                                              \
        generate_tile(world, b, t0, tile_g0, ch, rows, per, M);                                                       \
        if (world.rotated_out && tile_visit++ < chunks) {                                                             \
            __syncthreads();                                                                                          \
            store_tile(world, b, ((long)tile_g0 * n + (ch) * M) * cols, rows, cols);                                  \
        }                                                                                                             \
    } while (0)
#define VN_REWARD(g, k) (rewards ? rewards[g] : 0.0f)
#include "value_net_body.inc"
#undef VN_BEGIN_JOB
#undef VN_TILE_SOURCE
#undef VN_LOAD_TILE
#undef VN_REWARD
}

} // namespace

extern "C" int cs_value_net_state(int kind, const int32_t* dims, int n_dims, const float* d_weights, size_t n_weight_floats, int W, int n,
                                  int theta_and_omega_visible, const float* d_current, const float* d_robot, int robot_stride,
                                  const float* d_rewards, float gamma, float dt, float* d_rotated_out, float* d_values, void* stream)
{
    VnPlan p;
    const int rc = build_plan(kind, dims, n_dims, theta_and_omega_visible ? 15 : 13, 0, p);
    if (rc != CS_OK) return rc;
    // (check_decide_args' checks in its order, without the action table: d_rewards and d_rotated_out may be null)
    if (W < 1) return fail(CS_ERR_ARG, "W must be positive");
    if (n < 1) return fail(CS_ERR_ARG, "n must be at least 1: a value network needs a human to look at");
    if (W > INT_MAX / 2 || (long)W * n > (1L << 40)) return fail(CS_ERR_ARG, "W * n is too large");
    if (!d_weights || !d_current || !d_robot || !d_values) return fail(CS_ERR_ARG, "null argument");
    if (n_weight_floats != (size_t)p.total_floats) return fail(CS_ERR_ARG, "the weight blob does not have the size of this network (cs_value_net_pack)");
    if (robot_stride < 8) return fail(CS_ERR_ARG, "robot rows need at least 8 columns: px,py,vx,vy,r,gx,gy,v_pref");
    VnLaunch q;
    const int rc2 = prepare_launch<k_value_net_state>(p, n, JROWS * LA_FRAME_FLOATS, W, 1, q);      // (the tail: the frame table)
    if (rc2 != CS_OK) return rc2;
    hipLaunchKernelGGL(k_value_net_state, dim3(q.grid), dim3(NT), q.shmem, (hipStream_t)stream, p, q.m, q.tail, TILE_M, d_weights, q.NG, n,
                       theta_and_omega_visible ? 1 : 0, d_current, d_robot, robot_stride, d_rewards, gamma, dt, d_rotated_out, d_values);
    HIP_TRY(hipGetLastError());
    return CS_OK;
}
