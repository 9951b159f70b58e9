// episodes.hip -- the device episode buffer: the per-world trajectory store behind crowd_nav/utils/explorer.py's update_memory /
// run_k_episodes (lines 80-153), and the flush that turns finished episodes into replay-memory samples with the reference's arithmetic,
// order and ring semantics (crowd_nav/utils/memory.py push, K times, world-ascending then step-ascending).  include/crowdstep.h states
// the contract; DESIGN.md 4.7 the reasons.
//
// cs_episode_append is two launches: k_episode_append_copy reads cursor[w] and stores the step's row, reward and target at [w][cursor[w]],
// k_episode_append_advance (one lane per world) moves the cursor or raises the overflow flag.  The launch boundary is the ordering: no lane
// of the copy can see a cursor the advance has moved.
//
// cs_episode_flush is three launches on the caller's stream, nothing read back:
//   k_episode_flush_scan    one block: kept_w and its exclusive prefix sum over the worlds (integers: the order cannot matter), K behind it
//   k_episode_flush_copy    one block per done world: the discount table gamma^(k dt v_w) and the rewards in LDS as float64, the ring slot of
//                           every step, the values (the return-to-go as the reference's direct sum in ascending t, rounded once; or the
//                           stored target), the float64 discounted return of the episode for the figures, and the row copy
//   k_episode_flush_finish  one block: the figures (counts, and the two float64 sums in a fixed shape: per-lane strided partial sums, then
//                           a tree), the ring's position and count, the cursors and overflow flags of the done worlds
// No floating-point atomics anywhere; a world's samples depend on that world's rows alone, so they are the same bits at W = 1 and in any
// batch.  The row copy moves 16 bytes per lane when a row is a multiple of 16 bytes and both bases are aligned (then every row start is),
// one dword per lane otherwise (F = 13: rows are not 16-byte aligned from one to the next).  gfx950 only.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "common.h"

// the reference multiplies, then adds, in float64 (explorer.py:99, 132): no fused multiply-add may replace the pair
#pragma clang fp contract(off)

namespace {

using csimpl::fail;

constexpr int EP_NT = 256;          // append, and one world's block of the flush
constexpr int EP_SCAN_NT = 1024;    // the single block of the prefix sum and of the figures
constexpr int EP_MAX_T = 2048;      // 2 x 8 + 4 bytes of LDS per step of a world: 40 KiB at 2048

template <typename V>
__global__ __launch_bounds__(EP_NT) void k_episode_append_copy(long total, int T, int FV, const V* __restrict__ state,
                                                               const float* __restrict__ reward, const float* __restrict__ target,
                                                               V* __restrict__ states, float* __restrict__ rewards, float* __restrict__ targets,
                                                               const int* __restrict__ cursor)
{
    const long idx = (long)blockIdx.x * EP_NT + threadIdx.x;
    if (idx >= total) return;
    const int w = (int)(idx / FV), col = (int)(idx - (long)w * FV);
    const int t = cursor[w];
    if (t < 0 || t >= T) return;
    const long at = (long)w * T + t;
    states[at * FV + col] = state[idx];
    if (col == 0) {
        rewards[at] = reward[w];
        if (target && targets) targets[at] = target[w];
    }
}

__global__ __launch_bounds__(EP_NT) void k_episode_append_advance(int W, int T, int* __restrict__ cursor, int* __restrict__ overflow)
{
    const int w = blockIdx.x * EP_NT + threadIdx.x;
    if (w >= W) return;
    const int t = cursor[w];
    if (t >= 0 && t < T) cursor[w] = t + 1;
    else overflow[w] = 1;
}

__device__ inline int episode_length(const int* cursor, int w, int T)
{
    const int L = cursor[w];
    return L < 0 ? 0 : (L > T ? T : L);
}

__global__ __launch_bounds__(EP_SCAN_NT) void k_episode_flush_scan(int W, int T, const int* __restrict__ cursor, const int* __restrict__ overflow,
                                                                   const uint8_t* __restrict__ done, const int* __restrict__ code,
                                                                   unsigned keep_mask, int* __restrict__ off /* [W + 1] */)
{
    __shared__ int s_wave[EP_SCAN_NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int carry = 0;
    for (int base = 0; base < W; base += EP_SCAN_NT) {
        const int w = base + tid;
        int kept = 0;
        if (w < W && done[w] && overflow[w] == 0) {
            const int c = code[w];
            if (c >= 0 && c < 32 && ((keep_mask >> c) & 1u)) kept = episode_length(cursor, w, T);
        }
        int incl = kept;
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int before = 0, chunk = 0;
        for (int k = 0; k < EP_SCAN_NT / 64; ++k) {
            const int s = s_wave[k];
            if (k < wave) before += s;
            chunk += s;
        }
        if (w < W) off[w] = carry + before + incl - kept;
        carry += chunk;
        __syncthreads();
    }
    if (tid == 0) off[W] = carry;
}

template <typename V>
__global__ __launch_bounds__(EP_NT) void k_episode_flush_copy(int W, int T, int FV, const V* __restrict__ states, const float* __restrict__ rewards,
                                                              const float* __restrict__ targets, const int* __restrict__ cursor,
                                                              const uint8_t* __restrict__ done, const int* __restrict__ off, int mode, double gamma,
                                                              double dt, double v_pref, const double* __restrict__ d_v_pref, int capacity,
                                                              V* __restrict__ mem_states, float* __restrict__ mem_values,
                                                              const long long* __restrict__ position, double* __restrict__ disc)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int w = blockIdx.x, tid = threadIdx.x;
    if (!done[w]) return;
    double* tab = reinterpret_cast<double*>(smem);          // gamma^(k dt v_w), k < L: the reference's pow(gamma, k * time_step * desired_speed)
    double* rew = tab + T;
    int* slot = reinterpret_cast<int*>(rew + T);            // the ring slot of step i, -1: not stored
    const int L = episode_length(cursor, w, T);
    const int first = off[w], kept = off[w + 1] - first;
    const long long K = off[W], pos = *position;
    const double v = d_v_pref ? d_v_pref[w] : v_pref;
    for (int t = tid; t < L; t += EP_NT) {
        tab[t] = pow(gamma, ((double)t * dt) * v);
        rew[t] = (double)rewards[(long)w * T + t];
        const long long g = (long long)first + t;
        slot[t] = kept > 0 && g >= K - (long long)capacity ? (int)((pos + g) % (long long)capacity) : -1;
    }
    if (L == 0 && tid == 0) disc[w] = 0.0;
    __syncthreads();
    for (int i = tid; i < L; i += EP_NT) {
        const int s = slot[i];
        const bool returns = mode == CS_EPISODE_RETURNS && s >= 0;
        if (returns || i == 0) {
            double sum = 0.0;
            for (int t = i; t < L; ++t) sum = sum + tab[t - i] * rew[t];
            if (i == 0) disc[w] = sum;
            if (returns) mem_values[s] = (float)sum;
        }
        if (s >= 0 && mode != CS_EPISODE_RETURNS) mem_values[s] = targets[(long)w * T + i];
    }
    if (kept == 0) return;
    // the rows: consecutive lanes on consecutive elements of the world's L rows; (row, col) advance without a division
    const V* src = states + (long)w * T * FV;
    const int drow = EP_NT / FV, dcol = EP_NT - drow * FV;
    int row = tid / FV, col = tid - row * FV;
    while (row < L) {
        const int s = slot[row];
        if (s >= 0) mem_states[(long)s * FV + col] = src[(long)row * FV + col];
        row += drow;
        col += dcol;
        if (col >= FV) { col -= FV; ++row; }
    }
}

__global__ __launch_bounds__(EP_SCAN_NT) void k_episode_flush_finish(int W, int T, int* __restrict__ cursor, int* __restrict__ overflow,
                                                                     const uint8_t* __restrict__ done, const int* __restrict__ code,
                                                                     const int* __restrict__ off, const double* __restrict__ disc, double dt,
                                                                     int capacity, long long* __restrict__ position, long long* __restrict__ count,
                                                                     double* __restrict__ figures)
{
    __shared__ double s_nav[EP_SCAN_NT], s_disc[EP_SCAN_NT];
    __shared__ int s_count[4];
    const int tid = threadIdx.x;
    if (tid < 4) s_count[tid] = 0;
    __syncthreads();
    int episodes = 0, n2 = 0, n3 = 0, n4 = 0;
    double nav = 0.0, dsum = 0.0;
    for (int w = tid; w < W; w += EP_SCAN_NT) {
        if (!done[w]) continue;
        const int c = code[w];
        ++episodes;
        if (c == 2) { ++n2; nav = nav + (double)episode_length(cursor, w, T) * dt; }
        else if (c == 3) ++n3;
        else if (c == 4) ++n4;
        dsum = dsum + disc[w];
        cursor[w] = 0;
        overflow[w] = 0;
    }
    s_nav[tid] = nav;
    s_disc[tid] = dsum;
    if (episodes) atomicAdd(&s_count[0], episodes);
    if (n2) atomicAdd(&s_count[1], n2);
    if (n3) atomicAdd(&s_count[2], n3);
    if (n4) atomicAdd(&s_count[3], n4);
    __syncthreads();
    for (int half = EP_SCAN_NT / 2; half > 0; half >>= 1) {
        if (tid < half) {
            s_nav[tid] = s_nav[tid] + s_nav[tid + half];
            s_disc[tid] = s_disc[tid] + s_disc[tid + half];
        }
        __syncthreads();
    }
    if (tid == 0) {
        for (int k = 0; k < 4; ++k) figures[k] = figures[k] + (double)s_count[k];
        figures[4] = figures[4] + s_nav[0];
        figures[5] = figures[5] + s_disc[0];
        const long long K = off[W];
        *position = (*position + K) % (long long)capacity;
        const long long have = *count + K;
        *count = have < (long long)capacity ? have : (long long)capacity;
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

} // namespace

extern "C" int cs_episode_append(int W, int T, int F, const float* d_state, const float* d_reward, const float* d_target, float* d_states,
                                 float* d_rewards, float* d_targets, int32_t* d_cursor, int32_t* d_overflow, void* stream)
{
    if (!d_state || !d_reward || !d_states || !d_rewards || !d_cursor || !d_overflow) return fail(CS_ERR_ARG, "null argument");
    if (W < 1 || T < 1 || F < 1) return fail(CS_ERR_ARG, "W, T, F must be positive");
    if (T > EP_MAX_T) return fail(CS_ERR_ARG, "max_steps above 2048");
    if ((long)W * T > INT_MAX) return fail(CS_ERR_ARG, "W * T is too large");
    if (d_target && !d_targets) return fail(CS_ERR_ARG, "a target given to a store without targets");
    hipStream_t s = (hipStream_t)stream;
    const bool wide = F % 4 == 0 && aligned16(d_state) && aligned16(d_states);
    const int FV = wide ? F / 4 : F;
    const long total = (long)W * FV;
    const long grid = (total + EP_NT - 1) / EP_NT;
    if (grid > INT_MAX) return fail(CS_ERR_ARG, "W * F is too large");
    if (wide)
        hipLaunchKernelGGL(k_episode_append_copy<float4>, dim3((unsigned)grid), dim3(EP_NT), 0, s, total, T, FV,
                           reinterpret_cast<const float4*>(d_state), d_reward, d_target, reinterpret_cast<float4*>(d_states), d_rewards, d_targets,
                           d_cursor);
    else
        hipLaunchKernelGGL(k_episode_append_copy<float>, dim3((unsigned)grid), dim3(EP_NT), 0, s, total, T, FV, d_state, d_reward, d_target,
                           d_states, d_rewards, d_targets, d_cursor);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_episode_append_advance, dim3((W + EP_NT - 1) / EP_NT), dim3(EP_NT), 0, s, W, T, d_cursor, d_overflow);
    HIP_TRY(hipGetLastError());
    return CS_OK;
}

extern "C" int cs_episode_flush(int W, int T, int F, const float* d_states, const float* d_rewards, const float* d_targets, int32_t* d_cursor,
                                int32_t* d_overflow, const uint8_t* d_done, const int32_t* d_code, unsigned keep_mask, int target_mode,
                                double gamma, double dt, double v_pref, const double* d_v_pref, int capacity, float* d_mem_states,
                                float* d_mem_values, void* d_position, void* d_count, double* d_figures, void* d_scratch, void* stream)
{
    if (!d_states || !d_rewards || !d_cursor || !d_overflow || !d_done || !d_code || !d_mem_states || !d_mem_values || !d_position || !d_count ||
        !d_figures || !d_scratch)
        return fail(CS_ERR_ARG, "null argument");
    if (W < 1 || T < 1 || F < 1 || capacity < 1) return fail(CS_ERR_ARG, "W, T, F and the capacity must be positive");
    if (T > EP_MAX_T) return fail(CS_ERR_ARG, "max_steps above 2048");
    if ((long)W * T > INT_MAX) return fail(CS_ERR_ARG, "W * T is too large");
    if (target_mode != CS_EPISODE_RETURNS && target_mode != CS_EPISODE_STORED)
        return fail(CS_ERR_ARG, "unknown target mode (CS_EPISODE_RETURNS, CS_EPISODE_STORED)");
    if (target_mode == CS_EPISODE_STORED && !d_targets) return fail(CS_ERR_ARG, "CS_EPISODE_STORED needs the targets given at append");
    if (!(gamma > 0.0 && gamma <= 1.0)) return fail(CS_ERR_ARG, "gamma must lie in (0, 1]");
    if (!(dt > 0.0)) return fail(CS_ERR_ARG, "the time step must be positive");
    if (reinterpret_cast<uintptr_t>(d_scratch) & 7u) return fail(CS_ERR_ARG, "d_scratch must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    double* disc = static_cast<double*>(d_scratch);
    int* off = reinterpret_cast<int*>(disc + W);
    hipLaunchKernelGGL(k_episode_flush_scan, dim3(1), dim3(EP_SCAN_NT), 0, s, W, T, d_cursor, d_overflow, d_done, d_code, keep_mask, off);
    HIP_TRY(hipGetLastError());
    const bool wide = F % 4 == 0 && aligned16(d_states) && aligned16(d_mem_states);
    const int FV = wide ? F / 4 : F;
    const size_t lds = (size_t)T * (2 * sizeof(double) + sizeof(int));
    if (wide)
        hipLaunchKernelGGL(k_episode_flush_copy<float4>, dim3(W), dim3(EP_NT), lds, s, W, T, FV, reinterpret_cast<const float4*>(d_states), d_rewards,
                           d_targets, d_cursor, d_done, off, target_mode, gamma, dt, v_pref, d_v_pref, capacity,
                           reinterpret_cast<float4*>(d_mem_states), d_mem_values, static_cast<const long long*>(d_position), disc);
    else
        hipLaunchKernelGGL(k_episode_flush_copy<float>, dim3(W), dim3(EP_NT), lds, s, W, T, FV, d_states, d_rewards, d_targets, d_cursor, d_done, off,
                           target_mode, gamma, dt, v_pref, d_v_pref, capacity, d_mem_states, d_mem_values,
                           static_cast<const long long*>(d_position), disc);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_episode_flush_finish, dim3(1), dim3(EP_SCAN_NT), 0, s, W, T, d_cursor, d_overflow, d_done, d_code, off, disc, dt, capacity,
                       static_cast<long long*>(d_position), static_cast<long long*>(d_count), d_figures);
    HIP_TRY(hipGetLastError());
    return CS_OK;
}
