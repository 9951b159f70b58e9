// occupancy_map.hip -- the local occupancy maps of OM-SARL (crowd_nav/policy/multi_human_rl.py:133-187 build_occupancy_maps), for W worlds:
// for every human i a grid of cell_num x cell_num cells of cell_size metres, centred on i, whose x axis is i's velocity (the world's when
// i stands), filled from the OTHER humans of its world -- occupied or not, and / or the mean velocity of a cell's members in that frame.
// The maps depend on the humans alone, not on the robot's action: one row [C = cell_num^2 * channels] per (world, human).
//
// Mapping: one lane per output cell (world, human, cell).  The lane walks the other humans j in ascending order, recomputes j's cell (a
// handful of float operations: the loads are the same addresses for the lanes of one human, served as broadcasts from L1) and adds j's
// frame velocity when the cell is its own.  So there is no per-lane accumulator array with a run-time index (scratch), no LDS, no atomics,
// and the sums run in ascending j whatever the batch: a world gives the same bits alone and among 4096.  The frame is applied by dot and
// cross products with u = v_i / |v_i| -- the same point as the reference's |d| (cos, sin)(atan2(d) - atan2(v_i)) without the three
// transcendentals; a coincident pair gives exactly (0, 0), a NaN fails every comparison and is counted nowhere.  gfx950 only.
#include <hip/hip_runtime.h>

#include <climits>

#include "common.h"

namespace {

using csimpl::fail;

constexpr int OM_NT = 256;
constexpr int OM_MAX_COLS = 241;       // 15 + C <= 256, the widest layer input of the value-network kernels

__global__ __launch_bounds__(OM_NT) void k_occupancy_maps(int total, int n, const float* __restrict__ humans, int stride, int vel_col, int cell_num,
                                                          float cell_size, int channels, float* __restrict__ maps)
{
    const int idx = blockIdx.x * OM_NT + threadIdx.x;
    if (idx >= total) return;
    const int cells = cell_num * cell_num;
    const int wi = idx / cells, cell = idx - wi * cells;       // wi = world * n + human
    const int w = wi / n, i = wi - w * n;
    const float* world = humans + (long)w * n * stride;
    const float* me = world + (long)i * stride;
    const float px = me[0], py = me[1], vx = me[vel_col], vy = me[vel_col + 1];
    const float speed = hypotf(vx, vy);
    const float ux = speed == 0.0f ? 1.0f : vx / speed, uy = speed == 0.0f ? 0.0f : vy / speed;     // atan2(0, 0) = 0: the world's frame
    const float half = 0.5f * (float)cell_num, edge = (float)cell_num;
    float count = 0.0f, sx = 0.0f, sy = 0.0f;
    for (int j = 0; j < n; ++j) {
        if (j == i) continue;
        const float* o = world + (long)j * stride;
        const float dx = o[0] - px, dy = o[1] - py;
        const float fx = floorf((dx * ux + dy * uy) / cell_size + half);
        const float fy = floorf((dy * ux - dx * uy) / cell_size + half);
        if (!(fx >= 0.0f && fx < edge && fy >= 0.0f && fy < edge)) continue;
        if ((int)fy * cell_num + (int)fx != cell) continue;
        const float ovx = o[vel_col], ovy = o[vel_col + 1];
        count += 1.0f;
        sx += ovx * ux + ovy * uy;
        sy += ovy * ux - ovx * uy;
    }
    const float occ = count > 0.0f ? 1.0f : 0.0f;
    const float mx = count > 0.0f ? sx / count : 0.0f, my = count > 0.0f ? sy / count : 0.0f;
    float* out = maps + (long)idx * channels;
    if (channels == 1) out[0] = occ;
    else if (channels == 2) { out[0] = mx; out[1] = my; }
    else { out[0] = occ; out[1] = mx; out[2] = my; }
}

} // namespace

extern "C" int cs_occupancy_maps(int W, int n, const float* d_humans, int stride, int vel_col, int cell_num, float cell_size, int channels,
                                 float* d_maps, void* stream)
{
    if (W < 1 || n < 1) return fail(CS_ERR_ARG, "W and n must be positive");
    if (!d_humans || !d_maps) return fail(CS_ERR_ARG, "null argument");
    if (stride < 4) return fail(CS_ERR_ARG, "human rows need at least 4 columns: px, py and a velocity");
    if (vel_col < 2 || vel_col > stride - 2) return fail(CS_ERR_ARG, "vel_col must lie in 2 .. stride - 2");
    if (cell_num < 1) return fail(CS_ERR_ARG, "cell_num must be positive");
    if (!(cell_size > 0.0f)) return fail(CS_ERR_ARG, "cell_size must be positive");
    if (channels < 1 || channels > 3) return fail(CS_ERR_ARG, "om_channel_size must be 1, 2 or 3");
    if (cell_num > 15 || cell_num * cell_num * channels > OM_MAX_COLS)
        return fail(CS_ERR_ARG, "cell_num^2 * om_channel_size exceeds 241 map columns (15 + 241 = 256, a layer's widest input)");
    const long total = (long)W * n * cell_num * cell_num;
    if (total * channels > INT_MAX) return fail(CS_ERR_ARG, "W * n * cell_num^2 * om_channel_size is too large");
    const int grid = (int)((total + OM_NT - 1) / OM_NT);
    hipLaunchKernelGGL(k_occupancy_maps, dim3(grid), dim3(OM_NT), 0, (hipStream_t)stream, (int)total, n, d_humans, stride, vel_col, cell_num,
                       cell_size, channels, d_maps);
    HIP_TRY(hipGetLastError());
    return CS_OK;
}
