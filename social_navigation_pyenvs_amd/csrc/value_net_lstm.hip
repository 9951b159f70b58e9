// value_net_lstm.hip -- LSTM-RL's decision (crowd_nav/policy/lstm_rl.py with multi_human_rl.py:46-63): for every (world, action) the n
// rotated rows sorted by decreasing distance to the robot's next position (column 11), [mlp1 on every row,] an LSTM over the rows from
// zero (h, c), mlp on (the first six columns of the first row, h_n), then compute_action_value and the per-world pick of the other
// decision kernels (value_net_pick.h).  Not a variant of value_net_body.inc: the order of a group's rows depends on the action, and the
// network is n dependent steps.
//
// Shape of the work.  A workgroup (4 wavefronts) owns a tile of 32 sequences = 32 consecutive (world, action) pairs.
//   order       the sort keys of the tile's 32 x n distances go to LDS as integers that order like the floats (NaN above everything, the
//               zeros equal); the rank of row j is the number of rows k with key_k > key_j, or key_k == key_j and k > j -- O(n^2) compares,
//               always a permutation; perm[s][rank] = j stays in LDS.  sorted_by_distance = 0: the identity.
//   step t      the 32 rows perm[s][t] are gathered from d_rotated (the gather of step t + 1 is issued before the products of step t);
//               network 2 runs mlp1 on them (lstm_layer: layer_fwd of value_net_plan.h for one row block).  A sequence's joint row in LDS
//               is (h of the step before | x_t), double-buffered: the gates read one row, with no choice of source per k-group.
//   gates       the TRANSPOSED product on v_mfma_f32_32x32x2_f32: the A operand is the gate weights, the B operand the sequences' joint
//               rows from LDS, so the MFMA's column (lane & 31) is the sequence and its 32 rows are gate rows.  The pack orders the gate
//               rows of block b as 8 * gate + unit (8 hidden units x the gates i, f, g, o; ceil(H / 8) blocks); with the C/D map row =
//               (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) a lane holds i, f, g, o of four hidden units of one sequence in its own 16
//               accumulators: the pointwise part needs no LDS round trip, c stays in registers for all n steps, and only h goes back to
//               LDS (into the other joint-row buffer, one barrier per step) as the next step's B operand.  Wavefront w owns the blocks w, w + 4, ...
//   weights     a network of at most 8 blocks and at most 14 k-groups of 8 (H <= 64 and, each rounded up to 8, inputs + H <= 112: the
//               reference's defaults are H = 50 on 13 columns, 7 blocks x 9 k-groups, and on mlp1's 50, 7 x 14) keeps its wavefront's gate
//               weights in registers across steps and tiles (k_value_net_lstm<true, .>); wider ones read them from the blob at every step
//               (<false, .>).  Same operations in the same order.  The second template argument is network 2's mlp1 in the step loop.
//   end         mlp on the 32 joint rows (self state, h_n) as one 32-row block, the action value, one float per sequence goes out.
//   map columns OM-LSTM-RL (lstm_rl.with_om = true; cs_value_net_decide_lstm_om) is the same body, value_net_lstm_body.inc, included a second
//               time as k_value_net_lstm_om<WREG, MLP1>: a row is the rotated row followed by the om_cols columns of a map row of its world,
//               d_maps [W][n][om_cols] read in place.  Which map: the row's own (CS_VN_MAPS_OWN) or the one at that place of the order of the
//               world's action 0 (CS_VN_MAPS_FIRST_ACTION, the reference's serial decision), for which every workgroup ranks the rows of its
//               sequences' (world, action 0) itself: a second key array and rank pass in LDS.  Network 1's joint row and gate k range widen,
//               network 2's gather tile and mlp1's first layer do; the register-resident build holds 15 k-groups (16 would leave one wave per
//               SIMD: DESIGN.md 4.5), and network 1's P buffer lies over the joint rows, dead by then, to keep two workgroups a CU.  The four
//               builds of k_value_net_lstm are the preprocessor's LSTM_OM 0 text: the instructions they had before.
//   shared      with k_value_net_lstm_bf16 (value_net_lstm_bf16.hip), in value_net_lstm_kernel.h: the layer table, a job's start, the rank pass,
//               the self state, h_n into J, the value store, lstm_layer (both arithmetics; here false, false) and lstm_chain, and the host's
//               checks and (wreg, mlp1) choice of a decide entry.  This file keeps what is its own: the pack of the gates, the gather with
//               map columns, the two kernels around the body and its step loop, the entries (the LDS map is value_net_lstm_f32.h's).
//   worlds      k_value_net_lstm_worlds (value_net_lstm_worlds.hip, cs_value_net_decide_lstm_worlds) is the body a third time, LSTM_OM 0, with
//               the three seams of a job's input (value_net_lstm_kernel.h) redefined: its rows are generated from the worlds, not gathered.
//
// Numerics: float32.  Every gate pre-activation is one fixed fmaf chain from b_ih + b_hh (summed in float32 by the pack) over the k-groups in
// descending order (x_t's, then h's); sigmoid(x) = rcp(1 + exp2(-x * log2 e)), tanh(x) = sign(x) * (1 - e) * rcp(1 + e) with e = exp2(-2 |x| * log2 e) on
// v_exp_f32 and v_rcp_f32 (1 ulp each): an absolute error below 3e-7 each, no overflow (e <= 1; exp2 -> inf gives sigmoid 0), NaN stays.
// Hidden units beyond H are stored as 0 whatever the inputs.  A sequence's result depends on its own rows alone: the same bits for W = 1 as
// inside any batch, at any position of a tile.  No atomics.  gfx950 only.
#include <hip/hip_runtime.h>

#include "value_net_lstm_f32.h"

namespace {

// (RKG, RKG_OM, the register-resident k-groups, and LstmLds / lstm_lds_map, the LDS map, are value_net_lstm_f32.h's: value_net_lstm_worlds.hip
// uses them too)

// the gate rows where the lanes of the transposed product read them: row 8 * gate + u of block b is torch's row gate * H + 8 b + u of
// weight_hh (k-groups below kg_split: h comes first in a joint row) and weight_ih (behind them); bias = b_ih + b_hh in float32; blob zeroed before
inline void pack_gates(const LstmPlan& q, const float* wih, const float* whh, const float* bih, const float* bhh, float* blob)
{
    const VnLayer& g = q.g;
    for (int cb = 0; cb < g.ncb; ++cb) {
        for (int j = 0; j < 32; ++j) {
            const int unit = cb * 8 + (j & 7), row = (j >> 3) * q.H + unit;
            if (unit >= q.H) continue;
            blob[g.b_off + cb * 32 + j] = bih[row] + bhh[row];
            for (int kg = 0; kg < g.kg_total; ++kg)
                for (int hh = 0; hh < 2; ++hh)
                    for (int s = 0; s < 4; ++s) {
                        const int kk = kg * 8 + 4 * hh + s;
                        float w = 0.0f;
                        if (kg < g.kg_split) { if (kk < g.K1) w = whh[(size_t)row * g.K1 + kk]; }
                        else if (kk - g.kg_split * 8 < g.K2) w = wih[(size_t)row * g.K2 + kk - g.kg_split * 8];
                        blob[g.w_off + ((cb * g.kg_total + kg) * 64 + hh * 32 + j) * 4 + s] = w;
                    }
        }
    }
}

// (lstm_key and lstm_gather, the order's key and a step's gather, are value_net_lstm_plan.h's: value_net_lstm_bf16.hip uses them too)

// What the rows with map columns add to a launch (cs_value_net_decide_lstm_om): the maps [W][n][om_cols], which map a step pairs with its
// row, xw = cols + om_cols rounded up to 8 (the columns a gathered row holds) and where the keys and the order of a world's action 0 lie in LDS.
struct LstmOm { const float* maps; int om_cols, map_order, xw, key0, perm0; };

// lstm_gather for such rows, eight lanes a sequence: rotated[g][perm[s][t]][0..cols) | maps[world of g][mperm[s][t]][0..om_cols), zeros up to xw
__device__ __forceinline__ void lstm_gather_om(float* X, int ld, const float* __restrict__ rotated, const LstmOm& om, const int* perm, const int* mperm,
                                               long gbase, int ng, int A, int n, int cols, int t)
{
    const int s = threadIdx.x >> 3;
    const bool live = s < ng;
    long rrow = 0, mrow = 0;
    if (live) {
        rrow = ((gbase + s) * n + perm[s * n + t]) * cols;
        mrow = (((gbase + s) / A) * n + mperm[s * n + t]) * om.om_cols;
    }
    for (int c = threadIdx.x & 7; c < om.xw; c += 8) {
        float v = 0.0f;
        if (live && c < cols) v = rotated[rrow + c];
        else if (live && c < cols + om.om_cols) v = om.maps[mrow + c - cols];
        X[s * ld + c] = v;
    }
}

template <bool WREG, bool MLP1>
__global__ __launch_bounds__(NT) void k_value_net_lstm(LstmPlan q, LstmLds m, const float* __restrict__ wb, int NG, int A, int n, int sorted,
                                                       const float* __restrict__ rotated, const float* __restrict__ rewards,
                                                       const float* __restrict__ robot, int rstride, float gamma, float dt, float* __restrict__ values)
{
#define LSTM_OM 0
#include "value_net_lstm_body.inc"
#undef LSTM_OM
}

// the rows widened by occupancy-map columns (OM-LSTM-RL, cs_value_net_decide_lstm_om)
template <bool WREG, bool MLP1>
__global__ __launch_bounds__(NT) void k_value_net_lstm_om(LstmPlan q, LstmLds m, const float* __restrict__ wb, int NG, int A, int n, int sorted,
                                                          const float* __restrict__ rotated, const float* __restrict__ rewards,
                                                          const float* __restrict__ robot, int rstride, float gamma, float dt,
                                                          float* __restrict__ values, LstmOm om)
{
#define LSTM_OM 1
#include "value_net_lstm_body.inc"
#undef LSTM_OM
}

// the pack entries' common part
inline int pack_lstm(const LstmPlan& q, const float* const* params, float* blob, size_t* n_floats)
{
    if (!n_floats) return fail(CS_ERR_ARG, "null argument");
    *n_floats = (size_t)q.v.total_floats;
    if (!blob) return CS_OK;
    if (!params) return fail(CS_ERR_ARG, "null argument");
    const int n1 = q.v.c0[1], n_params = 2 * q.v.n_layers + 4;
    for (int i = 0; i < n_params; ++i)
        if (!params[i]) return fail(CS_ERR_ARG, "null weight or bias array");
    memset(blob, 0, (size_t)q.v.total_floats * sizeof(float));
    for (int l = 0; l < n1; ++l) pack_layer_f32(q.v.L[l], params[2 * l], params[2 * l + 1], blob);
    pack_gates(q, params[2 * n1], params[2 * n1 + 1], params[2 * n1 + 2], params[2 * n1 + 3], blob);
    for (int l = n1; l < q.v.n_layers; ++l) pack_layer_f32(q.v.L[l], params[2 * l + 4], params[2 * l + 5], blob);
    return CS_OK;
}

} // namespace

#include "value_net_pick.h"

extern "C" int cs_value_net_pack_lstm(const int32_t* dims, int n_dims, int cols, const float* const* params, float* blob, size_t* n_floats)
{
    LstmPlan q;
    const int rc = build_lstm_plan(dims, n_dims, cols, q);
    if (rc != CS_OK) return rc;
    return pack_lstm(q, params, blob, n_floats);
}

extern "C" int cs_value_net_pack_lstm_om(const int32_t* dims, int n_dims, int cols, int om_cols, const float* const* params, float* blob,
                                         size_t* n_floats)
{
    LstmPlan q;
    const int rc = build_lstm_plan(dims, n_dims, cols, q, true, om_cols);
    if (rc != CS_OK) return rc;
    return pack_lstm(q, params, blob, n_floats);
}

extern "C" int cs_value_net_decide_lstm(const int32_t* dims, int n_dims, const float* d_weights, size_t n_weight_floats, int W, int A, int n, int cols,
                                        int sorted_by_distance, const float* d_rotated, const float* d_rewards, const float* d_actions,
                                        const float* d_robot, int robot_stride, float gamma, float dt, const int32_t* d_override, float* d_values,
                                        int32_t* d_choice, float* d_action_out, void* stream)
{
    LstmPlan q;
    const int rc = build_lstm_plan(dims, n_dims, cols, q);
    if (rc != CS_OK) return rc;
    const int rc2 = lstm_check_decide("cs_value_net_decide_lstm", q.v, d_weights, n_weight_floats, W, A, n, sorted_by_distance, d_rotated, d_rewards, d_actions,
                                      d_robot, robot_stride, d_values, d_action_out);
    if (rc2 != CS_OK) return rc2;
    const LstmLds m = lstm_lds_map(q, n);
    const bool wreg = q.g.ncb <= 4 * RB && q.g.kg_total <= RKG, mlp1 = q.v.c0[1] > 0;
    const int rc3 = lstm_launch(m.total, W, A, wreg, mlp1, [&](auto WR, auto M1, size_t shmem, int NG, int grid) {
        constexpr auto kernel = k_value_net_lstm<decltype(WR)::value, decltype(M1)::value>;
        const int rc4 = grant_lds<kernel>(shmem);
        if (rc4 != CS_OK) return rc4;
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(NT), shmem, (hipStream_t)stream, q, m, d_weights, NG, A, n, sorted_by_distance, d_rotated, d_rewards,
                           d_robot, robot_stride, gamma, dt, d_values);
        return (int)CS_OK;
    });
    if (rc3 != CS_OK) return rc3;
    return launch_pick(W, A, d_values, d_actions, d_robot, robot_stride, d_override, d_choice, d_action_out, stream);
}

extern "C" int cs_value_net_decide_lstm_om(const int32_t* dims, int n_dims, const float* d_weights, size_t n_weight_floats, int W, int A, int n, int cols,
                                           int om_cols, int sorted_by_distance, int map_order, const float* d_rotated, const float* d_maps,
                                           const float* d_rewards, const float* d_actions, const float* d_robot, int robot_stride, float gamma, float dt,
                                           const int32_t* d_override, float* d_values, int32_t* d_choice, float* d_action_out, void* stream)
{
    LstmPlan q;
    const int rc = build_lstm_plan(dims, n_dims, cols, q, true, om_cols);
    if (rc != CS_OK) return rc;
    const int rc2 = lstm_check_decide("cs_value_net_decide_lstm_om", q.v, d_weights, n_weight_floats, W, A, n, sorted_by_distance, d_rotated, d_rewards,
                                      d_actions, d_robot, robot_stride, d_values, d_action_out, true, d_maps, map_order);
    if (rc2 != CS_OK) return rc2;
    LstmOm om{d_maps, om_cols, map_order, up(cols + om_cols, 8), 0, 0};
    LstmLds m = lstm_lds_map(q, n, om.xw + 4, true);
    om.key0 = m.total;                          // the keys and the order of action 0, behind the narrow kernel's map
    om.perm0 = om.key0 + up(TILE_M * n, 4);
    m.total = om.perm0 + up(TILE_M * n, 4);
    const bool wreg = q.g.ncb <= 4 * RB && q.g.kg_total <= RKG_OM, mlp1 = q.v.c0[1] > 0;
    const int rc3 = lstm_launch(m.total, W, A, wreg, mlp1, [&](auto WR, auto M1, size_t shmem, int NG, int grid) {
        constexpr auto kernel = k_value_net_lstm_om<decltype(WR)::value, decltype(M1)::value>;
        const int rc4 = grant_lds<kernel>(shmem);
        if (rc4 != CS_OK) return rc4;
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(NT), shmem, (hipStream_t)stream, q, m, d_weights, NG, A, n, sorted_by_distance, d_rotated, d_rewards,
                           d_robot, robot_stride, gamma, dt, d_values, om);
        return (int)CS_OK;
    });
    if (rc3 != CS_OK) return rc3;
    return launch_pick(W, A, d_values, d_actions, d_robot, robot_stride, d_override, d_choice, d_action_out, stream);
}
