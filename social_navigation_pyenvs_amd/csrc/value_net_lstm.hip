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
//
// Numerics: float32.  Every gate pre-activation is one fixed fmaf chain from b_ih + b_hh (summed in float32 by the pack) over the k-groups in
// descending order (x_t's, then h's); sigmoid(x) = rcp(1 + exp2(-x * log2 e)), tanh(x) = sign(x) * (1 - e) * rcp(1 + e) with e = exp2(-2 |x| * log2 e) on
// v_exp_f32 and v_rcp_f32 (1 ulp each): an absolute error below 3e-7 each, no overflow (e <= 1; exp2 -> inf gives sigmoid 0), NaN stays.
// Hidden units beyond H are stored as 0 whatever the inputs.  A sequence's result depends on its own rows alone: the same bits for W = 1 as
// inside any batch, at any position of a tile.  No atomics.  gfx950 only.
#include <hip/hip_runtime.h>

#include "value_net_lstm_plan.h"

namespace {

constexpr int RB = 2, RKG = 14;    // register-resident gate weights: blocks a wavefront, k-groups a block
constexpr int RKG_OM = 15;         // ... of the kernel with map columns: the reference's [om] defaults are 7 blocks x (7 + 8) k-groups
constexpr int GB = 8;              // blocks a wavefront at the widest H (256 / 8 / 4)

struct LstmLds { int key, perm, X, XH, P, Q, J, LT, total; };

// ldg: the row stride of network 2's gather tile.  share_p: network 1's P lies over the joint rows, which are dead when mlp starts (h_n has
// gone to J, a barrier behind it) -- the kernel with map columns asks for it where P fits, to stay at two workgroups a CU with its wider rows
inline LstmLds lstm_lds_map(const LstmPlan& q, int n, int ldg = LDX, bool share_p = false)
{
    LstmLds m{};
    int o = 0;
    auto take = [&](int floats) { const int at = o; o += up(floats, 4); return at; };
    m.key = take(TILE_M * n);
    m.perm = take(TILE_M * n);
    m.XH = take(2 * TILE_M * q.ld_xh);
    m.X = q.v.c0[1] > 0 ? take(2 * TILE_M * ldg) : m.XH;
    m.P = share_p && q.v.c0[1] == 0 && q.v.ld_pq <= 2 * q.ld_xh ? m.XH : take(TILE_M * q.v.ld_pq);
    m.Q = take(TILE_M * q.v.ld_pq);
    m.J = take(JROWS * q.v.ld_j);
    m.LT = take(VN_MAX_LAYERS * 8);
    m.total = o;
    return m;
}

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

// One float32 layer of the tile's 32 rows, dst[32][ncb * 32] = act(src[32][K] x Wt + b): value_net_plan.h's layer_fwd for one row block and
// one source -- the same blob layout, the same k order, zeros beyond N -- with a one-deep weight prefetch.
// The layer's fields come from the table the kernel keeps in LDS (LT_*), one register each.  Fetched from the kernel's arguments (p.L[l], as
// layer_fwd does) beside the gates, the build reported a private segment of 20 - 36 bytes that no instruction used: a dead 16-byte spill slot
// of the scalar allocator and its scavenging slot.  With the table it reports 0.
enum { LT_N, LT_KG, LT_NCB, LT_RELU, LT_W, LT_B, LT_STRIDE = 8 };

__device__ __forceinline__ void lstm_layer(const int* lt, const float* __restrict__ wb, const float* src, int lds_, float* dst, int ldd)
{
    const auto field = [&](int k) { return __builtin_amdgcn_readfirstlane(lt[k]); };
    const struct { int N, kg_total, ncb, relu, w_off, b_off; } L{field(LT_N), field(LT_KG), field(LT_NCB), field(LT_RELU), field(LT_W), field(LT_B)};
    const int lane = threadIdx.x & 63, h = lane >> 5, li = lane & 31, KG = L.kg_total;
    const float* a1 = src + li * lds_ + 4 * h;
    for (int cb = threadIdx.x >> 6; cb < L.ncb; cb += 4) {
        const float4* bw = reinterpret_cast<const float4*>(wb + L.w_off) + cb * KG * 64 + lane;
        const float bias = wb[L.b_off + cb * 32 + li];
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = bias;
        float4 nw = bw[0];
        for (int kg = 0; kg < KG; ++kg) {
            const float4 w = nw;
            nw = bw[(kg + 1 < KG ? kg + 1 : kg) * 64];
            const float4 a = *reinterpret_cast<const float4*>(a1 + kg * 8);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, w.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, w.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, w.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, w.w, acc, 0, 0, 0);
        }
        float* d = dst + 4 * h * ldd + cb * 32 + li;
        const bool pad = cb * 32 + li >= L.N;              // (the zero weights give 0 * inf = NaN there when an input is infinite)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = acc[r];
            if (L.relu) v = v < 0.0f ? 0.0f : v;          // (a NaN stays a NaN, as torch's ReLU leaves it)
            d[((r & 3) + 8 * (r >> 2)) * ldd] = pad ? 0.0f : v;
        }
    }
}

// layers [first, last) from `src`, a barrier behind each; outputs alternate P, Q, the last one goes to final_dst when given.  Returns where
// the result is, out_ld its row stride.
__device__ __forceinline__ const float* lstm_chain(const int* ltab, int ld_pq, const float* __restrict__ wb, float* P, float* Q, int first, int last, const float* src,
                                                   int lds_, float* final_dst, int final_ld, int& out_ld)
{
    const float* cur = src;
    int cur_ld = lds_;
    for (int l = first; l < last; ++l) {
        const bool fin = l == last - 1 && final_dst;
        float* dst = fin ? final_dst : (((l - first) & 1) ? Q : P);
        const int ldd = fin ? final_ld : ld_pq;
        lstm_layer(ltab + l * LT_STRIDE, wb, cur, cur_ld, dst, ldd);
        __syncthreads();
        cur = dst;
        cur_ld = ldd;
    }
    out_ld = cur_ld;
    return cur;
}

#define LSTM_KSTEP(WV, KGI)                                                                                                  \
    {                                                                                                                        \
        const float4 xv = *reinterpret_cast<const float4*>(brow + (KGI) * 8);                                                \
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(WV.x, xv.x, acc, 0, 0, 0);                                                \
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(WV.y, xv.y, acc, 0, 0, 0);                                                \
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(WV.z, xv.z, acc, 0, 0, 0);                                                \
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(WV.w, xv.w, acc, 0, 0, 0);                                                \
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
#undef LSTM_KSTEP

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
    const int rc2 = check_decide_args(q.v, d_weights, n_weight_floats, W, A, n, d_rotated, d_rewards, d_actions, d_robot, robot_stride, d_values, d_action_out);
    if (rc2 != CS_OK) return rc2;
    if (sorted_by_distance != 0 && sorted_by_distance != 1) return fail(CS_ERR_ARG, "sorted_by_distance is 0 or 1");
    if (n > LSTM_MAX_N) return fail(CS_ERR_ARG, "cs_value_net_decide_lstm takes at most 128 humans a world (CS_VN_LSTM_MAX_N)");
    const LstmLds m = lstm_lds_map(q, n);
    const size_t shmem = (size_t)m.total * sizeof(float);
    if (shmem > 160 * 1024) return fail(CS_ERR_ARG, "the tile buffers of this network do not fit the 160 KiB of LDS");
    int NG, grid;
    job_grid(W, A, NG, grid);
    const bool wreg = q.g.ncb <= 4 * RB && q.g.kg_total <= RKG, mlp1 = q.v.c0[1] > 0;
#define LSTM_LAUNCH(WR, M1)                                                                                                          \
    {                                                                                                                                \
        const int rc3 = grant_lds<k_value_net_lstm<WR, M1>>(shmem);                                                                  \
        if (rc3 != CS_OK) return rc3;                                                                                                \
        hipLaunchKernelGGL((k_value_net_lstm<WR, M1>), dim3(grid), dim3(NT), shmem, (hipStream_t)stream, q, m, d_weights, NG, A, n,  \
                           sorted_by_distance, d_rotated, d_rewards, d_robot, robot_stride, gamma, dt, d_values);                    \
    }
    if (wreg && mlp1) LSTM_LAUNCH(true, true)
    else if (wreg) LSTM_LAUNCH(true, false)
    else if (mlp1) LSTM_LAUNCH(false, true)
    else LSTM_LAUNCH(false, false)
#undef LSTM_LAUNCH
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
    const int rc2 = check_decide_args(q.v, d_weights, n_weight_floats, W, A, n, d_rotated, d_rewards, d_actions, d_robot, robot_stride, d_values, d_action_out);
    if (rc2 != CS_OK) return rc2;
    if (!d_maps) return fail(CS_ERR_ARG, "null argument");
    if (sorted_by_distance != 0 && sorted_by_distance != 1) return fail(CS_ERR_ARG, "sorted_by_distance is 0 or 1");
    if (map_order != CS_VN_MAPS_OWN && map_order != CS_VN_MAPS_FIRST_ACTION) return fail(CS_ERR_ARG, "map_order is CS_VN_MAPS_OWN or CS_VN_MAPS_FIRST_ACTION");
    if (n > LSTM_MAX_N) return fail(CS_ERR_ARG, "cs_value_net_decide_lstm_om takes at most 128 humans a world (CS_VN_LSTM_MAX_N)");
    LstmOm om{d_maps, om_cols, map_order, up(cols + om_cols, 8), 0, 0};
    LstmLds m = lstm_lds_map(q, n, om.xw + 4, true);
    om.key0 = m.total;                          // the keys and the order of action 0, behind the narrow kernel's map
    om.perm0 = om.key0 + up(TILE_M * n, 4);
    m.total = om.perm0 + up(TILE_M * n, 4);
    const size_t shmem = (size_t)m.total * sizeof(float);
    if (shmem > 160 * 1024) return fail(CS_ERR_ARG, "the tile buffers of this network do not fit the 160 KiB of LDS");
    int NG, grid;
    job_grid(W, A, NG, grid);
    const bool wreg = q.g.ncb <= 4 * RB && q.g.kg_total <= RKG_OM, mlp1 = q.v.c0[1] > 0;
#define LSTM_LAUNCH(WR, M1)                                                                                                             \
    {                                                                                                                                   \
        const int rc3 = grant_lds<k_value_net_lstm_om<WR, M1>>(shmem);                                                                  \
        if (rc3 != CS_OK) return rc3;                                                                                                   \
        hipLaunchKernelGGL((k_value_net_lstm_om<WR, M1>), dim3(grid), dim3(NT), shmem, (hipStream_t)stream, q, m, d_weights, NG, A, n,  \
                           sorted_by_distance, d_rotated, d_rewards, d_robot, robot_stride, gamma, dt, d_values, om);                   \
    }
    if (wreg && mlp1) LSTM_LAUNCH(true, true)
    else if (wreg) LSTM_LAUNCH(true, false)
    else if (mlp1) LSTM_LAUNCH(false, true)
    else LSTM_LAUNCH(false, false)
#undef LSTM_LAUNCH
    return launch_pick(W, A, d_values, d_actions, d_robot, robot_stride, d_override, d_choice, d_action_out, stream);
}
