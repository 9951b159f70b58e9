// value_net_lstm_kernel.h -- what LSTM-RL's decision kernels share beside their plan (value_net_lstm_plan.h): k_value_net_lstm and
// k_value_net_lstm_om (value_net_lstm.hip, value_net_lstm_body.inc), k_value_net_lstm_bf16 (value_net_lstm_bf16.hip) and
// k_value_net_lstm_om_bf16 (value_net_lstm_om_bf16.hip; both value_net_lstm_bf16_body.inc), and the two that generate their rows from the
// worlds, k_value_net_lstm_worlds and k_value_net_lstm_worlds_bf16 (value_net_lstm_worlds[_bf16].hip: the same two texts).  Device: the layer
// table in LDS, the order of a tile's rows, the ends of a job around its step loop (the step loops themselves differ by design and stay with
// their kernels), the layer of 32 rows in its two arithmetics and the chain of layers.  Host: what a decide entry does between its plan and
// its launch.  The gradient kernel (value_net_lstm_grad.hip) needs none of it: the one piece it shares with the step loop here, LSTM_KSTEP, is
// value_net_lstm_plan.h's.  Unnamed namespace: each translation unit gets its own copy.
#pragma once
#include <string>
#include <type_traits>

#include "value_net_bf16.h"
#include "value_net_lstm_plan.h"

namespace {

constexpr int RB = 2;              // register-resident gate weights: blocks a wavefront
constexpr int GB = 8;              // blocks a wavefront at the widest H (256 / 8 / 4)

// The layers' fields come from a table the kernel keeps in LDS (LT_*), one register each.  Fetched from the kernel's arguments (p.L[l], as
// layer_fwd does) beside the gates, the build reported a private segment of 20 - 36 bytes that no instruction used: a dead 16-byte spill slot
// of the scalar allocator and its scavenging slot.  With the table it reports 0.
enum { LT_N, LT_KG, LT_NCB, LT_RELU, LT_W, LT_B, LT_STRIDE = 8 };

// Three pieces with loops are macros, text in the kernel as value_net_lstm_body.inc is: as inline functions, whose control flow the compiler
// simplifies on its own before it inlines them, each moved the registers and the schedule of all eight float32 kernels.  They expect
// `tid` = threadIdx.x in scope, LSTM_RANK `row8` = tid >> 3 as well (eight lanes a sequence), as LSTM_KSTEP expects `brow` and `acc`.

// the layer table of plan P into LTAB (the first barrier of the first job publishes it)
#define LSTM_FILL_TABLE(LTAB, P)                                                                                             \
    if (tid == 0)                                                                                                            \
        for (int l = 0; l < (P).n_layers; ++l) {                                                                             \
            int* e = (LTAB) + l * LT_STRIDE;                                                                                 \
            const VnLayer& layer = (P).L[l];                                                                                 \
            e[LT_N] = layer.N; e[LT_KG] = layer.kg_total; e[LT_NCB] = layer.ncb; e[LT_RELU] = layer.relu;                    \
            e[LT_W] = layer.w_off; e[LT_B] = layer.b_off;                                                                    \
        }

// a job's start: the sort keys of its NG sequences' N rows (column 11: the distance to the robot's next position) and J zeroed
#define LSTM_BEGIN_JOB(KEY, J, LD_J, ROTATED, GBASE, NG, N, COLS)                                                            \
    {                                                                                                                        \
        for (int i = tid; i < (NG) * (N); i += NT) (KEY)[i] = lstm_key((ROTATED)[((GBASE) * (N) + i) * (COLS) + 11]);        \
        for (int i = tid; i < JROWS * (LD_J); i += NT) (J)[i] = 0.0f;                                                        \
    }

// The order of the tile's sequences, eight lanes a sequence: PERM[s][rank of row j] = j, the rank of row j being the number of rows k with
// key_k > key_j, or key_k == key_j and k > j -- decreasing keys, equal keys by decreasing row (numpy's stable argsort, flipped); O(n^2)
// compares, always a permutation.  SORTED = 0: the identity.
#define LSTM_RANK(KEY, PERM, N, NG, SORTED)                                                                                  \
    for (int j = tid & 7; j < (N) && row8 < (NG); j += 8) {                                                                  \
        int rank = j;                                                                                                        \
        if (SORTED) {                                                                                                        \
            const unsigned kj = (KEY)[row8 * (N) + j];                                                                       \
            rank = 0;                                                                                                        \
            _Pragma("unroll 1") for (int k = 0; k < (N); ++k) {                                                              \
                const unsigned kk = (KEY)[row8 * (N) + k];                                                                   \
                rank += (kk > kj || (kk == kj && k > j)) ? 1 : 0;                                                            \
            }                                                                                                                \
        }                                                                                                                    \
        (PERM)[row8 * (N) + rank] = j;                                                                                       \
    }

// lstm_rl.py:25 / :53: the self state is read from the first row in evaluation order -- the first columns of step 0's gathered rows G
__device__ __forceinline__ void lstm_self_state(float* J, int ld_j, const float* G, int ldg, int ng, int tid)
{
    const int row8 = tid >> 3, c = tid & 7;
    if (row8 < ng && c < SELF_DIM) J[row8 * ld_j + c] = G[row8 * ldg + c];
}

// h_n behind the self state in J, eight lanes a sequence; hn: rows of ldh elements, float32 or the bf16 kernel's rounded h
template <class T>
__device__ __forceinline__ void lstm_hn_to_j(float* J, int ld_j, const T* hn, int ldh, int H, int tid)
{
    const int row8 = tid >> 3;
    for (int u = tid & 7; u < H; u += 8) J[row8 * ld_j + SELF_DIM + u] = static_cast<float>(hn[row8 * ldh + u]);
}

// cadrl.py:85-90 compute_action_value of the job's ng sequences; out: the rows of mlp's output, stride out_ld.  rewards: the look-ahead's
// [W][A] (PITCH 0), or a table of the job's own sequences, PITCH floats apart (the kernels that generate their rows: their frame table)
template <int PITCH = 0>
__device__ __forceinline__ void lstm_store_values(const float* out, int out_ld, long gbase, int ng, int A, const float* __restrict__ rewards,
                                                  const float* __restrict__ robot, int rstride, float gamma, float dt, float* __restrict__ values, int tid)
{
    if (tid < ng) {
        const long g = gbase + tid;
        const float vpref = robot[(g / A) * rstride + 7];
        values[g] = rewards[PITCH ? (long)PITCH * tid : g] + powf(gamma, dt * vpref) * out[tid * out_ld];
    }
}

// The input of a job sits behind three seams, and the two kernel texts (value_net_lstm_body.inc, value_net_lstm_bf16_body.inc) name their
// input through them alone: LSTM_BEGIN_JOB above (the sort keys), LSTM_STEP_ROWS (the rows perm[s][T] of the tile's sequences into X, rows
// of stride LD) and LSTM_STORE_VALUES (where a sequence's reward comes from).  Here: the look-ahead tensor `rotated` and `rewards` of the
// kernel's arguments.  A unit whose kernels generate their rows redefines the three (value_net_lstm_worlds.h).
#define LSTM_STEP_ROWS(X, LD, T) lstm_gather(X, LD, rotated, perm, gbase, ng, n, cols, T)
#define LSTM_STORE_VALUES(OUT, OUT_LD) lstm_store_values(OUT, OUT_LD, gbase, ng, A, rewards, robot, rstride, gamma, dt, values, tid)

// One layer of the tile's 32 rows, dst[32][ncb * 32] = act(src[32][K] x Wt + b), the waves over the 32-column output blocks: value_net_plan.h's
// layer_fwd for one row block and one source -- the same blob layout, the same k order, zeros beyond N -- with the fields from the table in
// LDS and a one-deep weight prefetch, in two arithmetics.  in_bf16: src holds bfloat16 rows (stride lds_ floats) and the weights are k-steps
// of 16 (value_net_bf16.hip's layer_fwd_h); else the float32 layer.  out_bf16: the output is the operand of a bf16 layer -- dst holds
// bfloat16 rows of 2 * ldd elements, each value rounded to nearest even after the bias and the ReLU.  The float32 kernels pass false, false.
// The two are arguments, uniform over the workgroup, not template arguments: one copy of the layer per call site keeps the bf16 kernel at
// two workgroups a CU.
__device__ __forceinline__ void lstm_layer(const int* lt, const float* __restrict__ wb, const float* src, int lds_, float* dst, int ldd, bool in_bf16, bool out_bf16)
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
            if (in_bf16) {
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, w), acc, 0, 0, 0);
            } else {
                LSTM_MFMA4(acc, a, w)
            }
        }
        // C/D map of the 32x32 forms: column = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5).  (The float32 destination is formed in
        // front of `pad` and the branch, as a chain of three offsets: the float32 kernels' schedules follow the order of this text)
        float* d = dst + 4 * h * ldd + cb * 32 + li;
        const bool pad = cb * 32 + li >= L.N;              // (the zero weights give 0 * inf = NaN there when an input is infinite)
        if (out_bf16) {
            __bf16* dh = reinterpret_cast<__bf16*>(dst) + 4 * h * 2 * ldd + (cb * 32 + li);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = acc[r];
                if (L.relu) v = v < 0.0f ? 0.0f : v;      // (a NaN stays a NaN, as torch's ReLU leaves it)
                dh[((r & 3) + 8 * (r >> 2)) * 2 * ldd] = static_cast<__bf16>(pad ? 0.0f : v);
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = acc[r];
                if (L.relu) v = v < 0.0f ? 0.0f : v;
                d[((r & 3) + 8 * (r >> 2)) * ldd] = pad ? 0.0f : v;
            }
        }
    }
}

// the arithmetic of a chain: float32 throughout; or the bf16 kernel's, whose first layer reads float32 rows and every later one bf16 rows --
// mlp1, whose every output is a bf16 operand (the last one the gates'), and mlp, whose last output stays float32; or what lies behind an
// mlp1 layer 0 that its kernel ran itself (the rows with map columns, value_net_lstm_om_bf16.hip): bf16 rows in, bf16 rows out
enum { LC_F32, LC_BF16_MLP1, LC_BF16_MLP, LC_BF16_MLP1_REST };

// layers [first, last) from `src`, a barrier behind each; outputs alternate P, Q, the last one goes to final_dst when given.  Returns where
// the result is, out_ld its row stride.
template <int ARITH>
__device__ __forceinline__ const float* lstm_chain(const int* ltab, int ld_pq, const float* __restrict__ wb, float* P, float* Q, int first, int last, const float* src,
                                                   int lds_, float* final_dst, int final_ld, int& out_ld)
{
    const float* cur = src;
    int cur_ld = lds_;
    for (int l = first; l < last; ++l) {
        const bool fin = l == last - 1, given = fin && final_dst;
        float* dst = given ? final_dst : (((l - first) & 1) ? Q : P);
        const int ldd = given ? final_ld : ld_pq;
        lstm_layer(ltab + l * LT_STRIDE, wb, cur, cur_ld, dst, ldd, ARITH != LC_F32 && (l != first || ARITH == LC_BF16_MLP1_REST),
                   ARITH == LC_BF16_MLP1 || ARITH == LC_BF16_MLP1_REST || (ARITH == LC_BF16_MLP && !fin));
        __syncthreads();
        cur = dst;
        cur_ld = ldd;
    }
    out_ld = cur_ld;
    return cur;
}

// The checks of a recurrent decide entry behind its plan, in the order the entries give them: check_decide_args', the flag of the order and
// the humans a world, with the entry's name in that sentence.  om: the entry with map columns, which checks d_maps and map_order in between.
inline int lstm_check_decide(const char* entry, const VnPlan& p, const void* d_weights, size_t n_weight_floats, int W, int A, int n, int sorted_by_distance,
                             const void* d_rotated, const void* d_rewards, const void* d_actions, const void* d_robot, int robot_stride,
                             const void* d_values, const void* d_action_out, bool om = false, const void* d_maps = nullptr, int map_order = CS_VN_MAPS_OWN)
{
    const int rc = check_decide_args(p, d_weights, n_weight_floats, W, A, n, d_rotated, d_rewards, d_actions, d_robot, robot_stride, d_values, d_action_out);
    if (rc != CS_OK) return rc;
    if (om && !d_maps) return fail(CS_ERR_ARG, "null argument");
    if (sorted_by_distance != 0 && sorted_by_distance != 1) return fail(CS_ERR_ARG, "sorted_by_distance is 0 or 1");
    if (om && map_order != CS_VN_MAPS_OWN && map_order != CS_VN_MAPS_FIRST_ACTION) return fail(CS_ERR_ARG, "map_order is CS_VN_MAPS_OWN or CS_VN_MAPS_FIRST_ACTION");
    if (n > LSTM_MAX_N) return fail(CS_ERR_ARG, std::string(entry) + " takes at most 128 humans a world (CS_VN_LSTM_MAX_N)");
    return CS_OK;
}

// What follows the LDS map: its 160 KiB bound, the grid, and the kernel's build for (wreg: the gate weights in registers; mlp1: network 2):
// launch(WR, M1, shmem, NG, grid) is the entry's generic lambda, WR and M1 two std::bool_constant; returns its status.
template <class Launch>
inline int lstm_launch(int lds_floats, int W, int A, bool wreg, bool mlp1, Launch&& launch)
{
    const size_t shmem = (size_t)lds_floats * sizeof(float);
    if (shmem > 160 * 1024) return fail(CS_ERR_ARG, "the tile buffers of this network do not fit the 160 KiB of LDS");
    int NG, grid;
    job_grid(W, A, NG, grid);
    const auto with = [&](auto wr) { return mlp1 ? launch(wr, std::true_type{}, shmem, NG, grid) : launch(wr, std::false_type{}, shmem, NG, grid); };
    return wreg ? with(std::true_type{}) : with(std::false_type{});
}

} // namespace
