// value_net_lstm_plan.h -- what LSTM-RL's decision kernels (value_net_lstm.hip) and its gradient kernel (value_net_lstm_grad.hip) share: the
// plan of a network description (the Linear layers and the gates as a layer of the blob), the activations on v_exp_f32 / v_rcp_f32, the
// quad of float32 MFMAs and the gates' k-step on it (LSTM_MFMA4, LSTM_KSTEP) and, for the decision kernels of value_net_lstm.hip and
// value_net_lstm_bf16.hip, the sort key of a row and the gather of a step's rows (what else those share is value_net_lstm_kernel.h).
// Unnamed namespace: each translation unit gets its own copy.
#pragma once
#include "value_net_plan.h"

namespace {

constexpr int LSTM_MAX_N = CS_VN_LSTM_MAX_N;

struct LstmPlan {
    VnPlan v;                      // the Linear layers: mlp1 = [c0[0], c0[1]) (empty for network 1), mlp = [c0[1], c0[2]); cols, total_floats
    VnLayer g;                     // the gates as a layer: K1 = H (h comes first in a joint row), K2 = the LSTM's input width, ncb = blocks of 8 units
    int H, xin, hpad, ld_xh;       // xin: the LSTM's input width (cols, or mlp1's last width); hpad: H rounded up to 8; the joint rows' stride
};

// om_cols: the occupancy-map columns behind the rotated ones in a row (cs_value_net_decide_lstm_om; 0 with om = false: none)
inline int build_lstm_plan(const int32_t* dims, int n_dims, int cols, LstmPlan& q, bool om = false, int om_cols = 0)
{
    memset(&q, 0, sizeof q);
    VnPlan& p = q.v;
    if (cols != 13 && cols != 15) return fail(CS_ERR_ARG, "rotated rows have 13 or 15 columns");
    if (om && om_cols < 1) return fail(CS_ERR_ARG, "om_cols must be at least 1");
    if (om && cols + om_cols > VN_MAX_WIDTH) return fail(CS_ERR_ARG, "rotated and map columns together exceed a layer's 256 inputs");
    if (!dims || n_dims < 4) return fail(CS_ERR_ARG, "null or empty layer description");
    p.cols = cols;
    q.H = dims[0];
    if (q.H < 1 || q.H > VN_MAX_WIDTH) return fail(CS_ERR_ARG, "the LSTM's hidden width must be between 1 and 256");
    q.hpad = up(q.H, 8);
    int at = 1, off = 0, k1 = cols + om_cols;
    for (int c = 0; c < 2; ++c) {
        if (at >= n_dims) return fail(CS_ERR_ARG, "layer description ends early");
        const int nl = dims[at++];
        if (nl < (c == 0 ? 0 : 1) || at + nl > n_dims) return fail(CS_ERR_ARG, "mlp1 has zero or more layers, mlp at least one, each with its widths");
        if (p.n_layers + nl > VN_MAX_LAYERS) return fail(CS_ERR_ARG, "at most 16 layers in all");
        p.c0[c] = p.n_layers;
        if (c == 1) {               // the gates lie between the two chains in the blob
            q.xin = k1;
            VnLayer& g = q.g;
            g.K1 = q.H; g.K2 = k1; g.N = 4 * q.H;
            g.kg_split = q.hpad / 8;
            g.kg_total = g.kg_split + up(k1, 8) / 8;
            g.ncb = q.hpad / 8;
            place_layer(g, off);
            k1 = SELF_DIM + q.H;
        }
        for (int i = 0; i < nl; ++i) {
            const int wdt = dims[at++];
            const int rc = add_layer(p, k1, 0, wdt, i != nl - 1, off);             // lstm_rl.py: mlp() without last_relu for both chains
            if (rc != CS_OK) return rc;
            k1 = wdt;
        }
        if (c == 1 && k1 != 1) return fail(CS_ERR_ARG, "mlp ends in one output");
    }
    p.c0[2] = p.n_layers;
    if (at != n_dims) return fail(CS_ERR_ARG, "layer description has trailing entries");
    set_ld_pq(p);
    q.ld_xh = q.hpad + (p.c0[1] > 0 ? up(q.xin, 32) : up(cols + om_cols, 8)) + 4;        // (mlp1's last layer stores whole 32-column blocks)
    p.ld_j = up(SELF_DIM + q.H, 8) + 4;
    p.total_floats = off;
    return CS_OK;
}

// an integer that orders like the distance: NaN above everything (numpy's argsort leaves it last, the flip first), -0 = +0
__device__ __forceinline__ unsigned lstm_key(float x)
{
    if (x != x) return 0xFFFFFFFFu;
    unsigned u = __float_as_uint(x);
    if (x == 0.0f) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// rows perm[s][t] of the tile's sequences into rows of stride ld: 16 columns a row, zeros beyond the columns and the sequences
__device__ __forceinline__ void lstm_gather(float* X, int ld, const float* __restrict__ rotated, const int* perm, long gbase, int ng, int n, int cols, int t)
{
    for (int i = threadIdx.x; i < TILE_M * 16; i += NT) {
        const int s = i >> 4, c = i & 15;
        float v = 0.0f;
        if (s < ng && c < cols) v = rotated[((gbase + s) * n + perm[s * n + t]) * cols + c];
        X[s * ld + c] = v;
    }
}

__device__ __forceinline__ float lstm_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504f * x)); }

__device__ __forceinline__ float lstm_tanh(float x)
{
    const float e = __builtin_amdgcn_exp2f(-2.88539008f * fabsf(x));
    const float t = (1.0f - e) * __builtin_amdgcn_rcpf(1.0f + e);
    return x != x ? x : copysignf(t, x);
}

// four v_mfma_f32_32x32x2_f32 on a float4 pair (two float4 variables): the lane's four k of one k-group of 8, in order.  A macro: as an
// inline function it moved the schedule of every kernel that uses it, the gradient kernel at 256 VGPRs among them
#define LSTM_MFMA4(ACC, A, B)                                                                                                \
    ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(A.x, B.x, ACC, 0, 0, 0);                                                      \
    ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(A.y, B.y, ACC, 0, 0, 0);                                                      \
    ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(A.z, B.z, ACC, 0, 0, 0);                                                      \
    ACC = __builtin_amdgcn_mfma_f32_32x32x2f32(A.w, B.w, ACC, 0, 0, 0);

// k-group KGI of the gates' transposed product in a step loop: the lane's weights WV against its joint row `brow`, into `acc`
#define LSTM_KSTEP(WV, KGI)                                                                                                  \
    {                                                                                                                        \
        const float4 xv = *reinterpret_cast<const float4*>(brow + (KGI) * 8);                                                \
        LSTM_MFMA4(acc, WV, xv)                                                                                              \
    }

} // namespace
