// value_net_lstm_grad.hip -- the training side of LSTM-RL's value networks (crowd_nav/policy/lstm_rl.py:9-65, ValueNetwork1 and ValueNetwork2),
// fused: for a minibatch of B stored states the forward pass, the mean-squared-error loss against B targets and the gradient of that loss
// with respect to every parameter by backpropagation through time (cs_value_net_loss_grad_lstm), and the packing of the flat parameters into
// the decision kernel's blob on the device (cs_value_net_pack_lstm_device).  Replaces, per optimiser step, crowd_nav/utils/trainer.py:50-71
// (zero_grad, model(inputs), MSELoss, backward) for the recurrent family; the optimiser stays torch's, or runs fused behind the gradient
// (cs_value_net_train_step_lstm: value_net_grad.h k_vn_sgd on this blob's map, LstmGrad::SgdMap).  value_net_grad.hip is the
// feed-forward family's; the two share value_net_grad.h (the forward layer of a tile, the three backward products, the chains, the value
// head, the sum, and the entries' host side: its templates over this file's LstmGrad).
// OM-LSTM-RL (the *_lstm_om entries: cs_value_net_loss_grad_lstm_om, ...) is the same kernel on stored rows of cols + om_cols columns, a human's
// map columns behind its rotated ones: network 1's LSTM or network 2's first mlp1 layer reads the wide row, nothing behind it changes.
//
// Shape of the work.  A workgroup (4 wavefronts) takes jobs of 32 sequences (samples); a sample's n rows are evaluated as they lie
// (cs_value_net_decide_lstm's sorted_by_distance = 0).  A job runs in three phases.
//   forward   t = 0 .. n-1: the 32 rows of step t (a stored row: 13 | 15 rotated columns and, for OM-LSTM-RL, its map columns behind them),
//             [mlp1 on them (layer_fwd32),] the gates as value_net_lstm_body.inc forms them -- the
//             transposed product, accumulators from b_ih + b_hh, the k-groups in descending order, weights streamed from the blob -- and the
//             pointwise part in the lanes' own accumulators; h goes to the other joint-row buffer, c comes back from the lane's own tape store.  Every step's i, f,
//             g, o, c and h go to the TAPE, the workgroup's own floats of d_scratch behind its partial gradient: [n][6][32][up(H, 8)].
//   value     mlp on (self state, h_n), the values, the loss terms, dV = 2 (V - target) / B, mlp backward: dJ; dh_n = dJ's columns 6 ..
//   backward  t = n-1 .. 0: the rows of step t again [and mlp1's forward recomputed with every layer kept, as the feed-forward kernel
//             recomputes its tile]; the gate gradients from the tape (sigma' = s (1 - s), tanh' = 1 - t^2 of the stored outputs, tanh(c_t)
//             recomputed by the forward's formula) as dZ [32][4H] in torch's column order; then dW_ih += dZt x_t, dW_hh += dZt h_(t-1) (read
//             from the tape in place), db_ih += sum dZ, dh = dZ W_hh and, network 2, dx_t = dZ W_ih through mlp1's backward -- all of them
//             value_net_grad.h's products on v_mfma_f32_32x32x2_f32.  Step 0 has no h before it: W_hh gets nothing there, so n = 1 leaves
//             its gradient exactly 0.
// The tape is kept, not recomputed: at the reference's widths (H = 50, n = 5) it is 6 x 32 x 5 x 56 floats = 215 KB a workgroup, beyond the
// LDS, and recomputing a step needs the h before it, that is the whole prefix of the sequence (O(n^2) steps) or checkpoints, which are a
// tape again.  A workgroup writes and reads only its own tape, with barriers between; it stays in the L2.
//
// Sums.  As value_net_grad.hip: a workgroup owns one region of d_scratch ([P parameters + 1 loss term], then its tape); it zeroes the
// partial gradient, and every dW block and db column is added to it by the same lane in step order (plain loads and stores, no atomics).
// bias_hh's partial gradient is a copy of bias_ih's.  k_vn_grad_sum then adds the regions in index order into d_grad.  The bits depend on B
// (the number of workgroups), never on timing.  Hidden units beyond H: their dZ columns do not exist (dZ is [32][4H]), nothing reads their
// tape.  gfx950 only.
#include <hip/hip_runtime.h>

#include "value_net_grad.h"
#include "value_net_lstm_plan.h"

namespace {

constexpr int TAPE = 6;            // arrays a step: i, f, g, o, c, h
enum { TP_I, TP_F, TP_G, TP_O, TP_C, TP_H };

struct LstmGradOff { int wih, whh, bih, bhh; };        // floats into the flat parameters: the LSTM's four tensors between mlp1's and mlp's

// LDS map (floats).  v: the input tile (32 rows of v.ldx floats: a stored row's columns rounded up to 8, plus 4), the layers' outputs (mlp's over mlp1's: mlp1's are dead between the forward and the backward steps),
// the two gradient buffers, J / dJ, the loss terms.  XH [2][32][ld_xh] (the forward's joint rows) shares its floats with the backward's dZ
// [32][ldz], dh and dc [32][ldh].
struct LstmGradLds { GradLds v; int XH, dZ, dh, dc, ldz, ldh; };

// the columns of a stored row, the rotated ones and the map columns behind them: what the LSTM (network 1) or mlp1's first layer reads
inline int row_width(const LstmPlan& q) { return q.v.c0[1] > 0 ? q.v.L[0].K1 : q.xin; }

inline LstmGradLds lstm_grad_lds_map(const LstmPlan& q)
{
    LstmGradLds m{};
    const VnPlan& p = q.v;
    int o = 0, widest = 8, end = 0;
    auto take = [&](int floats) { const int at = o; o += up(floats, 4); return at; };
    m.v.ldx = up(row_width(q), 8) + 4;
    m.v.X0 = take(32 * m.v.ldx);
    const int base = o;
    for (int l = 0; l < p.n_layers; ++l) {
        if (l == p.c0[1]) { end = o; o = base; }
        m.v.ld[l] = ld8(p.L[l].N);
        m.v.act[l] = take(32 * m.v.ld[l]);
        widest = p.L[l].N > widest ? p.L[l].N : widest;
    }
    o = o > end ? o : end;
    m.v.D0 = take(32 * ld8(widest));
    m.v.D1 = take(32 * ld8(widest));
    m.ldz = ld8(4 * q.H);
    m.ldh = q.hpad + 4;
    m.XH = take(2 * 32 * q.ld_xh);
    end = o;
    o = m.XH;
    m.dZ = take(32 * m.ldz);
    m.dh = take(32 * m.ldh);
    m.dc = take(32 * m.ldh);
    o = o > end ? o : end;
    m.v.J = take(32 * p.ld_j);
    m.v.dJ = take(32 * p.ld_j);
    m.v.val = take(32);
    m.v.total = o;
    return m;
}

// (LSTM_KSTEP, a k-group of the gates in the forward step, is value_net_lstm_plan.h's: the decision kernels' step)

// gpart: the floats of a region before its tape (P + 1, rounded up to 4).  MLP1: network 2's mlp1 in the step loops.
template <bool MLP1>
__global__ __launch_bounds__(NT) void k_vn_lstm_grad(LstmPlan q, LstmGradLds m, GradOffsets o, LstmGradOff og, const float* __restrict__ wb,
                                                     const float* __restrict__ params, int B, int n, const float* __restrict__ rows_in,
                                                     const float* __restrict__ targets, float* __restrict__ scratch, int region, int gpart,
                                                     float* __restrict__ values)
{
    extern __shared__ float lds[];
    const VnPlan& p = q.v;
    GradBufs b{};
    b.lds = lds; b.X0 = lds + m.v.X0; b.D0 = lds + m.v.D0; b.D1 = lds + m.v.D1; b.J = lds + m.v.J; b.dJ = lds + m.v.dJ; b.val = lds + m.v.val;
    float *XH = lds + m.XH, *dZ = lds + m.dZ, *dh = lds + m.dh, *dc = lds + m.dc;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), hh = lane >> 5, li = lane & 31;
    // K0: the columns of a stored row (row_width).  The input tile's stride: value_net_grad.h tile_ldx says why network 2 holds it in a vector
    // register; network 1's build, which reads the tile in its backward products alone, reports a private segment of 0 with the scalar.
    const int K0 = MLP1 ? p.L[0].K1 : q.xin, ldx = MLP1 ? tile_ldx(m.v) : m.v.ldx, H = q.H, hpad = q.hpad, ldxh = q.ld_xh, KG = q.g.kg_total, ldz = m.ldz, ldh = m.ldh, xin = q.xin;
    constexpr bool with_mlp1 = MLP1;
    const int nbw = (q.g.ncb - wave + 3) >> 2;              // this wavefront's blocks: wave, wave + 4, ...
    const float4* gw = reinterpret_cast<const float4*>(wb + q.g.w_off) + lane;
    // x_t as the backward products read it: mlp1's last output, or the rows themselves
    const int l_x = with_mlp1 ? p.c0[1] - 1 : 0;
    const float* xact = with_mlp1 ? lds + m.v.act[l_x] : b.X0;
    const int ldxa = with_mlp1 ? m.v.ld[l_x] : ldx;
    const int plane = 32 * hpad;                            // one array of one step of the tape
    float* g = scratch + (long)blockIdx.x * region;
    float* tape = g + gpart;

#pragma unroll 1
    for (int i = tid; i < gpart; i += NT) g[i] = 0.0f;
    float loss = 0.0f;                  // thread 0's: the job sums, in job order
    __syncthreads();

    for (int job = blockIdx.x; (long)job * JROWS < B; job += gridDim.x) {
        const int gbase = job * JROWS;
        const int ng = B - gbase < JROWS ? B - gbase : JROWS;
        // the 32 rows of step t: a row's K0 columns, zeros up to K0 rounded up to 8 and beyond the sequences
        auto load = [&](float* dst, int ld, int t) {
            const int kpad = ldx - 4, sh = kpad <= 16 ? 4 : 6;      // 16 lanes a row of 13 | 15 columns, a wavefront a wide one
#pragma unroll 1
            for (int s = tid >> sh; s < 32; s += NT >> sh)
#pragma unroll 1
                for (int c = tid & ((1 << sh) - 1); c < kpad; c += 1 << sh)
                    dst[s * ld + c] = (s < ng && c < K0) ? rows_in[((long)(gbase + s) * n + t) * K0 + c] : 0.0f;
        };
#pragma unroll 1
        for (int i = tid; i < JROWS * p.ld_j; i += NT) b.J[i] = 0.0f;
#pragma unroll 1
        for (int i = tid; i < 2 * 32 * ldxh; i += NT) XH[i] = 0.0f;                                  // h0 = 0
        __syncthreads();
        // A job is 2 n + 1 visits: the steps t = 0 .. n-1 forward, the value head, the steps t = n-1 .. 0 backward.  A visit is: its rows
        // (a step's 32 rows of the minibatch; the head's joint rows), a chain forward with every layer's output kept (network 2's mlp1; the
        // head's mlp), its own part, and -- behind a backward step and the head -- that chain backward.  The chains' text exists once.
        for (int it = 0; it <= 2 * n; ++it) {
            const bool fwd = it < n, head = it == n;
            const int t = fwd ? it : head ? 0 : 2 * n - it;
            float* cur = XH + (t & 1) * 32 * ldxh;
            float* nxt = XH + ((t + 1) & 1) * 32 * ldxh;
            if (head) {
                const float* hn = XH + (n & 1) * 32 * ldxh;
#pragma unroll 1
                for (int i = tid; i < 32 * H; i += NT) {
                    const int s = i / H, u = i - s * H;
                    b.J[s * p.ld_j + SELF_DIM + u] = hn[s * ldxh + u];
                }
            } else if (with_mlp1 || !fwd) load(b.X0, ldx, t);
            else load(cur + hpad, ldxh, t);
            __syncthreads();
            if (it == 0) {      // lstm_rl.py:25 / :53: the self state is read from the first row
                const float* first = with_mlp1 ? b.X0 : cur + hpad;
                const int ldf = with_mlp1 ? ldx : ldxh;
#pragma unroll 1
                for (int i = tid; i < ng * SELF_DIM; i += NT) b.J[(i / SELF_DIM) * p.ld_j + i % SELF_DIM] = first[(i / SELF_DIM) * ldf + i % SELF_DIM];
            }
            const bool chain = head || with_mlp1;
            const int c_first = head ? p.c0[1] : p.c0[0], c_last = head ? p.c0[2] : p.c0[1];
            const float* c_src = head ? b.J : b.X0;
            const int c_ld = head ? p.ld_j : ldx;
            if (chain) chain_fwd(p, m.v, b, wb, c_first, c_last, c_src, c_ld, nullptr, 0);
            if (fwd) {
                if (with_mlp1) {
                    const int xw = (xin + 7) & ~7;
#pragma unroll 1
                    for (int i = tid; i < 32 * xw; i += NT) {
                        const int s = i / xw, cc = i - s * xw;
                        cur[s * ldxh + hpad + cc] = xact[s * ldxa + cc];
                    }
                    __syncthreads();
                }
                const float* brow = cur + li * ldxh + 4 * hh;
                float* tp = tape + (long)t * TAPE * plane;
#pragma unroll 1
                for (int bi = 0; bi < nbw; ++bi) {
                    const int blk = wave + 4 * bi;
                    float* tq = tp + li * hpad + blk * 8 + 4 * hh;
                    // c of the step before: this lane's own store to the tape (c0 = 0)
                    const float4 cb4 = t > 0 ? *reinterpret_cast<const float4*>(tq - TAPE * plane + TP_C * plane) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    const float cb[4] = {cb4.x, cb4.y, cb4.z, cb4.w};
                    f32x16 acc;
                    const float* bias = wb + q.g.b_off + blk * 32 + 4 * hh;
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[r] = bias[(r & 3) + 8 * (r >> 2)];
                    {   // the k-groups in descending order (x_t's, then h's), as the decision kernel walks them
                        const float4* w = gw + (long)blk * KG * 64;
                        float4 nw = w[(long)(KG - 1) * 64];
#pragma unroll 1
                        for (int kg = KG - 1; kg >= 0; --kg) {
                            const float4 wv = nw;
                            nw = w[(long)(kg > 0 ? kg - 1 : 0) * 64];
                            LSTM_KSTEP(wv, kg)
                        }
                    }
                    float iv[4], fv[4], gv[4], ov[4], cv[4], hv[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const float ig = lstm_sigmoid(acc[u]), fg = lstm_sigmoid(acc[4 + u]), gg = lstm_tanh(acc[8 + u]), og_ = lstm_sigmoid(acc[12 + u]);
                        const float cn = fg * cb[u] + ig * gg;
                        hv[u] = blk * 8 + 4 * hh + u < H ? og_ * lstm_tanh(cn) : 0.0f;      // (zero weights give 0 for finite inputs only)
                        iv[u] = ig; fv[u] = fg; gv[u] = gg; ov[u] = og_; cv[u] = cn;
                    }
                    *reinterpret_cast<float4*>(nxt + li * ldxh + blk * 8 + 4 * hh) = make_float4(hv[0], hv[1], hv[2], hv[3]);
                    *reinterpret_cast<float4*>(tq + TP_I * plane) = make_float4(iv[0], iv[1], iv[2], iv[3]);
                    *reinterpret_cast<float4*>(tq + TP_F * plane) = make_float4(fv[0], fv[1], fv[2], fv[3]);
                    *reinterpret_cast<float4*>(tq + TP_G * plane) = make_float4(gv[0], gv[1], gv[2], gv[3]);
                    *reinterpret_cast<float4*>(tq + TP_O * plane) = make_float4(ov[0], ov[1], ov[2], ov[3]);
                    *reinterpret_cast<float4*>(tq + TP_C * plane) = make_float4(cv[0], cv[1], cv[2], cv[3]);
                    *reinterpret_cast<float4*>(tq + TP_H * plane) = make_float4(hv[0], hv[1], hv[2], hv[3]);
                }
                __syncthreads();
                continue;
            }
            if (head) {
                VG_LOSS_HEAD(m.v, _Pragma("unroll 1"))
            } else {
                const float* tp = tape + (long)t * TAPE * plane;
                const float* tb = tape + (long)(t > 0 ? t - 1 : 0) * TAPE * plane;      // the step before (unused at t = 0)
#pragma unroll 1
                for (int i = tid; i < 32 * H; i += NT) {
                    const int s = i / H, u = i - s * H, at = s * hpad + u;
                    const float ig = tp[TP_I * plane + at], fg = tp[TP_F * plane + at], gg = tp[TP_G * plane + at], og_ = tp[TP_O * plane + at];
                    const float tc = lstm_tanh(tp[TP_C * plane + at]);
                    const float cp = t > 0 ? tb[TP_C * plane + at] : 0.0f;
                    const float dhv = dh[s * ldh + u];
                    const float dcv = dc[s * ldh + u] + dhv * og_ * (1.0f - tc * tc);
                    dZ[s * ldz + u] = dcv * gg * ig * (1.0f - ig);
                    dZ[s * ldz + H + u] = dcv * cp * fg * (1.0f - fg);
                    dZ[s * ldz + 2 * H + u] = dcv * ig * (1.0f - gg * gg);
                    dZ[s * ldz + 3 * H + u] = dhv * tc * og_ * (1.0f - og_);
                    dc[s * ldh + u] = dcv * fg;
                }
                __syncthreads();
                bwd_dw(g + og.wih, xin, 0, xin, 4 * H, dZ, ldz, xact, ldxa, nullptr);
                if (t > 0) bwd_dw(g + og.whh, H, 0, H, 4 * H, dZ, ldz, tb + TP_H * plane, hpad, nullptr);
                bwd_db(g + og.bih, 4 * H, dZ, ldz);
                if (t > 0) bwd_dx(params + og.whh, H, 0, H, 4 * H, dZ, ldz, dh, ldh, false, nullptr);
                if (with_mlp1) bwd_dx(params + og.wih, xin, 0, xin, 4 * H, dZ, ldz, b.D0, ldxa, false, nullptr);
                __syncthreads();
            }
            // the head's mlp back to dJ; network 2's mlp1 back from dx_t (D0), its input's gradient wanted by nobody
            if (chain) chain_bwd(p, m.v, b, params, o, g, c_first, c_last, b.D0, c_src, c_ld, nullptr, 0, head ? b.dJ : nullptr, p.ld_j, false, nullptr, 0);
            if (head) {
                // (the joint rows are dead: h_n went to J two barriers ago)
#pragma unroll 1
                for (int i = tid; i < 32 * ldh; i += NT) {
                    const int s = i / ldh, u = i - s * ldh;
                    dh[i] = u < H ? b.dJ[s * p.ld_j + SELF_DIM + u] : 0.0f;      // the self-state columns get no gradient
                    dc[i] = 0.0f;
                }
#pragma unroll 1
                for (int i = tid; i < 32 * ldz; i += NT) dZ[i] = 0.0f;
                __syncthreads();
            }
        }
    }
#pragma unroll 1
    for (int c = tid; c < 4 * H; c += NT) g[og.bhh + c] = g[og.bih + c];       // (the thread that summed the column: bwd_db)
    if (tid == 0) g[o.total] = loss;
}

// blob float i from the flat parameters: pack_layer_f32's and pack_gates' maps, read backwards
__global__ void k_vn_pack_lstm(LstmPlan q, GradOffsets o, LstmGradOff og, const float* __restrict__ params, float* __restrict__ blob)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const VnPlan& p = q.v;
    if (i >= p.total_floats) return;
    float v = 0.0f;
    const VnLayer& G = q.g;
    if (i >= G.w_off && i < G.b_off + G.ncb * 32) {
        if (i >= G.b_off) {
            const int j = i - G.b_off, cb = j >> 5, unit = cb * 8 + (j & 7), row = ((j & 31) >> 3) * q.H + unit;
            if (unit < q.H) v = params[og.bih + row] + params[og.bhh + row];
        } else {
            int cb, j, kg, kk;
            blob_weight_of(G, i - G.w_off, cb, j, kg, kk);
            const int unit = cb * 8 + (j & 7), row = (j >> 3) * q.H + unit;
            if (unit < q.H) {
                if (kg < G.kg_split) { if (kk < G.K1) v = params[og.whh + (long)row * G.K1 + kk]; }
                else if (kk - G.kg_split * 8 < G.K2) v = params[og.wih + (long)row * G.K2 + kk - G.kg_split * 8];
            }
        }
    } else {
        int l = 0;
        while (l + 1 < p.n_layers && i >= p.L[l + 1].w_off) ++l;
        v = unpack_layer_at(p.L[l], i, params + o.w[l], params + o.b[l]);
    }
    blob[i] = v;
}

// the flat layout: mlp1's (weight, bias) pairs, weight_ih [4H][in], weight_hh [4H][H], bias_ih, bias_hh, mlp's pairs
inline void lstm_param_offsets(const LstmPlan& q, GradOffsets& o, LstmGradOff& og)
{
    const VnPlan& p = q.v;
    int at = 0;
    for (int l = 0; l < p.n_layers; ++l) {
        if (l == p.c0[1]) {
            og.wih = at; at += 4 * q.H * q.xin;
            og.whh = at; at += 4 * q.H * q.H;
            og.bih = at; at += 4 * q.H;
            og.bhh = at; at += 4 * q.H;
        }
        o.w[l] = at; at += p.L[l].N * p.L[l].K1;
        o.b[l] = at; at += p.L[l].N;
    }
    o.total = at;
}

// The recurrent family as value_net_grad.h's host templates ask it (GradCall: the call; om, om_cols: build_lstm_plan's -- the map columns
// behind the rotated ones in a stored row, the *_lstm_om entries)
struct LstmGrad {
    struct Launch {
        LstmPlan q; GradOffsets o; LstmGradOff og; LstmGradLds m; int grid, region, gpart; size_t shmem;
        size_t blob_floats() const { return (size_t)q.v.total_floats; }
    };
    static constexpr const char *pack_entry = "cs_value_net_pack_lstm", *sizes_entry = "cs_value_net_grad_sizes_lstm",
                                *loss_grad_entry = "cs_value_net_loss_grad_lstm";

    static int describe(const GradCall& c, Launch& a)
    {
        const int rc = build_lstm_plan(c.dims, c.n_dims, c.cols, a.q, c.om, c.om_cols);
        if (rc != CS_OK) return rc;
        a.o = GradOffsets{};
        a.og = LstmGradOff{};
        lstm_param_offsets(a.q, a.o, a.og);
        return CS_OK;
    }

    static int check_n(const GradCall& c)
    {
        return c.n > LSTM_MAX_N ? fail(CS_ERR_ARG, std::string(loss_grad_entry) + " takes at most 128 humans a sample (CS_VN_LSTM_MAX_N)") : CS_OK;
    }

    static int plan(const GradCall& c, Launch& a)
    {
        a.m = lstm_grad_lds_map(a.q);
        a.shmem = (size_t)a.m.v.total * sizeof(float);
        if (a.shmem > 160 * 1024)
            return fail(CS_ERR_ARG, "the activations and gradients of a tile of this network (rows of " + std::to_string(c.cols) + " + " +
                                        std::to_string(c.om_cols) + " columns, H = " + std::to_string(a.q.H) + ": " + std::to_string(a.shmem) +
                                        " bytes) do not fit the 160 KiB of LDS");
        const int jobs = (c.B + JROWS - 1) / JROWS;
        a.grid = jobs < GRAD_MAX_GROUPS ? jobs : GRAD_MAX_GROUPS;
        a.gpart = up(a.o.total + 1, 4);
        a.region = a.gpart + c.n * TAPE * 32 * a.q.hpad;
        return CS_OK;
    }

    // the job kernel: every workgroup's partial gradient and loss term into its region of the scratch; network 2's build has mlp1 in its step loops
    static int launch_jobs(const Launch& a, const GradCall& c)
    {
#define LSTM_GRAD_LAUNCH(M1)                                                                                                           \
    {                                                                                                                                  \
        const int rc2 = grant_lds<k_vn_lstm_grad<M1>>(a.shmem);                                                                        \
        if (rc2 != CS_OK) return rc2;                                                                                                  \
        hipLaunchKernelGGL((k_vn_lstm_grad<M1>), dim3(a.grid), dim3(NT), a.shmem, (hipStream_t)c.stream, a.q, a.m, a.o, a.og, c.d_weights, \
                           c.d_params, c.B, c.n, c.d_rows, c.d_targets, c.d_scratch, a.region, a.gpart, c.d_values);                   \
    }
        if (a.q.v.c0[1] > 0) LSTM_GRAD_LAUNCH(true)
        else LSTM_GRAD_LAUNCH(false)
#undef LSTM_GRAD_LAUNCH
        HIP_TRY(hipGetLastError());
        return CS_OK;
    }

    // k_vn_sgd's map of the recurrent blob: the Linear layers as the feed-forward blob holds them; the gates' rows in the order 8 * gate + unit
    // within a block of 8 units, weight_hh's columns before weight_ih's; bias_ih and bias_hh share one float, which bias_ih's thread writes
    struct SgdMap {
        LstmPlan q;
        GradOffsets o;
        LstmGradOff og;
        __host__ __device__ int operator()(int i, int& twin) const
        {
            twin = -1;
            const int H = q.H;
            const VnLayer& G = q.g;
            if (i >= og.wih && i < og.bhh + 4 * H) {
                if (i >= og.bhh) return -1;
                int row, kk = -1;
                if (i >= og.bih) {
                    row = i - og.bih;
                    twin = og.bhh + row;
                } else if (i >= og.whh) {
                    row = (i - og.whh) / H;
                    kk = i - og.whh - row * H;
                } else {
                    row = (i - og.wih) / q.xin;
                    kk = G.kg_split * 8 + i - og.wih - row * q.xin;
                }
                const int gate = row / H, unit = row - gate * H;
                const int cb = unit >> 3, col = 8 * gate + (unit & 7);
                return kk < 0 ? G.b_off + cb * 32 + col : blob_weight_at(G, cb, col, kk);
            }
            const VnPlan& p = q.v;
            int l = 0;
            while (l + 1 < p.n_layers && i >= o.w[l + 1]) ++l;
            return blob_layer_at(p.L[l], i - o.w[l]);
        }
    };
    static SgdMap sgd_map(const Launch& a) { return SgdMap{a.q, a.o, a.og}; }

    static void launch_pack(const Launch& a, const GradCall& c)
    {
        hipLaunchKernelGGL(k_vn_pack_lstm, dim3((a.q.v.total_floats + 255) / 256), dim3(256), 0, (hipStream_t)c.stream, a.q, a.o, a.og, c.d_params, c.d_weights);
    }
};

} // namespace

// ---- LSTM-RL on rows of 13 | 15 columns: no map columns (the entries of this file take no `kind`: 0)
extern "C" int cs_value_net_grad_sizes_lstm(const int32_t* dims, int n_dims, int cols, int B, int n, size_t* n_param_floats, size_t* n_scratch_floats)
{
    const GradCall c = describe_call(0, dims, n_dims, cols, false, 0, B, n);
    return grad_sizes<LstmGrad>(c, n_param_floats, n_scratch_floats);
}

extern "C" int cs_value_net_loss_grad_lstm(const int32_t* dims, int n_dims, const float* d_weights, size_t n_weight_floats, const float* d_params,
                                           size_t n_param_floats, int B, int n, int cols, const float* d_rows, const float* d_targets, float* d_grad,
                                           float* d_loss, float* d_values, float* d_scratch, size_t n_scratch_floats, void* stream)
{
    GradCall c = describe_call(0, dims, n_dims, cols, false, 0, B, n);
    set_minibatch(c, d_weights, n_weight_floats, d_params, n_param_floats, d_rows, d_targets, d_grad, d_loss, d_values, d_scratch, n_scratch_floats, stream);
    return loss_grad<LstmGrad>(c);
}

extern "C" int cs_value_net_train_step_lstm(const int32_t* dims, int n_dims, float* d_weights, size_t n_weight_floats, float* d_params,
                                            size_t n_param_floats, float* d_momentum, size_t n_momentum_floats, float lr, float momentum, int B,
                                            int n, int cols, const float* d_rows, const float* d_targets, float* d_grad, float* d_loss,
                                            double* d_loss_sum, float* d_values, float* d_scratch, size_t n_scratch_floats, void* stream)
{
    GradCall c = describe_call(0, dims, n_dims, cols, false, 0, B, n);
    set_minibatch(c, d_weights, n_weight_floats, d_params, n_param_floats, d_rows, d_targets, d_grad, d_loss, d_values, d_scratch, n_scratch_floats, stream);
    set_sgd(c, d_momentum, n_momentum_floats, lr, momentum, d_loss_sum);
    return train_step<LstmGrad>(c);
}

extern "C" int cs_value_net_blob_index_lstm(const int32_t* dims, int n_dims, int cols, int32_t* index, size_t n_param_floats)
{
    return blob_index<LstmGrad>(describe_call(0, dims, n_dims, cols, false, 0), index, n_param_floats);
}

extern "C" int cs_value_net_pack_lstm_device(const int32_t* dims, int n_dims, int cols, const float* d_params, size_t n_param_floats, float* d_blob,
                                             size_t n_blob_floats, void* stream)
{
    GradCall c = describe_call(0, dims, n_dims, cols, false, 0);
    set_pack(c, d_params, n_param_floats, d_blob, n_blob_floats, stream);
    return pack_device<LstmGrad>(c);
}

// ---- OM-LSTM-RL: rows of cols + om_cols columns (build_lstm_plan refuses om_cols < 1)
extern "C" int cs_value_net_grad_sizes_lstm_om(const int32_t* dims, int n_dims, int cols, int om_cols, int B, int n, size_t* n_param_floats,
                                               size_t* n_scratch_floats)
{
    const GradCall c = describe_call(0, dims, n_dims, cols, true, om_cols, B, n);
    return grad_sizes<LstmGrad>(c, n_param_floats, n_scratch_floats);
}

extern "C" int cs_value_net_loss_grad_lstm_om(const int32_t* dims, int n_dims, const float* d_weights, size_t n_weight_floats, const float* d_params,
                                              size_t n_param_floats, int B, int n, int cols, int om_cols, const float* d_rows, const float* d_targets,
                                              float* d_grad, float* d_loss, float* d_values, float* d_scratch, size_t n_scratch_floats, void* stream)
{
    GradCall c = describe_call(0, dims, n_dims, cols, true, om_cols, B, n);
    set_minibatch(c, d_weights, n_weight_floats, d_params, n_param_floats, d_rows, d_targets, d_grad, d_loss, d_values, d_scratch, n_scratch_floats, stream);
    return loss_grad<LstmGrad>(c);
}

extern "C" int cs_value_net_train_step_lstm_om(const int32_t* dims, int n_dims, float* d_weights, size_t n_weight_floats, float* d_params,
                                               size_t n_param_floats, float* d_momentum, size_t n_momentum_floats, float lr, float momentum, int B,
                                               int n, int cols, int om_cols, const float* d_rows, const float* d_targets, float* d_grad, float* d_loss,
                                               double* d_loss_sum, float* d_values, float* d_scratch, size_t n_scratch_floats, void* stream)
{
    GradCall c = describe_call(0, dims, n_dims, cols, true, om_cols, B, n);
    set_minibatch(c, d_weights, n_weight_floats, d_params, n_param_floats, d_rows, d_targets, d_grad, d_loss, d_values, d_scratch, n_scratch_floats, stream);
    set_sgd(c, d_momentum, n_momentum_floats, lr, momentum, d_loss_sum);
    return train_step<LstmGrad>(c);
}

extern "C" int cs_value_net_blob_index_lstm_om(const int32_t* dims, int n_dims, int cols, int om_cols, int32_t* index, size_t n_param_floats)
{
    return blob_index<LstmGrad>(describe_call(0, dims, n_dims, cols, true, om_cols), index, n_param_floats);
}

extern "C" int cs_value_net_pack_lstm_om_device(const int32_t* dims, int n_dims, int cols, int om_cols, const float* d_params, size_t n_param_floats,
                                                float* d_blob, size_t n_blob_floats, void* stream)
{
    GradCall c = describe_call(0, dims, n_dims, cols, true, om_cols);
    set_pack(c, d_params, n_param_floats, d_blob, n_blob_floats, stream);
    return pack_device<LstmGrad>(c);
}
