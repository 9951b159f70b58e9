// value_net_lstm_bf16_body.inc -- the body of k_value_net_lstm_bf16<WREG, MLP1> (value_net_lstm_bf16.hip, LSTM_OM 0) and of
// k_value_net_lstm_om_bf16<WREG, MLP1> (value_net_lstm_om_bf16.hip, LSTM_OM 1), as value_net_lstm_body.inc is the float32 pair's.  LSTM_OM 1:
// a row carries `om.om_cols` occupancy-map columns behind the rotated ones -- a second key / rank pass for CS_VN_MAPS_FIRST_ACTION, the map
// columns of a step staged as bf16 rows MB beside the gather tile G, network 2's mlp1 layer 0 and network 1's x slots split by column
// (lom_first_layer, lom_x_slot), NX resident slots of the x part.  With LSTM_OM 0 the preprocessor leaves the text k_value_net_lstm_bf16
// had before the two were one: its four builds keep their device code.  The arithmetic is stated in value_net_lstm_bf16.h; the fixed ends
// of a job and the layers are value_net_lstm_kernel.h's.  The LSTM_OM 1 declarations stand where k_value_net_lstm_om_bf16 had them, not in
// one block: moved together in front of `tid` they reordered scalar instructions of its <true, false> build.  The input is named through
// the three seams of value_net_lstm_kernel.h alone: k_value_net_lstm_worlds_bf16 (value_net_lstm_worlds_bf16.hip) is this text under LSTM_OM 0
// with the seams of value_net_lstm_worlds.h.
    extern __shared__ float lds[];
    constexpr int NB = WREG ? RB : GB;
#if LSTM_OM
    constexpr int NX = MLP1 ? RKX : KGF + RKM;              // register-resident slots of the x part a block
#else
    constexpr int NX = RKX;
#endif
    const LstmPlan& q = s.q;
    const VnPlan& p = q.v;
    float *P = lds + m.P, *Q = lds + m.Q, *J = lds + m.J, *G = lds + m.G, *HB = lds + m.HB, *XB = lds + m.XB;
#if LSTM_OM
    float* MB = lds + m.MB;                                 // [2][32][ld_m]: the map columns of a step as bf16 rows
#endif
    unsigned* key = reinterpret_cast<unsigned*>(lds + m.key);
    int* perm = reinterpret_cast<int*>(lds + m.perm);
#if LSTM_OM
    unsigned* key0 = reinterpret_cast<unsigned*>(lds + m.key0);
    int* perm0 = reinterpret_cast<int*>(lds + m.perm0);
#endif
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), hh = lane >> 5, li = lane & 31;
    const int row8 = tid >> 3;
    const int cols = p.cols, H = q.H, ldh = s.ld_h, ksh = s.ksh, ksx = s.ksx, KT = q.g.kg_total;
    const int nbw = (q.g.ncb - wave + 3) >> 2;              // this wavefront's blocks: wave, wave + 4, ...
    constexpr int gbuf = TILE_M * LDX;
#if LSTM_OM
    const int ldm = om.ld_m, mbuf = TILE_M * ldm;
#endif
    const float4* gw = reinterpret_cast<const float4*>(wb + q.g.w_off) + lane;
    int out_ld;

    int* ltab = reinterpret_cast<int*>(lds + m.LT);
    LSTM_FILL_TABLE(ltab, p)

    float4 wh[RB][RKH], wx[RB][NX];
    if constexpr (WREG) {
        const int slots = q.g.ncb * KT;
#pragma unroll
        for (int bi = 0; bi < RB; ++bi) {
            const int at = ((tid >> 6) + 4 * bi) * KT;             // (clamped: what lies beyond the wavefront's blocks and slots is never used)
#pragma unroll
            for (int k = 0; k < RKH; ++k) wh[bi][k] = gw[(at + k < slots ? at + k : 0) * 64];
#pragma unroll
            for (int j = 0; j < NX; ++j) wx[bi][j] = gw[(at + ksh + j < slots ? at + ksh + j : 0) * 64];
        }
    }

    for (int job = blockIdx.x; job * JROWS < NG; job += gridDim.x) {
        const long gbase = (long)job * JROWS;
        const int ng = NG - gbase < JROWS ? (int)(NG - gbase) : JROWS;
        LSTM_BEGIN_JOB(key, J, p.ld_j, rotated, gbase, ng, n, cols)
        for (int i = tid; i < 2 * TILE_M * ldh; i += NT) HB[i] = 0.0f;           // h0 = 0, and the columns between H and the last k-step's end
#if LSTM_OM
        // which map a step takes: its row's own (mperm = perm), or the one at that place in the order of the world's action 0, which is worked
        // out from that pair's own rows of `rotated`, whichever tile they lie in (uniform over the workgroup: every barrier is reached by all)
        const bool first_order = om.map_order == CS_VN_MAPS_FIRST_ACTION && sorted;
        const int* mperm = first_order ? perm0 : perm;
        if (first_order) {
            const long pair0 = (gbase + (row8 < ng ? row8 : 0)) / A * A;
            for (int j = tid & 7; j < n && row8 < ng; j += 8) key0[row8 * n + j] = lstm_key(rotated[(pair0 * n + j) * cols + 11]);
        }
#endif
        __syncthreads();
#if LSTM_OM
        if (first_order) LSTM_RANK(key0, perm0, n, ng, true)
#endif
        LSTM_RANK(key, perm, n, ng, sorted)
        __syncthreads();
        // a step's rows into buffer B of the gather tile (and of MB); slot J_ of the x part of the gates
#if LSTM_OM
#define LH_GATHER(B, T)                                                                                                      \
    {                                                                                                                        \
        lstm_gather(G + (B) * gbuf, LDX, rotated, perm, gbase, ng, n, cols, T);                                              \
        lom_gather_maps(reinterpret_cast<__bf16*>(MB + (B) * mbuf), 2 * ldm, om, mperm, gbase, ng, A, n, T);                 \
    }
#define LH_X_SLOT(ACC, W, J_) lom_x_slot<MLP1>(ACC, W, J_, xrow, mrow)
#else
#define LH_GATHER(B, T) LSTM_STEP_ROWS(G + (B) * gbuf, LDX, T);
#define LH_X_SLOT(ACC, W, J_) lh_x_slot<MLP1>(ACC, W, xrow + 8 * (J_))
#endif
        LH_GATHER(0, 0)
        float c[NB][4];
#pragma unroll
        for (int bi = 0; bi < NB; ++bi)
#pragma unroll
            for (int u = 0; u < 4; ++u) c[bi][u] = 0.0f;
        __syncthreads();
        lstm_self_state(J, p.ld_j, G, LDX, ng, tid);

        for (int t = 0; t < n; ++t) {
            const float* hrow = HB + (t & 1) * TILE_M * ldh + li * ldh + 4 * hh;
            __bf16* hdst = reinterpret_cast<__bf16*>(HB + ((t + 1) & 1) * TILE_M * ldh + li * ldh);
            if (t + 1 < n) LH_GATHER((t + 1) & 1, t + 1)
#if LSTM_OM
            if constexpr (MLP1) {
                // mlp1: its first layer here (into Q, or straight into the gates' operand rows when it is the only one), the others as the narrow kernel's
                const bool only = p.c0[1] - p.c0[0] == 1;
                lom_first_layer(ltab + p.c0[0] * LT_STRIDE, wb, G + (t & 1) * gbuf, LDX, MB + (t & 1) * mbuf, ldm, only ? XB : Q, only ? s.ld_xb : p.ld_pq);
                __syncthreads();
                if (!only) lstm_chain<LC_BF16_MLP1_REST>(ltab, p.ld_pq, wb, P, Q, p.c0[0] + 1, p.c0[1], Q, p.ld_pq, XB, s.ld_xb, out_ld);
            }
#else
            if constexpr (MLP1) lstm_chain<LC_BF16_MLP1>(ltab, p.ld_pq, wb, P, Q, p.c0[0], p.c0[1], G + (t & 1) * gbuf, LDX, XB, s.ld_xb, out_ld);
#endif
            const float* xrow = (MLP1 ? XB + li * s.ld_xb : G + (t & 1) * gbuf + li * LDX) + 4 * hh;
#if LSTM_OM
            const float* mrow = MB + (t & 1) * mbuf + li * ldm + 4 * hh;
#endif
            if constexpr (WREG) {
                // the x part of every block of the wavefront, then the barrier that publishes h_{t-1}, then W_hh and the pointwise part
                f32x16 acc[RB];
#pragma unroll
                for (int bi = 0; bi < RB; ++bi) {
                    if (bi >= nbw) break;
                    const float* bias = wb + q.g.b_off + (wave + 4 * bi) * 32 + 4 * hh;
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[bi][r] = bias[(r & 3) + 8 * (r >> 2)];
#pragma unroll
                    for (int j = 0; j < NX; ++j)
                        if (j < ksx) LH_X_SLOT(acc[bi], wx[bi][j], j);
                }
                __syncthreads();
#pragma unroll
                for (int bi = 0; bi < RB; ++bi) {
                    if (bi >= nbw) break;
#pragma unroll
                    for (int k = 0; k < RKH; ++k)
                        if (k < ksh) lh_h_slot(acc[bi], wh[bi][k], hrow + 8 * k);
                    lh_pointwise(acc[bi], c[bi], (wave + 4 * bi) * 8 + 4 * hh, H, hdst);
                }
            } else {
                // the same chain per block, its weights from the blob; the second barrier keeps the next step's gather and mlp1 off this step's rows
                __syncthreads();
#pragma unroll
                for (int bi = 0; bi < NB; ++bi) {
                    if (bi >= nbw) break;
                    const int blk = wave + 4 * bi;
                    const float* bias = wb + q.g.b_off + blk * 32 + 4 * hh;
                    f32x16 acc;
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[r] = bias[(r & 3) + 8 * (r >> 2)];
                    const float4* w = gw + (long)blk * KT * 64;
                    float4 nw = w[(long)ksh * 64];
                    for (int j = 0; j < ksx; ++j) {
                        const float4 wv = nw;
                        nw = w[(long)(j + 1 < ksx ? ksh + j + 1 : 0) * 64];
                        LH_X_SLOT(acc, wv, j);
                    }
                    for (int k = 0; k < ksh; ++k) {
                        const float4 wv = nw;
                        nw = w[(long)(k + 1 < ksh ? k + 1 : k) * 64];
                        lh_h_slot(acc, wv, hrow + 8 * k);
                    }
                    lh_pointwise(acc, c[bi], blk * 8 + 4 * hh, H, hdst);
                }
                __syncthreads();
            }
        }
#undef LH_GATHER
#undef LH_X_SLOT
        if constexpr (WREG) __syncthreads();          // (publishes h_n)

        lstm_hn_to_j(J, p.ld_j, reinterpret_cast<const __bf16*>(HB + (n & 1) * TILE_M * ldh), 2 * ldh, H, tid);
        __syncthreads();
        const float* out = lstm_chain<LC_BF16_MLP>(ltab, p.ld_pq, wb, P, Q, p.c0[1], p.c0[2], J, p.ld_j, nullptr, 0, out_ld);
        LSTM_STORE_VALUES(out, out_ld);
        __syncthreads();
    }
