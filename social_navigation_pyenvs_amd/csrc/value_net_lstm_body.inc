// value_net_lstm_body.inc -- the body of k_value_net_lstm<WREG, MLP1> and of k_value_net_lstm_om<WREG, MLP1> (value_net_lstm.hip), which
// includes it once with LSTM_OM 0 and once with LSTM_OM 1.  LSTM_OM 1: a row carries `om.om_cols` occupancy-map columns behind the rotated
// ones (cs_value_net_decide_lstm_om), the register-resident weights hold RKG_OM k-groups.  With LSTM_OM 0 the preprocessor leaves the text
// k_value_net_lstm had before there were map columns: its four builds keep their device code.  The fixed ends of a job (LSTM_FILL_TABLE,
// LSTM_BEGIN_JOB, LSTM_RANK, lstm_self_state, lstm_hn_to_j, lstm_store_values) and the layers (lstm_chain<LC_F32>) are value_net_lstm_kernel.h's,
// shared with k_value_net_lstm_bf16; the step loop between them is this kernel's own.  The input is named through the three seams of
// value_net_lstm_kernel.h alone (LSTM_BEGIN_JOB, LSTM_STEP_ROWS, LSTM_STORE_VALUES): k_value_net_lstm_worlds (value_net_lstm_worlds.hip) is
// this text under LSTM_OM 0 with the seams of value_net_lstm_worlds.h, which generate the rows from the worlds.
    extern __shared__ float lds[];
    constexpr int NB = WREG ? RB : GB;
#if LSTM_OM
    constexpr int RK = RKG_OM;
#else
    constexpr int RK = RKG;
#endif
    const VnPlan& p = q.v;
    float *P = lds + m.P, *Q = lds + m.Q, *J = lds + m.J;
    unsigned* key = reinterpret_cast<unsigned*>(lds + m.key);
    int* perm = reinterpret_cast<int*>(lds + m.perm);
    float* XH = lds + m.XH;                                 // [2][32][ld_xh]: a sequence's joint row (h of the step before | x_t)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), hh = lane >> 5, li = lane & 31;
    const int row8 = tid >> 3;
    const int cols = p.cols, H = q.H, hpad = q.hpad, ldxh = q.ld_xh, KG = q.g.kg_total;
    const int nbw = (q.g.ncb - wave + 3) >> 2;              // this wavefront's blocks: wave, wave + 4, ...
    constexpr bool with_mlp1 = MLP1;
    // where the gather puts a step's rows: network 1 straight into the joint rows' x part, network 2 into a tile of their own for mlp1
    float* G = with_mlp1 ? lds + m.X : XH + hpad;
#if LSTM_OM
    const int ldx = om.xw + 4;                              // (the gather tile's stride: the columns rounded up to 8, plus 4, as k_value_net_om's)
#else
    constexpr int ldx = LDX;
#endif
    const int ldg = with_mlp1 ? ldx : ldxh, gbuf = TILE_M * ldg;
    const float4* gw = reinterpret_cast<const float4*>(wb + q.g.w_off) + lane;
    int out_ld;

    int* ltab = reinterpret_cast<int*>(lds + m.LT);
    LSTM_FILL_TABLE(ltab, p)

    float4 wreg[RB][RK];
    if constexpr (WREG) {
#pragma unroll
        for (int bi = 0; bi < RB; ++bi)
#pragma unroll
            for (int kg = 0; kg < RK; ++kg) {
                const int at = ((tid >> 6) + 4 * bi) * KG + kg;    // (clamped: what lies beyond the wavefront's blocks and k-groups is never used)
                wreg[bi][kg] = gw[(at < q.g.ncb * KG ? at : 0) * 64];
            }
    }

    for (int job = blockIdx.x; job * JROWS < NG; job += gridDim.x) {
        const long gbase = (long)job * JROWS;
        const int ng = NG - gbase < JROWS ? (int)(NG - gbase) : JROWS;
        LSTM_BEGIN_JOB(key, J, p.ld_j, rotated, gbase, ng, n, cols)
        for (int i = tid; i < TILE_M * ldxh; i += NT) XH[i] = 0.0f;                                  // h0 = 0
#if LSTM_OM
        // which map a step takes: its row's own (mperm = perm), or the one at that place in the order of the world's action 0, which is worked
        // out from that pair's own rows of `rotated`, whichever tile they lie in (uniform over the workgroup: every barrier is reached by all)
        const bool first_order = om.map_order == CS_VN_MAPS_FIRST_ACTION && sorted;
        unsigned* key0 = reinterpret_cast<unsigned*>(lds + om.key0);
        int* perm0 = reinterpret_cast<int*>(lds + om.perm0);
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
#if LSTM_OM
#define LSTM_GATHER(X, T) lstm_gather_om(X, ldg, rotated, om, perm, mperm, gbase, ng, A, n, cols, T)
#else
#define LSTM_GATHER(X, T) LSTM_STEP_ROWS(X, ldg, T)
#endif
        LSTM_GATHER(G, 0);
        float c[NB][4];
#pragma unroll
        for (int bi = 0; bi < NB; ++bi)
#pragma unroll
            for (int u = 0; u < 4; ++u) c[bi][u] = 0.0f;
        __syncthreads();
        lstm_self_state(J, p.ld_j, G, ldg, ng, tid);

        for (int t = 0; t < n; ++t) {
            float* cur = XH + (t & 1) * TILE_M * ldxh;
            float* nxt = XH + ((t + 1) & 1) * TILE_M * ldxh;
            if (t + 1 < n) LSTM_GATHER(G + ((t + 1) & 1) * (with_mlp1 ? gbuf : TILE_M * ldxh), t + 1);
            if constexpr (with_mlp1) lstm_chain<LC_F32>(ltab, p.ld_pq, wb, P, Q, p.c0[0], p.c0[1], G + (t & 1) * gbuf, ldx, cur + hpad, ldxh, out_ld);
            const float* brow = cur + li * ldxh + 4 * hh;
#pragma unroll
            for (int bi = 0; bi < NB; ++bi) {
                if (bi >= nbw) break;
                const int blk = wave + 4 * bi;
                f32x16 acc;
                const float* bias = wb + q.g.b_off + blk * 32 + 4 * hh;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = bias[(r & 3) + 8 * (r >> 2)];
                // the k-groups in descending order (x_t's, then h's), whichever kernel
                if constexpr (WREG) {
#if LSTM_OM
                    static_assert(RKG_OM == RKG + 1, "the step below runs the one k-group beyond the switch");
                    if (KG > RKG) LSTM_KSTEP(wreg[bi][RKG], RKG)
                    switch (KG > RKG ? RKG : KG) {
#else
                    switch (KG) {
#endif
                    case 14: LSTM_KSTEP(wreg[bi][13], 13) [[fallthrough]];
                    case 13: LSTM_KSTEP(wreg[bi][12], 12) [[fallthrough]];
                    case 12: LSTM_KSTEP(wreg[bi][11], 11) [[fallthrough]];
                    case 11: LSTM_KSTEP(wreg[bi][10], 10) [[fallthrough]];
                    case 10: LSTM_KSTEP(wreg[bi][9], 9) [[fallthrough]];
                    case 9: LSTM_KSTEP(wreg[bi][8], 8) [[fallthrough]];
                    case 8: LSTM_KSTEP(wreg[bi][7], 7) [[fallthrough]];
                    case 7: LSTM_KSTEP(wreg[bi][6], 6) [[fallthrough]];
                    case 6: LSTM_KSTEP(wreg[bi][5], 5) [[fallthrough]];
                    case 5: LSTM_KSTEP(wreg[bi][4], 4) [[fallthrough]];
                    case 4: LSTM_KSTEP(wreg[bi][3], 3) [[fallthrough]];
                    case 3: LSTM_KSTEP(wreg[bi][2], 2) [[fallthrough]];
                    default: LSTM_KSTEP(wreg[bi][1], 1) LSTM_KSTEP(wreg[bi][0], 0)
                    }
                } else {
                    const float4* w = gw + (long)blk * KG * 64;
                    float4 nw = w[(long)(KG - 1) * 64];
                    for (int kg = KG - 1; kg >= 0; --kg) {
                        const float4 wv = nw;
                        nw = w[(long)(kg > 0 ? kg - 1 : 0) * 64];
                        LSTM_KSTEP(wv, kg)
                    }
                }
                float hv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float ig = lstm_sigmoid(acc[u]), fg = lstm_sigmoid(acc[4 + u]), gg = lstm_tanh(acc[8 + u]), og = lstm_sigmoid(acc[12 + u]);
                    const float cn = fg * c[bi][u] + ig * gg;
                    c[bi][u] = cn;
                    hv[u] = blk * 8 + 4 * hh + u < H ? og * lstm_tanh(cn) : 0.0f;      // (zero weights give 0 for finite inputs only)
                }
                *reinterpret_cast<float4*>(nxt + li * ldxh + blk * 8 + 4 * hh) = make_float4(hv[0], hv[1], hv[2], hv[3]);
            }
            __syncthreads();
        }
#undef LSTM_GATHER

        lstm_hn_to_j(J, p.ld_j, XH + (n & 1) * TILE_M * ldxh, ldxh, H, tid);
        __syncthreads();
        const float* out = lstm_chain<LC_F32>(ltab, p.ld_pq, wb, P, Q, p.c0[1], p.c0[2], J, p.ld_j, nullptr, 0, out_ld);
        LSTM_STORE_VALUES(out, out_ld);
        __syncthreads();
    }
