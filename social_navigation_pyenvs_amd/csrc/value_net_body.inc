// value_net_body.inc -- the body of the value-network kernel (value_net.hip's header comment describes it), stated once for its three
// kernels: k_value_net (value_net.hip) copies a tile's rows from cs_lookahead's tensor, k_value_net_worlds (value_net_worlds.hip) generates
// them from the resident worlds, k_value_net_bf16 (value_net_bf16.hip) copies them and runs the bf16 layers.  The including kernel has the
// parameters p, m, M, wb, NG, A, n, robot, rstride, gamma, dt, values, declares `extern __shared__ float lds[]` and `const int gsum` (floats
// from the start of lds to the running sum of a chunked crowd mean) and defines, over the names of this body (b, t0, M, cols, n, ...):
//   VN_BEGIN_JOB(gbase, ng)        once per job of ng groups from gbase, before the job's first barrier
//   VN_TILE_SOURCE(g0)             a declaration, once per tile whose first group is g0
//   VN_LOAD_TILE(ch, rows, per)    chunk ch of the tile into b.X0 and b.grp as load_tile leaves them: `rows` rows, `per` humans a group
//   VN_REWARD(g, k)                the reward of group g, the job's k-th
// From value_net_plan.h it takes VnBufs, the CH_* tags and the constants; from its arithmetic (value_net_f32.h or value_net_bf16_layers.h):
//   run_chain<CH>(...)             the layers of one chain; the tag says which chain, for an arithmetic that treats them differently
//   vn_m1(buf, ld, r, c)           element (r, c) of mlp1's output or of the crowd mean, as float
//   vn_mean_store(buf, ld, k, c, v)  element c of group k's crowd mean into G
//   vn_m1pad(p)                    the columns of mlp1's output that the attention's k-steps read of the mean
//   vn_sum_cols(p, m1pad)          the columns of the running sum that a chunked mean zeroes
//   vn_mean_pass(p)                whether a group in chunks runs the mean pre-pass
// The input tile's row stride is LDX, a compile-time constant, unless the kernel defines VN_INPUT_STRIDE (k_value_net_om: an int
// argument, the wide first layer's K rounded up to 8, plus 4).
    VnBufs b;
    b.X0 = lds + m.X0; b.M1 = lds + m.M1; b.P = lds + m.P; b.Q = lds + m.Q; b.G = lds + m.G; b.Gsum = lds + gsum; b.J = lds + m.J;
    b.sc = lds + m.sc; b.den = lds + m.den; b.val = lds + m.val; b.grp = reinterpret_cast<int*>(lds + m.grp);
    const int tid = threadIdx.x;
    const int rbs = M / 32, cols = p.cols;
    const bool sarl = p.kind == CS_VN_SARL;
    const int chunks = n <= M ? 1 : (n + M - 1) / M;
    const int gpt = n <= M ? M / n : 1;
    const int m1pad = vn_m1pad(p);
#ifdef VN_INPUT_STRIDE
    const int ldx = VN_INPUT_STRIDE;
#else
    constexpr int ldx = LDX;
#endif
    int out_ld;

    for (int job = blockIdx.x; job * JROWS < NG; job += gridDim.x) {
        const int gbase = job * JROWS;
        const int ng = NG - gbase < JROWS ? NG - gbase : JROWS;
        VN_BEGIN_JOB(gbase, ng);
        if (sarl) {
            for (int i = tid; i < JROWS * p.ld_j; i += NT) b.J[i] = 0.0f;
            if (tid < JROWS) b.den[tid] = 0.0f;
        } else if (tid < JROWS) b.val[tid] = INFINITY;
        __syncthreads();

        for (int t0 = 0; t0 < ng; t0 += gpt) {
            const int tg = ng - t0 < gpt ? ng - t0 : gpt;
            VN_TILE_SOURCE(gbase + t0);
            if (sarl && chunks > 1 && vn_mean_pass(p)) {
                // more humans than a tile holds: a first pass over the chunks for the mean of mlp1 (sarl.py:42), a float32 running sum in Gsum
                for (int c = tid; c < vn_sum_cols(p, m1pad); c += NT) b.Gsum[c] = 0.0f;
                for (int ch = 0; ch < chunks; ++ch) {
                    const int rows = n - ch * M < M ? n - ch * M : M;
                    VN_LOAD_TILE(ch, rows, n);
                    __syncthreads();
                    run_chain<CH_MLP1>(p, wb, b, p.c0[0], p.c0[1], b.X0, ldx, nullptr, 0, rbs, b.M1, p.ld_m1, out_ld);
                    for (int c = tid; c < m1pad; c += NT) {
                        float s = b.Gsum[c];
                        for (int r = 0; r < rows; ++r) s += vn_m1(b.M1, p.ld_m1, r, c);
                        b.Gsum[c] = s;
                    }
                    __syncthreads();
                }
                for (int c = tid; c < m1pad; c += NT) vn_mean_store(b.G, p.ld_m1, 0, c, b.Gsum[c] / (float)n);
                __syncthreads();
            }
            // phase 0: a tile holds its groups whole -- denominator, weights and weighted sum in one visit.  A group in chunks needs the
            // softmax denominator of ALL its humans before the first weight (sarl.py:52-53): phase 1 sums it, phase 2 recomputes and weighs.
            for (int phase = chunks > 1 ? 1 : 0; phase <= (chunks > 1 ? 2 : 0); ++phase)
            for (int ch = 0; ch < chunks; ++ch) {
                const int per = chunks > 1 ? (n - ch * M < M ? n - ch * M : M) : n;      // humans of each group in this tile
                const int rows = chunks > 1 ? per : tg * n;
                VN_LOAD_TILE(ch, rows, per);
                __syncthreads();
                if (!sarl) {
                    if (phase == 1) continue;
                    const float* out = run_chain<CH_CADRL>(p, wb, b, p.c0[0], p.c0[1], b.X0, ldx, nullptr, 0, rbs, nullptr, 0, out_ld);
                    if (tid < tg) {         // cadrl.py:269: the minimum over the humans
                        float v = b.val[t0 + tid];
                        for (int j = 0; j < per; ++j) {      // (torch.min's order: a NaN stays)
                            const float x = out[(tid * per + j) * out_ld];
                            v = (x < v || x != x) ? x : v;
                        }
                        b.val[t0 + tid] = v;
                    }
                    __syncthreads();
                    continue;
                }
                if (ch == 0)                // sarl.py:36: the self state is read from the first human's row
                    for (int i = tid; i < tg * SELF_DIM; i += NT) b.J[(t0 + i / SELF_DIM) * p.ld_j + i % SELF_DIM] = b.X0[(i / SELF_DIM) * per * ldx + i % SELF_DIM];
                run_chain<CH_MLP1>(p, wb, b, p.c0[0], p.c0[1], b.X0, ldx, nullptr, 0, rbs, b.M1, p.ld_m1, out_ld);
                if (p.with_global && chunks == 1 && n > 1) {
                    for (int i = tid; i < tg * m1pad; i += NT) {
                        const int k = i / m1pad, c = i - k * m1pad;
                        float s = 0.0f;
                        for (int j = 0; j < n; ++j) s += vn_m1(b.M1, p.ld_m1, k * n + j, c);
                        vn_mean_store(b.G, p.ld_m1, k, c, s / (float)n);
                    }
                    __syncthreads();
                }
                {   // attention scores and the masked softmax's terms exp(s) * (s != 0) (sarl.py:48-52)
                    const float* out = run_chain<CH_REDUCED>(p, wb, b, p.c0[2], p.c0[3], b.M1, p.ld_m1, p.with_global ? b.G : nullptr, p.ld_m1, rbs, nullptr, 0, out_ld);
                    for (int r = tid; r < M; r += NT) {
                        const float s = out[r * out_ld];
                        b.sc[r] = (r < rows && s != 0.0f) ? expf(s) : 0.0f;
                    }
                    __syncthreads();
                }
                if (phase != 2) {           // the denominator, in human order
                    if (tid < tg) {
                        float s = b.den[t0 + tid];
                        for (int j = 0; j < per; ++j) s += b.sc[tid * per + j];
                        b.den[t0 + tid] = s;
                    }
                    __syncthreads();
                    if (phase == 1) continue;
                }
                for (int r = tid; r < rows; r += NT) b.sc[r] = b.sc[r] / b.den[t0 + r / per];
                __syncthreads();
                {   // mlp2 and the weighted sum of its rows (sarl.py:57-60)
                    const float* f = run_chain<CH_REDUCED>(p, wb, b, p.c0[1], p.c0[2], b.M1, p.ld_m1, nullptr, 0, rbs, nullptr, 0, out_ld);
                    const int fw = p.feat;
                    for (int i = tid; i < tg * fw; i += NT) {
                        const int k = i / fw, c = i - k * fw;
                        float s = b.J[(t0 + k) * p.ld_j + SELF_DIM + c];
                        for (int j = 0; j < per; ++j) s = fmaf(b.sc[k * per + j], f[(k * per + j) * out_ld + c], s);
                        b.J[(t0 + k) * p.ld_j + SELF_DIM + c] = s;
                    }
                    __syncthreads();
                }
            }
        }

        if (sarl) {
            const float* out = run_chain<CH_MLP3>(p, wb, b, p.c0[3], p.c0[4], b.J, p.ld_j, nullptr, 0, 1, nullptr, 0, out_ld);
            if (tid < ng) b.val[tid] = out[tid * out_ld];
            __syncthreads();
        }
        if (tid < ng) {                     // cadrl.py:85-90 compute_action_value
            const int g = gbase + tid;
            const float vpref = robot[(long)(g / A) * rstride + 7];
            values[g] = VN_REWARD(g, tid) + powf(gamma, dt * vpref) * b.val[tid];
        }
        __syncthreads();
    }
