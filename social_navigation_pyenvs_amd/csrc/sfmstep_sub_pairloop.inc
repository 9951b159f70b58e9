// sfmstep_sub_pairloop.inc -- a fragment of k_sfm_step (sfmstep_kernel.h), included inside the kernel body: the pair-once loop (each unordered pair evaluated once, reaction handed over through LDS), the reaction sum, and the contact pass behind a wave vote.
// Not a translation unit and not a function: it reads and writes the kernel's locals (the lane's row in registers, the LDS views, the
// template parameters).  The split is textual -- the token stream of the kernel is what it was in one file -- so that each phase can be
// read on its own; sfmstep_kernel.h lists the phases in order.  gfx950 only.
        STAMP(1);
        if constexpr (N3L) {
            if (valid) {
                float2* acc = lds_acc + pbase + row + 1;                 // acc[u * 2T + k]: that partner's slot in row u
                float2* accw = lds_acc + pbase;                          // compile-time row builds: slot aoff[k] of the world
                float ex = 0.0f, ey = 0.0f, rdmax = -1.0e30f;   // max over my partners of rs_j - dist
                if constexpr (!(LEAN && NO_WALLS)) { if (Hf >= UA) { fetch(qa, va, 0); fetch_pp(pa, 0); } }
                // (fx, fy): the force on me, in units of sign(A_me); (gx, gy): what goes to the partner's reaction slot -- the same force
                // when all parameters are equal (exact antisymmetry), the partner's OWN law on the shared geometry otherwise (PP)
                auto pair_once = [&](const float4 q, const float2 vq, const float4 pj, float& fx, float& fy, float& gx, float& gy) {
                    const float dx = px - q.x, dy = py - q.y;
                    if constexpr (SOC == 2) {
                        // (without the k1 / k2 contact terms: the contact pass below adds them for the rows that touch somebody)
                        float rd;
                        pair_force_moussaid_once<false>(sp, dx, dy, vx - vq.x, vy - vq.y, my_rs + q.z, fx, fy, &rd);
                        gx = fx; gy = fy;
                        rdmax = fmaxf(rdmax, rd - my_rs);                        // (the vote's form: max over my partners of rs_j - dist)
                    } else {
                        // [A e^{rd/B}] n + [C e^{rd/D}] t, in units of sign(A); the k1 / k2 contact parts are exact
                        // zeros unless rd > 0 and are added by the contact pass below
                        const float d2 = fmaf(dx, dx, dy * dy);
                        const float inv = rsq_fast(d2);
                        const float rd = fmaf(-d2, inv, q.z);                     // rs_j - dist  (= rij - dist - rs_i)
                        const float ga = exp2_fast(fmaf(rd, sp.cB, lAi)) * inv;   // |A| e^{(rij - dist)/B} / dist
                        fx = ga * dx; fy = ga * dy;
                        if constexpr (SOC == 1) {
                            const float gc = exp2_fast(fmaf(rd, sp.cD, lCi)) * (inv * sp.sAC); // +-|C| e^{(rij - dist)/D} / dist
                            fx = fmaf(-gc, dy, fx); fy = fmaf(gc, dx, fy);                       // along t = (-ny, nx)
                        }
                        if constexpr (PP) {
                            const float rdi = fmaf(-d2, inv, my_rs);                  // rs_me - dist: the partner's exponent offset holds its own rs
                            const float gb = exp2_fast(fmaf(rdi, pj.y, pj.x)) * inv;
                            gx = gb * dx; gy = gb * dy;
                            if constexpr (SOC == 1) {
                                const float gd = exp2_fast(fmaf(rdi, pj.w, pj.z)) * (inv * q.w);   // q.w: sign(C_j) sign(A_j)
                                gx = fmaf(-gd, dy, gx); gy = fmaf(gd, dx, gy);
                            }
                        } else {
                            gx = fx; gy = fy;
                        }
                        rdmax = fmaxf(rdmax, rd);
                    }
                };
                // groups of UA partners; the partner rows of the NEXT group are fetched while the current group is
                // evaluated (two register sets, a compiler memory barrier pins the prefetch), and the accumulator
                // slots are read before the evaluation and written after it
                // What the compiler emits here: the accumulator slots so[u] are separate address registers and stay single ds_read_b64 /
                // ds_write_b64; the partner rows and the two rows of the reaction sum below are constant offsets off one base register and
                // become ds_read2_b64 / ds_read2st64_b64 (the stride-64 form reaches the 1 KiB row pitch).  The MI355X LDS table prices a
                // paired read at 8 LDS-array cycles against 2 + 2 for two single ones, but forcing the single form on the 8-byte rows
                // (volatile LDS reads: 24 ds_read_b64 per substep, no register more) measured 0.03 us SLOWER per launch of the headline
                // build in six of six alternating runs, and on no build faster by more than the runs' spread (HISTORY.md): the paired
                // forms stay.
                constexpr int AR = ACC_PITCH;
                auto group = [&](const float4 (&q)[UA], const float2 (&vq)[UA], const float4 (&pq)[PP ? UA : 1], float2 (&ac)[UA], const int (&so)[UA]) {
                    if constexpr (SOC == 2) {
#pragma unroll
                        for (int u = 0; u < UA; ++u) {
                            float fx, fy, gx, gy;
                            pair_once(q[u], vq[u], make_float4(0.0f, 0.0f, 0.0f, 0.0f), fx, fy, gx, gy);
                            ex += fx; ey += fy;
                            ac[u].x += gx; ac[u].y += gy;
                        }
                    } else {
                        // Helbing / Guo: the UA partners advance stage by stage (scheduling barriers between the
                        // stages), so the UA v_rsq_f32 and the UA v_exp_f32 issue back to back and each result is
                        // consumed ~UA instructions later instead of right behind its transcendental
                        float dx[UA], dy[UA], d2[UA], inv[UA], rd[UA], ea[UA], ec[UA], eb[UA], ed[UA];
#pragma unroll
                        for (int u = 0; u < UA; ++u) {
                            dx[u] = px - q[u].x; dy[u] = py - q[u].y;
                            d2[u] = fmaf(dx[u], dx[u], dy[u] * dy[u]);
                        }
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int u = 0; u < UA; ++u) inv[u] = rsq_fast(d2[u]);
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int u = 0; u < UA; ++u) {
                            rd[u] = fmaf(-d2[u], inv[u], q[u].z);
                            ea[u] = fmaf(rd[u], sp.cB, lAi);
                            if constexpr (SOC == 1) ec[u] = fmaf(rd[u], sp.cD, lCi);
                            if constexpr (PP) {   // the partner's side of the same pair, from its parameter row
                                const float rdi = fmaf(-d2[u], inv[u], my_rs);
                                eb[u] = fmaf(rdi, pq[u].y, pq[u].x);
                                if constexpr (SOC == 1) ed[u] = fmaf(rdi, pq[u].w, pq[u].z);
                            }
                        }
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int u = 0; u < UA; ++u) {
                            ea[u] = exp2_fast(ea[u]);
                            if constexpr (SOC == 1) ec[u] = exp2_fast(ec[u]);
                            if constexpr (PP) {
                                eb[u] = exp2_fast(eb[u]);
                                if constexpr (SOC == 1) ed[u] = exp2_fast(ed[u]);
                            }
                        }
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int u = 0; u < UA; ++u) {
                            const float ga = ea[u] * inv[u];
                            if constexpr (PP) {
                                const float gb = eb[u] * inv[u];
                                if constexpr (SOC == 1) {
                                    const float gc = ec[u] * (inv[u] * sp.sAC), gd = ed[u] * (inv[u] * q[u].w);
                                    ex += fmaf(-gc, dy[u], ga * dx[u]); ey += fmaf(gc, dx[u], ga * dy[u]);
                                    ac[u].x += fmaf(-gd, dy[u], gb * dx[u]); ac[u].y += fmaf(gd, dx[u], gb * dy[u]);
                                } else {
                                    ex = fmaf(ga, dx[u], ex); ey = fmaf(ga, dy[u], ey);
                                    ac[u].x = fmaf(gb, dx[u], ac[u].x); ac[u].y = fmaf(gb, dy[u], ac[u].y);
                                }
                            } else if constexpr (SOC == 1) {
                                const float gc = ec[u] * (inv[u] * sp.sAC);
                                const float fx = fmaf(-gc, dy[u], ga * dx[u]), fy = fmaf(gc, dx[u], ga * dy[u]);
                                ex += fx; ey += fy;
                                ac[u].x += fx; ac[u].y += fy;
                            } else {
                                // Helbing: f = ga d goes into my sum and into the partner's slot by one FMA each (4 instead of
                                // 2 multiplies + 4 adds; the two sums see the same product, rounded once per sum)
                                ex = fmaf(ga, dx[u], ex); ey = fmaf(ga, dy[u], ey);
                                ac[u].x = fmaf(ga, dx[u], ac[u].x); ac[u].y = fmaf(ga, dy[u], ac[u].y);
                            }
                        }
#pragma unroll
                        for (int u = 0; u < UA; ++u) rdmax = fmaxf(rdmax, rd[u]);   // (pairs of them fuse into v_max3_f32)
                    }
#pragma unroll
                    for (int u = 0; u < UA; ++u) accw[u * AR + so[u]] = ac[u];
                    LDS_ORDER_FENCE(); // the next group's slots were written by other lanes in this group
                };
                // reaction slot of the partner at ring distance k + 1: its row index inside the world, (row + 1 + k) mod rows
                auto slot_rt = [&](int k) { const int t = row + 1 + k; return t >= rows ? t - rows : t; };
                int k0 = 0;
                if constexpr (ROWS_CT > 0) {
                    // rows known at compile time: the groups are laid out one after the other, no loop, no scalar branches
                    constexpr int NG = ((ROWS_CT - 1) / 2) / UA;
                    float4 qb[UA], pb[PP ? UA : 1];
                    float2 vb[UA], ac[UA];
                    for_each_index([&](auto gtag) {
                        constexpr int g = decltype(gtag)::value;
                        int so[UA];
#pragma unroll
                        for (int u = 0; u < UA; ++u) {
                            so[u] = aoff[g * UA + u];
                            ac[u] = g == 0 ? make_float2(0.0f, 0.0f) : accw[u * AR + so[u]];   // the first group stores: no zeroing pass
                        }
                        if constexpr (g + 1 < NG) {
                            if constexpr (g & 1) { fetch(qa, va, (g + 1) * UA); fetch_pp(pa, (g + 1) * UA); } else { fetch(qb, vb, (g + 1) * UA); fetch_pp(pb, (g + 1) * UA); }
                        }
                        asm volatile("" ::: "memory");
                        if constexpr (g & 1) group(qb, vb, pb, ac, so); else group(qa, va, pa, ac, so);
                    }, std::make_integer_sequence<int, NG>{});
                    k0 = NG * UA;
                } else if (Hf >= UA) {
                    float4 qb[UA], pb[PP ? UA : 1];
                    float2 vb[UA], ac[UA];
                    int so[UA];
                    bool first = true;
                    for (;;) {
#pragma unroll
                        for (int u = 0; u < UA; ++u) {
                            so[u] = slot_rt(k0 + u);
                            ac[u] = first ? make_float2(0.0f, 0.0f) : accw[u * AR + so[u]];   // (uniform: the first group stores)
                        }
                        first = false;
                        const bool more_b = k0 + 2 * UA <= Hf;
                        if (more_b) { fetch(qb, vb, k0 + UA); fetch_pp(pb, k0 + UA); }
                        asm volatile("" ::: "memory");
                        group(qa, va, pa, ac, so);
                        k0 += UA;
                        if (!more_b) break;
#pragma unroll
                        for (int u = 0; u < UA; ++u) { so[u] = slot_rt(k0 + u); ac[u] = accw[u * AR + so[u]]; }
                        const bool more_a = k0 + 2 * UA <= Hf;
                        if (more_a) { fetch(qa, va, k0 + UA); fetch_pp(pa, k0 + UA); }
                        asm volatile("" ::: "memory");
                        group(qb, vb, pb, ac, so);
                        k0 += UA;
                        if (!more_a) break;
                    }
                }
                if constexpr (ROWS_CT > 0) {
                    constexpr int HC = (ROWS_CT - 1) / 2;
                    if constexpr (HC % UA != 0) {   // (UA = 2: at most one partner left over)
                        static_assert(HC % UA == 1 || UA > 2, "remainder of the compile-time group layout");
#pragma unroll
                        for (int k = (HC / UA) * UA; k < HC; ++k) {
                            float fx, fy, gx, gy;
                            float2 vq = make_float2(0.0f, 0.0f);
                            if constexpr (SOC == 2) vq = rv[k];
                            float4 qk;
                            if constexpr (PP) qk = rp[k];
                            else if constexpr (XY_ROWS) { const float2 xy = rxy[k]; qk = make_float4(xy.x, xy.y, rsj[k], 0.0f); }
                            else { const float2 xy = *reinterpret_cast<const float2*>(&rp[k]); qk = make_float4(xy.x, xy.y, rsj[k], 0.0f); }
                            pair_once(qk, vq, PP ? rpp[k] : make_float4(0.0f, 0.0f, 0.0f, 0.0f), fx, fy, gx, gy);
                            ex += fx; ey += fy;
                            float2 ac = (k == 0) ? make_float2(0.0f, 0.0f) : accw[aoff[k]];   // (partner 0 without a full group: first writer of row 0)
                            ac.x += gx; ac.y += gy;
                            accw[aoff[k]] = ac;
                            LDS_ORDER_FENCE();
                        }
                    }
                } else
                for (int k = k0; k < Hf; ++k) {   // (fewer than UA partners left; k - k0 is the accumulator row they go to when no group ran)
                    float fx, fy, gx, gy;
                    float2 vq = make_float2(0.0f, 0.0f);
                    if constexpr (SOC == 2) vq = rv[k];
                    pair_once(rp[k], vq, PP ? rpp[k] : make_float4(0.0f, 0.0f, 0.0f, 0.0f), fx, fy, gx, gy);
                    ex += fx; ey += fy;
                    const int so = slot_rt(k);
                    float2 ac = (k == 0) ? make_float2(0.0f, 0.0f) : accw[so];   // partner 0 of a world without a full group: first writer of row 0
                    ac.x += gx; ac.y += gy;
                    accw[so] = ac;
                    LDS_ORDER_FENCE();
                }
                if ((rows & 1) == 0) { // antipodal partner: each end evaluates it for itself (lean build: row fetched at the top)
                    float fx, fy;
                    if constexpr (!(LEAN && NO_WALLS)) {
                        if constexpr (ROWS_CT > 0 && N3L) { const float2 xy = *reinterpret_cast<const float2*>(&rp[(ROWS_CT - 1) / 2]); qz = make_float4(xy.x, xy.y, rsj[(ROWS_CT - 1) / 2], 0.0f); }
                        else qz = rp[Hf];
                        if constexpr (SOC == 2) vz = rv[Hf];
                    }
                    float gx, gy;   // (each end evaluates its own side: nothing handed over)
                    pair_once(qz, vz, make_float4(0.0f, 0.0f, 0.0f, 0.0f), fx, fy, gx, gy);
                    ex += fx; ey += fy;
                }
                STAMP(9);
                LDS_ORDER_FENCE(); // the reaction slots of this lane were written by its partners
                const float2* rr = lds_acc + pbase + row;
                // one slot per accumulator row; a row no group wrote in this substep (fewer partners than rows: worlds of <= 4 rows) holds
                // nothing.  (Left-over partners of a world without any full group all go to row 0 -- one of them at most with UA = 2.)
                const int nr = Hf >= UA ? UA : (Hf > 0 ? 1 : 0);
                float rx = 0.0f, ry = 0.0f;
                if (nr > 0) { const float2 lo = rr[0]; rx = lo.x; ry = lo.y; }
#pragma unroll
                for (int u = 1; u < UA; ++u)
                    if (u < nr) { const float2 lo = rr[u * AR]; rx += lo.x; ry += lo.y; }
                fsx = ex - rx; fsy = ey - ry;
                STAMP(10);
                if constexpr (SOC == 2) {
                    // Moussaid's k1 / k2 body-contact terms (round 6): exact zeros unless two bodies overlap, left out of the pair loop
                    // (pair_force_moussaid_once<false>) and added here, behind a wave vote, for the rows that touch somebody -- as SOURCES
                    // broadcast from their lane's registers, every lane of the world adding its own term (the Helbing / Guo pass below).
                    // (the one-wavefront pair-once loop runs with equal parameters only: per-agent Moussaid keeps the all-partners loop)
                    // (the vote is taken on the UNREFINED distance d2 * v_rsq(d2), 2.5 ulp off: a tenth of a millimetre of slack -- a pair that is
                    //  not in contact after all adds exact zeros)
                    const bool touches = rdmax > -my_rs - 1.0e-4f;
                    if (CS_RARE(__builtin_amdgcn_ballot_w64(touches) != 0)) {
#ifdef CS_STAMPS
                        st_acc[11] += 1000;
#endif
                        auto bcast = [](float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); };
                        unsigned long long T2 = __builtin_amdgcn_ballot_w64(touches);
                        for (unsigned long long m2 = T2; m2 != 0; m2 &= m2 - 1) {
                            const int sa = __builtin_ctzll(m2);
                            const float ax_ = bcast(px, sa), ay_ = bcast(py, sa), ars = bcast(my_rs, sa);
                            const float dx = px - ax_, dy = py - ay_, lim = my_rs + ars + 1.0e-3f;
                            const bool same = sa >= base && sa < base + rows && sa != tid;
                            T2 |= __builtin_amdgcn_ballot_w64(same && fmaf(dx, dx, dy * dy) < lim * lim);
                        }
                        for (unsigned long long m2 = T2; m2 != 0; m2 &= m2 - 1) {
                            const int sa = __builtin_ctzll(m2);
                            const float qx = bcast(px, sa), qy = bcast(py, sa), qrs = bcast(my_rs, sa);
                            const float qvx = bcast(vx, sa), qvy = bcast(vy, sa);
                            const bool same = sa >= base && sa < base + rows && sa != tid;
                            float tx, ty;
                            moussaid_contact_term(sp, same ? px - qx : 1.0e15f, same ? py - qy : 0.0f, vx - qvx, vy - qvy, my_rs + qrs, tx, ty);
                            fsx += same ? tx : 0.0f;
                            fsy += same ? ty : 0.0f;
                        }
                    }
                }
                if constexpr (SOC != 2) {
                    fsx *= sp.sA; fsy *= sp.sA;
                    if (CS_RARE(__builtin_amdgcn_ballot_w64(rdmax > -my_rs) != 0)) { // contact somewhere in this wavefront
#ifdef CS_STAMPS
                        st_acc[11] += 1000;   // (diagnostic: how often the contact pass runs, per mille of the substeps)
#endif
                        if constexpr (!PP) {
                            // Equal parameters: every term of the all-partners sum below is an exact zero except those of the rows that
                            // touch somebody, so only those rows are gone through -- as SOURCES, broadcast from their lane's registers (the
                            // published position and, here, velocity of a row ARE its lane's registers), every lane of the world adding its
                            // own term from the source in the order of the loop it replaces (increasing row): the same bits, ~25 instructions
                            // per touching row instead of 16 x rows.  The launch waits for the wavefront that takes this path.
                            auto bcast = [](float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); };
                            // S: the lower ends of the overlapping pairs (they saw it in the pair loop); T: S and whoever overlaps one of S
                            unsigned long long T2 = __builtin_amdgcn_ballot_w64(rdmax > -my_rs);
                            for (unsigned long long m2 = T2; m2 != 0; m2 &= m2 - 1) {
                                const int sa = __builtin_ctzll(m2);
                                const float ax_ = bcast(px, sa), ay_ = bcast(py, sa), ars = bcast(my_rs, sa);
                                const float dx = px - ax_, dy = py - ay_, lim = my_rs + ars + 1.0e-3f;
                                const bool same = sa >= base && sa < base + rows && sa != tid;
                                T2 |= __builtin_amdgcn_ballot_w64(same && fmaf(dx, dx, dy * dy) < lim * lim);
                            }
                            for (unsigned long long m2 = T2; m2 != 0; m2 &= m2 - 1) {
                                const int sa = __builtin_ctzll(m2);
                                const float4 q = make_float4(bcast(px, sa), bcast(py, sa), bcast(my_rs, sa), 0.0f);
                                const float2 vj = make_float2(bcast(vx, sa), bcast(vy, sa));
                                const bool same = sa >= base && sa < base + rows && sa != tid;
                                const float dx = px - q.x, dy = py - q.y;
                                const float d2 = fmaf(dx, dx, dy * dy);
                                const float inv = rsq_fast(d2);
                                const float m0 = fmaxf(0.0f, (my_rs + q.z) - dist_refined(d2, inv));
                                const float nx = dx * inv, ny = dy * inv;
                                const float dv = (vj.y - vy) * nx - (vj.x - vx) * ny;     // (v_j - v_i) . t
                                const float fn = sp.k1 * m0, ft = (sp.k2 * m0) * dv;
                                const float tx = fn * nx - ft * ny, ty = fn * ny + ft * nx;
                                fsx += same ? tx : 0.0f;
                                fsy += same ? ty : 0.0f;
                            }
                        } else {
                        const float4* pp = lds_p + cur * TP + pbase;
                        float2* pvel = lds_v + cur * TP + pbase;
                        if constexpr (VEL_ON_DEMAND) {
                            pvel[row] = make_float2(vx, vy); // every lane of the wavefront is here: publish the velocities now
                            LDS_ORDER_FENCE();
                        }
                        // per-agent parameters: my refreshed velocity, partner j < i refreshed, j > i stored (prange == range order)
                        const float vix = PP ? cvx : vx, viy = PP ? cvy : vy;
                        const float2* vr = lds_vr + cur * T + base;
#pragma unroll 8
                        for (int j = 0; j < rows; ++j) { // rare path, but the launch waits for the wavefront that takes it: eight partner rows requested per trip
                            const float4 q = pp[j];
                            float2 vj = pvel[j];
                            if constexpr (PP && HEADED > 0) { if (j < row) vj = vr[j]; }
                            const float dx = px - q.x, dy = py - q.y;
                            const float d2 = (j == row) ? 1.0e30f : fmaf(dx, dx, dy * dy);
                            const float inv = rsq_fast(d2);
                            const float m0 = fmaxf(0.0f, (my_rs + q.z) - dist_refined(d2, inv));
                            const float nx = dx * inv, ny = dy * inv;
                            const float dv = (vj.y - viy) * nx - (vj.x - vix) * ny;     // (v_j - v_i) . t
                            const float fn = sp.k1 * m0, ft = (sp.k2 * m0) * dv;
                            fsx += fn * nx - ft * ny;
                            fsy += fn * ny + ft * nx;
                        }
                        }
                    }
                }
            }
        }
