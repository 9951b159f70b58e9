// sfmstep_sub_tail.inc -- a fragment of k_sfm_step (sfmstep_kernel.h), included inside the kernel body: all partners per lane (per-agent parameters on Moussaid, worlds of more than one wavefront), part B: total force, body frame, torque, the Euler step, the rows published for the next substep.
// Not a translation unit and not a function: it reads and writes the kernel's locals (the lane's row in registers, the LDS views, the
// template parameters).  The split is textual -- the token stream of the kernel is what it was in one file -- so that each phase can be
// read on its own; sfmstep_kernel.h lists the phases in order.  gfx950 only.
        STAMP(2);
        if (human) {
            // -- social force, every lane evaluates all its partners: O(N) rows broadcast from LDS, :43-84
            if constexpr (!N3L) {
                // all_params_equal: every row's stored velocity (the reference evaluates all pairs
                // before any in-place refresh); else: my refreshed velocity, partner j<i refreshed,
                // j>i stored (prange == range order; identical from the 2nd fused substep on)
                const float vix = PEQ ? vx : cvx, viy = PEQ ? vy : cvy;
                const float4* pp = lds_p + cur * TP + pbase;
                const float2* pvel = lds_v + cur * TP + pbase;
                const float2* vr = lds_vr + cur * T + base;
                auto partner_vel = [&](int j) {
                    float2 v2 = pvel[j];
                    if constexpr (!PEQ && HEADED > 0) { if (j < row) v2 = vr[j]; }
                    return v2;
                };
                if constexpr (SOC == 2) {
                    for (int j = 0; j < rows; ++j) {
                        const float4 q = pp[j];
                        const float2 vj = partner_vel(j);
                        pair_force_moussaid(sp, px, py, vix, viy, q.x, q.y, vj.x, vj.y, my_rs + q.z, j == row, fsx, fsy);
                    }
                } else {
                    // Helbing / Guo (:117-118).  Per partner the force is
                    //   [A e^{rd/B} + k1 max(0,rd)] n + [C e^{rd/D} + k2 max(0,rd) dv] t      (C = 0: Helbing)
                    // Main loop: the exponential parts for every partner, branch-free (one ds_read_b128,
                    // ~13 VALU + 2 transcendental ops each; A and C folded into the exponent; the next group
                    // of four is fetched from LDS while the current one is evaluated).  The k1 / k2 contact
                    // parts are exact zeros unless rd > 0: they are added by a second pass that a wavefront
                    // runs only when one of its lanes touched a partner in this substep.
                    float eax = 0.0f, eay = 0.0f, ecx = 0.0f, ecy = 0.0f, rdmax = -1.0e30f;   // max over the partners of rs_j - dist
                    constexpr int U = 8;                  // partners in flight per lane (independent rsq -> exp chains)
                    const float4* rp = pp + row + 1;      // partner k of mine = row (i + 1 + k) mod rows, k = 0 .. rows-2
                    const int np = rows - 1;
                    auto group = [&](const float4 (&q)[U], int rem, auto tail_tag) {
                        constexpr bool TAIL = decltype(tail_tag)::value;
                        float rdk[U];
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            const float dx = px - q[u].x, dy = py - q[u].y;
                            float d2 = fmaf(dx, dx, dy * dy);
                            if constexpr (TAIL) d2 = (u >= rem) ? 1.0e30f : d2; // padding slot (wave-uniform): dist 1e15 -> 0
                            const float inv = rsq_fast(d2);
                            const float rd = fmaf(-d2, inv, q[u].z);                  // rs_j - dist: my own rs sits in the exponent offsets (lAi, lCi)
                            const float ga = exp2_fast(fmaf(rd, sp.cB, lAi)) * inv;   // |A| e^{(rij - dist)/B} / dist
                            eax = fmaf(ga, dx, eax); eay = fmaf(ga, dy, eay);
                            if constexpr (SOC == 1) {
                                const float gc = exp2_fast(fmaf(rd, sp.cD, lCi)) * inv;   // |C| e^{(rij - dist)/D} / dist
                                ecx = fmaf(-gc, dy, ecx); ecy = fmaf(gc, dx, ecy);       // along t = (-ny, nx)
                            }
                            rdk[u] = rd;
                        }
#pragma unroll
                        for (int u = 0; u < U; u += 2) rdmax = fmaxf(fmaxf(rdmax, rdk[u]), rdk[u + 1]); // v_max3_f32
                    };
                    auto run = [&](const float4 (&q)[U], int rem) {
                        if (rem >= U) group(q, U, std::false_type{});
                        else group(q, rem, std::true_type{});
                    };
                    // two register sets, filled alternately: the next group's LDS reads are in flight
                    // while the current one is evaluated (no copies, no re-load at the point of use)
                    float4 qa[U], qb[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) qa[u] = rp[u];
                    for (int k0 = 0; k0 < np; k0 += 2 * U) {
                        if (k0 + U < np) {
#pragma unroll
                            for (int u = 0; u < U; ++u) qb[u] = rp[k0 + U + u]; // rows past np are finite padding
                        }
                        asm volatile("" ::: "memory");
                        run(qa, np - k0);
                        if (k0 + U >= np) break;
                        if (k0 + 2 * U < np) {
#pragma unroll
                            for (int u = 0; u < U; ++u) qa[u] = rp[k0 + 2 * U + u];
                        }
                        asm volatile("" ::: "memory");
                        run(qb, np - k0 - U);
                    }
                    fsx = sp.sA * eax; fsy = sp.sA * eay;
                    if constexpr (SOC == 1) { fsx = fmaf(sp.sC, ecx, fsx); fsy = fmaf(sp.sC, ecy, fsy); }
                    if (CS_RARE(__builtin_amdgcn_ballot_w64(rdmax > -my_rs) != 0)) { // contact somewhere in this wavefront
                        for (int j = 0; j < rows; ++j) {
                            const float4 q = pp[j];
                            const float2 vj = partner_vel(j);
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
            STAMP(6);
            // -- part B: total force, body frame, torque  :262-271, :165-182
            // (no-walls builds: fo = 0 is a compile-time fact, and x + 0 is not an identity the compiler may drop)
            const float fix = NO_WALLS ? fdx + fsx : fdx + fox + fsx, fiy = NO_WALLS ? fdy + fsy : fdy + foy + fsy;
            const float fpx = NO_WALLS ? fsx : fox + fsx, fpy = NO_WALLS ? fsy : foy + fsy;   // what acts across the heading: fo + fs
            float gfx = fix, gfy = fiy, torque = torque_a;
            if constexpr (HEADED > 0) {
                if constexpr (HEADED == 2) {  // torque on the total force
                    const float kf = klam * norm2(fix, fiy);
                    const float k_theta = inertia * kf;
                    const float k_omega = inertia * (1.0f + alpha) * sqrt_fast(kf * inv_alpha);
                    // bound_angle(theta - atan2(Fy, Fx)) is the signed angle from F to the heading:
                    // atan2(|F| sin(theta - phi), |F| cos(theta - phi)) -- one atan2, no wrap needed
                    const float delta = atan2_fast(s * fix - c * fiy, c * fix + s * fiy);
                    torque = -k_theta * delta - k_omega * om;
                }
                gfx = fix * c + fiy * s;
                gfy = ko * (fpx * (-s) + fpy * c) - kd * bvy;
            }
            // -- explicit Euler, :273-283 (position uses the velocity stored in the incoming row)
            const float in_vx = cvx, in_vy = cvy; // what the reference leaves in agents_state[i,3:5]
            px += vx * dt; py += vy * dt;
            if constexpr (EARLY_VOTES) {
                // the row this tail stores against the goals[0] of behind the switch: what the respawn rule tests behind this tail and the
                // goal switch at the next head, voted on here -- the rest of the tail away from the first branch, a back edge from the other
                const float ndx = g0x - px, ndy = g0y - py;
                const float nd2 = fmaf(ndx, ndx, ndy * ndy);
                hit_next = __builtin_amdgcn_ballot_w64(nd2 <= r * r);
                flag_any = (__builtin_amdgcn_ballot_w64(nd2 < 9.0f) & respawn_mask) != 0ull;
            }
            if constexpr (HEADED > 0) {
                th = th_n;
                bvx = fmaf(gfx, dt_m, bvx); bvy = fmaf(gfy, dt_m, bvy);
                const float nb2 = fmaf(bvx, bvx, bvy * bvy);
                const float ninv = rsq_fast(fmaxf(nb2, 1e-30f));
                if (nb2 * ninv > vd) { const float sc = vd * ninv; bvx *= sc; bvy *= sc; }
                om = fmaf(torque, dt_inertia, om);
                sn = sn_n; cs = cs_n;
                if constexpr (CARRY_CV) {
                    // The stored velocity and the next substep's refreshed velocity are the same expression of the same operands, but not
                    // the same bits: the compiler contracts a b + c d into fma(a, b, c d) or fma(c, d, a b) as it sees fit, and chose
                    // differently for the y component here and in part A.  Both are written out as it chose them (the bits of every build
                    // so far), so x is carried and y costs one multiply and one FMA instead of two of each.
                    vx = fmaf(cs, bvx, -(sn * bvy));
                    vy = fmaf(sn, bvx, cs * bvy);
                    cvx_c = vx; cvy_c = fmaf(cs, bvy, sn * bvx);
                } else {
                vx = cs * bvx + (-sn) * bvy;
                vy = sn * bvx + cs * bvy;
                }
            } else {
                vx = fmaf(gfx, dt_m, vx); vy = fmaf(gfy, dt_m, vy);
                const float nb2 = fmaf(vx, vx, vy * vy);
                const float ninv = rsq_fast(fmaxf(nb2, 1e-30f));
                if (nb2 * ninv > vd) { const float sc = vd * ninv; vx *= sc; vy *= sc; }
            }
            if ((kmode & M_MUTATE_INPUT) && sub == 0) {
                float* si = a.Sin + sidx * a.in_as;
                if (HEADED > 0) { si[3 * a.in_fs] = in_vx; si[4 * a.in_fs] = in_vy; }
                si[10 * a.in_fs] = gx; si[11 * a.in_fs] = gy;
            }
            publish(nxt);
            publish_v(nxt);
            if constexpr (!PEQ && HEADED > 0) lds_vr[nxt * T + tid] = make_float2(vx, vy);
            STAMP(3);
        } else if (is_robot) {
            // the robot's move of the NEXT substep happens before that substep's update_humans
            if (robot_moves && sub + 1 < a.nsub) robot_step();
            publish(nxt);
            publish_v(nxt);
            if constexpr (!PEQ && HEADED > 0) lds_vr[nxt * T + tid] = make_float2(vx, vy);
        }
        // block of one wavefront: its LDS operations execute in order, program order is all the next substep needs
        // (no s_waitcnt lgkmcnt(0) + s_barrier on the published rows)
        if constexpr (MAXT == 64) LDS_ORDER_FENCE(); else __syncthreads();
