// sfmstep_sub_part_a.inc -- a fragment of k_sfm_step (sfmstep_kernel.h), included inside the kernel body: part A: what does not depend on this substep's social force -- the wall pairs' pass, refreshed velocity, desired force, the all-lanes wall pass, heading and torque.
// Not a translation unit and not a function: it reads and writes the kernel's locals (the lane's row in registers, the LDS views, the
// template parameters).  The split is textual -- the token stream of the kernel is what it was in one file -- so that each phase can be
// read on its own; sfmstep_kernel.h lists the phases in order.  gfx950 only.
        STAMP(0);
        // -- social force, pair-once form (:87-133).  Lane i evaluates its partners at ring distance 1 .. (rows-1)/2
        //    inside its world (rows even: plus the antipodal one, evaluated by both ends).  The partner's share -f
        //    is added to accumulator slot [k mod UA][i + distance] of UA LDS rows: plain read-modify-write, no
        //    atomics -- one wavefront executes its LDS operations in order, so each of the UA chains is race-free.
        //    Index i + distance runs past the world's rows without a modulo: receiver j sums slots j and j + rows.
        //    Order of a substep: the first group's partner rows are requested from LDS, then everything that does not
        //    depend on this substep's social force is computed while they are in flight (rotation, desired and wall
        //    forces, the Farina torque, the new heading and its sine / cosine), then the partner groups, and only the
        //    short force-dependent tail (body-frame projection, Euler step, publish) follows the reaction sum.
        float fsx = 0.0f, fsy = 0.0f;
        // (the reaction accumulators need no zeroing: the first partner group of a substep stores into them)
        STAMP(8);
        // -- wall pairs: one (agent, polygon) pair per lane and pass, numbered in the prologue (two passes for more than 64 pairs)
        const bool wp_step = wp_on;
        if constexpr (LEAN == 2 && MAXT == 64) {
            if (wp_on && wp_count > 0) {
                {   // every agent's refreshed linear velocity, for the contact terms of a pair whose agent touches its polygon
                    float wvx = vx, wvy = vy;
                    if constexpr (HEADED > 0) { wvx = cs * bvx + (-sn) * bvy; wvy = sn * bvx + cs * bvy; }   // (the statements of part A below)
                    lds_wcv[tid] = make_float2(wvx, wvy);
                }
                LDS_ORDER_FENCE();
                const float4 law = *lds_wlaw;
                for (int k0 = 0; k0 < wp_count; k0 += 64) {                                             // (wave-uniform trip count)
                    const int k = k0 + tid;
                    if (k < wp_count) {
                        const int wr = lds_wrec[k];
                        const float2 wq = lds_wrs[k];
                        const float2 ap = *reinterpret_cast<const float2*>(&lds_p[cur * TP + (wr & 0xFF)]);   // the agent's incoming position
                        const float4* sgp = lds_seg + ((wr >> 8) & 0xFFF);
                        const float* sip = lds_sinv + ((wr >> 8) & 0xFFF);
                        float best = INFINITY, bdx = 0.0f, bdy = 0.0f;
                        // first argmin over the polygon's segments; WP_NW slots per trip, their LDS reads in flight together (a slot per trip
                        // waited for its own read each time)
                        auto wtrip = [&](int s0, auto width) {
                            constexpr int NW = decltype(width)::value;
                            float4 e[NW];
                            float iv[NW];
#pragma unroll
                            for (int j = 0; j < NW; ++j) { e[j] = sgp[s0 + j]; iv[j] = sip[s0 + j]; }
#pragma unroll
                            for (int j = 0; j < NW; ++j) {
                                const float qx = ap.x - e[j].x, qy = ap.y - e[j].y;
                                const float t = fmaf(qx, e[j].z, qy * e[j].w) * iv[j];
                                const float ts = fminf(fmaxf(t, 0.0f), 1.0f);
                                const float ddx = fmaf(-ts, e[j].z, qx), ddy = fmaf(-ts, e[j].w, qy);
                                const float d = fmaf(ddx, ddx, ddy * ddy);
                                const bool better = d < best;
                                best = better ? d : best; bdx = better ? ddx : bdx; bdy = better ? ddy : bdy;
                            }
                        };
                        {
                            int s0 = 0;
                            for (; s0 + WP_NW <= a.Smax; s0 += WP_NW) wtrip(s0, std::integral_constant<int, WP_NW>{});
                            for (; s0 < a.Smax; ++s0) wtrip(s0, std::integral_constant<int, 1>{});
                        }
                        const float bcl = fmaxf(best, 1e-30f);
                        const float inv = rsq_fast(bcl);
                        const float dist = best * inv;
                        const float nx = bdx * inv, ny = bdy * inv;
                        const float rd = wq.x - dist + wq.y;
                        float2 f;
                        if (rd > -1.0e-3f) {   // (rare, lane-divergent) body contact: the k1 / k2 terms on the refined distance and the tangential velocity
                            const float2 cv = lds_wcv[wr >> 20];
                            const float dv = -(cv.y * nx - cv.x * ny);
                            const float m0 = fmaxf(0.0f, wq.x - dist_refined(bcl, inv) + wq.y);
                            const float fn = fmaf(law.x, exp2_fast(rd * law.y), law.z * m0);
                            const float ft = -(law.w * m0) * dv;
                            f = make_float2(fn * nx - ft * ny, fn * ny + ft * nx);
                        } else {
#pragma clang fp contract(off)
                            const float fn = law.x * exp2_fast(rd * law.y);
                            f = make_float2(fn * nx, fn * ny);
                        }
                        lds_wres[k] = f;
                    }
                }
                LDS_ORDER_FENCE();
            }
        }
        // -- part A of the per-agent update: everything that does not need this substep's social force
        const float c = cs, s = sn;          // rotation matrix of the incoming heading, :254-256
        float cvx = vx, cvy = vy;            // refreshed linear velocity
        if constexpr (CARRY_CV) { cvx = cvx_c; cvy = cvy_c; }   // (carried from the previous substep's tail: sfmstep_kernel.h)
        float fdx = 0.0f, fdy = 0.0f, fox = 0.0f, foy = 0.0f;
        float th_n = th, sn_n = sn, cs_n = cs, torque_a = 0.0f;
        if (human) {
            if constexpr (HEADED > 0 && !CARRY_CV) {
                cvx = c * bvx + (-s) * bvy;
                cvy = s * bvx + c * bvy;
            }
            // -- desired force, :23-40
            {
                const float dx = gx - px, dy = gy - py;
                const float d2 = fmaf(dx, dx, dy * dy);
                const float inv = rsq_fast(fmaxf(d2, 1e-30f));
                const float wx = m_tau * (dx * inv * vd - cvx), wy = m_tau * (dy * inv * vd - cvy);
                const bool far_ = d2 * inv > r;   // selects, not a branch: a data-dependent branch costs ~55 cycles of latency
                fdx = far_ ? wx : 0.0f;
                fdy = far_ ? wy : 0.0f;
            }
            // -- obstacle force: closest point per polygon :236-252, then :136-162
            if (obst != nullptr && wp_step) {
                // (wall pairs) my pairs' forces in polygon order -- the reference's order of summation; a polygon beyond my reach left its zero
#pragma clang fp contract(off)
                for (int o = 0; o < a.O; ++o) {
                    const float2 f = lds_wres[(wp_mine >> (8 * o)) & 0xFFu];
                    fox = fox + f.x;
                    foy = foy + f.y;
                }
                fox *= inv_O; foy *= inv_O;
            } else if (obst != nullptr) {
                for (int o = 0; o < a.O; ++o) {
                    // first argmin over the polygon's segments, on squared distances (same order)
                    float best = INFINITY, bdx = 0.0f, bdy = 0.0f;   // the first slot always beats +inf: a first argmin
                    if (a.seg_tab > 0) {
                        {   // nobody of this wavefront within reach of the polygon: its force is < 5e-13 N on everyone, skip it
                            const float4 pc = lds_poly[(sbase / a.Smax) + o];
                            const float dxc = px - pc.x, dyc = py - pc.y, lim = pc.z + wall_cut;
                            if (__builtin_amdgcn_ballot_w64(fmaf(dxc, dxc, dyc * dyc) < lim * lim) == 0) continue;
                        }
                        // branch-free, four slots per trip (then two, then one): the LDS reads of a trip (uniform addresses,
                        // broadcasts) are issued before its arithmetic; a NaN slot is a far-away degenerate segment in the table
                        const float4* sgp = lds_seg + sbase + o * a.Smax;
                        const float* sip = lds_sinv + sbase + o * a.Smax;
                        auto trip = [&](int s0, auto width) {
                            constexpr int NW = decltype(width)::value;
                            float4 e[NW];
                            float iv[NW];
#pragma unroll
                            for (int j = 0; j < NW; ++j) { e[j] = sgp[s0 + j]; iv[j] = sip[s0 + j]; }
#pragma unroll
                            for (int j = 0; j < NW; ++j) {
                                const float qx = px - e[j].x, qy = py - e[j].y;
                                const float t = fmaf(qx, e[j].z, qy * e[j].w) * iv[j];
                                const float ts = fminf(fmaxf(t, 0.0f), 1.0f);
                                const float ddx = fmaf(-ts, e[j].z, qx), ddy = fmaf(-ts, e[j].w, qy);   // p - (a + ts e)
                                const float d = fmaf(ddx, ddx, ddy * ddy);
                                const bool better = d < best;
                                best = better ? d : best;
                                bdx = better ? ddx : bdx;
                                bdy = better ? ddy : bdy;
                            }
                        };
                        int s0 = 0;
                        // polygons of up to six slots (triangles to hexagons) in ONE trip: all their LDS reads are in flight together
                        if (a.Smax == 5) { trip(0, std::integral_constant<int, 5>{}); s0 = 5; }
                        else if (a.Smax == 6) { trip(0, std::integral_constant<int, 6>{}); s0 = 6; }
                        else if (a.Smax == 3) { trip(0, std::integral_constant<int, 3>{}); s0 = 3; }
                        for (; s0 + 4 <= a.Smax; s0 += 4) trip(s0, std::integral_constant<int, 4>{});
                        if (s0 + 2 <= a.Smax) { trip(s0, std::integral_constant<int, 2>{}); s0 += 2; }
                        if (s0 < a.Smax) trip(s0, std::integral_constant<int, 1>{});
                    } else {
                        for (int sg = 0; sg < a.Smax; ++sg) {
                            const float4 seg = *reinterpret_cast<const float4*>(obst + ((long)o * a.Smax + sg) * 4);
                            const float x1 = seg.x, y1 = seg.y, ex = seg.z - seg.x, ey = seg.w - seg.y;
                            float d, ddx = 0.0f, ddy = 0.0f;
                            if (isnan(seg.x)) {
                                d = 3.0e38f; // NaN slot: the reference stores iinfo(int64).max as the distance (:247)
                            } else {
                                const float t = ((px - x1) * ex + (py - y1) * ey) * rcp_fast(fmaf(ex, ex, ey * ey));
                                const float ts = fminf(fmaxf(t, 0.0f), 1.0f);
                                ddx = px - fmaf(ts, ex, x1); ddy = py - fmaf(ts, ey, y1);
                                d = fmaf(ddx, ddx, ddy * ddy);
                            }
                            if (d < best) { best = d; bdx = ddx; bdy = ddy; }
                        }
                    }
                    const float bcl = fmaxf(best, 1e-30f);
                    const float inv = rsq_fast(bcl);
                    const float dist = best * inv;
                    const float nx = bdx * inv, ny = bdy * inv;
                    const float rd = r - dist + safety;
                    // Helbing walls: the body-contact terms (k1, k2; the refined distance, the tangential velocity) are exact zeros
                    // unless somebody overlaps the polygon -- a wave vote, with a millimetre of margin for the unrefined distance; the
                    // short branch leaves the same bits as the long one with m0 = 0 (fn = A e + k1 0, ft = -(k2 0) dv = -+0: the
                    // products rounded once, then the sums).  8192 x 50 + 3 polygons: 221.5 -> 215.5 us
                    if (obs_type != 0 || __builtin_amdgcn_ballot_w64(rd > -1.0e-3f) != 0) {
                        const float dv = -(cvy * nx - cvx * ny);                 // -(v . t), t = (-ny, nx)
                        const float m0 = fmaxf(0.0f, r - dist_refined(bcl, inv) + safety);
                        const float fn = fmaf(Aw, exp2_fast(rd * cBw), k1 * m0);
                        float ft;                                                 // coefficient of t
                        if (obs_type == 0) ft = -(k2 * m0) * dv;
                        else ft = (-Cw * exp2_fast(rd * cDw) - k2 * m0) * dv;
                        fox += fn * nx - ft * ny;
                        foy += fn * ny + ft * nx;
                    } else {
#pragma clang fp contract(off)
                        const float fn = Aw * exp2_fast(rd * cBw);
                        const float tx = fn * nx, ty = fn * ny;   // (not contracted into the sums: the long branch rounds the products too)
                        fox = fox + tx;
                        foy = foy + ty;
                    }
                }
                fox *= inv_O; foy *= inv_O;
            }
            if constexpr (HEADED > 0) {
                th_n = wrap_angle(fmaf(om, dt, th));   // :278; the new heading needs omega of the incoming row only
                sincos_fast(th_n, sn_n, cs_n);
            }
            if constexpr (HEADED == 1) {               // Farina: the torque follows the desired force alone, :165-182
                const float kf = klam * norm2(fdx, fdy);
                const float k_theta = inertia * kf;
                const float k_omega = inertia * (1.0f + alpha) * sqrt_fast(kf * inv_alpha);
                const float delta = atan2_fast(s * fdx - c * fdy, c * fdx + s * fdy);
                torque_a = -k_theta * delta - k_omega * om;
            }
        }
