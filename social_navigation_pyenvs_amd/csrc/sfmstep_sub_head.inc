// sfmstep_sub_head.inc -- a fragment of k_sfm_step (sfmstep_kernel.h), included inside the kernel body: head of a substep: priority turn, recorders (imitation snapshot, cs_step_trace), the robot under its own motion model (LEAN = 4), partner-row fetch helpers, the goal switch.
// Not a translation unit and not a function: it reads and writes the kernel's locals (the lane's row in registers, the LDS views, the
// template parameters).  The split is textual -- the token stream of the kernel is what it was in one file -- so that each phase can be
// read on its own; sfmstep_kernel.h lists the phases in order.  gfx950 only.
        // (prio_young is a scalar, sfmstep_kernel.h, where the test of a vector vblock opened an exec region in every substep.  As compiled in the
        //  headline build the turn sits in front of the loop's head: the older wavefront of a SIMD takes the back edge straight to the head
        //  -- its priority test IS the back edge --, the younger falls out of it, jumps to the turn and falls into the head.  The turn as
        //  "1, then 2 on an odd substep": one branch inside it instead of two around its two arms; priorities as before, 2 / 1 on odd / even.)
        if constexpr (MAXT == 64) { if (CS_RARE(prio_young)) { __builtin_amdgcn_s_setprio(1); if (sub & 1) __builtin_amdgcn_s_setprio(2); } }
        const int nxt = cur ^ 1;
        STAMP(7);
        if (CS_RARE(a.snap != nullptr || a.trace != nullptr)) {   // (one scalar branch for both recorders: neither is on in a plain cs_step)
            // imitation block: what the robot's own integrator sees of the crowd at this substep (it runs before update_humans)
            if (a.snap != nullptr && human) a.snap[((long)sub * a.W + w) * n + row] = make_float4(px, py, vx, vy);
            // cs_step_trace: my row as the previous substep left it (the last one is written behind the loop)
            if (a.trace != nullptr && (human || is_robot) && sub > 0)
                write_trace(a.trace + (((long)(sub - 1) * a.W + w) * rows + row) * 12, px, py, th, vx, vy, bvx, bvy, om, gx, gy, g0x, g0y);
        }
        const int Hf = (rows - 1) >> 1;
        const float4* rp = XY_ROWS ? nullptr : lds_p + cur * TP + pbase + row + 1;   // rp[k]: partner at ring distance k + 1 (XY_ROWS builds: rxy below)
        const float2* rv = lds_v + cur * TP + pbase + row + 1;
        const float2* rxy = lds_xy + cur * TP + pbase + row + 1;   // (XY_ROWS) the 8-byte rows: rxy[k] partner at ring distance k + 1
        const float4* rpp = lds_pp + pbase + row + 1;            // (PP) ... and its parameter row
        float4 qa[UA], pa[PP ? UA : 1];
        float2 va[UA];
        auto fetch_pp = [&](float4 (&pq)[PP ? UA : 1], int kk) {
            if constexpr (PP) {
#pragma unroll
                for (int u = 0; u < UA; ++u) {
                    if constexpr (ROWS_CT > 0) pq[u] = ppj[kk + u];   // (kk is a compile-time constant at every call of these builds)
                    else pq[u] = rpp[kk + u];
                }
            }
        };
        auto fetch = [&](float4 (&q)[UA], float2 (&vq)[UA], int kk) {
#pragma unroll
            for (int u = 0; u < UA; ++u) {
                if constexpr (XY_ROWS) {
                    const float2 xy = rxy[kk + u];
                    q[u] = make_float4(xy.x, xy.y, rsj[kk + u], 0.0f);
                } else if constexpr (ROWS_CT > 0 && N3L) {   // (kk is a compile-time constant at every call of these builds)
                    const float2 xy = *reinterpret_cast<const float2*>(&rp[kk + u]);
                    q[u] = make_float4(xy.x, xy.y, rsj[kk + u], PP ? sacj[kk + u] : 0.0f);
                } else {
                    q[u] = rp[kk + u];
                }
                if constexpr (N3L && SOC == 2) vq[u] = rv[kk + u]; else vq[u] = make_float2(0.0f, 0.0f);
            }
        };
        if constexpr (IMIT) {
            // -- update_robot(t, dt) (motion_model_manager.py:615-629) BEFORE update_humans: the robot's model sees the humans as they
            //    stand, the crowd then sees the moved robot (its row is re-published into THIS substep's buffer).  Same operations,
            //    same order as k_robot_model_step (robot_model.h): the fused launch equals the alternating launches bit for bit.
            const int rsoc = a.rm_type % 3;
            const bool rheaded = a.rm_type >= 3;
            float rsn = 0.0f, rcs = 1.0f;
            rmodel::RState rs;
            if (is_robot) {
                rs.px = px; rs.py = py; rs.yaw = th; rs.vx = vx; rs.vy = vy; rs.bvx = bvx; rs.bvy = bvy; rs.om = om;
                rs.radius = r; rs.mass = m; rs.gx = gx; rs.gy = gy; rs.vd = vd; rs.fdx = rm_fdx; rs.fdy = rm_fdy;
                rmodel::refresh_velocity(rs, rheaded, rsn, rcs);
                lds_rob[2 * lw] = make_float4(rs.px, rs.py, rs.vx, rs.vy);
                lds_rob[2 * lw + 1] = make_float4(r + a.rm_margin, 0.0f, 0.0f, 0.0f);   // (the region is the prologue's scratch: rewritten here)
            }
            LDS_ORDER_FENCE();
            if (human) {
                const float4 rq = lds_rob[2 * lw];
                const float rme = lds_rob[2 * lw + 1].x;
                float tx, ty;
                rmodel::pair_term(rsoc, a.rm_P, rq.x, rq.y, rq.z, rq.w, px, py, vx, vy, rme + r + rm_hm, tx, ty);
                lds_rf[tid] = make_float2(tx, ty);
            }
            LDS_ORDER_FENCE();
            if (is_robot) {
                float sx = 0.0f, sy = 0.0f;
                const float2* tf = lds_rf + base;
#pragma unroll 8
                for (int j = 0; j < n; ++j) { const float2 t = tf[j]; sx += t.x; sy += t.y; }   // (eight terms requested per trip; summed in index order)
                rmodel::integrate(rs, a.rm_type, a.rm_P, sx, sy, 0.0f, 0.0f, rsn, rcs, dt, 0);
                px = rs.px; py = rs.py; th = rs.yaw; vx = rs.vx; vy = rs.vy; bvx = rs.bvx; bvy = rs.bvy; om = rs.om;
                rm_fdx = rs.fdx; rm_fdy = rs.fdy;
                publish(cur);
                publish_v(cur);
            }
            LDS_ORDER_FENCE();
        }
        // lean build without walls: request the first group's partner rows first thing; the goal test and part A below run
        // while they are in flight.  With walls the rows would be held in registers across the segment loops (17 spilled VGPRs
        // in the 50-row build at the three-wave budget), so they are fetched at the head of the group loop instead (fetching
        // between the segment loops and the heading / torque arithmetic spills as well); worth 1 % on the 8192 x 50 shard
        if constexpr (LEAN && NO_WALLS) { if (valid && Hf >= UA) fetch(qa, va, 0); }
        // even row counts: the antipodal partner (evaluated by both ends, no hand-over) is requested up front as well
        float4 qz = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float2 vz = make_float2(0.0f, 0.0f);
        if constexpr (LEAN && NO_WALLS) {
            if (valid && (rows & 1) == 0) {
                if constexpr (XY_ROWS) { const float2 xy = rxy[(ROWS_CT - 1) / 2]; qz = make_float4(xy.x, xy.y, rsj[(ROWS_CT - 1) / 2], 0.0f); }
                else if constexpr (ROWS_CT > 0 && N3L) { const float2 xy = *reinterpret_cast<const float2*>(&rp[(ROWS_CT - 1) / 2]); qz = make_float4(xy.x, xy.y, rsj[(ROWS_CT - 1) / 2], 0.0f); }
                else qz = rp[Hf];
                if constexpr (SOC == 2) vz = rv[Hf];
            }
        }
        if constexpr (LEAN) {
            // -- goal switch, forces_parallel.py:226-234, predicated: lists of <= 2 goals rotate in registers.  In the plain one-wavefront
            //    builds (VOTED_SWITCH, sfmstep_kernel.h) behind one scalar branch on the vote the previous substep's tail took on this
            //    very row: a wavefront none of whose lanes stands within r of its goal -- the common case -- skips the block.
            if (!VOTED_SWITCH || CS_RARE(carried_hit != 0ull)) {
                const float gdx = g0x - px, gdy = g0y - py;
                const bool hit = human && fmaf(gdx, gdx, gdy * gdy) <= r * r;
                const bool sw = hit && gk == 2;
                const float t0 = g0x, t1 = g0y;
                g0x = sw ? g1x : g0x; g0y = sw ? g1y : g0y;
                g1x = sw ? t0 : g1x; g1y = sw ? t1 : g1y;
                if constexpr (VOTED_SWITCH) gdirty_votes |= __builtin_amdgcn_ballot_w64(sw);   // (a scalar pair: a lane mask carried round a uniform branch costs four scalar instructions on the path around it)
                else gdirty = gdirty || sw;
                gx = hit ? g0x : gx; gy = hit ? g0y : gy;
            }
        } else if (human) {
            // -- goal switch, forces_parallel.py:226-234 (on the incoming position)
            const float gdx = g0x - px, gdy = g0y - py;
            if (fmaf(gdx, gdx, gdy * gdy) <= r * r) { // |goals[i][0] - p| <= r ; rare, divergent
                const int k = gk;
                if (k <= 2) {                       // rotation of a list of 0, 1 or 2 goals: registers only
                    if (k == 2) {
                        const float t0 = g0x, t1 = g0y;
                        g0x = g1x; g0y = g1y; g1x = t0; g1y = t1;
                        gdirty = true;
                    }
                } else if (kmode & M_COMMIT_GOALS) {
                    const float r0 = gi[0], r1 = gi[1];
                    for (int g = 0; g + 1 < k; ++g) { gi[2 * g] = gi[2 * g + 2]; gi[2 * g + 1] = gi[2 * g + 3]; }
                    if (k > 0) { gi[2 * (k - 1)] = r0; gi[2 * (k - 1) + 1] = r1; }
                    g0x = gi[0]; g0y = gi[1];
                } else if (k > 1) {
                    g0x = gi[2]; g0y = gi[3];
                }
                gx = g0x; gy = g0y;
            }
        }
