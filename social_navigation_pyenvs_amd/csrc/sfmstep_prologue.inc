// sfmstep_prologue.inc -- a fragment of k_sfm_step (sfmstep_kernel.h), included inside the kernel body: the prologue: per-launch constants, wall segments and polygon circles staged in LDS, the Gym step's head (cs_gym_step), substep-0 rows published, the (agent, polygon) pairs of the wall pass numbered (LEAN = 2).
// Not a translation unit and not a function: it reads and writes the kernel's locals (the lane's row in registers, the LDS views, the
// template parameters).  The split is textual -- the token stream of the kernel is what it was in one file -- so that each phase can be
// read on its own; sfmstep_kernel.h lists the phases in order.  gfx950 only.
#ifdef CS_STAMPS
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(pst_loaded)::"memory");   // every load of the load phase has returned
#endif
    // ---- compute phase --------------------------------------------------------------------
    if (!valid) {   // (selects: what the rows of a lane without a world have always been)
        px = 0; py = 0; th = 0; vx = 0; vy = 0; bvx = 0; bvy = 0; om = 0; r = 0; m = 1; gx = 0; gy = 0; vd = 0;
        safety = 0; ax = 0; ay = 0;
    }
    if (!robot_moves) { ax = 0; ay = 0; }
    // (D: the default of a value that only lanes with a human read -- the substep loop's one exec region, the epilogue's `human &&`
    //  stores.  LAUNCH_TRIM builds leave it unspecified: as a constant it is a v_mov per value on every launch for lanes that never read it)
#define D(v) unread_default<LAUNCH_TRIM>(v)
    float m_tau = D(0.0f), Aw = D(0.0f), cBw = D(0.0f), Cw = D(0.0f), cDw = D(0.0f), k1 = D(0.0f), k2 = D(0.0f), ko = D(0.0f), kd = D(0.0f), alpha = D(1.0f), klam = D(0.0f);
    float dt_m = D(0.0f), inv_alpha = D(1.0f), inertia = D(1.0f), dt_inertia = D(0.0f), wall_cut = D(0.0f);
    SocP sp = socp_unread_default<LAUNCH_TRIM>();
    float g0x = gx, g0y = gy, g1x = 0, g1y = 0;
    int gk = 0;          // length of the non-NaN prefix of my goal list
    bool gdirty = false; // a two-goal list rotated in registers, to be written back in the epilogue
    if (N3L && PEQ && valid) sp = make_socp(sraw);
    if (human) {
        m_tau = m / Pm[0];                      // m / relax_t              (:39)
        Aw = Pm[1]; cBw = LOG2E / Pm[2]; Cw = Pm[3]; cDw = LOG2E / Pm[4]; k1 = Pm[5]; k2 = Pm[6];
        // beyond this distance a wall's force on me is below |A| e^-wall_efolds (22: 5.6e-7 N, crowdstep.hip; its contact terms are exact zeros there):
        // a polygon that every agent of the wavefront is that far from is skipped in the substep loop
        wall_cut = r + safety + a.wall_efolds * fmaxf(Pm[2], obs_type == 1 ? Pm[4] : 0.0f);
        ko = Pm[7]; kd = Pm[8]; alpha = Pm[9]; klam = Pm[10];
        dt_m = a.dt / m;                        // (F / m) * dt             (:277,:282)
        inv_alpha = 1.0f / alpha;
        inertia = 0.5f * m * r * r;             // :265
        dt_inertia = a.dt / inertia;            // (torque / I) * dt        (:279)
        if constexpr (!N3L || PP) sp = make_socp(sraw);
        g0x = gl[0]; g0y = gl[1];
        // goal lists of <= 2 entries (every Gym scenario) rotate in registers; longer ones go through memory
        gk = a.G;
        for (int g = a.G - 1; g >= 2; --g)
            if (isnan(gi[2 * g]) || isnan(gi[2 * g + 1])) gk = g;
        if (a.G >= 2 && (isnan(gl[2]) || isnan(gl[3]))) gk = 1;
        if (isnan(gl[0]) || isnan(gl[1])) gk = 0;
        if (gk == 2) { g1x = gl[2]; g1y = gl[3]; }
    }
    const bool respawn_here = valid && (!has_wflags || (wflag_raw & 1));

    auto robot_step = [&]() { // robot_agent.py:114-136
        if (a.flags & CS_ROBOT_UNICYCLE) {
            float c, s;
            sincos_fast(th + ay, s, c);
            px += c * ax * dt; py += s * ax * dt;
            th = mod_two_pi(th + ay);
            sincos_fast(th, s, c);
            vx = c * ax; vy = s * ax;
        } else {
            px += ax * dt; py += ay * dt; vx = ax; vy = ay;
        }
    };

    float cs = 1.0f, sn = 0.0f; // cos / sin of my theta, carried from one substep to the next

    // imitation learning (LEAN = 4): the robot lane integrates the robot's own motion model; the humans' lanes each hand it their
    // term of its social force.  LDS (aliases of regions this build does not use): per world [state (x, y, vx, vy)] [radius + margin],
    // and one float2 slot per lane for the terms.
    float4* lds_rob = reinterpret_cast<float4*>(lds_vr);
    float2* lds_rf = reinterpret_cast<float2*>(lds_g0x);

    // ---- cs_gym_step_policy (POLICY builds): the robot's no-train policy, decided HERE from the rows as they came in -- the robot columns of
    //      the load phase (d_robot: what cs_policy_no_train reads) and the humans' rows in their lanes (px, py, vx, vy, r: the columns the
    //      observation rows cs_policy_no_train reads were written from; DESIGN.md 4.3) -- so that the head below, the swept test and the
    //      robot's advance consume it as they consume an action row.  Every lane of a world ends up with its world's action; the lane of
    //      row 0 leaves it in the action buffer (one 8-byte store).  policy_no_train.h states the policies; the sum over humans is its
    //      world_sum: k_policy_no_train's butterfly, world by world.  The policy id is a kernel argument: wave-uniform branches.
    if constexpr (POLICY) {
        const float qx = hrb[0], qy = hrb[1], qr = hrb[2], qgx = hrb[3], qgy = hrb[4], qvx = prb[0], qvy = prb[1], qvd = prb[2];
        float dax = 0.0f, day = 0.0f;
        if (a.pnt_policy == CS_PNT_BP) pnt::toward_goal(qx, qy, qgx, qgy, qvd, dax, day);
        else if (a.pnt_policy == CS_PNT_SSP) {
            const bool near = human && pnt::ssp_near(px, py, r, qx, qy, qr);
            const unsigned long long mine = (rows >= 64 ? ~0ull : ((1ull << rows) - 1ull)) << base;   // the lanes of my world
            if ((__builtin_amdgcn_ballot_w64(near) & mine) == 0ull) pnt::toward_goal(qx, qy, qgx, qgy, qvd, dax, day);
        } else {
            float tx = 0.0f, ty = 0.0f;
            if (human) {
                float ux, uy;
                rmodel::pair_term(a.pnt_policy - CS_PNT_SFM_HELBING, a.pnt_P, qx, qy, qvx, qvy, px, py, vx, vy, qr + r, ux, uy);
                pnt::add_term(tx, ty, ux, uy);
            }
            const float fx = pnt::world_sum(tx, tid, lw, rows, n, a.wpb), fy = pnt::world_sum(ty, tid, lw, rows, n, a.wpb);
            pnt::sfm_decide(a.pnt_P[0], a.pnt_mass, a.pnt_time_step, qx, qy, qvx, qvy, qr, qgx, qgy, qvd, fx, fy, dax, day);
        }
        ax = valid ? dax : 0.0f; ay = valid ? day : 0.0f;
        hact[0] = ax; hact[1] = ay;
        if (valid && row == 0) *reinterpret_cast<float2*>(a.pnt_action + (long)w * 2) = make_float2(ax, ay);
    }
    // ---- cs_gym_step: the head of the Gym step, on the rows as they came in (social_nav_gym.py:229-233) -- the swept robot-human
    //      distances by the humans' lanes, then the lane of row 0 walks its world's in index order and does the episode bookkeeping
    //      (gymhead.h: the very code of k_collision_reward_wave).  One scalar branch in a plain cs_step.
    if constexpr (MAXT == 64) {
        if (CS_RARE_HEAD(a.gym.out != nullptr)) {
            float* clo = lds_g0x;                              // [T] (the block-respawn scratch: unused by a block of one wavefront)
            const float rpx = hrb[0], rpy = hrb[1], rr = hrb[2], rgx = hrb[3], rgy = hrb[4];   // (loaded at the top)
            float gax = hact[0], gay = hact[1];
            gym_action_velocity(a.gym.unicycle, hrb[5], gax, gay);   // (a uniform branch: an ActionRot's velocity from the yaw BEFORE the move)
            clo[tid] = human ? gym_swept_closest(px, py, vx, vy, r, rpx, rpy, rr, gax, gay, a.gym.T) : INFINITY;
            LDS_ORDER_FENCE();
            int head_code = 0;                                 // (FOLD) what the head decided for its world: 0 keep stepping, 1 deferred, 2 + slot: take that slot over
            if (valid && row == 0) {
                const bool take = gym_head_world(a.gym, w, n, clo + base, rpx, rpy, rr, rgx, rgy, gax, gay, hpre);
                if constexpr (FOLD) { if (a.gym.fold.on) head_code = gym_fold_decide(a.gym, w, take, take && !((a.gym.bk.mode == 2 && hpre.prev) || hpre.pending), hpre); }
            }
            LDS_ORDER_FENCE();
            if constexpr (FOLD) {
                // every lane of the world learns the code from the head's lane (row 0 = lane `base`) through the LDS crossbar -- read back from
                // pending[w] in the epilogue it was a dependent global round trip at the end of every Gym launch (2 us of its 6)
                fold_code_world = __builtin_amdgcn_ds_bpermute(base << 2, head_code);
            }
        }
    }
    // invisible robot (it does not interact with the crowd): the lane of row 0 advances it over the launch's substeps from the columns the load
    // phase brought (the head above has the state BEFORE the move in its own registers) and stores it at once -- a world that takes a staged
    // episode over at the end of the launch overwrites the row behind this store (same wavefront, same address: program order)
    if (CS_RARE(robot_moves && a.robot != nullptr) && moves_invisible_robot) {   // (the wave-uniform half first: a launch without a robot branches once)
        float* rb = a.robot + (long)w * 13;
        float qx = irb[0], qy = irb[1], qt = irb[2], qvx = irb[3], qvy = irb[4];
        if (a.flags & CS_ROBOT_UNICYCLE) {
            for (int sub = 0; sub < a.nsub; ++sub) {
                const float c = cosf(qt + ay), s = sinf(qt + ay);
                qx += c * ax * dt; qy += s * ax * dt;
                qt = mod_two_pi(qt + ay);
                qvx = cosf(qt) * ax; qvy = sinf(qt) * ax;
            }
        } else if (a.nsub > 0) {
            // holonomic: the substeps' sums one after the other (the reference's float accumulation, one fused multiply-add each as before) without
            // the flag test and the loop's bookkeeping between them: the chain of 2 x nsub dependent operations is what is left
#pragma unroll 4
            for (int sub = 0; sub < a.nsub; ++sub) { qx = fmaf(ax, dt, qx); qy = fmaf(ay, dt, qy); }
            qvx = ax; qvy = ay;
        }
        rb[0] = qx; rb[1] = qy; rb[2] = qt; rb[3] = qvx; rb[4] = qvy;
    }

    // ---- prologue: publish substep-0 rows ----------------------------------------------
    if (is_robot && robot_moves) robot_step();
    const float my_rs = r + safety;
    // Helbing / Guo exponents with MY radius + safety space folded into the offset: (r_ij - d) cB + lA = (rs_j - d) cB + (lA + rs_i cB),
    // one add less per pair; the contact test rd > 0 becomes max(rs_j - d) > -rs_i
    float lAi = 0.0f, lCi = 0.0f;
    // (XY_ROWS builds: no zeroing pass.  Nothing there reads a row that was not published: every LDS read of the substep loop and of the
    // rsj[] fill sits inside `if (valid)`, and a valid lane reads the rows pbase + row + 1 + k, k <= (rows - 1) / 2, of the position
    // (Moussaid: and velocity) buffer -- below pbase + 2 rows, the two copies its own world's lanes publish before the first read -- and
    // the rows base .. base + rows - 1 of lds_rs; the padding behind the buffers is never touched.)
    if constexpr (!XY_ROWS)
    for (int i = tid; i < 2 * TP; i += T) { // padding stays finite
        lds_p[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        lds_v[i] = make_float2(0.0f, 0.0f);
    }
    if constexpr (PP)
        for (int i = tid; i < TP; i += T) lds_pp[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if constexpr (MAXT == 64) LDS_ORDER_FENCE(); else __syncthreads();   // (a one-wavefront block: its LDS operations execute in order; the wavefronts of a workgroup share nothing)
    // bounding circle of every staged polygon (centre = mean of its segments' midpoints, radius = farthest endpoint)
    for (int q = tid; q < (NO_WALLS || a.Smax <= 0 ? 0 : a.seg_tab / a.Smax); q += T) {
        float cx = 0.0f, cy = 0.0f, cnt = 0.0f;
        for (int sg = 0; sg < a.Smax; ++sg) {
            const float4 e = lds_seg[q * a.Smax + sg];
            if (lds_sinv[q * a.Smax + sg] > 0.0f) { cx += e.x + 0.5f * e.z; cy += e.y + 0.5f * e.w; cnt += 1.0f; }
        }
        const float ic = cnt > 0.0f ? 1.0f / cnt : 0.0f;
        cx *= ic; cy *= ic;
        float r2 = 0.0f;
        for (int sg = 0; sg < a.Smax; ++sg) {
            const float4 e = lds_seg[q * a.Smax + sg];
            if (lds_sinv[q * a.Smax + sg] > 0.0f) {
                const float ax0 = e.x - cx, ay0 = e.y - cy, bx0 = ax0 + e.z, by0 = ay0 + e.w;
                r2 = fmaxf(r2, fmaxf(fmaf(ax0, ax0, ay0 * ay0), fmaf(bx0, bx0, by0 * by0)));
            }
        }
        lds_poly[q] = make_float4(cx, cy, cnt > 0.0f ? sqrtf(r2) : -1.0e30f, 0.0f);   // an empty polygon is never near
    }
    // radius + safety space never changes during a launch: it is stored once (in both buffers' rows; XY_ROWS builds: in lds_rs, beside
    // rows that hold nothing but (x, y)), a substep only rewrites (x, y) -- two 8-byte LDS stores instead of two 16-byte ones
    auto publish = [&](int buf) {      // my position, both copies
        const float2 me = make_float2(px, py);
        if constexpr (XY_ROWS) {
            lds_xy[buf * TP + pbase + row] = me;
            lds_xy[buf * TP + pbase + rows + row] = me;
        } else {
        *reinterpret_cast<float2*>(&lds_p[buf * TP + pbase + row]) = me;
        *reinterpret_cast<float2*>(&lds_p[buf * TP + pbase + rows + row]) = me;
        }
    };
    // Helbing / Guo pair-once builds read partner velocities only in the (rare) contact pass, which publishes them itself
    constexpr bool VEL_ON_DEMAND = N3L && SOC != 2 && PEQ;
    auto publish_v = [&](int buf) {    // stored linear velocity; second copy only where the rotated loop reads it
        if constexpr (!VEL_ON_DEMAND) {
            lds_v[buf * TP + pbase + row] = make_float2(vx, vy);
            if constexpr (N3L && SOC == 2) lds_v[buf * TP + pbase + rows + row] = make_float2(vx, vy);
        }
    };
    if (valid) {
        // (PP: the sign of my C / A goes along in the free fourth slot: the partner that evaluates my side needs it)
        if constexpr (XY_ROWS) {
            publish(0);
            publish(1);
            lds_rs[tid] = my_rs;   // (tid = base + row)
        } else {
        const float4 me = make_float4(px, py, my_rs, PP ? sp.sAC : 0.0f);
        for (int buf = 0; buf < 2; ++buf) {
            lds_p[buf * TP + pbase + row] = me;
            lds_p[buf * TP + pbase + rows + row] = me;
        }
        }
        if constexpr (PP) {
            // my side of a pair as my partner will evaluate it: exponent (rs_partner - dist) cB + (lA + cB rs_me); a row without
            // parameters (the robot: a source only, its own sum is never used) publishes finite zeros
            const float4 mine = make_float4(fmaf(sp.cB, my_rs, sp.lA), sp.cB, fmaf(sp.cD, my_rs, sp.lC), sp.cD);
            lds_pp[pbase + row] = mine;
            lds_pp[pbase + rows + row] = mine;
        }
        publish_v(0);
        float rvx = vx, rvy = vy;
        if (HEADED > 0 && human) {
            sincos_fast(th, sn, cs);
            rvx = cs * bvx + (-sn) * bvy;
            rvy = sn * bvx + cs * bvy;
        }
        lds_vr[tid] = make_float2(rvx, rvy);
    }
    if constexpr (MAXT == 64) LDS_ORDER_FENCE(); else __syncthreads();   // (a one-wavefront block: its LDS operations execute in order; the wavefronts of a workgroup share nothing)

#ifdef CS_STAMPS
    unsigned long long st_acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long st_last;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(st_last)::"memory");
    pst_loop = st_last;
#endif
    int cur = 0;
    lAi = fmaf(sp.cB, my_rs, sp.lA); lCi = fmaf(sp.cD, my_rs, sp.lC);
    // compile-time row counts: radius + safety space of my partners (ring distance k + 1) never changes during a launch -- held in
    // registers, so that a substep reads 8-byte (x, y) partner rows from the LDS instead of 12-byte ones (the LDS pipe is a co-bottleneck)
    constexpr int RSN = (ROWS_CT > 0 && N3L) ? (ROWS_CT - 1) / 2 + 1 : 1;
    float rsj[RSN];
#pragma unroll
    for (int k = 0; k < RSN; ++k) rsj[k] = D(0.0f);
    // ... and the reaction slot of partner k: (row + 1 + k) mod rows.  With the modulo every slot of an accumulator row is written by
    // exactly one lane in every group, so the FIRST group stores instead of accumulating (no zeroing pass, no read), and a receiver reads
    // one slot per row instead of a low and a high copy -- a quarter of the loop's LDS bytes at 25 rows
    int aoff[RSN];
#pragma unroll
    for (int k = 0; k < RSN; ++k) aoff[k] = D(0);
#undef D
    if constexpr (LAUNCH_TRIM) {
        // a function of the lane's row alone: formed by every lane, outside the `if (valid)` below, so that no default is merged in behind
        // it; and without a compare and a select per slot -- t - ROWS_CT wraps to a huge unsigned exactly when t < ROWS_CT
#pragma unroll
        for (int k = 0; k < RSN; ++k) aoff[k] = (int)min((unsigned)(row + 1 + k), (unsigned)(row + 1 + k - ROWS_CT));
    }
    // ... and, with per-agent parameters (PP), its parameter row and the sign of its C / A: nothing but (x, y) is read per pair
    constexpr int PPN = (ROWS_CT > 0 && PP) ? RSN : 1;
    float4 ppj[PPN];
    float sacj[PPN];
#pragma unroll
    for (int k = 0; k < PPN; ++k) { ppj[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); sacj[k] = 0.0f; }
    if constexpr (ROWS_CT > 0 && N3L) {
        if (valid) {
#pragma unroll
            for (int k = 0; k < RSN; ++k) {
                if constexpr (!XY_ROWS) {
                const float4 pk = lds_p[pbase + row + 1 + k];
                rsj[k] = pk.z;
                if constexpr (PP) { sacj[k] = pk.w; ppj[k] = lds_pp[pbase + row + 1 + k]; }
                }
                const int t = row + 1 + k;
                if constexpr (!LAUNCH_TRIM) aoff[k] = t >= ROWS_CT ? t - ROWS_CT : t;
                if constexpr (XY_ROWS) rsj[k] = lds_rs[base + aoff[k]];   // (a 4-byte read of the partner's own row: lds_rs is not doubled)
            }
        }
    }
    // Two wavefronts share a SIMD at the benchmark's 4096 worlds, and of two ready wavefronts of equal priority the arbiter issues the OLDER:
    // the first half of the grid finished its 20 substeps 16 % ahead of the second (s_memtime stamps: two classes of exactly 1024
    // wavefronts), which then ran its last three substeps alone, at a lone wavefront's latency-bound pace.  The younger wavefront of a
    // SIMD (a.young_from, set by the launcher for a grid of exactly two per SIMD) raises its priority in every other substep: the two
    // take turns (priority 2 / 1) and finish within 3 % of each other (31.1 -> 29.4 us with the short rare paths, -> 28.3 us with this).
    // ---- wall pairs (LEAN = 2: the 50-row crowd with polygon walls, cfg5's per-GPU shard) --------------------------------------------
    // Every lane used to walk every polygon some agent of its wavefront is near: with 50 agents somebody is near each of the three
    // polygons, so the wave vote never skips -- 3 x (vote + 5 segments x 13 + force) = 252 of a substep's 710 vector instructions --
    // while half to two thirds of the 150 (agent, polygon) pairs are within the reach of the force in that window, none before it
    // (tools/wall_pairs_stats.py).
    // Round 4 compacted the pairs inside every substep (votes, prefix counts, rows handed over through LDS): 90 instructions of
    // bookkeeping per substep and no gain.  Here the pairs are numbered ONCE per launch: an agent that starts farther than
    // reach + n_substeps dt v_desired from a polygon cannot get within its reach during the launch (speeds are clamped to v_desired and
    // the respawn rule -- the only jump -- keeps the builds with CS_RESPAWN on the old pass), so the numbering holds for all substeps.
    // A substep then costs ONE closest-point + force per lane and pass (two passes for 65 .. 128 pairs; more: the old pass for this
    // launch) and three LDS reads per agent; a lane whose agent touches its polygon adds the k1 / k2 terms from the agent's refreshed
    // velocity (published by every agent at the head of the substep).  Same operations on the same operands per pair; a polygon beyond
    // an agent's reach adds an exact zero instead of a force below the reach's bound.  8192 x 50 + 3 polygons, Gym steps 20-70:
    // 211 -> 197 us at the old reach of 36 e-folding lengths, 205 -> 191 us at 22 (profiles/r5e_wall_pairs_ab.txt).
    constexpr int WP_O = 4;                    // polygons per world the pair numbers of an agent cover (one byte each)
    bool wp_on = false;
    int wp_count = 0;
    unsigned wp_mine = 0x80808080u;            // my pairs' numbers, one byte per polygon; WP_MAX = none (lds_wres[WP_MAX] stays zero)
    if constexpr (LEAN == 2 && MAXT == 64) {
        if (a.wall_pairs != 0) {                                              // (kernel argument: wave-uniform)
            const float travel = (float)a.nsub * a.dt * vd + 1.0e-3f;
            int total = 0;
            for (int o = 0; o < a.O; ++o) {
                const float4 pc = lds_poly[(sbase / a.Smax) + o];
                const float dxc = px - pc.x, dyc = py - pc.y, lim = pc.z + wall_cut + travel;
                const bool reach = human && fmaf(dxc, dxc, dyc * dyc) < lim * lim;
                const unsigned long long mk = __builtin_amdgcn_ballot_w64(reach);
                const int rank = total + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mk, 0u));
                if (reach && rank < WP_MAX) {
                    lds_wrec[rank] = (pbase + row) | ((sbase + o * a.Smax) << 8) | (tid << 20);
                    lds_wrs[rank] = make_float2(r, safety);
                    wp_mine = (wp_mine & ~(0xFFu << (8 * o))) | ((unsigned)rank << (8 * o));
                }
                total += __builtin_popcountll(mk);
            }
            if (tid == 0) { lds_wres[WP_MAX] = make_float2(0.0f, 0.0f); *lds_wlaw = make_float4(Aw, cBw, k1, k2); }   // (lane 0 is a human of the block's first world)
            wp_count = total;
            wp_on = total <= WP_MAX;             // (more: this launch walks the polygons as before)
            LDS_ORDER_FENCE();
        }
    }
