// sfmstep_sub_respawn.inc -- a fragment of k_sfm_step (sfmstep_kernel.h), included inside the kernel body: the parallel-traffic respawn rule, sequential inside a world, by wave ballot.
// Not a translation unit and not a function: it reads and writes the kernel's locals (the lane's row in registers, the LDS views, the
// template parameters).  The split is textual -- the token stream of the kernel is what it was in one file -- so that each phase can be
// read on its own; sfmstep_kernel.h lists the phases in order.  gfx950 only.
        STAMP(4);
        // -- parallel-traffic respawn, motion_model_manager.py:407-422 (sequential inside a world)
        if (a.flags & CS_RESPAWN) {
            const float rdx = px - g0x, rdy = py - g0y;
            const int flag = (human && respawn_here && fmaf(rdx, rdx, rdy * rdy) < 9.0f) ? 1 : 0; // |p - g| < 3
            if constexpr (MAXT == 64) {
                // one wavefront holds whole worlds: no barrier, no serial lane.  The reference respawns the flagged
                // humans of a world in index order, each behind everybody else (:411-417): x_0 = max(max_x + 2 max_r,
                // bound), and the c-th flagged one (c lower-indexed flagged rows in its world) lands at
                // x_c = max(x_{c-1} + 2 max_r, bound) because x_{c-1} is then the rightmost human.
                // ONE data-dependent branch in the common (nobody flagged) case: the vote is taken inside the branch, where
                // only the flagged lanes are active -- exactly the lanes it has to count
                if (flag) {
                    const unsigned long long fm = __builtin_amdgcn_ballot_w64(true);
                    const unsigned long long wm = (rows >= 64 ? ~0ull : ((1ull << rows) - 1ull)) << base;
                    const int c = __builtin_popcountll(fm & wm & ((1ull << tid) - 1ull));
                    const float4* pvn = XY_ROWS ? nullptr : lds_p + nxt * TP + pbase;
                    float mx, mr;
                    if constexpr (XY_ROWS) {
                        // x from the 8-byte rows, radius + safety space from its own row (n == rows here: no robot row).  Up to 32 rows:
                        // every row requested before the first wait (a scheduling barrier between the requests and the maxima) -- one LDS
                        // round trip where the compiler, left alone, waited four times; the maxima in the order they have always had.
                        const float2* xyn = lds_xy + nxt * TP + pbase;
                        const float* rsn = lds_rs + base;
                        if constexpr (ROWS_CT <= 32 && OCC == 1) {
                            float xs[ROWS_CT], rss[ROWS_CT];
#pragma unroll
                            for (int j = 0; j < ROWS_CT; ++j) { xs[j] = xyn[j].x; rss[j] = rsn[j]; }
                            __builtin_amdgcn_sched_barrier(0);
                            mx = xs[0]; mr = rss[0];
#pragma unroll
                            for (int j = 1; j < ROWS_CT; ++j) { mx = fmaxf(mx, xs[j]); mr = fmaxf(mr, rss[j]); }
                        } else {
                            mx = xyn[0].x; mr = rsn[0];
#pragma unroll 8
                            for (int j = 1; j < ROWS_CT; ++j) { mx = fmaxf(mx, xyn[j].x); mr = fmaxf(mr, rsn[j]); }
                        }
                    } else {
                    mx = pvn[0].x; mr = pvn[0].z;
                    // (the rows requested together -- all of them when the row count is a compile-time constant, eight per trip otherwise:
                    // one at a time was 24 dependent LDS round trips per respawn, and the launch waits for its slowest wavefront: 31.1 -> 29.9 us at cfg3)
                    if constexpr (ROWS_CT > 0 && ROWS_CT <= 32) {
#pragma unroll
                        for (int j = 1; j < ROWS_CT; ++j) {
                            if (j < n) { mx = fmaxf(mx, pvn[j].x); mr = fmaxf(mr, pvn[j].z); }
                        }
                    } else {
#pragma unroll 8
                        for (int j = 1; j < n; ++j) {
                            mx = fmaxf(mx, pvn[j].x);
                            mr = fmaxf(mr, pvn[j].z);
                        }
                    }
                    if (robot_row) { // consider_robot: the robot where it stands in THIS substep
                        const float4 qr = lds_p[cur * TP + pbase + n];
                        mx = fmaxf(mx, qr.x);
                        mr = fmaxf(mr, qr.z);
                    }
                    }
                    px = csimpl::respawn_x(mx, mr, a.bx, c);   // (respawnx.h: the reference's float64 sum, rounded once)
                    py = (py >= 0.0f) ? fminf(py, a.by) : fmaxf(py, -a.by);
                    publish(nxt);
                    g0y = py;               // human.set_goals([[goals[0][0], position[1]]])   :418
                    bvy = g0x; om = g0y;    // states[i,6:8] = goal  (reference writes cols 6:8) :421
                    if constexpr (CARRY_CV) { cvx_c = fmaf(cs, bvx, -(sn * bvy)); cvy_c = fmaf(cs, bvy, sn * bvx); }   // (the carried refreshed velocity saw the old bvy)
                    for (int g = 0; g < a.G; ++g) { gi[2 * g] = g0x; gi[2 * g + 1] = g0y; } //   :422
                    gk = a.G; g1x = g0x; g1y = g0y;
                }
            } else if (__syncthreads_or(flag) != 0) {
                lds_flag[tid] = flag;
                lds_g0x[tid] = g0x;
                __syncthreads();
                if (valid && row == 0) {
                    float4* pvn = lds_p + nxt * TP + pbase;
                    // the maxima of the world as the first respawned human finds it; the c-th lands c steps behind (respawnx.h)
                    float mx = pvn[0].x, mr = pvn[0].z;
                    for (int j = 1; j < n; ++j) {
                        mx = fmaxf(mx, pvn[j].x);
                        mr = fmaxf(mr, pvn[j].z);
                    }
                    if (robot_row) { // consider_robot: the robot where it stands in THIS substep
                        const float4 qr = lds_p[cur * TP + pbase + n];
                        mx = fmaxf(mx, qr.x);
                        mr = fmaxf(mr, qr.z);
                    }
                    int c = 0;
                    for (int i = 0; i < n; ++i) {
                        if (!lds_flag[base + i]) continue;
                        float4 q = pvn[i];
                        q.x = csimpl::respawn_x(mx, mr, a.bx, c++);
                        q.y = (q.y >= 0.0f) ? fminf(q.y, a.by) : fmaxf(q.y, -a.by);
                        pvn[i] = q;
                        pvn[rows + i] = q;
                    }
                }
                __syncthreads();
                if (flag) {
                    const float4 q = lds_p[nxt * TP + pbase + row];
                    px = q.x; py = q.y;
                    g0y = py;               // human.set_goals([[goals[0][0], position[1]]])   :418
                    bvy = g0x; om = g0y;    // states[i,6:8] = goal  (reference writes cols 6:8) :421
                    for (int g = 0; g < a.G; ++g) { gi[2 * g] = g0x; gi[2 * g + 1] = g0y; } //   :422
                    gk = a.G; g1x = g0x; g1y = g0y;
                }
            }
        }
