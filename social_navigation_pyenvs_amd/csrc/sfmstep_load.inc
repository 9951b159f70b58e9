// sfmstep_load.inc -- a fragment of k_sfm_step (sfmstep_kernel.h), included inside the kernel body: the load phase: every global load of the prologue issued before the first use (one memory round trip); the row, the parameter rows, the goal list, the world flag, the action, the Gym head's inputs.
// Not a translation unit and not a function: it reads and writes the kernel's locals (the lane's row in registers, the LDS views, the
// template parameters).  The split is textual -- the token stream of the kernel is what it was in one file -- so that each phase can be
// read on its own; sfmstep_kernel.h lists the phases in order.  gfx950 only.
    // ---- load phase ---------------------------------------------------------------------
    // Every global load of the prologue is issued before the first result is used: ONE memory round trip.  (Until round 4 the row,
    // the parameter rows, the goal list -- a NaN scan that loaded and waited slot by slot --, the world's respawn flag and the action
    // were seven dependent round trips, ~3.2 us of a 33 us launch by the s_memtime stamps of tools/launch_floor.sh's probe.)
    // Straight-line code on purpose: a load inside a branch whose other arm is a constant gets its first use hoisted into the branch
    // (and a wait with it), so lanes without a world / a human row load world 0's / row 0's (never used) and an absent optional array is
    // replaced by a readable dummy address instead of being branched around.
#ifdef CS_STAMPS
    unsigned long long pst_entry, pst_loaded = 0, pst_loop, pst_loop_end;   // (diagnostic build: where a launch's time around its substeps goes)
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(pst_entry)::"memory");
#endif
    const long sidx = (long)w * rows + row;
    const int wc = valid ? w : 0, rowh = human ? row : 0;
    const long sidx_c = valid ? sidx : 0;
    const float* dummy = a.Sin;
    // LAUNCH_TRIM builds (sfmstep_kernel.h): every dword of this phase is addressed as (kernel argument + scalar terms) + an unsigned 32-bit
    // byte offset of the lane -- a scalar base and ONE vector register per array, where the pointer arithmetic of the other arm costs two
    // to five 64-bit vector instructions per load.  The byte offsets of the shapes these builds are launched for fit 32 bits
    // (crowdstep.hip offsets_fit_32).  srow: my row in the per-row arrays (row 0 for a lane without a world), used again by the epilogue.
    const unsigned srow = LAUNCH_TRIM ? (valid ? (unsigned)(w * rows + row) : 0u) : 0u;
    float px, py, th, vx, vy, bvx, bvy, om, r, m, gx, gy, vd;
    if constexpr (LAUNCH_TRIM) {
        const float* s = a.Sin;   // column k starts at s + k * fs: scalar arithmetic
        const long fs = a.in_fs;
        const unsigned so = srow * (unsigned)a.in_as * 4u;
        px = ld_off(s, so); py = ld_off(s + fs, so); th = ld_off(s + 2 * fs, so); vx = ld_off(s + 3 * fs, so); vy = ld_off(s + 4 * fs, so);
        bvx = ld_off(s + 5 * fs, so); bvy = ld_off(s + 6 * fs, so); om = ld_off(s + 7 * fs, so); r = ld_off(s + 8 * fs, so);
        m = ld_off(s + 9 * fs, so); gx = ld_off(s + 10 * fs, so); gy = ld_off(s + 11 * fs, so); vd = ld_off(s + 12 * fs, so);
    } else {
        const float* s = a.Sin + sidx_c * a.in_as;
        const long fs = a.in_fs;
        px = s[0]; py = s[fs]; th = s[2 * fs]; vx = s[3 * fs]; vy = s[4 * fs]; bvx = s[5 * fs];
        bvy = s[6 * fs]; om = s[7 * fs]; r = s[8 * fs]; m = s[9 * fs]; gx = s[10 * fs]; gy = s[11 * fs];
        vd = s[12 * fs];
    }
    float safety = LAUNCH_TRIM ? ld_off(a.safety, srow * 4u) : a.safety[sidx_c];
    const bool has_wflags = a.world_flags != nullptr;
    // bit 0: the respawn rule applies to my world  (LAUNCH_TRIM without world flags: word wc of the state array, never used -- the state
    // holds more words than there are worlds)
    const int wflag_raw = LAUNCH_TRIM ? ld_off(has_wflags ? a.world_flags : reinterpret_cast<const int*>(dummy), (unsigned)wc * 4u)
                                      : *(has_wflags ? a.world_flags + wc : reinterpret_cast<const int*>(dummy));
    const bool robot_moves = a.action != nullptr; // (lean build: only the invisible robot of the epilogue)
    float ax, ay;                                 // robot action (held for the whole block, social_nav_gym.py:240-243)
    if constexpr (LAUNCH_TRIM) {
        // behind the wave-uniform test of its kernel argument: a launch without an action issues no load for it; one with an action issues
        // it here, ahead of the phase's one wait (its first use is in the prologue)
        ax = 0.0f; ay = 0.0f;
        if constexpr (!POLICY) {   // (POLICY: the action is decided in the prologue)
            if (CS_RARE(robot_moves)) { ax = ld_off(a.action, (unsigned)wc * 8u); ay = ld_off(a.action + 1, (unsigned)wc * 8u); }
        }
    } else {
        const float* ap = (robot_moves && !POLICY) ? a.action + (long)wc * 2 : dummy;   // (POLICY: the action is decided in the prologue)
        ax = ap[0]; ay = ap[1];
    }
    // parameters: my own row of P for the single-agent forces; P[0] of my world for the pair loop
    // when all_params_equal (forces_parallel.py:220), else my own row (:261)
    const long pw = (a.flags & CS_PARAMS_SHARED) ? 0 : (long)wc * n * 20;
    const float* Prow = a.params + pw + (long)rowh * 20;
    // (LAUNCH_TRIM: the same rows as byte offsets -- my world's table, my row in it -- and my goal list's, which the epilogue uses again)
    const unsigned pwoff = LAUNCH_TRIM ? ((a.flags & CS_PARAMS_SHARED) ? 0u : (unsigned)wc * (unsigned)(n * 80)) : 0u;
    const unsigned poff = LAUNCH_TRIM ? pwoff + (unsigned)rowh * 80u : 0u;
    const unsigned goff = LAUNCH_TRIM ? (unsigned)(wc * n + rowh) * (unsigned)a.G * 8u : 0u;
    float Pm[11];                                 // my P[0], [2], [4], [6], [8], [10], [11], [16], [17], [18], [19]
    if constexpr (LAUNCH_TRIM) {
        const float* P = a.params;
        Pm[0] = ld_off(P, poff); Pm[1] = ld_off(P + 2, poff); Pm[2] = ld_off(P + 4, poff); Pm[3] = ld_off(P + 6, poff); Pm[4] = ld_off(P + 8, poff);
        Pm[5] = ld_off(P + 10, poff); Pm[6] = ld_off(P + 11, poff); Pm[7] = ld_off(P + 16, poff); Pm[8] = ld_off(P + 17, poff);
        Pm[9] = ld_off(P + 18, poff); Pm[10] = ld_off(P + 19, poff);
    } else {
    Pm[0] = Prow[0]; Pm[1] = Prow[2]; Pm[2] = Prow[4]; Pm[3] = Prow[6]; Pm[4] = Prow[8]; Pm[5] = Prow[10]; Pm[6] = Prow[11];
    Pm[7] = Prow[16]; Pm[8] = Prow[17]; Pm[9] = Prow[18]; Pm[10] = Prow[19];
    }
    const SocRaw sraw = LAUNCH_TRIM ? load_socraw_off(a.params, PEQ ? pwoff : poff) : load_socraw(PEQ ? a.params + pw : Prow);
    // my goal list (row 0's for a lane without a human)
    float* gi = LAUNCH_TRIM ? reinterpret_cast<float*>(reinterpret_cast<char*>(a.goals) + goff) : a.goals + ((long)wc * n + rowh) * a.G * 2;
    float gl[4];                                  // its first two slots
    if constexpr (LAUNCH_TRIM) {
        const float* g2 = a.G >= 2 ? a.goals + 2 : a.goals;   // (a scalar choice of the base)
        gl[0] = ld_off(a.goals, goff); gl[1] = ld_off(a.goals + 1, goff);
        gl[2] = ld_off(g2, goff); gl[3] = ld_off(g2 + 1, goff);
    } else {
    gl[0] = gi[0]; gl[1] = gi[1];
    {
        const float* g2 = a.G >= 2 ? gi + 2 : gi;
        gl[2] = g2[0]; gl[3] = g2[1];
    }
    }
    if (valid && is_robot && (kmode & M_ROBOT_FROM_ARRAY)) {   // (divergent: the robot's lane)
        const float* rb = a.robot + (long)w * 13;
        px = rb[0]; py = rb[1]; th = rb[2]; vx = rb[3]; vy = rb[4]; bvx = rb[5]; bvy = rb[6]; om = rb[7];
        r = rb[8]; m = rb[9]; gx = rb[10]; gy = rb[11]; vd = rb[12];
    }
    // an invisible robot (no row of its own) is advanced by the lane of row 0; its five dynamic columns come with the other loads -- requested
    // in the epilogue they were one more memory round trip at the end of every launch that moves a robot (~1 us of a Gym step)
    const bool moves_invisible_robot = valid && !robot_row && row == 0 && robot_moves && a.robot != nullptr && !(kmode & M_PEEK);
    float irb[5] = {0, 0, 0, 0, 0};
    // (ROBOT_LOADS_BRANCH, sfmstep_kernel.h: behind the wave-uniform half of that test -- a launch that moves no invisible robot issues none
    //  of the five; one that does issues them here, ahead of the phase's one wait, as the other arm does)
    if (!ROBOT_LOADS_BRANCH || CS_RARE(robot_moves && a.robot != nullptr && !(kmode & M_PEEK))) {
        const float* rb = moves_invisible_robot ? a.robot + (long)w * 13 : dummy;
        irb[0] = rb[0]; irb[1] = rb[1]; irb[2] = rb[2]; irb[3] = rb[3]; irb[4] = rb[4];
    }
    // (cs_gym_step: the robot as the head sees it and the action, see below)
    float hrb[6] = {0, 0, 0, 0, 0, 0}, hact[2] = {0, 0};
    float prb[3] = {0, 0, 0};   // (POLICY) what the robot's policy reads beside them: its velocity and v_pref
    // cs_gym_step_staged's take-over in the epilogue (gymhead.h GymFold): compiled into the builds without walls only -- the 50-row wall build
    // has no register to spare (its shard went 191 -> 200 us with the fold compiled in), and a Gym with polygon walls keeps the two launches
#ifdef CS_NO_FOLD   // (diagnostic variant build: what the fold's code costs the launches that do not use it)
    constexpr bool FOLD = false;
#else
    constexpr bool FOLD = MAXT == 64 && !(LEAN == 2 || LEAN == 5);
#endif
    GymPre hpre = {0.0f, 0, 0, 0, 0u, 0u};
    int fold_code_world = 0;   // (FOLD) the head's verdict for my world, in every lane of it (set in the prologue)
    if constexpr (MAXT == 64) {
        if (CS_RARE_HEAD(a.gym.out != nullptr) && valid) {
            const float* rb = a.robot + (long)w * 13;      // the robot BEFORE its move of substep 1
            hrb[0] = rb[0]; hrb[1] = rb[1]; hrb[2] = rb[8]; hrb[3] = rb[10]; hrb[4] = rb[11]; hrb[5] = rb[2];
            if constexpr (POLICY) { prb[0] = rb[3]; prb[1] = rb[4]; prb[2] = rb[12]; }
            else { hact[0] = a.action[(long)w * 2]; hact[1] = a.action[(long)w * 2 + 1]; }
            if (row == 0) hpre = gym_head_preload<MAXT == 64 && !(LEAN == 2 || LEAN == 5)>(a.gym, w);   // (last: the compiler waits for these right here)
        }
    }
    // imitation learning (LEAN = 4)
    float rm_hm = 0.0f, rm_fdx = 0.0f, rm_fdy = 0.0f;
    if constexpr (IMIT) {
        if (human) rm_hm = a.rm_hmargin[sidx];
        if (is_robot) { rm_fdx = a.rm_memory[(long)w * 2]; rm_fdy = a.rm_memory[(long)w * 2 + 1]; }
    }
#ifdef CS_STAMPS
    unsigned long long pst_issued;   // the last load of the phase has been issued (none waited for): entry -> here is the issue side, here -> pst_loaded the round trip
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(pst_issued)::"memory");
#endif

    const float inv_O = a.O > 0 ? 1.0f / (float)a.O : 0.0f;
    const float* obst = nullptr;
    if (!NO_WALLS && a.O > 0) obst = a.obstacles + ((a.flags & CS_OBSTACLES_SHARED) ? 0 : (long)w * a.O * a.Smax * 4);
    // (their loads belong to the load phase: the LDS stores below are the first use of anything loaded so far)
    // wall segments are constant over the launch: stage (x1, y1, e, 1/|e|^2) in LDS once instead of re-loading and
    // re-deriving them in every substep (3 polygons x 5 segments cost as much as the whole 50-agent pair loop otherwise)
    const int nseg = NO_WALLS ? 0 : a.O * a.Smax;
    const int sbase = (a.flags & CS_OBSTACLES_SHARED) ? 0 : lw * nseg;
    for (int i = tid; i < (NO_WALLS ? 0 : a.seg_tab); i += T) {
        const int lwi = i / (nseg > 0 ? nseg : 1);
        const long wi = (long)vblock * a.wpb + lwi;
        // a NaN slot becomes a degenerate segment 1e18 m away: squared distance 2e36, never the polygon's minimum (the reference
        // stores the largest int64 as that slot's distance, forces_parallel.py:247) -- no per-slot test in the substep loop
        float4 e = make_float4(1.0e18f, 1.0e18f, 0.0f, 0.0f);
        float inv = 0.0f;
        if ((a.flags & CS_OBSTACLES_SHARED) || wi < a.W) {
            const float* src = a.obstacles + ((a.flags & CS_OBSTACLES_SHARED) ? (long)i * 4 : (wi * nseg + (i - lwi * nseg)) * 4);
            const float4 seg = *reinterpret_cast<const float4*>(src);
            if (!isnan(seg.x)) {
                e = make_float4(seg.x, seg.y, seg.z - seg.x, seg.w - seg.y);
                inv = rcp_fast(fmaf(e.z, e.z, e.w * e.w));
            }
        }
        lds_seg[i] = e;
        lds_sinv[i] = inv;
    }

