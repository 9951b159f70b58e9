// sfmstep_epilogue.inc -- a fragment of k_sfm_step (sfmstep_kernel.h), included inside the kernel body: the epilogue: the row written back once per launch, goal lists, observation rows, robot rows, and the take-over of a staged episode (cs_gym_step_staged).
// Not a translation unit and not a function: it reads and writes the kernel's locals (the lane's row in registers, the LDS views, the
// template parameters).  The split is textual -- the token stream of the kernel is what it was in one file -- so that each phase can be
// read on its own; sfmstep_kernel.h lists the phases in order.  gfx950 only.
    // ---- epilogue ---------------------------------------------------------------------------
    // The epilogue's own kernel arguments (output pointers and strides, the observation and robot arrays, the Gym head's) are read HERE,
    // from the kernarg segment through a base the optimiser cannot see through: read as `a.x` every kernel argument is requested at the
    // kernel's entry and held in a scalar register -- or a spilled vector lane -- across the substep loop.  (`a` is the kernel's only
    // parameter: its bytes start the segment.)
#ifdef __HIP_DEVICE_COMPILE__
    unsigned long long karg_base = (unsigned long long)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(karg_base));
#define KARG(field) (*(const __attribute__((address_space(4))) decltype(((const KArgs*)nullptr)->field)*)(karg_base + __builtin_offsetof(KArgs, field)))
#else
#define KARG(field) (a.field)
#endif
    if (kmode & M_PEEK) {
        if (human) {
            float* o = KARG(peek_out) + ((long)w * n + row) * 8;
            o[0] = px; o[1] = py; o[2] = th; o[3] = vx; o[4] = vy; o[5] = om;
            o[6] = g0x; o[7] = g0y; // human.goals[0] (the goals array), not the state's goal columns (:297)
        }
        return;
    }
    // cs_gym_step_staged: what the head decided for my world (gymhead.h GymFold).  A world that takes over its staged episode writes
    // nothing of the stepped rows; the wavefront copies the slot over it below.
    int fold_code = 0;
    if constexpr (FOLD) fold_code = valid ? fold_code_world : 0;   // (from the head's lane, prologue; 0 in a launch without a head or without the fold)
    const bool taken_over = fold_code >= 2;
    if (human && gdirty && (kmode & M_COMMIT_GOALS) && !taken_over) {
        if constexpr (LAUNCH_TRIM) {   // (the list's base read here, not held across the loop; goff: the load phase's offset)
            float* gb = KARG(goals);
            st_off(gb, goff, g0x); st_off(gb + 1, goff, g0y); st_off(gb + 2, goff, g1x); st_off(gb + 3, goff, g1y);
        } else { gi[0] = g0x; gi[1] = g0y; gi[2] = g1x; gi[3] = g1y; }
    }
    if constexpr (LAUNCH_TRIM) {
        // the same stores off scalar bases: column k of the output at Sout + k * out_fs, the lane's 32-bit byte offset in one register
        // (these builds hold humans only: human == valid, no robot row; r, m and v_desired are written out of place only)
        if (valid && !taken_over) {
            float* o = KARG(Sout);
            const long fs = KARG(out_fs);
            const unsigned so = srow * (unsigned)KARG(out_as) * 4u;
            st_off(o, so, px); st_off(o + fs, so, py); st_off(o + 2 * fs, so, th); st_off(o + 3 * fs, so, vx); st_off(o + 4 * fs, so, vy);
            st_off(o + 5 * fs, so, bvx); st_off(o + 6 * fs, so, bvy); st_off(o + 7 * fs, so, om); st_off(o + 10 * fs, so, gx); st_off(o + 11 * fs, so, gy);
            if (KARG(Sout) != KARG(Sin)) { st_off(o + 8 * fs, so, r); st_off(o + 9 * fs, so, m); st_off(o + 12 * fs, so, vd); }
        }
    }
    if (valid && !taken_over) {
        float* o = KARG(Sout) + sidx * KARG(out_as);
        const long fs = KARG(out_fs);
        if (!LAUNCH_TRIM && (human || is_robot)) {
            o[0] = px; o[fs] = py; o[2 * fs] = th; o[3 * fs] = vx; o[4 * fs] = vy; o[5 * fs] = bvx;
            o[6 * fs] = bvy; o[7 * fs] = om; o[10 * fs] = gx; o[11 * fs] = gy;
            if (KARG(Sout) != KARG(Sin) || is_robot) { o[8 * fs] = r; o[9 * fs] = m; o[12 * fs] = vd; }
        }
        // the Gym's observation of the stepped crowd (SocialNavGym.compute_humans_observable_state, social_nav_gym.py:100-105) straight
        // from the registers: what cs_gym_observe would read back from the rows just written
        if (CS_RARE(KARG(obs) != nullptr) && human) {
            float* ob = KARG(obs) + ((long)w * n + row) * KARG(obs_cols);
            ob[0] = px; ob[1] = py; ob[2] = vx; ob[3] = vy; ob[4] = r;
            if (KARG(obs_cols) == 7) { ob[5] = th; ob[6] = om; }
        }
        if (CS_RARE(robot_moves && KARG(robot) != nullptr) && is_robot) {
            float* rb = KARG(robot) + (long)w * 13;
            rb[0] = px; rb[1] = py; rb[2] = th; rb[3] = vx; rb[4] = vy;
        }
        if constexpr (IMIT) {
            if (is_robot) {   // what cs_robot_model_step leaves: the robot's dynamic columns and its model's remembered desired force
                float* rb = KARG(robot) + (long)w * 13;
                rb[0] = px; rb[1] = py; rb[2] = th; rb[3] = vx; rb[4] = vy; rb[5] = bvx; rb[6] = bvy; rb[7] = om;
                KARG(rm_memory)[(long)w * 2] = rm_fdx; KARG(rm_memory)[(long)w * 2 + 1] = rm_fdy;
            }
        }
    }
    if constexpr (FOLD) {
        if (CS_RARE(KARG(gym.out) != nullptr && KARG(gym.fold.on))) {
            // The take-over's arguments (GymFold: the copy's twenty pointers and strides) are read HERE, through a pointer the optimiser cannot
            // see through: read as kernel arguments they are all requested at the kernel's entry and held in scalar registers across the
            // substep loop -- the per-agent build spilled 350 of them to vector lanes and lost 4 % on every launch, folding or not.
            // (the kernel's only parameter is `a`: its bytes start the kernarg segment; taking &a.gym.fold instead would copy `a` to scratch)
            const GymFold f = KARG(gym.fold);
            for (int l = 0; l < a.wpb; ++l) {                                   // the worlds of this wavefront, one after the other (wave-uniform)
                const int wl = vblock * a.wpb + l;
                if (wl >= a.W) break;
                const int code = __builtin_amdgcn_readlane(fold_code, l * rows);  // (the lane of the world's row 0 holds its code like every lane of the world)
                if (code == 0) continue;
                if (code >= 2) {
                    const long slot = code - 2;
                    const int status = csimpl::copy_world<true>(f.copy, slot, wl, tid, f.staged_status + slot);   // (a world that could not be generated is not copied)
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");              // every load of the slot has returned
                    if (tid == 0) {
                        f.failed[wl] = status != 0 ? 1 : 0;
                        __hip_atomic_store(f.pending + wl, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        // LAST: from here on the refill may overwrite the slot (it now belongs to episode epoch + depth)
                        __hip_atomic_store(f.epoch + wl, f.epoch[wl] + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                } else if (code < 0) {
                    // the staged episode could not be generated: the world kept its stepped rows (stored above: taken_over was false); the
                    // slot's turn is over all the same -- what k_consume_staged does with such a slot (generate.hip)
                    if (tid == 0) {
                        f.failed[wl] = 1;
                        __hip_atomic_store(f.pending + wl, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_store(f.epoch + wl, f.epoch[wl] + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                } else if (tid == 0) {
                    f.failed[wl] = 2;                                             // deferred: the slot was not staged yet (pending[wl] stays 1)
                }
            }
        }
    }
#ifdef CS_STAMPS
    {   // slots 0 .. 11: the substep sections (STAMP); 12: entry -> every load returned, 13: -> first substep, 14: last substep -> stores issued,
        // 15: -> stores acknowledged (s_waitcnt vmcnt(0): what the wavefront itself would not wait for)
        unsigned long long pst_stored, pst_acked;
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(pst_stored)::"memory");
        asm volatile("s_waitcnt vmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(pst_acked)::"memory");
        if (a.stamps != nullptr && (threadIdx.x & 63) == 0) {
            unsigned long long* o = a.stamps + ((size_t)blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64) * 20;
            for (int k = 0; k < 12; ++k) o[k] = st_acc[k];
            o[12] = pst_loaded - pst_entry; o[13] = pst_loop - pst_loaded; o[14] = pst_stored - pst_loop_end; o[15] = pst_acked - pst_stored;
            o[16] = pst_entry - pst_first;                      // first instruction -> kernel arguments loaded
            unsigned long long rt_end;
            asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt_end)::"memory");
            o[17] = pst_first_rt; o[18] = rt_end;               // the wall clock at the wavefront's first and last instruction (10 ns ticks)
            o[19] = pst_issued - pst_entry;                     // entry -> the last load of the load phase issued (the issue side of slot 12)
        }
    }
#endif
#undef KARG
