// sfmstep_substep.inc -- a fragment of k_sfm_step (sfmstep_kernel.h), included inside the kernel body: ONE substep, the five phases in order.
// Not a translation unit and not a function: it reads and writes the kernel's locals.  Whoever includes it has `sub` (the substep's index) and
// `cur` (the LDS buffer the substep reads) in scope and advances `cur` behind it; the head declares `nxt`.  The kernel states the substep here
// once and instantiates it where its loop needs it (sfmstep_kernel.h: the loop of every build, and the single exec region of the plain
// one-wavefront builds, where `valid` and `human` are compile-time facts).  gfx950 only.
        // head of a substep: priority turn, recorders (imitation snapshot, cs_step_trace), the robot under its own motion model (LEAN = 4), partner-row fetch helpers, the goal switch
#include "sfmstep_sub_head.inc"
        // part A: what does not depend on this substep's social force -- the wall pairs' pass, refreshed velocity, desired force, the all-lanes wall pass, heading and torque
#include "sfmstep_sub_part_a.inc"
        // the pair-once loop (each unordered pair evaluated once, reaction handed over through LDS), the reaction sum, and the contact pass behind a wave vote
#include "sfmstep_sub_pairloop.inc"
        // all partners per lane (per-agent parameters on Moussaid, worlds of more than one wavefront), part B: total force, body frame, torque, the Euler step, the rows published for the next substep
#include "sfmstep_sub_tail.inc"
        // the parallel-traffic respawn rule, sequential inside a world, by wave ballot.  The plain one-wavefront builds enter it through one
        // scalar branch on the tail's vote (EARLY_VOTES, sfmstep_kernel.h); a wavefront that does re-runs the next goal switch (the rule
        // moves rows and their goals[0]: the tail's vote was on the rows of before), the others hand the tail's vote on as it is
        if constexpr (EARLY_VOTES) {
            if (CS_RARE(flag_any)) {
#include "sfmstep_sub_respawn.inc"
                hit_next = ~0ull;
            }
            carried_hit = hit_next;
        } else {
#include "sfmstep_sub_respawn.inc"
        }
        STAMP(5);
        LDS_ORDER_FENCE(); // rows republished by the respawn rule are read by other lanes in the next substep
