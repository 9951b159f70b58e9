// sfmstep_policy.hip -- builds of the fused SFM / HSFM step kernel (sfmstep_kernel.h, k_sfm_step<SOC, HEADED, PEQ, MAXT, OCC, ROWS_CT, LEAN_ARG>):
// LEAN_ARG = 8 + 1 -- the plain crowd batch with an INVISIBLE robot whose no-train policy (bp, ssp, sfm_helbing, sfm_guo, sfm_moussaid:
// policy_no_train.h) is decided in the launch's prologue, before the Gym head consumes the action: cs_gym_step_policy, the seam
// `action = robot.act(ob); ob, reward, done, info = env.step(action)` of Explorer.run_k_episodes (crowd_nav/utils/explorer.py:57-58) as ONE launch.
// Each build is the twin of the LEAN = 1 build of the same budget and row count (sfmstep_lean25.hip, sfmstep_leanrt.hip): 25 humans, and
// any other row count with the run-time partner loop.  gfx950 only.
#include "sfmstep_kernel.h"

namespace cstep {

kfn sfm_builds_policy(const Variant& v, int type)
{
    CS_V(64, 1, 25, 9) CS_V(64, 4, 25, 9) CS_V(64, 3, 0, 9)
    return nullptr;
}

} // namespace cstep
