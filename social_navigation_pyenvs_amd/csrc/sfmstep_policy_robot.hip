// sfmstep_policy_robot.hip -- builds of the fused SFM / HSFM step kernel (sfmstep_kernel.h, k_sfm_step<SOC, HEADED, PEQ, MAXT, OCC, ROWS_CT, LEAN_ARG>):
// LEAN_ARG = 8 + 3 -- the plain crowd batch with a VISIBLE robot as the last row whose no-train policy (policy_no_train.h) is decided in
// the launch's prologue, before the Gym head consumes the action (cs_gym_step_policy; see sfmstep_policy.hip).
// Each build is the twin of the LEAN = 3 build of the same budget and row count (sfmstep_robot26.hip, sfmstep_robotx.hip,
// sfmstep_leanrt.hip): 25 and 5 humans + robot, and any other row count with the run-time partner loop.  gfx950 only.
#include "sfmstep_kernel.h"

namespace cstep {

kfn sfm_builds_policy_robot(const Variant& v, int type)
{
    CS_V(64, 1, 26, 11) CS_V(64, 4, 26, 11) CS_V(64, 4, 6, 11) CS_V(64, 3, 0, 11)
    return nullptr;
}

} // namespace cstep
