// forces_ref.h -- the SFM / HSFM force laws in the reference's own form, each stated ONCE for the kernels that follow the reference
// operation by operation: rk45.hip, robot_model.h / robot_model.hip (and through pair_term the robot of the fused crowd launches and
// the no-train policies) and sfmstep_f64.hip.  (The headline step kernels state the pair law in another algebraic form, stepcommon.h.)
//   social_gym/src/forces.py:9-16, 27-53, 63-128, 153-218, 279-290   the single-agent functions
//   social_gym/src/forces_parallel.py:23-40, 60-83, 109-130, 136-162  the same laws over arrays;  utils.py:7-13 bound_angle
// P: an agent's 20 parameters (agent.py:269): 0 relaxation_time 1 Ai 2 Aw 3 Bi 4 Bw 5 Ci 6 Cw 7 Di 8 Dw 9 Ei 10 k1 11 k2 12 lambda
// 13 gamma 14 ns 15 ns1 16 ko 17 kd 18 alpha 19 k_lambda;  soc = type % 3: 0 Helbing, 1 Guo, 2 Moussaid.
//
// What differs between the users is a math policy M of the pair law -- Libm<float> (rk45's crowd), FastF (robot_model.h), CrD (float64) --
// and floating-point contraction, which belongs to the text of a function and not to its caller: the laws (forces_ref_laws.inc) are read twice, as
// fref::fused (the compiler may form fma, as in the kernels that stated them inline) and as fref::strict (every operation one IEEE
// operation, what robot_model.h and the float64 kernel promise).  A caller names the mode it had.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "atan2_cr.h"

namespace fref {

// utils.py:7-13
template <class T> __device__ __forceinline__ T bound_angle(T a)
{
    constexpr T two_pi = T(2.0 * M_PI), pi = T(M_PI);
    if (a >= two_pi) a = fmod(a, two_pi);
    if (a <= -two_pi) a = fmod(a, two_pi);
    if (a > pi) a -= two_pi;
    if (a < -pi) a += two_pi;
    return a;
}

// max(0, x) as each precision has always taken it
__device__ __forceinline__ float pos(float x) { return fmaxf(0.0f, x); }
__device__ __forceinline__ double pos(double x) { return x > 0 ? x : 0.0; }

} // namespace fref

#define FREF_MODE fused
#define FREF_FP
#include "forces_ref_laws.inc"
#undef FREF_MODE
#undef FREF_FP
#define FREF_MODE strict
#define FREF_FP _Pragma("clang fp contract(off)")
#include "forces_ref_laws.inc"
#undef FREF_MODE
#undef FREF_FP
