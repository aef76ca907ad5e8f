// pass_driver.hpp -- what surrounds a backward pass (src/ilqr_core.cpp:136-159), stated once for every chain: how lambda is
// raised after a pass in which a box-QP failed, the term of the gradient norm, and the constant of the early exit.
//
// Every helper here is straight-line arithmetic on values.  That is on purpose: a helper with control flow of its own (the
// retry loop, the "gnorm < tolGrad && lambda < 1e-5" test, the write-out under `mode == 1`) reaches the chain in another shape
// than the same text written in place (a function is simplified by itself before it is inlined, it seems), and the register
// allocation of the chain's step loop moves with it (profiles/pass_driver_isa.txt: every such form that was tried, kernel by
// kernel).  With these, every kernel is the instructions it was.  The loop around a pass and the write-out stay with
// the chains (backward_quad.hpp, backward_hex.hpp, kernels_wide.hpp, kernels_wide2.hpp, backward_thread.hpp,
// backward_wave2.hpp, backward_wave3.hpp) and call in here for what they decide.
// Device code: not for boxqp.hpp, layout.hpp or route.hpp, which tests/native compiles for the host.
#pragma once
#include "common.hpp"

namespace ilqr {

// ilqr_core.cpp:142-148  a box-QP failed in the pass: dlambda, then lambda, go up; the pass runs again unless lambda has
// passed lambda_max.   dlambda = raised_dlambda(dlambda, sp);  lambda = raised_lambda(lambda, dlambda, sp);
__device__ __forceinline__ double raised_dlambda(double dlambda, const SolverParams& sp) {
  return fmax(dlambda * sp.lambda_factor, sp.lambda_factor);
}
__device__ __forceinline__ double raised_lambda(double lambda, double dlambda, const SolverParams& sp) {
  return fmax(lambda * dlambda, sp.lambda_min);
}
// (STEP 4's schedule after a line search is accept_one's, rollout.hpp: another statement of the reference, :242-282)

// ilqr_core.cpp:154  "gnorm < tolGrad and lambda < 1e-5" ends a trajectory in STEP 2
constexpr double kLambdaConverged = 1e-5;

}  // namespace ilqr
