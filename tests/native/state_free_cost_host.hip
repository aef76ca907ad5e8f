// Host-side instantiation of the finite-difference helpers of the derivative sweep (derivatives.hpp: fd_gradient and fd_hessian
// are __host__ __device__, and so is the acrobot's running cost) on the cx, cxx and cxu of one knot t < T, as derivatives_of_knot
// calls them for a full record (cxu: its four-point stencil, copied -- the sweep has it inline) -- next to the one number the
// compact ring record carries in their place.  TEST INFRASTRUCTURE.
#include "../../ilqr_amd/csrc/derivatives.hpp"
using namespace ilqr;

// derivatives.cpp:114-144: the four-point stencil of d2 f / dx_i du_j
template <int NX, int NU, class real, class F>
static real fd_cross(const real* x, const real* u, int i, int j, F f) {
  real px[NX], mx[NX], pu[NU], mu[NU];
#pragma unroll
  for (int q = 0; q < NX; q++) px[q] = mx[q] = x[q];
#pragma unroll
  for (int q = 0; q < NU; q++) pu[q] = mu[q] = u[q];
  px[i] += real(kEps);
  mx[i] -= real(kEps);
  pu[j] += real(kEps);
  mu[j] -= real(kEps);
  return (f(px, pu) - f(mx, pu) - f(px, mu) + f(mx, mu)) * real(1.0 / (4 * (kEps * kEps)));
}


template <class real>
static void dropped(const real* x, real u0, real* out /* cx[4], cxx[16], cxu[4], then c - c */) {
  static_assert(state_free_running_cost<AcrobotModelT<real>>::value, "the acrobot's running cost ignores the state");
  AcrobotModelT<real> m{};
  const real u[1] = {u0};
  fd_gradient<4>(x, [&](const real* xx) { return m.cost(xx, u); }, out);
  fd_hessian<4>(x, [&](const real* xx) { return m.cost(xx, u); }, out + 4);
  for (int i = 0; i < 4; i++) out[20 + i] = fd_cross<4, 1>(x, u, i, 0, [&](const real* xx, const real* uu) { return m.cost(xx, uu); });
  const real c = m.cost(x, u);
  out[24] = c - c;
}
extern "C" void devfn_acrobot_dropped_entries(const double* x, double u, double* out) { dropped<double>(x, u, out); }
// (a float handle takes its finite differences in double -- MFD is the model's double twin -- so the sweep never runs this
//  instantiation; it is here to show that the claim does not rest on the arithmetic)
extern "C" void devfn_acrobot_dropped_entries_f32(const float* x, float u, float* out) { dropped<float>(x, u, out); }
