// tests/native/user_model_coupled4.hpp -- a TEST twin (ILQR_MODEL_USER), not an example: a four-state linear-quadratic model whose
// running cost couples state and control,
//
//     xdot = A x + B u,   cost = 0.5 x'Qx + 0.5 u'Ru + x'N u,   final_cost = 0.5 x'Qf x,
//
// so that the finite differences of the lane-quad kernels (k_derivatives, the sweeps of the persistent routes) produce a cxu that is
// not zero, and every backward pass of the nx = 4 routes -- k_backward_q, k_backward_t, the fused sweeps, k_solve_tile, k_solve_hex's
// ring record, the wide tiles -- starts Qux from a cxu' that matters.  Both shipped nx = 4 models have cxu = 0.
//   NU: ILQR_COUPLED4_NU (1 unless defined; user_model_coupled4_nu2.hpp defines it as 2)
//   user_params: A [4][4], B [4][NU], Q [4][4], R [NU][NU], Qf [4][4], N [4][NU], row-major; with fewer values: A = B = N = 0, Q = R = Qf = I
// (tests/test_gpu_coupled_twin.py; the oracle's twin is Model("lq", ..., cross=N), oracle/orc_models.inc)
#ifndef ILQR_COUPLED4_NU
#define ILQR_COUPLED4_NU 1
#endif
template <class real_>
struct UserModelT {
  using real = real_;
  static constexpr int NX = 4;
  static constexpr int NU = ILQR_COUPLED4_NU;
  real u_min[NU], u_max[NU];  // filled by ilqr_create from ilqr_desc.u_min / u_max
  real A[NX][NX], B[NX][NU], Q[NX][NX], R[NU][NU], Qf[NX][NX], N[NX][NU];

  void set_params(const double* p, int n) {  // host side: ilqr_desc.user_params
    const int oB = NX * NX, oQ = oB + NX * NU, oR = oQ + NX * NX, oQf = oR + NU * NU, oN = oQf + NX * NX, need = oN + NX * NU;
    const bool have = n >= need;
    for (int i = 0; i < NX; i++)
      for (int j = 0; j < NX; j++) {
        A[i][j] = have ? (real)p[i * NX + j] : real(0);
        Q[i][j] = have ? (real)p[oQ + i * NX + j] : real(i == j);
        Qf[i][j] = have ? (real)p[oQf + i * NX + j] : real(i == j);
      }
    for (int i = 0; i < NX; i++)
      for (int j = 0; j < NU; j++) {
        B[i][j] = have ? (real)p[oB + i * NU + j] : real(0);
        N[i][j] = have ? (real)p[oN + i * NU + j] : real(0);
      }
    for (int i = 0; i < NU; i++)
      for (int j = 0; j < NU; j++) R[i][j] = have ? (real)p[oR + i * NU + j] : real(i == j);
  }

  __device__ __forceinline__ void dynamics(const real* x, const real* u, real* dx) const {
#pragma clang fp contract(on)  // every inlined copy must round identically (commit / getter re-integrate from checkpoints)
#pragma unroll
    for (int i = 0; i < NX; i++) {
      real acc = 0;
#pragma unroll
      for (int j = 0; j < NX; j++) acc += A[i][j] * x[j];
#pragma unroll
      for (int j = 0; j < NU; j++) acc += B[i][j] * u[j];
      dx[i] = acc;
    }
  }
  template <int K>
  __device__ __forceinline__ real quad(const real (&M)[K][K], const real* v) const {
#pragma clang fp contract(on)
    real s = 0;
#pragma unroll
    for (int i = 0; i < K; i++) {
      real r = 0;
#pragma unroll
      for (int j = 0; j < K; j++) r += M[i][j] * v[j];
      s += v[i] * r;
    }
    return s;
  }
  __device__ __forceinline__ real cost(const real* x, const real* u) const {
#pragma clang fp contract(on)
    real c = real(0.5) * (quad<NX>(Q, x) + quad<NU>(R, u));
#pragma unroll
    for (int i = 0; i < NX; i++) {  // + x'N u
      real r = 0;
#pragma unroll
      for (int j = 0; j < NU; j++) r += N[i][j] * u[j];
      c += x[i] * r;
    }
    return c;
  }
  __device__ __forceinline__ real final_cost(const real* x) const {
#pragma clang fp contract(on)
    return real(0.5) * quad<NX>(Qf, x);
  }
  // (no analytic_record: finite differences only -- the point of this twin is the cxu they produce)
};
