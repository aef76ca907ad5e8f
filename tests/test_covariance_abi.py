"""CPU-side checks of the covariance entry points (ilqr_get_covariance, ilqr_copy_covariance_to_device): declared, exported, bound,
refusing a null handle without a device -- and the yardstick of tests/test_gpu_covariance.py itself: on every input of its generic and
nx = 4 cases the float64 recursion agrees with np.longdouble within 1e-10 x max(1, max|.|), a factor 10 inside the bound the device is
held to; the inputs neither blow up nor decay over the horizon; and the expected cost equals what the value model predicts."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COV_SYMBOLS = ("ilqr_get_covariance", "ilqr_copy_covariance_to_device")
SIZES = [(32, 16), (20, 5), (8, 3), (17, 17), (24, 20), (32, 32), (6, 1), (6, 2), (4, 1), (4, 2)]


def test_header_library_and_ctypes_table_carry_the_calls():
    from ilqr_amd import capi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ilqr_amd.h")).read(), flags=re.S)
    lib = capi.load()
    for name in COV_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*ilqr_batch\s*\*\s*h\s*,\s*int\s+t0\s*,\s*int\s+n_knots\s*," % name, src), name
        assert hasattr(lib, name) and name in capi.SYMBOLS
        assert len(capi.SYMBOLS[name][1]) == 8 and capi.SYMBOLS[name][1][1:3] == [C.c_int, C.c_int]
    assert lib.ilqr_abi_version() == 6  # additive: the ABI number and ilqr_desc stay


def test_null_handle_is_refused():
    from ilqr_amd import capi
    lib = capi.load()
    buf = np.zeros(16)
    p = buf.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.ilqr_get_covariance(None, 0, 1, p, p, p, None, p) == -1 and b"null handle" in lib.ilqr_last_error()
    assert lib.ilqr_copy_covariance_to_device(None, 0, 1, None, None, buf.ctypes.data, None, None) == -1


@pytest.mark.parametrize("n,m", SIZES)
def test_the_yardstick_has_its_headroom(n, m):
    from tests.test_gpu_covariance import cov_reference, generic_case
    d, k, K, S0, W, (Sg, Su, J) = generic_case(n, m)  # (asserts the 1e-10 agreement with np.longdouble)
    # neither blown up nor decayed over the horizon, and Sigma[T] well away from singular
    assert 1.0 < np.abs(Sg).max() < 100.0, np.abs(Sg).max()
    assert np.linalg.eigvalsh(Sg[:, -1]).min() > 1e-3
    assert np.all(np.isfinite(J)) and np.abs(Su).max() > 1e-3
    # a pure function of (records, K, Sigma0, W): each of them matters
    assert np.abs(cov_reference(d, np.zeros_like(K), S0, W)[0] - Sg).max() > 1e-3
    assert np.abs(cov_reference(d, K, None, W)[0] - Sg).max() > 1e-3 and np.abs(cov_reference(d, K, S0, None)[0] - Sg).max() > 1e-3


def test_yardstick_on_a_scalar_problem():
    """n = m = 1, T = 1, by hand."""
    from tests.test_gpu_covariance import cov_reference
    fx, fu, cxx, cxu, cuu, K, s0, w, cxxT = 0.9, 0.5, 2.0, 0.1, 1.5, -0.7, 0.8, 0.05, 3.0
    d = {name: np.zeros((1, 2, 1, 1)) for name in ("fx", "fu", "cxx", "cxu", "cuu")}
    d.update(cx=np.zeros((1, 2, 1)), cu=np.zeros((1, 2, 1)))
    for name, val in (("fx", fx), ("fu", fu), ("cxx", cxx), ("cxu", cxu), ("cuu", cuu)):
        d[name][0, 0, 0, 0] = val
    d["cxx"][0, 1, 0, 0] = cxxT
    Sg, Su, J = cov_reference(d, np.array([[[[K]]]]), np.array([[[s0]]]), np.array([[[w]]]))
    a = fx + fu * K
    s1 = a * s0 * a + w
    assert Sg[0, 0, 0, 0] == s0 and abs(Sg[0, 1, 0, 0] - s1) < 1e-15 and abs(Su[0, 0, 0, 0] - K * K * s0) < 1e-15
    assert abs(J[0] - (0.5 * (cxx * s0 + cuu * K * K * s0 + 2 * cxu * s0 * K) + 0.5 * cxxT * s1)) < 1e-14


@pytest.mark.parametrize("n,m", SIZES)
def test_expected_cost_is_what_the_value_model_predicts(n, m):
    """J == 1/2 <Vxx[0], Sigma0> + 1/2 sum_t <Vxx[t+1], W>: the forward and the backward recursion describe one quadratic form."""
    from tests.test_gpu_covariance import generic_case
    from tests.test_gpu_value import value_reference
    d, k, K, S0, W, (_, _, J) = generic_case(n, m)
    _, Vxx = value_reference(d, k, K)
    dot = lambda X, Y: (X * Y).sum(axis=(-1, -2))
    want = 0.5 * dot(Vxx[:, 0], S0) + 0.5 * sum(dot(Vxx[:, t + 1], W) for t in range(K.shape[1]))
    assert np.abs(J - want).max() <= 1e-12 * np.abs(want).max(), (np.abs(J - want).max(), np.abs(want).max())


CALLER = r'''
#include "ilqr_amd.hpp"
#include <cmath>
#include <cstdio>
int main() {
  using namespace ilqr_amd;
  const int T = 20;
  VectorXd goal(4);
  goal(0) = 1.0; goal(1) = 0.5; goal(2) = 0.0; goal(3) = 0.0;
  iLQR s(new DoubleIntegrator(goal), 0.02);
  s.verbose = false;
  VectorXd x0(4);
  x0(0) = 0.2; x0(1) = -0.1; x0(2) = 0.0; x0(3) = 0.1;
  VectorXd u(2);
  u(0) = 0.0; u(1) = 0.0;
  VecOfVecXd u0(T, u);
  s.init_traj(x0, u0);
  s.generate_trajectory();
  MatrixXd S0(4, 4), W(4, 4);
  for (int i = 0; i < 4; i++) { S0(i, i) = 0.5 + 0.1 * i; W(i, i) = 0.01; }
  S0(0, 1) = S0(1, 0) = 0.05;
  VecOfMatXd Sg, Su;
  double J = 0;
  s.covariance(S0, W, Sg, &Su, &J);  // with Su: the knots 0 .. T - 1
  if ((int)Sg.size() != T || (int)Su.size() != T || Sg[0].rows() != 4 || Sg[0].cols() != 4 || Su[0].rows() != 2 || Su[0].cols() != 2) return 1;
  VecOfMatXd All;
  s.covariance(S0, W, All);  // Sigma alone: the knots 0 .. T
  if ((int)All.size() != T + 1) return 1;
  double asym = 0, big = 0, first = 0, same = 0;
  for (int t = 0; t < T; t++)
    for (int i = 0; i < 4; i++)
      for (int j = 0; j < 4; j++) {
        asym = std::fmax(asym, std::fabs(Sg[t](i, j) - Sg[t](j, i)));
        big = std::fmax(big, std::fabs(Sg[t](i, j)));
        same = std::fmax(same, std::fabs(Sg[t](i, j) - All[t](i, j)));
        if (t == 0) first = std::fmax(first, std::fabs(Sg[0](i, j) - S0(i, j)));
      }
  VecOfMatXd Win, WinU;
  s.covariance(S0, W, Win, &WinU, nullptr, 3, 2);  // a window
  double win = 0;
  for (int i = 0; i < 4; i++) win = std::fmax(win, std::fabs(Win[1](i, 2) - Sg[4](i, 2)));
  for (int i = 0; i < 2; i++) win = std::fmax(win, std::fabs(WinU[0](i, 1) - Su[3](i, 1)));
  VecOfMatXd Z;
  s.covariance(MatrixXd(), MatrixXd(), Z, nullptr, nullptr, 0, 3);  // no uncertainty, no noise: zero
  double zero = 0;
  for (int t = 0; t < 3; t++)
    for (int i = 0; i < 4; i++) zero = std::fmax(zero, std::fabs(Z[t](i, i)));
  std::printf("knots %d asym %g max %g window %g first %g same %g zero %g J %g\n", (int)Sg.size(), asym, big, win, first, same, zero, J);
  return (asym == 0 && big > 0 && win == 0 && first == 0 && same == 0 && zero == 0 && J > 0 && Win.size() == 2) ? 0 : 2;
}
'''

BATCH_CALLER = r'''
#include "ilqr_amd.hpp"
#include <cmath>
#include <cstdio>
int main() {
  using namespace ilqr_amd;
  const int B = 3, T = 15;
  VectorXd goal(4);
  goal(0) = 1.0; goal(1) = 0.5; goal(2) = 0.0; goal(3) = 0.0;
  BatchILQR b(std::make_shared<DoubleIntegrator>(goal), B, T, 0.02);
  std::vector<double> x0((size_t)B * 4), u0((size_t)B * T * 2, 0.0);
  for (size_t i = 0; i < x0.size(); i++) x0[i] = 0.1 * (double)(i % 5) - 0.2;
  b.init_traj(x0, u0);
  b.iterate(2);
  std::vector<double> S0((size_t)B * 16, 0.0), W((size_t)B * 16, 0.0), Sg, Su, J, Win, OnlyJ;
  for (int t = 0; t < B; t++)
    for (int i = 0; i < 4; i++) { S0[(size_t)t * 16 + 5 * i] = 0.3 + 0.1 * t; W[(size_t)t * 16 + 5 * i] = 0.02; }
  b.covariance(&S0, &W, &Sg, &Su, &J);
  if (Sg.size() != (size_t)B * T * 16 || Su.size() != (size_t)B * T * 4 || J.size() != (size_t)B) return 1;
  b.covariance(&S0, &W, &Win, nullptr, nullptr, 3, 4);
  b.covariance(&S0, &W, nullptr, nullptr, &OnlyJ);
  double win = 0, asym = 0, dj = 0;
  for (int t = 0; t < B; t++) {
    dj = std::fmax(dj, std::fabs(OnlyJ[t] - J[t]));
    for (int s = 0; s < 4; s++)
      for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
          const double v = Sg[((size_t)t * T + 3 + s) * 16 + i + 4 * j];
          win = std::fmax(win, std::fabs(Win[((size_t)t * 4 + s) * 16 + i + 4 * j] - v));
          asym = std::fmax(asym, std::fabs(v - Sg[((size_t)t * T + 3 + s) * 16 + j + 4 * i]));
        }
  }
  std::printf("window %g asym %g dJ %g J0 %g\n", win, asym, dj, J[0]);
  return (win == 0 && asym == 0 && dj == 0 && J[0] > 0) ? 0 : 2;
}
'''


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["iLQR", "BatchILQR"])
def test_facade_covariance_members(tmp_path, which):
    """C++ callers of the facade's covariance(): the single-problem iLQR (Eigen-typed or plain matrices, as value()) and BatchILQR's
    plain vectors; a window is a slice, Sigma[t] is symmetric, Sigma[0] is Sigma0, a J-only call gives the same J."""
    from ilqr_amd import _build
    _build.build()
    src = tmp_path / "covariance_caller.cpp"
    src.write_text(CALLER if which == "iLQR" else BATCH_CALLER)
    exe = str(tmp_path / "covariance_caller")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-DILQR_AMD_NO_EIGEN", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe,
                           "-L" + os.path.join(ROOT, "ilqr_amd", "lib"), "-lilqr_amd", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "ilqr_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


def test_facade_covariance_caller_compiles(tmp_path):
    """The same members compile without a device: a translation unit that only names them."""
    src = tmp_path / "covariance_names.cpp"
    src.write_text(r'''
#include "ilqr_amd.hpp"
void f(ilqr_amd::iLQR& s, ilqr_amd::BatchILQR& b, void* dev) {
  ilqr_amd::MatrixXd S0(4, 4), W; ilqr_amd::VecOfMatXd Sg, Su; double J;
  s.covariance(S0, W, Sg); s.covariance(S0, W, Sg, &Su, &J); s.covariance(S0, W, Sg, nullptr, &J, 0, 1);
  std::vector<double> s0, w, sg, su, j; b.covariance(&s0, &w, &sg, &su, &j); b.covariance(nullptr, nullptr, &sg, nullptr, nullptr, 2, 3);
  b.copy_covariance_to_device(0, 1, dev, nullptr, dev, nullptr, dev);
}
''')
    for extra in (["-DILQR_AMD_NO_EIGEN"], []):  # (without the macro: Eigen's types where Eigen is installed, the stand-ins elsewhere)
        subprocess.check_call(["g++", "-std=c++14", "-O0", "-Wall"] + extra + ["-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "covariance_names.o")])
