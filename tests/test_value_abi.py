"""CPU-side checks of the value-model entry points (ilqr_get_value, ilqr_copy_value_to_device): declared, exported, bound, refusing a
null handle without a device -- and the yardstick of tests/test_gpu_value.py itself: on every input of its generic cases the float64
recursion agrees with np.longdouble within 1e-10 x max(1, max|.|), a factor 10 inside the bound the device is held to."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUE_SYMBOLS = ("ilqr_get_value", "ilqr_copy_value_to_device")


def test_header_library_and_ctypes_table_carry_the_calls():
    from ilqr_amd import capi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ilqr_amd.h")).read(), flags=re.S)
    lib = capi.load()
    for name in VALUE_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*ilqr_batch\s*\*\s*h\s*,\s*int\s+t0\s*,\s*int\s+n_knots\s*," % name, src), name
        assert hasattr(lib, name) and name in capi.SYMBOLS
    assert capi.SYMBOLS["ilqr_get_value"][1][1:3] == [C.c_int, C.c_int]
    assert lib.ilqr_abi_version() == 6  # additive: the ABI number and ilqr_desc stay


def test_null_handle_is_refused():
    from ilqr_amd import capi
    lib = capi.load()
    buf = np.zeros(16)
    p = buf.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.ilqr_get_value(None, 0, 1, p, p) == -1 and b"null handle" in lib.ilqr_last_error()
    assert lib.ilqr_copy_value_to_device(None, 0, 1, buf.ctypes.data, buf.ctypes.data) == -1


@pytest.mark.parametrize("n,m", [(32, 16), (20, 5), (8, 3), (17, 17), (24, 20), (32, 32), (6, 1), (6, 2)])
def test_the_yardstick_has_its_headroom(n, m):
    from tests.test_gpu_value import random_policy, reference_with_headroom, value_reference
    d, k, K = random_policy(n, m)
    Vx, Vxx = reference_with_headroom(d, k, K)
    assert 1e-3 < np.abs(Vxx).max() < 1e6 and np.all(np.isfinite(Vx))  # neither decayed nor blown up over the horizon
    # a pure function of (records, k, K): the gains matter
    Vx0, _ = value_reference(d, np.zeros_like(k), np.zeros_like(K))
    assert np.abs(Vx0 - Vx).max() > 1e-3


def test_yardstick_on_a_scalar_problem():
    """n = m = 1, T = 1, by hand: Vx[0] = Qx + K Quu k + K Qu + Qux k, Vxx[0] = Qxx + K Quu K + 2 K Qux."""
    from tests.test_gpu_value import value_reference
    fx, fu, cx, cu, cxx, cxu, cuu, k, K = 0.9, 0.5, 0.3, -0.2, 2.0, 0.1, 1.5, 0.4, -0.7
    cxT, cxxT = 1.1, 3.0
    d = {name: np.zeros((1, 2, 1, 1)) for name in ("fx", "fu", "cxx", "cxu", "cuu")}
    d.update(cx=np.array([[[cx], [cxT]]]), cu=np.array([[[cu], [0.0]]]))
    for name, val in (("fx", fx), ("fu", fu), ("cxx", cxx), ("cxu", cxu), ("cuu", cuu)):
        d[name][0, 0, 0, 0] = val
    d["cxx"][0, 1, 0, 0] = cxxT
    Vx, Vxx = value_reference(d, np.array([[[k]]]), np.array([[[[K]]]]))
    Qx, Qu, Qxx, Qux, Quu = cx + fx * cxT, cu + fu * cxT, cxx + fx * cxxT * fx, cxu + fu * cxxT * fx, cuu + fu * cxxT * fu
    assert abs(Vx[0, 0, 0] - (Qx + K * Quu * k + K * Qu + Qux * k)) < 1e-14
    assert abs(Vxx[0, 0, 0, 0] - (Qxx + K * Quu * K + 2 * K * Qux)) < 1e-14
    assert Vx[0, 1, 0] == cxT and Vxx[0, 1, 0, 0] == cxxT


@pytest.mark.gpu
def test_facade_value_members(tmp_path):
    """A C++ caller of the facade's value(): the single-problem iLQR (Eigen-typed or plain vectors, as gains_K) and BatchILQR's plain
    vectors give the same numbers; Vxx[t] is symmetric for t < T."""
    from ilqr_amd import _build
    _build.build()
    src = tmp_path / "value_caller.cpp"
    src.write_text(r'''
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
  VecOfVecXd Vx;
  VecOfMatXd Vxx;
  s.value(Vx, Vxx);
  if ((int)Vx.size() != T + 1 || (int)Vxx.size() != T + 1 || Vxx[0].rows() != 4 || Vxx[0].cols() != 4) return 1;
  double asym = 0, big = 0;
  for (int t = 0; t < T; t++)
    for (int i = 0; i < 4; i++)
      for (int j = 0; j < 4; j++) {
        asym = std::fmax(asym, std::fabs(Vxx[t](i, j) - Vxx[t](j, i)));
        big = std::fmax(big, std::fabs(Vxx[t](i, j)));
      }
  VecOfVecXd Wx;
  VecOfMatXd Wxx;
  s.value(Wx, Wxx, 3, 2);  // a window
  double win = 0;
  for (int i = 0; i < 4; i++) win = std::fmax(win, std::fabs(Wx[1](i) - Vx[4](i)) + std::fabs(Wxx[0](i, 2) - Vxx[3](i, 2)));
  std::printf("knots %d asym %g max %g window %g\n", (int)Vx.size(), asym, big, win);
  return (asym == 0 && big > 0 && win == 0 && Wx.size() == 2) ? 0 : 2;
}
''')
    exe = str(tmp_path / "value_caller")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-DILQR_AMD_NO_EIGEN", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe,
                           "-L" + os.path.join(ROOT, "ilqr_amd", "lib"), "-lilqr_amd", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "ilqr_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


def test_facade_value_caller_compiles(tmp_path):
    """The same members compile without a device: a translation unit that only names them."""
    src = tmp_path / "value_names.cpp"
    src.write_text(r'''
#include "ilqr_amd.hpp"
void f(ilqr_amd::iLQR& s, ilqr_amd::BatchILQR& b, void* dev) {
  ilqr_amd::VecOfVecXd Vx; ilqr_amd::VecOfMatXd Vxx; s.value(Vx, Vxx); s.value(Vx, Vxx, 0, 1);
  std::vector<double> vx, vxx; b.value(&vx, &vxx); b.value(&vx, nullptr, 2, 3); b.copy_value_to_device(0, 1, dev, nullptr);
}
''')
    subprocess.check_call(["g++", "-std=c++14", "-O0", "-Wall", "-DILQR_AMD_NO_EIGEN", "-I" + os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "value_names.o")])
