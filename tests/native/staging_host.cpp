// Host build of the product's staging plans (ilqr_amd/csrc/staging.hpp: host code only) so the layout every host getter gives its arrays in
// the staging buffer can be tested on a machine without a GPU.  TEST INFRASTRUCTURE.
#include <stdint.h>

#include "../../ilqr_amd/csrc/staging.hpp"
using namespace ilqr;

// The getters' own declarations are called with pointers that are only ever compared with null: bit i of `mask` set = the i-th pointer
// argument is given.  Resolved against a made-up buffer address, never dereferenced.
static double* const kBase = reinterpret_cast<double*>(uintptr_t(1) << 32);
template <class T>
static T* given(unsigned mask, int i) {
  return (mask >> i & 1) ? reinterpret_cast<T*>(uintptr_t(0x1000) * (i + 1)) : nullptr;
}
// out[0] = segments, out[1] = total (doubles), then per segment {offset (doubles), room (doubles), bytes copied, up, ints, device pointer as
// a byte offset into the buffer or -1 for null}
static void report(StagePlan p, long long* out) {
  p.resolve(kBase);
  out[0] = p.n, out[1] = (long long)p.total;
  for (int i = 0; i < p.n; i++) {
    const StageSeg& s = p.seg[i];
    long long* o = out + 2 + 6 * i;
    o[0] = (long long)s.offset, o[1] = (long long)s.doubles(), o[2] = (long long)s.bytes(), o[3] = s.up, o[4] = s.ints;
    o[5] = s.dev ? (long long)(reinterpret_cast<const char*>(s.dev) - reinterpret_cast<const char*>(kBase)) : -1;
  }
}
#define D(i) given<double>(mask, i)

extern "C" {
int stage_max_segments(void) { return StagePlan::kMaxSegs; }
// dims[5] = {B, T, nx, nu, NTP}
void stage_value_plan(const size_t* d, size_t t0, size_t nk, size_t nd, size_t ny, size_t nw, size_t ns, unsigned mask, long long* out) {
  report(stage_value({d[0], d[1], d[2], d[3], d[4]}, nk, D(0), D(1)), out);
}
void stage_covariance_plan(const size_t* d, size_t t0, size_t nk, size_t nd, size_t ny, size_t nw, size_t ns, unsigned mask, long long* out) {
  report(stage_covariance({d[0], d[1], d[2], d[3], d[4]}, nk, D(0), D(1), D(2), D(3), D(4)), out);
}
void stage_tangent_plan(const size_t* d, size_t t0, size_t nk, size_t nd, size_t ny, size_t nw, size_t ns, unsigned mask, long long* out) {
  report(stage_tangent({d[0], d[1], d[2], d[3], d[4]}, t0, nk, nd, D(0), D(1), D(2), D(3)), out);
}
void stage_adjoint_plan(const size_t* d, size_t t0, size_t nk, size_t nd, size_t ny, size_t nw, size_t ns, unsigned mask, long long* out) {
  report(stage_adjoint({d[0], d[1], d[2], d[3], d[4]}, t0, nk, nd, D(0), D(1), D(2), D(3)), out);
}
void stage_lq_solve_plan(const size_t* d, size_t t0, size_t nk, size_t nd, size_t ny, size_t nw, size_t ns, unsigned mask, long long* out) {
  report(stage_lq_solve({d[0], d[1], d[2], d[3], d[4]}, nd, D(0), D(1), D(2), D(3), D(4), D(5), given<int>(mask, 6)), out);
}
void stage_estimator_plan(const size_t* d, size_t t0, size_t nk, size_t nd, size_t ny, size_t nw, size_t ns, unsigned mask, long long* out) {
  report(stage_estimator({d[0], d[1], d[2], d[3], d[4]}, nk, ny, D(0), D(1), D(2), D(3), D(4), D(5), D(6), D(7), D(8), D(9), given<int>(mask, 10)), out);
}
void stage_risk_plan(const size_t* d, size_t t0, size_t nk, size_t nd, size_t ny, size_t nw, size_t ns, unsigned mask, long long* out) {
  report(stage_risk({d[0], d[1], d[2], d[3], d[4]}, nw, D(0), D(1), D(2), D(3), D(4), D(5), given<int>(mask, 6)), out);
}
void stage_evaluate_plan(const size_t* d, size_t t0, size_t nk, size_t nd, size_t ny, size_t nw, size_t ns, unsigned mask, long long* out) {
  report(stage_evaluate({d[0], d[1], d[2], d[3], d[4]}, ns, D(0), D(1), D(2), D(3)), out);
}
void stage_param_gradient_plan(const size_t* d, size_t t0, size_t nk, size_t nd, size_t ny, size_t nw, size_t ns, unsigned mask, long long* out) {
  report(stage_param_gradient({d[0], d[1], d[2], d[3], d[4]}, nd, D(0), D(1), D(2), D(3), D(4)), out);
}
}
