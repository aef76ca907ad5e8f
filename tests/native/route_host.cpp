// Host build of the product's route plan (ilqr_amd/csrc/route.hpp: host code only) so the kernel a handle runs for each stage can be
// tested on a machine without a GPU.  TEST INFRASTRUCTURE.
#include "../../ilqr_amd/csrc/route.hpp"
using namespace ilqr;

// names[ILQR_NUM_STAGES]: what ilqr_stage_kernel_name reports for a handle created from these inputs.  cands_allocated < 0: as
// ilqr_create allocates the LQ search's candidate buffers when the device can spare them.
extern "C" void route_kernel_names(int model, int nx, int nu, int flags, int route, int ntiles, int num_cus, int user_tiled, int user_small,
                                   int cands_allocated, const char** names) {
  const bool cands = cands_allocated < 0 ? lq_matrix_core_search(model, nu, route) && !(route & ILQR_ROUTE_LQ_RECOMMIT) : cands_allocated != 0;
  const RoutePlan p = plan_route({model, nx, nu, flags, route, ntiles, num_cus, user_tiled != 0, user_small != 0, cands});
  for (int s = 0; s < ILQR_NUM_STAGES; s++) names[s] = stage_kernel_name(p, s);
}

// out[6] = {nt, mt, full, lqf, regv, f32}: the k_backward_w3 instantiation (nt: also k_backward_w2's) of a generic handle created from
// these inputs, while its backward pass reads the model's own records (no ilqr_set_derivatives); returns the value kernel's name
extern "C" const char* route_wave_variants(int model, int nx, int nu, int flags, int route, int dtype, int* out) {
  const bool cands = lq_matrix_core_search(model, nu, route) && !(route & ILQR_ROUTE_LQ_RECOMMIT);
  const RoutePlan p = plan_route({model, nx, nu, flags, route, 4, 256, false, false, cands, dtype});
  const WaveVariant w = backward_wave_variant(p.backward, nx, nu, dtype, p.derivatives == Derivatives::fused_lq);
  const int fields[6] = {w.nt, w.mt, w.full, w.lqf, w.regv, w.f32};
  for (int i = 0; i < 6; i++) out[i] = fields[i];
  return value_kernel_name(generic_layout(model, route, false, false), value_wave_variant(nx, nu, dtype));
}

// ... for a null handle
extern "C" void route_default_names(const char** names) {
  for (int s = 0; s < ILQR_NUM_STAGES; s++) names[s] = stage_kernel_name(RoutePlan{}, s);
}
