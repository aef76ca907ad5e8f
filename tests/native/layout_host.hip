// Host build of the product's layout index maps (ilqr_amd/csrc/layout.hpp: __host__ __device__) so that where every element of a
// canonical array lives in a handle's array can be tested on a machine without a GPU.  TEST INFRASTRUCTURE.
#include "../../ilqr_amd/csrc/layout.hpp"
using namespace ilqr;

// out[(b * n + s) * E + e] = map(b, s, e) for the canonical array [B][n][E]
template <class Map>
static void fill(const Map& map, int B, int n, int E, long long* out) {
  for (int b = 0; b < B; b++)
    for (int s = 0; s < n; s++)
      for (int e = 0; e < E; e++) out[((size_t)b * n + s) * E + e] = (long long)map(b, s, e);
}
extern "C" void layout_tiled(int B, int S, int E, int t0, int n, long long* out) { fill(TiledMap{S, E, t0}, B, n, E, out); }
extern "C" void layout_tiled_rec(int B, int S, int REC, int off, int E, int t0, int n, long long* out) { fill(TiledRecMap{S, REC, off, t0}, B, n, E, out); }
extern "C" void layout_aos(int B, int S, int stride, int off, int E, int t0, int n, long long* out) { fill(AosMap{S, stride, off, t0}, B, n, E, out); }
extern "C" long long layout_alloc_elems(int aos, int B, int ntiles, int S, int E) { return (long long)layout_elems(aos != 0, B, ntiles, S, E); }
extern "C" int layout_rec_offsets(int nx, int nu, int* off, int* len) {
  rec_offsets(nx, nu, off, len);
  return rec_size(nx, nu);
}
