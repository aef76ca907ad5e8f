// Host build of the sizes of k_solve_hex's LDS rings (ilqr_amd/csrc/backward_hex.hpp: HexRing, HexRingSize, HexPair), so that the
// bounds the chain / producer protocol rests on can be tested on a machine without a GPU.  Compiling this file is part of the test:
// the header's static_asserts are checked for the four rings the library instantiates.
// TEST INFRASTRUCTURE.
#include "../../ilqr_amd/csrc/backward_hex.hpp"
using namespace ilqr;

template <class real, bool COMPACT>
static void fill(int* out) {
  using P = HexPair<real, 4, 1, COMPACT>;
  using S = HexRingSize<4, 1, real, COMPACT>;
  out[0] = P::RS::SLOTS;
  out[1] = P::LEAD;
  out[2] = S::STALE;
  out[3] = P::RS::ELEMS;
  out[4] = (int)sizeof(real);
  out[5] = S::TERM;
  out[6] = S::FIT;
  out[7] = (int)sizeof(P);
  out[8] = P::RS::Z;
  out[9] = P::RS::PAIRS * P::RS::ROW;
}
// out[10]: SLOTS, LEAD, STALE, ELEMS (`real`s per slot), sizeof(real), TERM (`real`s of the knot-T area), FIT (slots the bytes
// would hold), sizeof(HexPair), the largest element offset a load adds to a lane's address inside a slot (Z), `real`s of the pair rows
extern "C" void hex_ring_sizes(int is_float, int compact, int* out) {
  if (is_float)
    compact ? fill<float, true>(out) : fill<float, false>(out);
  else
    compact ? fill<double, true>(out) : fill<double, false>(out);
}
extern "C" int hex_slot_phases() { return kHexSlotPhases; }
extern "C" int hex_knots_per_round() { return kHexKnotsPerRound; }
extern "C" int hex_full_slots() { return kHexFullSlots; }
