// TEST INFRASTRUCTURE ONLY: the seeding arithmetic of csrc/sgw_seed.hpp run on the host.  tests/test_seed_rng_host.py builds it
// with the host sanitizers, feeds it seeds and compares what it prints with numpy and zlib.
//
//   seed_check < lines
//     p <seed> <flags>                    -> "p <state_hi> <state_lo> <inc_hi> <inc_lo>"   (resolve_seed without layout, then PCG64)
//     c <original_seed> <layout_seed>     -> "c <crc32>"
//     l <seed> <layout_seed> <flags>      -> "l <resolved seed> <state_hi> <state_lo> <inc_hi> <inc_lo>"
//     b <base> <index> <flags>            -> "b <resolved seed>"                           (the seeds == NULL form, mod 2^64)
// All numbers decimal, unsigned 64-bit.  Exit 0, or 1 on a line it cannot read.
#include <cinttypes>
#include <cstdio>

#include "../../ai_safety_gridworlds_amd/csrc/sgw_seed.hpp"

int main() {
  char kind;
  while (std::scanf(" %c", &kind) == 1) {
    uint64_t a = 0, b = 0, c = 0, w[4];
    if (kind == 'p') {
      if (std::scanf("%" SCNu64 " %" SCNu64, &a, &b) != 2) return 1;
      sgw::pcg64_from_seed(sgw::resolve_seed(&a, 0, nullptr, (int)b, 0), w);
      std::printf("p %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", w[0], w[1], w[2], w[3]);
    } else if (kind == 'c') {
      if (std::scanf("%" SCNu64 " %" SCNu64, &a, &b) != 2) return 1;
      std::printf("c %" PRIu32 "\n", sgw::layout_seed((uint32_t)a, (uint32_t)b));
    } else if (kind == 'l') {
      if (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64, &a, &b, &c) != 3) return 1;
      const uint32_t layout = (uint32_t)b;
      const uint64_t s = sgw::resolve_seed(&a, 0, &layout, (int)c, 0);
      sgw::pcg64_from_seed(s, w);
      std::printf("l %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", s, w[0], w[1], w[2], w[3]);
    } else if (kind == 'b') {
      if (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64, &a, &b, &c) != 3) return 1;
      std::printf("b %" PRIu64 "\n", sgw::resolve_seed(nullptr, a, nullptr, (int)c, (long long)b));
    } else {
      return 1;
    }
  }
  return 0;
}
