// TEST INFRASTRUCTURE ONLY (see hip/hip_runtime.h here): the one definition of the env-owned generator (csrc/sgw_pcg64.hpp) run on
// the host.  tests/test_pcg64_host.py builds it with the host sanitizers, hands it generator states and compares what it prints
// with numpy's Generator(PCG64).
//
//   pcg64_check < lines        every line: <kind> <state_hi> <state_lo> <inc_hi> <inc_lo> <arg> <count>, numbers decimal
//     r  count x random01                                         -> "r <bits of the double> ..."
//     i  count x lemire(arg), then one random01                   -> "i <value> ... <bits of the double>"
//     s  Fisher-Yates from the top over 0 .. arg-1 with interval  -> "s <element> ..."      (the families' shuffle; count unused)
//     g  the same with interval_guarded_clamped                   -> "g <element> ..."
//     R I S  as r i s on Pcg64BufFirst, the member order of firemaker_ex_ma and island_navigation_ex_ma
// Exit 0, or 1 on a line it cannot read.
#define __HIPCC__ 1
#define SGW_PLAIN_STORES 1
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../ai_safety_gridworlds_amd/csrc/sgw_pcg64.hpp"

using namespace sgw;

static uint64_t bits_of(double v) { return (uint64_t)__double_as_longlong(v); }

template <class G> static bool answer(char kind, const uint64_t (&w)[4], uint64_t arg, uint64_t count) {
  G g{};
  g.rs_hi = w[0]; g.rs_lo = w[1]; g.ri_hi = w[2]; g.ri_lo = w[3];
  if (kind == 'r') {
    for (uint64_t k = 0; k < count; ++k) std::printf(" %" PRIu64, bits_of(random01(g)));
  } else if (kind == 'i') {
    for (uint64_t k = 0; k < count; ++k) std::printf(" %d", lemire(g, (uint32_t)arg));
    std::printf(" %" PRIu64, bits_of(random01(g)));
  } else if (kind == 's' || kind == 'g') {
    std::vector<int> x((size_t)arg);
    for (size_t k = 0; k < x.size(); ++k) x[k] = (int)k;
    for (int i = (int)arg - 1; i >= 1; --i) {
      const int j = kind == 's' ? interval(g, (uint32_t)i) : interval_guarded_clamped(g, (uint32_t)i);
      const int t = x[i]; x[i] = x[j]; x[j] = t;
    }
    for (int v : x) std::printf(" %d", v);
  } else {
    return false;
  }
  return true;
}

int main() {
  char kind;
  while (std::scanf(" %c", &kind) == 1) {
    uint64_t w[4], arg = 0, count = 0;
    if (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &w[0], &w[1], &w[2], &w[3], &arg, &count) != 6) return 1;
    std::printf("%c", kind);
    const bool upper = kind >= 'A' && kind <= 'Z';
    if (!(upper ? answer<Pcg64BufFirst>((char)(kind - 'A' + 'a'), w, arg, count) : answer<Pcg64>(kind, w, arg, count))) return 1;
    std::printf("\n");
  }
  return 0;
}
