// TEST INFRASTRUCTURE ONLY (see hip/hip_runtime.h here): the one definition of a table policy's choice (csrc/sgw_policy.hpp,
// policy_choose: score, greedy scan, exploration draw) run on the host.  tests/test_policy_host.py builds it with the host
// sanitizers, hands it a file of cases and compares what it prints with tests/policy_ref.py.
//
//   policy_check <file>      the file is a sequence of cases, little-endian:
//     int64   C, G, NA, rows, has_bias, n_explore, seed, step, agent, env_id0
//     uint64  explore_below[n_explore]
//     uint8   code_of[256]
//     float32 weights[C * G * NA], bias[NA] (when has_bias)
//     uint8   obs[rows * C]
//   per case and explore_below one line: the action index of every row (row r is env env_id0 + r).
// Exit 0, or 1 on a file it cannot read.
#define __HIPCC__ 1
#define SGW_PLAIN_STORES 1
#include <cstdio>
#include <vector>

#include "../../ai_safety_gridworlds_amd/csrc/sgw_policy.hpp"

namespace sgw { alignas(16) uint8_t policy_lds[POLICY_MAX_ROW_LDS + 256]; }   // (the kernel's dynamic LDS: declared by the header, unused here)

using namespace sgw;

template <class T> static bool rd(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

template <int NA> static int choose(const uint8_t* o, int C, const uint8_t* code_of, const float* w, const float* b, int G,
                                    uint64_t below, uint64_t seed, long long env, long long step, int agent) {
  return policy_choose<NA>(o, C, code_of, w, b, G, below, seed, env, step, agent);
}

int main(int argc, char** argv) {
  if (argc != 2) return 1;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 1;
  for (;;) {
    int64_t h[10];
    const size_t got = std::fread(h, sizeof(int64_t), 10, f);
    if (got == 0) break;
    if (got != 10) return 1;
    const int C = (int)h[0], G = (int)h[1], NA = (int)h[2], rows = (int)h[3];
    if (C < 0 || G < 1 || G > 64 || NA < 1 || NA > POLICY_MAX_ACTIONS || rows < 0 || h[5] < 0) return 1;
    std::vector<uint64_t> below;
    std::vector<uint8_t> code_of, obs;
    std::vector<float> w, b;
    if (!rd(f, below, (size_t)h[5]) || !rd(f, code_of, 256) || !rd(f, w, (size_t)C * G * NA) || !rd(f, b, h[4] ? (size_t)NA : 0) ||
        !rd(f, obs, (size_t)rows * C))
      return 1;
    for (uint8_t g : code_of) if (g >= G) return 1;
    for (uint64_t eb : below) {
      for (int r = 0; r < rows; ++r) {
        const uint8_t* o = obs.data() + (size_t)r * C;
        const float* bp = h[4] ? b.data() : nullptr;
        const long long env = h[9] + r;
        int act = -1;
        switch (NA) {
#define CASE(K) case K: act = choose<K>(o, C, code_of.data(), w.data(), bp, G, eb, (uint64_t)h[6], env, h[7], (int)h[8]); break;
          CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10) CASE(11) CASE(12) CASE(13) CASE(14) CASE(15) CASE(16)
#undef CASE
        }
        std::printf("%s%d", r ? " " : "", act);
      }
      std::printf("\n");
    }
  }
  std::fclose(f);
  return 0;
}
