// TEST INFRASTRUCTURE ONLY (see hip/hip_runtime.h here): the element rules of the learning calls (csrc/sgw_learn.hpp:
// learn_scores_element over policy_score of sgw_policy.hpp, learn_quantise, learn_apply_element) run on the host.
// tests/test_learn_host.py builds it with the host sanitizers, hands it a file of sections and compares what it writes with
// tests/learn_ref.py.
//
//   learn_check <in> <out>      <in> is a sequence of sections, little-endian, each starting with int64 kind:
//     kind 1, scores:    int64 C, G, NA, rows, has_bias; uint8 code_of[256]; float32 weights[C * G * NA], bias[NA] (with has_bias);
//                        uint8 obs[rows * C]; int32 j[rows] (the index of the action played; outside 0 .. NA-1: none)
//                        -> float32 scores[rows * NA], float64 vmax[rows], float64 chosen[rows]
//     kind 2, quantise:  int64 n, frac_bits; float64 coef[n]                        -> int64 q[n]
//     kind 3, apply:     int64 n, frac_bits; float64 lr; float32 w[n]; int64 acc[n] -> float32 w[n] (acc == 0: not written)
// Every array is allocated at its exact size, so an access past a buffer is a sanitizer report.  Exit 0, or 1 on a bad file.
#define __HIPCC__ 1
#define SGW_PLAIN_STORES 1
#define SGW_LEARN_RULES_ONLY 1
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../ai_safety_gridworlds_amd/csrc/sgw_learn.hpp"

namespace sgw { alignas(16) uint8_t policy_lds[POLICY_MAX_ROW_LDS + 256]; }   // (k_policy_act's dynamic LDS: declared by sgw_policy.hpp, unused here)

using namespace sgw;

template <class T> static bool rd(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}
template <class T> static bool wr(FILE* f, const std::vector<T>& v) { return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

template <int NA> static void score_rows(int rows, int C, int G, const uint8_t* obs, const uint8_t* code_of, const float* w, const float* b,
                                         const int32_t* j, float* scores, double* vmax, double* chosen) {
  for (int r = 0; r < rows; ++r) {
    float s[NA];
    learn_scores_element<NA>(s, vmax[r], chosen[r], obs + (size_t)r * C, C, code_of, true, w, b, G, j[r]);
    for (int k = 0; k < NA; ++k) scores[(size_t)r * NA + k] = s[k];
  }
}

int main(int argc, char** argv) {
  if (argc != 3) return 1;
  FILE* f = std::fopen(argv[1], "rb");
  FILE* o = std::fopen(argv[2], "wb");
  if (!f || !o) return 1;
  for (;;) {
    int64_t kind;
    const size_t got = std::fread(&kind, sizeof(int64_t), 1, f);
    if (got == 0) break;
    if (kind == 1) {
      int64_t h[5];
      if (std::fread(h, sizeof(int64_t), 5, f) != 5) return 1;
      const int C = (int)h[0], G = (int)h[1], NA = (int)h[2], rows = (int)h[3];
      if (C < 0 || C > 4096 || G < 1 || G > 64 || NA < 1 || NA > POLICY_MAX_ACTIONS || rows < 0 || rows > 4096) return 1;
      std::vector<uint8_t> code_of, obs;
      std::vector<float> w, b;
      std::vector<int32_t> j;
      if (!rd(f, code_of, 256) || !rd(f, w, (size_t)C * G * NA) || !rd(f, b, h[4] ? (size_t)NA : 0) || !rd(f, obs, (size_t)rows * C) ||
          !rd(f, j, (size_t)rows))
        return 1;
      for (uint8_t g : code_of) if (g >= G) return 1;
      std::vector<float> scores((size_t)rows * NA);
      std::vector<double> vmax((size_t)rows), chosen((size_t)rows);
      const float* bp = h[4] ? b.data() : nullptr;
      switch (NA) {
#define CASE(K) case K: score_rows<K>(rows, C, G, obs.data(), code_of.data(), w.data(), bp, j.data(), scores.data(), vmax.data(), chosen.data()); break;
        CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10) CASE(11) CASE(12) CASE(13) CASE(14) CASE(15) CASE(16)
#undef CASE
      }
      if (!wr(o, scores) || !wr(o, vmax) || !wr(o, chosen)) return 1;
    } else if (kind == 2) {
      int64_t h[2];
      if (std::fread(h, sizeof(int64_t), 2, f) != 2 || h[0] < 0 || h[0] > (1 << 20) || h[1] < 0 || h[1] > 52) return 1;
      std::vector<double> coef;
      if (!rd(f, coef, (size_t)h[0])) return 1;
      std::vector<int64_t> q(coef.size());
      const double scale = std::ldexp(1.0, (int)h[1]);
      for (size_t i = 0; i < coef.size(); ++i) q[i] = learn_quantise(coef[i], scale);
      if (!wr(o, q)) return 1;
    } else if (kind == 3) {
      int64_t h[2];
      double lr;
      if (std::fread(h, sizeof(int64_t), 2, f) != 2 || h[0] < 0 || h[0] > (1 << 20) || h[1] < 0 || h[1] > 52) return 1;
      if (std::fread(&lr, sizeof(double), 1, f) != 1) return 1;
      std::vector<float> w;
      std::vector<int64_t> acc;
      if (!rd(f, w, (size_t)h[0]) || !rd(f, acc, (size_t)h[0])) return 1;
      const double inv = std::ldexp(1.0, -(int)h[1]);
      for (size_t i = 0; i < w.size(); ++i)
        if (acc[i] != 0) w[i] = learn_apply_element(w[i], acc[i], lr, inv);
      if (!wr(o, w)) return 1;
    } else {
      return 1;
    }
  }
  std::fclose(f);
  return std::fclose(o) == 0 ? 0 : 1;
}
