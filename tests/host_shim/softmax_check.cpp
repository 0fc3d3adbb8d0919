// TEST INFRASTRUCTURE ONLY (see hip/hip_runtime.h here): the element rules of the softmax table policy (csrc/sgw_softmax.hpp:
// softmax_exp2, softmax_weights, softmax_choose, softmax_pi, softmax_grad, over policy_score of sgw_policy.hpp) run on the host.
// tests/test_softmax_host.py builds it with the host sanitizers, hands it a file of sections and compares what it writes with
// tests/softmax_ref.py.
//
//   softmax_check <in> <out>    <in> is a sequence of sections, little-endian, each starting with int64 kind:
//     kind 1, exp2:  int64 n; float32 z[n] (every z <= 0 or NaN)                         -> float32 E[n]
//     kind 2, rows:  int64 C, G, NA, rows, has_bias, frac_bits, step, agent; uint64 explore_below, seed; float32 beta2, pad;
//                    uint8 code_of[256]; float32 weights[C * G * NA], bias[NA] (with has_bias); uint8 obs[rows * C];
//                    int32 j[rows] (the index of the action played); int64 env_id[rows]; float64 coef[rows]
//                    -> float32 w[rows * NA], float64 total[rows], int32 index[rows] (softmax_choose), float32 probs[rows * NA],
//                       float64 pi[rows * NA], int64 q[rows * NA] (all 0 for a degenerate row or a j outside 0 .. NA-1)
// Every array is allocated at its exact size, so an access past a buffer is a sanitizer report.  Exit 0, or 1 on a bad file.
#define __HIPCC__ 1
#define SGW_PLAIN_STORES 1
#define SGW_LEARN_RULES_ONLY 1
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../ai_safety_gridworlds_amd/csrc/sgw_softmax.hpp"

namespace sgw { alignas(16) uint8_t policy_lds[POLICY_MAX_ROW_LDS + 256]; }   // (k_policy_act's dynamic LDS: declared by sgw_policy.hpp, unused here)

using namespace sgw;

template <class T> static bool rd(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}
template <class T> static bool wr(FILE* f, const std::vector<T>& v) { return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

struct Rows {
  int rows, C, G, frac_bits, agent;
  long long step;
  unsigned long long explore_below, seed;
  float beta2;
  const uint8_t *obs, *code_of;
  const float *w, *b;
  const int32_t* j;
  const int64_t* env_id;
  const double* coef;
  float *wt, *probs;
  double *total, *pi;
  int32_t* index;
  int64_t* q;
};

template <int NA> static void run_rows(const Rows& r) {
  const double scale = std::ldexp(1.0, r.frac_bits);
  for (int i = 0; i < r.rows; ++i) {
    const uint8_t* o = r.obs + (size_t)i * r.C;
    float score[NA], wt[NA];
    policy_score<NA>(score, o, r.C, r.code_of, r.w, r.b, r.G);
    float top;
    policy_first_max<NA>(score, top);
    r.total[i] = softmax_weights<NA>(wt, score, top, r.beta2);
    r.index[i] = softmax_choose<NA>(o, r.C, r.code_of, r.w, r.b, r.G, r.beta2, r.explore_below, r.seed, (long long)r.env_id[i], r.step, r.agent);
    double pi[NA];
    const bool live = softmax_pi<NA>(pi, score, r.beta2);
    long long q[NA];
    for (int k = 0; k < NA; ++k) q[k] = 0;
    if (live && r.j[i] >= 0 && r.j[i] < NA) softmax_grad<NA>(q, pi, r.j[i], r.coef[i], scale);
    for (int k = 0; k < NA; ++k) {
      r.wt[(size_t)i * NA + k] = wt[k];
      r.probs[(size_t)i * NA + k] = (float)pi[k];
      r.pi[(size_t)i * NA + k] = pi[k];
      r.q[(size_t)i * NA + k] = q[k];
    }
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
      int64_t n;
      if (std::fread(&n, sizeof(int64_t), 1, f) != 1 || n < 0 || n > (1 << 26)) return 1;
      std::vector<float> z;
      if (!rd(f, z, (size_t)n)) return 1;
      std::vector<float> e(z.size());
      for (size_t i = 0; i < z.size(); ++i) {
        if (z[i] > 0.0f) return 1;
        e[i] = softmax_exp2(z[i]);
      }
      if (!wr(o, e)) return 1;
    } else if (kind == 2) {
      int64_t h[8];
      uint64_t u[2];
      float fl[2];
      if (std::fread(h, sizeof(int64_t), 8, f) != 8 || std::fread(u, sizeof(uint64_t), 2, f) != 2 || std::fread(fl, sizeof(float), 2, f) != 2) return 1;
      const int C = (int)h[0], G = (int)h[1], NA = (int)h[2], rows = (int)h[3];
      if (C < 0 || C > 4096 || G < 1 || G > 64 || NA < 1 || NA > POLICY_MAX_ACTIONS || rows < 0 || rows > (1 << 17) || h[5] < 0 || h[5] > 52 ||
          h[7] < 0 || h[7] >= SGW_MAX_AGENTS || !(fl[0] >= 0.0f) || std::isinf(fl[0]))
        return 1;
      std::vector<uint8_t> code_of, obs;
      std::vector<float> w, b;
      std::vector<int32_t> j;
      std::vector<int64_t> env_id;
      std::vector<double> coef;
      if (!rd(f, code_of, 256) || !rd(f, w, (size_t)C * G * NA) || !rd(f, b, h[4] ? (size_t)NA : 0) || !rd(f, obs, (size_t)rows * C) ||
          !rd(f, j, (size_t)rows) || !rd(f, env_id, (size_t)rows) || !rd(f, coef, (size_t)rows))
        return 1;
      for (uint8_t g : code_of) if (g >= G) return 1;
      std::vector<float> wt((size_t)rows * NA), probs((size_t)rows * NA);
      std::vector<double> total((size_t)rows), pi((size_t)rows * NA);
      std::vector<int32_t> index((size_t)rows);
      std::vector<int64_t> q((size_t)rows * NA);
      const Rows r{rows, C, G, (int)h[5], (int)h[7], (long long)h[6], u[0], u[1], fl[0], obs.data(), code_of.data(), w.data(),
                   h[4] ? b.data() : nullptr, j.data(), env_id.data(), coef.data(), wt.data(), probs.data(), total.data(), pi.data(),
                   index.data(), q.data()};
      switch (NA) {
#define CASE(K) case K: run_rows<K>(r); break;
        CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8) CASE(9) CASE(10) CASE(11) CASE(12) CASE(13) CASE(14) CASE(15) CASE(16)
#undef CASE
      }
      if (!wr(o, wt) || !wr(o, total) || !wr(o, index) || !wr(o, probs) || !wr(o, pi) || !wr(o, q)) return 1;
    } else {
      return 1;
    }
  }
  std::fclose(f);
  return std::fclose(o) == 0 ? 0 : 1;
}
