// TEST INFRASTRUCTURE ONLY (see hip/hip_runtime.h here): the one definition of the learning-target rule (csrc/sgw_targets.hpp:
// td_element, one element's backward loop with its grouped loads) run on the host.  tests/test_targets_host.py builds it with the
// host sanitizers, hands it a file of cases and compares what it writes with tests/targets_ref.py.
//
//   targets_check <in> <out>      <in> is a sequence of cases, little-endian:
//     int64   T, N, A, C, R, flags, has_value, outputs (bit 0 ret, bit 1 adv, bit 2 valid), src_rows, dst_rows
//     float64 lambda, gamma[C]
//     float64 reward[T * src_rows * A * C]
//     uint8   step_type[T * src_rows * A], term_reason[T * src_rows * R]
//     float64 value[T * dst_rows * A * C], value0[dst_rows * A * C]          (only with has_value)
//   <out> gets per case ret and adv as float64 [T * dst_rows * A * C] and valid as uint8 [T * dst_rows * A]; an output that was
//   not asked for, and every row n >= N, keeps the fill (-777.25, byte 0xEE).
// Every array is allocated at its exact size, so an access past a buffer is a sanitizer report.  Exit 0, or 1 on a bad file.
#define __HIPCC__ 1
#define SGW_PLAIN_STORES 1
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../ai_safety_gridworlds_amd/csrc/sgw_targets.hpp"

using namespace sgw;

template <class T> static bool rd(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc != 3) return 1;
  FILE* f = std::fopen(argv[1], "rb");
  FILE* o = std::fopen(argv[2], "wb");
  if (!f || !o) return 1;
  for (;;) {
    int64_t h[10];
    const size_t got = std::fread(h, sizeof(int64_t), 10, f);
    if (got == 0) break;
    if (got != 10) return 1;
    const int64_t T = h[0], N = h[1], A = h[2], C = h[3], R = h[4], flags = h[5], src_rows = h[8], dst_rows = h[9];
    const bool has_value = h[6] != 0;
    if (T < 1 || T > 4096 || N < 0 || N > 4096 || A < 1 || A > SGW_MAX_AGENTS || C < 1 || C > SGW_MAX_K || R < 1 || R > A || src_rows < N ||
        dst_rows < N || src_rows > 8192 || dst_rows > 8192)
      return 1;
    std::vector<double> head, reward, value, value0;
    std::vector<uint8_t> st, tr;
    if (!rd(f, head, (size_t)(1 + C)) || !rd(f, reward, (size_t)(T * src_rows * A * C)) || !rd(f, st, (size_t)(T * src_rows * A)) ||
        !rd(f, tr, (size_t)(T * src_rows * R)))
      return 1;
    if (has_value && (!rd(f, value, (size_t)(T * dst_rows * A * C)) || !rd(f, value0, (size_t)(dst_rows * A * C)))) return 1;
    std::vector<double> ret((size_t)(T * dst_rows * A * C), -777.25), adv(ret);
    std::vector<uint8_t> valid((size_t)(T * dst_rows * A), 0xEE);
    TdArgs a;
    std::memset(&a, 0, sizeof(a));
    a.reward = reward.data(); a.step_type = st.data();
    a.bootstrap = (flags & SGW_TD_BOOTSTRAP_TRUNCATED) ? 1 : 0;
    a.term_reason = a.bootstrap ? tr.data() : nullptr;
    a.value = has_value ? value.data() : nullptr;
    a.ret = (h[7] & 1) ? ret.data() : nullptr;
    a.adv = (h[7] & 2) ? adv.data() : nullptr;
    a.valid = (h[7] & 4) ? valid.data() : nullptr;
    if (a.adv && !has_value) return 1;
    a.value0 = a.adv ? value0.data() : nullptr;
    a.src_rows = src_rows; a.dst_rows = dst_rows; a.n_elems = N * A * C;
    a.T = (int)T; a.A = (int)A; a.C = (int)C; a.R = (int)R;
    a.lambda = head[0];
    for (int c = 0; c < C; ++c) a.gamma[c] = head[1 + c];
    for (long long i = 0; i < a.n_elems; ++i) td_element_any(a, i);
    if (std::fwrite(ret.data(), 8, ret.size(), o) != ret.size() || std::fwrite(adv.data(), 8, adv.size(), o) != adv.size() ||
        std::fwrite(valid.data(), 1, valid.size(), o) != valid.size())
      return 1;
  }
  std::fclose(f);
  return std::fclose(o) == 0 ? 0 : 1;
}
