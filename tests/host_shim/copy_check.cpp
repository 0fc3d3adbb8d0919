// TEST INFRASTRUCTURE ONLY (see hip/hip_runtime.h here): the per-item logic of csrc/sgw_copy.hpp (sgw_copy_envs) run on the host.
// tests/test_copy_envs_host.py builds it with the host sanitizers (address: a byte outside a buffer; undefined: an access wider
// than its alignment) and runs it; every check compares with a naive loop and the program counts what it checked.
//
//   copy_check rows    -> "rows <cases>"    copy_row: row sizes 1..40, 48, 289, 441 x source misalignment 0..15 x destination
//                                           misalignment 0..15 x 1, 2, 4 .. 64 cooperating lanes, between guard regions
//   copy_check state   -> "state <cases>"   copy_item over the whole grid of a launch: state words through state_index plus
//                                           output planes, engines of 130 and 70 envs, index lists with repeats, -1 and
//                                           out-of-range entries, NULL lists, one engine onto itself
// Exit 0, or 1 with a line on stderr at the first difference.
#define __HIPCC__ 1
#define SGW_PLAIN_STORES 1
#define SGW_COPY_HOST_ONLY 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../ai_safety_gridworlds_amd/csrc/sgw_copy.hpp"

using namespace sgw;

static uint64_t g_s = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_s ^= g_s << 13; g_s ^= g_s >> 7; g_s ^= g_s << 17; return g_s; }

#define FAIL(...) do { std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); return -1; } while (0)

static const int GUARD = 64;
static const uint8_t FILL = 0xA5;

static long check_rows() {
  std::vector<int> sizes;
  for (int n = 1; n <= 40; ++n) sizes.push_back(n);
  sizes.push_back(48); sizes.push_back(289); sizes.push_back(441);
  long cases = 0;
  for (int n : sizes)
    for (int sm = 0; sm < 16; ++sm)
      for (int dm = 0; dm < 16; ++dm)
        for (int lanes = 1; lanes <= 64; lanes *= 2) {
          const size_t room = GUARD + 16 + (size_t)n + GUARD;
          uint8_t* sb = static_cast<uint8_t*>(std::aligned_alloc(16, (room + 15) & ~(size_t)15));   // exactly as large as the
          uint8_t* db = static_cast<uint8_t*>(std::aligned_alloc(16, (room + 15) & ~(size_t)15));   // guards: ASan sees the rest
          std::memset(sb, FILL, (room + 15) & ~(size_t)15); std::memset(db, FILL, (room + 15) & ~(size_t)15);
          uint8_t* s = sb + GUARD + sm;
          uint8_t* d = db + GUARD + dm;
          for (int k = 0; k < n; ++k) { s[k] = (uint8_t)rnd(); d[k] = (uint8_t)~s[k]; }
          std::vector<uint8_t> want(s, s + n);
          for (int lane = 0; lane < lanes; ++lane) copy_row(s, d, n, lane, lanes);
          for (int k = 0; k < n; ++k)
            if (d[k] != want[k] || s[k] != want[k]) FAIL("rows: n %d src+%d dst+%d lanes %d: byte %d", n, sm, dm, lanes, k);
          for (size_t k = 0; k < ((room + 15) & ~(size_t)15); ++k) {
            const bool in_d = db + k >= d && db + k < d + n, in_s = sb + k >= s && sb + k < s + n;
            if ((!in_d && db[k] != FILL) || (!in_s && sb[k] != FILL)) FAIL("rows: n %d src+%d dst+%d lanes %d: guard byte %zu touched", n, sm, dm, lanes, k);
          }
          std::free(sb); std::free(db);
          ++cases;
        }
  return cases;
}

struct Engine {
  long long n, n_pad;
  int words;
  std::vector<uint64_t> state;                 // state_alloc_words + GUARD words behind it
  std::vector<std::vector<uint8_t>> planes;    // GUARD | n_pad rows | GUARD
  Engine(long long n_, int words_, const std::vector<int>& row_bytes) : n(n_), n_pad((n_ + 63) / 64 * 64), words(words_) {
    state.resize((size_t)state_alloc_words(words, n_pad) + GUARD);
    for (auto& w : state) w = rnd();
    for (int rb : row_bytes) {
      planes.emplace_back((size_t)GUARD + (size_t)n_pad * rb + GUARD);
      for (auto& b : planes.back()) b = (uint8_t)rnd();
    }
  }
};

// one launch on the host: every wave, every lane
static void run(CopyArgs a) {
  const long long waves = copy_plan(a);
  for (long long w = 0; w < waves; ++w)
    for (int lane = 0; lane < WAVE; ++lane) copy_item(a, (unsigned)w, lane);
}

static int check_launch(Engine& dst, Engine& src, bool same, const int32_t* di, const int32_t* si, long long n,
                        const std::vector<int>& row_bytes, const char* what) {
  const int words = dst.words;
  const Engine src0 = src;                      // (same: also the destination before the launch)
  const Engine dst0 = dst;
  Engine want = dst;
  std::vector<char> touched((size_t)dst.n_pad, 0);
  for (long long i = 0; i < n; ++i) {
    const long long s = si ? si[i] : i, d = di ? di[i] : i;
    if (s < 0 || s >= src.n || d < 0 || d >= dst.n || (same && s == d)) continue;
    touched[(size_t)d] = 1;
    for (int w = 0; w < words; ++w) want.state[(size_t)state_index(w, d, words)] = src0.state[(size_t)state_index(w, s, words)];
    for (size_t q = 0; q < row_bytes.size(); ++q)
      std::memcpy(&want.planes[q][GUARD + (size_t)d * row_bytes[q]], &src0.planes[q][GUARD + (size_t)s * row_bytes[q]], (size_t)row_bytes[q]);
  }
  CopyArgs a; std::memset(&a, 0, sizeof(a));
  a.src_state = src.state.data(); a.dst_state = dst.state.data(); a.src_idx = si; a.dst_idx = di;
  a.n = n; a.src_n = src.n; a.dst_n = dst.n; a.words = words; a.same = same ? 1 : 0;
  for (size_t q = 0; q < row_bytes.size(); ++q) {
    CopyPlane& pl = a.planes[a.n_planes++];
    pl.src = src.planes[q].data() + GUARD; pl.dst = dst.planes[q].data() + GUARD; pl.row_bytes = row_bytes[q];
  }
  run(a);
  // the words of every env: real words exactly; with odd `words` the padding half of a copied env's last pair may have moved,
  // that of an untouched env may not
  for (long long e = 0; e < dst.n_pad; ++e)
    for (int w = 0; w < (int)state_pairs(words) * 2; ++w) {
      const size_t k = (size_t)state_index(w, e, words);
      if (w >= words && touched[(size_t)e]) continue;
      if (dst.state[k] != want.state[k]) FAIL("%s: words %d env %lld word %d", what, words, e, w);
    }
  for (size_t k = (size_t)state_alloc_words(words, dst.n_pad); k < dst.state.size(); ++k)
    if (dst.state[k] != dst0.state[k]) FAIL("%s: words %d: allocation word %zu past n_pad written", what, words, k);
  for (size_t q = 0; q < row_bytes.size(); ++q)
    if (dst.planes[q] != want.planes[q]) FAIL("%s: plane %zu (%d-byte rows) differs", what, q, row_bytes[q]);
  if (!same) {
    if (src.state != src0.state) FAIL("%s: the source state was written", what);
    for (size_t q = 0; q < row_bytes.size(); ++q) if (src.planes[q] != src0.planes[q]) FAIL("%s: source plane %zu was written", what, q);
  }
  return 0;
}

static long check_state() {
  const std::vector<int> row_bytes = {1, 3, 8, 35, 48, 196, 289, 1156};     // 35- and 289-byte rows: alignments that disagree
  const int words_list[5] = {1, 2, 7, 10, 22};
  long cases = 0;
  for (int words : words_list) {
    // 130 -> 70 envs: distinct destinations across the 64-env boundary, repeated sources, -1 and out-of-range entries on both sides
    std::vector<int32_t> di, si;
    for (int k = 0; k < 60; ++k) { di.push_back((k * 11 + 3) % 70); si.push_back((int32_t)(rnd() % 130)); }  // 11 is coprime to 70: distinct
    for (int k = 0; k < 10; ++k) si[(size_t)k * 3] = 129 - (k % 3);                                        // repeats: fan-out
    const int32_t bad_d[6] = {-1, 70, 127, 128, 1000, -7}, bad_s[6] = {-1, 130, 191, 192, 100000, -2};
    for (int k = 0; k < 6; ++k) { di.push_back(bad_d[k]); si.push_back((int32_t)(rnd() % 130)); }
    for (int k = 0; k < 6; ++k) { di.push_back(((60 + k) * 11 + 3) % 70); si.push_back(bad_s[k]); }
    {
      Engine src(130, words, row_bytes), dst(70, words, row_bytes);
      if (check_launch(dst, src, false, di.data(), si.data(), (long long)di.size(), row_bytes, "gather/scatter")) return -1;
      ++cases;
    }
    {  // 70 -> 130 envs: no lists (pairs 70 .. 99 have no source env), and a source list alone
      Engine src(70, words, row_bytes), dst(130, words, row_bytes);
      if (check_launch(dst, src, false, nullptr, nullptr, 100, row_bytes, "NULL lists, n beyond the smaller engine")) return -1;
      ++cases;
      if (check_launch(dst, src, false, nullptr, si.data(), 64, row_bytes, "NULL destination list")) return -1;
      ++cases;
    }
    {  // one engine: envs 40..71 -> 96..127, plus pairs onto themselves (skipped)
      Engine e(130, words, row_bytes);
      std::vector<int32_t> d2, s2;
      for (int k = 0; k < 32; ++k) { s2.push_back(40 + k); d2.push_back(96 + k); }
      for (int k = 0; k < 5; ++k) { s2.push_back(k); d2.push_back(k); }
      if (check_launch(e, e, true, d2.data(), s2.data(), (long long)d2.size(), row_bytes, "one engine")) return -1;
      ++cases;
    }
  }
  return cases;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  if (!std::strcmp(argv[1], "rows")) {
    const long c = check_rows();
    if (c < 0) return 1;
    std::printf("rows %ld\n", c);
    return 0;
  }
  if (!std::strcmp(argv[1], "state")) {
    const long c = check_state();
    if (c < 0) return 1;
    std::printf("state %ld\n", c);
    return 0;
  }
  return 2;
}
