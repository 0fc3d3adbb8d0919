// TEST INFRASTRUCTURE ONLY (see hip/hip_runtime.h here): the one definition of the what-if rule and of the Q-value fold
// (csrc/sgw_whatif.hpp: whatif_moves, whatif_fold) run on the host.  tests/test_whatif_host.py builds it with the host
// sanitizers, hands it a file of cases and compares what it prints with tests/whatif_ref.py.
//
//   whatif_check <file>      the file is a sequence of cases, little-endian:
//     int64   H, W, NA, rows, relative, D, L
//     uint64  impassable (one character per byte, 0 = unused)
//     uint8   tile_chars[L]
//     uint8   board[rows * H*W], where[rows * 3] = (row, col, direction)
//     float64 q[rows * NA * D], table[rows * L * D]
//     uint8   seen[rows * L]
//   per case and row one line: 2 NA position bytes, NA tiles, NA blocked flags, then the row's table after the fold as L * D
//   int64 bit patterns, then its L seen bytes.
// Exit 0, or 1 on a file it cannot read.
#define __HIPCC__ 1
#define SGW_PLAIN_STORES 1
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../ai_safety_gridworlds_amd/csrc/sgw_whatif.hpp"

namespace sgw { alignas(16) uint8_t whatif_lds[1]; }   // (the kernel's dynamic LDS: declared by the header, unused here)

using namespace sgw;

template <class T> static bool rd(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

template <int NA> static void one_row(const uint8_t* board, int H, int W, const uint8_t* where, bool relative, uint64_t imp, const double* q,
                                      int D, const uint8_t* chars, int L, double* table, uint8_t* seen) {
  uint8_t pos[2 * NA], tile[NA], blk[NA];
  whatif_moves<NA>(board, H, W, where[0], where[1], where[2], relative, imp, pos, tile, blk);
  for (int d = 0; d < D; ++d) whatif_fold<NA>(tile, q + d, D, chars, L, table + d, seen, d == 0);
  for (int i = 0; i < 2 * NA; ++i) std::printf("%d ", pos[i]);
  for (int i = 0; i < NA; ++i) std::printf("%d ", tile[i]);
  for (int i = 0; i < NA; ++i) std::printf("%d ", blk[i]);
  for (int i = 0; i < L * D; ++i) { long long bits; std::memcpy(&bits, table + i, 8); std::printf("%lld ", bits); }
  for (int i = 0; i < L; ++i) std::printf("%d%s", seen[i], i + 1 < L ? " " : "\n");
}

int main(int argc, char** argv) {
  if (argc != 2) return 1;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 1;
  for (;;) {
    int64_t h[7];
    const size_t got = std::fread(h, sizeof(int64_t), 7, f);
    if (got == 0) break;
    if (got != 7) return 1;
    const int H = (int)h[0], W = (int)h[1], NA = (int)h[2], rows = (int)h[3], D = (int)h[5], L = (int)h[6];
    if (H < 1 || W < 1 || H * W > 4096 || NA < 1 || NA > WHATIF_MAX_ACTIONS || rows < 0 || D < 1 || L < 1 || L > WHATIF_MAX_TILES) return 1;
    std::vector<uint64_t> imp;
    std::vector<uint8_t> chars, board, where, seen;
    std::vector<double> q, table;
    if (!rd(f, imp, 1) || !rd(f, chars, (size_t)L) || !rd(f, board, (size_t)rows * H * W) || !rd(f, where, (size_t)rows * 3) ||
        !rd(f, q, (size_t)rows * NA * D) || !rd(f, table, (size_t)rows * L * D) || !rd(f, seen, (size_t)rows * L))
      return 1;
    for (int r = 0; r < rows; ++r) {
      switch (NA) {
#define CASE(K) case K: one_row<K>(board.data() + (size_t)r * H * W, H, W, where.data() + 3 * r, h[4] != 0, imp[0], q.data() + (size_t)r * NA * D, \
                                   D, chars.data(), L, table.data() + (size_t)r * L * D, seen.data() + (size_t)r * L); break;
        SGW_WHATIF_CASES(CASE)
#undef CASE
      }
    }
  }
  std::fclose(f);
  return 0;
}
