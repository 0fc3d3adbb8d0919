// sgw_seed.hpp -- seeding the env-owned numpy generators on the device: seed -> np.random.PCG64(np.random.SeedSequence(seed)),
// and the reference's layout-seed rule (safety_game_moma.py:845-852: crc32 of three big-endian words).
//
// The arithmetic is plain C++ (uint32 / uint64 / unsigned __int128, no HIP type), usable from the host: tests/host_shim/
// seed_check.cpp compiles this file with the host sanitizers and compares it with numpy and zlib.  The two kernels at the end
// are compiled by hipcc only.
#pragma once

#include <stdint.h>

#include "sgw_pcg64.hpp"

#if defined(__HIPCC__)
#define SGW_SEED_HD __host__ __device__
#else
#define SGW_SEED_HD
#endif

namespace sgw {

enum { SEED_LOW32 = 1, SEED_FLAGS_ALL = 1 };      // SGW_SEED_LOW32 of include/sgw.h
constexpr uint32_t SEED_LAYOUT_SALT = 17122023u;  // safety_game_moma.py:850

// numpy SeedSequence(seed) with an empty spawn key and pool size 4 (numpy/random/bit_generator.pyx: mix_entropy, generate_state
// for 4 uint64 words), then PCG64's seeding (pcg_setseq_128_srandom_r).  seed < 2^32 is one entropy word, else two.
// out = (state_hi, state_lo, inc_hi, inc_lo): the layout of sgw_set_rng_state.
SGW_SEED_HD inline void pcg64_from_seed(uint64_t seed, uint64_t out[4]) {
  const uint32_t ent[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  const int len = ent[1] ? 2 : 1;
  uint32_t hc = 0x43b0d7e5u;
  uint32_t pool[4];
#define SGW_SEED_HASHMIX(dst, src) { uint32_t v_ = (src); v_ ^= hc; hc *= 0x931e8875u; v_ *= hc; v_ ^= v_ >> 16; (dst) = v_; }
  for (int i = 0; i < 4; ++i) SGW_SEED_HASHMIX(pool[i], i < len ? ent[i] : 0u)
  for (int s = 0; s < 4; ++s)
    for (int d = 0; d < 4; ++d)
      if (s != d) {
        uint32_t y;
        SGW_SEED_HASHMIX(y, pool[s])
        uint32_t r = 0xca01f9ddu * pool[d] - 0x4973f715u * y;
        r ^= r >> 16;
        pool[d] = r;
      }
#undef SGW_SEED_HASHMIX
  uint32_t h = 0x8b51f9ddu;
  uint32_t w[8];
  for (int i = 0; i < 8; ++i) {
    uint32_t d = pool[i & 3] ^ h;
    h *= 0x58f38dedu;
    d *= h;
    d ^= d >> 16;
    w[i] = d;
  }
  uint64_t v[4];
  for (int j = 0; j < 4; ++j) v[j] = (uint64_t)w[2 * j] | ((uint64_t)w[2 * j + 1] << 32);
  typedef unsigned __int128 u128;
  const u128 mult = ((u128)PCG64_MULT_HI << 64) | PCG64_MULT_LO;
  const u128 initstate = ((u128)v[0] << 64) | v[1], initseq = ((u128)v[2] << 64) | v[3];
  const u128 inc = (initseq << 1) | 1u;
  u128 state = inc;
  state += initstate;
  state = state * mult + inc;
  out[0] = (uint64_t)(state >> 64); out[1] = (uint64_t)state; out[2] = (uint64_t)(inc >> 64); out[3] = (uint64_t)inc;
}

// zlib.crc32 (reflected, polynomial 0xEDB88320, init and final xor 0xFFFFFFFF) of a, b, c as big-endian 4-byte words: bit by bit,
// no table
SGW_SEED_HD inline uint32_t crc32_be3(uint32_t a, uint32_t b, uint32_t c) {
  const uint32_t words[3] = {a, b, c};
  uint32_t crc = 0xFFFFFFFFu;
  for (int i = 0; i < 3; ++i)
    for (int byte = 3; byte >= 0; --byte) {
      crc ^= (words[i] >> (8 * byte)) & 0xFFu;
      for (int k = 0; k < 8; ++k) crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1u)));
    }
  return ~crc;
}
SGW_SEED_HD inline uint32_t layout_seed(uint32_t original_seed, uint32_t env_layout_seed) {
  return crc32_be3(original_seed, env_layout_seed, SEED_LAYOUT_SALT);
}

// The seed of env i as sgw_seed_rng / sgw_pcg64_from_seeds define it: seeds[i], or base + i mod 2^64 (base = seed_base + the
// global id of env 0); cut to 32 bits with SEED_LOW32; replaced by the layout rule when layout_seeds is given.
SGW_SEED_HD inline uint64_t resolve_seed(const uint64_t* seeds, uint64_t base, const uint32_t* layout_seeds, int flags, long long i) {
  uint64_t s = seeds ? seeds[i] : base + (uint64_t)i;
  if (flags & SEED_LOW32) s &= 0xFFFFFFFFull;
  if (layout_seeds) s = layout_seed((uint32_t)s, layout_seeds[i]);
  return s;
}

}  // namespace sgw

#if defined(__HIPCC__)
namespace sgw {

// The engine form: what k_set_rng (sgw_kernels.hpp) writes, from seeds instead of uploaded words and under a mask.  One lane
// per env.  mask == nullptr: every env, and the padding lanes get k_set_rng's working pad stream; with a mask the padding lanes
// and the unmasked envs are not touched at all.
__global__ void k_seed_rng(uint64_t* state, long long n_pad, long long n, int words, const uint64_t* seeds, uint64_t base,
                           const uint32_t* layout_seeds, const uint8_t* mask, int flags) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_pad) return;
  if (mask && (e >= n || !mask[e])) return;
  uint64_t pcg[4] = {0x9E3779B97F4A7C15ull, (uint64_t)e, 0ull, 1ull};
  if (e < n) pcg64_from_seed(resolve_seed(seeds, base, layout_seeds, flags, e), pcg);
  for (int k = 0; k < 4; ++k) state[state_index(PCG64_WORD0 + k, e, words)] = pcg[k];
  state[state_index(PCG64_FLAG_WORD, e, words)] &= ~(1ull << PCG64_FLAG_BIT);       // the buffered next_uint32: flag and value
  state[state_index(PCG64_U32_WORD, e, words)] &= ~PCG64_U32_MASK;
}

// The stand-alone form: out uint64 [n, 4]
__global__ void k_pcg64_from_seeds(const uint64_t* seeds, uint64_t base, const uint32_t* layout_seeds, int flags, long long n,
                                   uint64_t* out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t pcg[4];
  pcg64_from_seed(resolve_seed(seeds, base, layout_seeds, flags, i), pcg);
  for (int k = 0; k < 4; ++k) out[i * 4 + k] = pcg[k];
}

}  // namespace sgw
#endif
