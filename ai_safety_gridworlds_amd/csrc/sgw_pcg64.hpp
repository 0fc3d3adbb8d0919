// sgw_pcg64.hpp -- numpy's Generator(PCG64) as the env-owned generator of firemaker_ex_ma, island_navigation_ex_ma and
// aintelope_savanna: the stream (numpy/random/src/pcg64/pcg64.h), the draws built on it (distributions.c, _generator.pyx) and the
// generator's place in an env's state.  Every family, the seeding kernels (sgw_seed.hpp) and k_set_rng (sgw_kernels.hpp) take all
// three from here.
//
// The first part is plain C++ (no HIP type): sgw_seed.hpp's host-checked arithmetic uses the multiplier.  The draws and the state
// access are compiled by hipcc (and, through tests/host_shim, for the host: tests/host_shim/pcg64_check.cpp pins them to numpy).
#pragma once

#include <stdint.h>

namespace sgw {

// PCG_DEFAULT_MULTIPLIER_128, as its two 64-bit halves
constexpr uint64_t PCG64_MULT_HI = 0x2360ED051FC65DA4ULL, PCG64_MULT_LO = 0x4385DF649FCCF645ULL;

// state (rs), increment (ri) and numpy's buffered half of a 64-bit draw (bitgen next_uint32: has_uint32, uinteger)
struct Pcg64 { uint64_t rs_hi, rs_lo, ri_hi, ri_lo; uint32_t has32, u32; };
// The same generator with the buffered half in front, for firemaker_ex_ma and island_navigation_ex_ma: their State has always held the
// fields in this order, and the order of a State's members decides the order of its registers -- with Pcg64 their sixteen engines
// come out with other register names and a few instructions moved.  Everything below takes either (`G`).
struct Pcg64BufFirst { uint32_t has32, u32; uint64_t rs_hi, rs_lo, ri_hi, ri_lo; };

// The generator's place in an env's state words, the same in every family that has one: the four words rs_hi, rs_lo, ri_hi, ri_lo
// from PCG64_WORD0 on, `has32` in bit PCG64_FLAG_BIT of word PCG64_FLAG_WORD, `u32` in the low half of word PCG64_U32_WORD (the
// families keep other fields in the rest of those two words).
constexpr int PCG64_WORD0 = 3, PCG64_FLAG_WORD = 0, PCG64_FLAG_BIT = 27, PCG64_U32_WORD = 2;
constexpr uint64_t PCG64_U32_MASK = 0xffffffffull;

}  // namespace sgw

#if defined(__HIPCC__)
#include "sgw_common.hpp"

namespace sgw {

// ---- the stream ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t pcg64_xsl_rr(uint64_t hi, uint64_t lo) {              // output function XSL-RR 128/64
  uint64_t x = hi ^ lo;
  unsigned rot = (unsigned)(hi >> 58);
  return (x >> rot) | (x << ((64u - rot) & 63u));
}
__device__ __forceinline__ double pcg64_to_double(uint64_t v) { return (double)(v >> 11) * (1.0 / 9007199254740992.0); }

template <class G> __device__ __forceinline__ uint64_t next64(G& g) {
  const uint64_t MH = PCG64_MULT_HI, ML = PCG64_MULT_LO;
  uint64_t lo = g.rs_lo * ML;
  uint64_t hi = __umul64hi(g.rs_lo, ML) + g.rs_hi * ML + g.rs_lo * MH;
  uint64_t nlo = lo + g.ri_lo;
  hi += g.ri_hi + (nlo < lo ? 1ull : 0ull);
  g.rs_lo = nlo; g.rs_hi = hi;
  return pcg64_xsl_rr(hi, nlo);
}
template <class G> __device__ __forceinline__ uint32_t next32(G& g) {
  if (g.has32) { g.has32 = 0; return g.u32; }
  uint64_t n = next64(g);
  g.has32 = 1; g.u32 = (uint32_t)(n >> 32);
  return (uint32_t)n;
}
template <class G> __device__ __forceinline__ double random01(G& g) { return pcg64_to_double(next64(g)); }          // Generator.random()

// ---- bounded draws --------------------------------------------------------------------------------------------------------
// distributions.c random_interval (Generator.shuffle), max < 2^32: masked rejection over the buffered next_uint32
template <class G> __device__ __forceinline__ int interval(G& g, uint32_t max) {
  uint32_t mask = max;
  mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
  uint32_t v;
  do { v = next32(g) & mask; } while (v > max);
  return (int)v;
}
// the same draw for a wave that must not spin on a dead stream (an all-zero generator returns 0 for ever; aintelope_savanna):
// at most 1024 draws, then the result is clamped into [0, max]
template <class G> __device__ __forceinline__ int interval_guarded_clamped(G& g, uint32_t max) {
  uint32_t mask = max;
  mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
  uint32_t v;
  int guard = 0;
  do { v = next32(g) & mask; } while (v > max && ++guard < 1024);     // p(reject) < 1/2 per draw
  return (int)(v > max ? max : v);
}
template <class G> __device__ __forceinline__ int lemire(G& g, uint32_t rng) {          // distributions.c bounded_lemire_uint32 (integers / choice)
  if (rng == 0u) return 0;
  const uint32_t ex = rng + 1u;
  uint64_t m = (uint64_t)next32(g) * ex;
  uint32_t left = (uint32_t)m;
  if (left < ex) {
    const uint32_t thr = (0xffffffffu - rng) % ex;
    // a live stream leaves after ~1 draw (thr / 2^32 < 2^-24 here); the cap keeps a wave with a dead stream from spinning
    for (int guard = 0; left < thr && guard < 64; ++guard) { m = (uint64_t)next32(g) * ex; left = (uint32_t)m; }
  }
  return (int)(m >> 32);
}

// ---- the generator in the state ---------------------------------------------------------------------------------------------
// a family's load / store: the cursor stands at word PCG64_WORD0
template <class G> __device__ __forceinline__ void pcg64_get(Cursor& c, G& g) { g.rs_hi = c.get(); g.rs_lo = c.get(); g.ri_hi = c.get(); g.ri_lo = c.get(); }
template <class G> __device__ __forceinline__ void pcg64_put(Cursor& c, const G& g) { c.put(g.rs_hi); c.put(g.rs_lo); c.put(g.ri_hi); c.put(g.ri_lo); }
// ... and its share of the two packed words
__device__ __forceinline__ uint32_t pcg64_flag_of(uint64_t flag_word) { return (uint32_t)((flag_word >> PCG64_FLAG_BIT) & 1); }
__device__ __forceinline__ uint32_t pcg64_u32_of(uint64_t u32_word) { return (uint32_t)(u32_word & PCG64_U32_MASK); }
template <class G> __device__ __forceinline__ uint64_t pcg64_flag_bits(const G& g) { return (uint64_t)(g.has32 & 1) << PCG64_FLAG_BIT; }
template <class G> __device__ __forceinline__ uint64_t pcg64_u32_bits(const G& g) { return (uint64_t)g.u32 & PCG64_U32_MASK; }

}  // namespace sgw
#endif
