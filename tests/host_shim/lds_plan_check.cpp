// TEST INFRASTRUCTURE ONLY (see hip/hip_runtime.h here): checks the LDS plan of one env-wave staging buffer (csrc/sgw_common.hpp
// lds_plan / lds_wave_bytes) for EVERY value of the output mask, against the bytes the kernels actually index.
// tests/test_output_subsets.py builds it with the host sanitizers and runs it as a subprocess.
//
//   lds_plan_check < geometries         one line per geometry: HW A K M pa vb cs vg
//
// pa: columns of term_reason / safety (A for the per-agent families, else 1); vb: bytes of one env's row of agent windows;
// cs: rows of the parked cumulative vectors (A * K for the CUM_IN_LDS families, else 0); vg: envs the views region holds at a time.
// The extents below are written out from what emit_stage / emit_drain / engine_body (csrc/sgw_kernels.hpp) index, on purpose NOT
// with lds_rows / lds_small_bytes: a region the plan makes too small for its users must show up here as an overlap.
// For every mask over LN_REWARD .. LN_FRM, LN_VIEWS, LN_OBSVIEWS: every enabled region inside [0, wave_bytes), enabled regions
// pairwise disjoint, the parked vectors wholly inside the reward rows / the cumulative rows / the returns rows exactly when the
// rule documented at lds_plan says so and disjoint from everything otherwise, wave_bytes == lds_wave_bytes(...) and a multiple
// of 16, the offsets of 16-byte accesses multiples of 16 and those of doubles multiples of 8.
// Exit 0, or the first violating (geometry, mask, region pair) on stdout and exit 1.
#define __HIPCC__ 1
#define SGW_PLAIN_STORES 1
#include <cstdio>
#include <cstdlib>
#include <string_view>
#include <vector>

#include "../../ai_safety_gridworlds_amd/csrc/sgw_common.hpp"

using namespace sgw;

struct Region { const char* name; long long off, bytes; int align; };

struct Geometry { int HW, A, K, M, pa, vb, cs, vg; };

static int violation(const Geometry& g, int need, const char* what, const char* r0, const char* r1) {
  std::printf("violation: geometry HW=%d A=%d K=%d M=%d pa=%d vb=%d cs=%d vg=%d mask=0x%x: %s (%s%s%s)\n", g.HW, g.A, g.K, g.M, g.pa,
              g.vb, g.cs, g.vg, need, what, r0, r1[0] ? ", " : "", r1);
  return 1;
}

static bool inside(const Region& a, const Region& b) { return a.off >= b.off && a.off + a.bytes <= b.off + b.bytes; }
static bool disjoint(const Region& a, const Region& b) { return a.off + a.bytes <= b.off || b.off + b.bytes <= a.off; }

static int check(const Geometry& g, int need) {
  const LdsPlan p = lds_plan(g.HW, g.A, g.K, g.M, g.pa, need, g.vb, g.cs, g.vg);
  const long long AK = (long long)g.A * g.K;
  const bool returns = (need & LN_RETURNS) != 0;
  std::vector<Region> r;
  r.push_back({"board", 0, 64LL * g.HW, 16});
  if (need & LN_REWARD) r.push_back({"vec_r", p.vec_r, AK * 512, 16});
  if (need & LN_CUMULATIVE) r.push_back({"vec_c", p.vec_c, AK * 512, 16});
  if ((need & LN_METRICS) && g.M > 0) r.push_back({"vec_m", p.vec_m, g.M * 512LL, 16});
  if (returns) r.push_back({"vec_a", p.vec_a, (AK + 1) * 512, 16});
  r.push_back({"trash", p.trash, 512, 8});
  r.push_back({"flag", p.flag, 16, 4});
  r.push_back({"ain", p.ain, 64LL * g.A, 1});
  if (need & LN_ST) r.push_back({"st", p.st, 64LL * g.A, 16});
  if (need & LN_TR) r.push_back({"tr", p.tr, 64LL * g.pa, 1});
  if (need & LN_ACT) r.push_back({"act", p.act, 64LL * g.A, 1});
  if (need & LN_POS) r.push_back({"pos", p.pos, 128LL * g.A, 1});
  if (need & LN_FLG) r.push_back({"flg", p.flg, 64LL * g.A, 1});
  if (need & LN_DISC) r.push_back({"disc", p.disc, 512, 8});
  if (need & LN_HID) r.push_back({"hid", p.hid, 512, 8});
  if (need & LN_SAF) r.push_back({"saf", p.saf, 256LL * g.pa, 4});
  if (need & LN_FRM) r.push_back({"frm", p.frm, 256, 4});
  if ((need & (LN_VIEWS | LN_OBSVIEWS)) && g.vb > 0) r.push_back({"views", p.views, (long long)g.vg * g.vb, 16});
  if (p.views_g != g.vg) return violation(g, need, "views_g is not the chunk the plan was asked for", "views", "");
  if (p.wave_bytes != (int)lds_wave_bytes(g.HW, g.A, g.K, g.M, g.pa, need, g.vb, g.cs, g.vg))
    return violation(g, need, "wave_bytes != lds_wave_bytes", "wave", "");
  if (p.wave_bytes % 16) return violation(g, need, "wave_bytes is no multiple of 16", "wave", "");
  for (const Region& a : r) {
    if (a.off < 0 || a.off + a.bytes > p.wave_bytes) return violation(g, need, "region outside [0, wave_bytes)", a.name, "");
    if (a.off % a.align) return violation(g, need, "region offset misaligned", a.name, "");
  }
  for (size_t i = 0; i < r.size(); ++i)
    for (size_t j = i + 1; j < r.size(); ++j)
      if (!disjoint(r[i], r[j])) return violation(g, need, "regions overlap", r[i].name, r[j].name);
  if (g.cs > 0) {
    // the documented rule: inside the reward rows if `reward` is requested, else inside the cumulative rows, else inside the
    // returns rows, else rows of its own
    const Region cst = {"cstash", p.cstash, g.cs * 512LL, 16};
    const char* host = (need & LN_REWARD) ? "vec_r" : (need & LN_CUMULATIVE) ? "vec_c" : returns ? "vec_a" : nullptr;
    if (cst.off < 0 || cst.off + cst.bytes > p.wave_bytes) return violation(g, need, "region outside [0, wave_bytes)", "cstash", "");
    if (cst.off % cst.align) return violation(g, need, "region offset misaligned", "cstash", "");
    for (const Region& a : r) {
      const bool is_host = host != nullptr && std::string_view(a.name) == host;
      if (is_host && !inside(cst, a)) return violation(g, need, "parked vectors not wholly inside the region they alias", "cstash", a.name);
      if (!is_host && !disjoint(cst, a)) return violation(g, need, "regions overlap", "cstash", a.name);
    }
  }
  return 0;
}

int main() {
  std::vector<int> bits;
  for (int b = LN_REWARD; b <= LN_FRM; b <<= 1) bits.push_back(b);
  bits.push_back(LN_VIEWS);
  bits.push_back(LN_OBSVIEWS);
  Geometry g;
  long long checked = 0;
  int n_geo = 0;
  while (std::scanf("%d %d %d %d %d %d %d %d", &g.HW, &g.A, &g.K, &g.M, &g.pa, &g.vb, &g.cs, &g.vg) == 8) {
    ++n_geo;
    for (unsigned m = 0; m < (1u << bits.size()); ++m) {
      int need = 0;
      for (size_t i = 0; i < bits.size(); ++i) if ((m >> i) & 1u) need |= bits[i];
      if (check(g, need)) return 1;
      ++checked;
    }
  }
  if (n_geo == 0) { std::printf("no geometry read\n"); return 2; }
  std::printf("ok: %d geometries, %lld plans\n", n_geo, checked);
  return 0;
}
