// lcx_diag_plan.hpp -- what lcx_diag_batch (include/lcx_diag.h) decides before a device is touched: validation of a request list,
// conversion of the bounds and powers, the order of the requests and the cut into passes.
//
// Host code only, no HIP include: lcx_core.hip plans with it (and converts the bounds of the classic diag_*_rng / diag_*_mom entries
// with the same functions), lcx_kernels.hpp takes the pass table's layout from it, lcx_diag_batch_check is its validation, and
// tools/diag_batch_plan_check.cpp compiles it alone under the host sanitizers.
#ifndef LCX_DIAG_PLAN_HPP
#define LCX_DIAG_PLAN_HPP

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/lcx_diag.h"

namespace lcx {
namespace diag {

// requests per pass at most: the pass table travels as a kernel argument (4 KiB at most: 32 x 88 B in double)
constexpr int MAX_PASS = 32;
// device result buffer + page-locked staging of a call with host output, together at most (one request per pass is always granted)
constexpr size_t SCRATCH_CAP = size_t(512) << 20;

// attribute index of the kernels: 0 rd3, 1 rw2, 2 kappa
inline int sel_attr(int sel) { return sel == LCX_DIAG_SEL_DRY ? 0 : sel == LCX_DIAG_SEL_KAPPA ? 2 : 1; }     // (WATER reads rw2)
inline int count_attr(int count) { return count == LCX_DIAG_DRY_MOM ? 0 : count == LCX_DIAG_KAPPA_MOM ? 2 : 1; }
inline bool sel_is_range(int sel) { return sel == LCX_DIAG_SEL_DRY || sel == LCX_DIAG_SEL_WET || sel == LCX_DIAG_SEL_KAPPA; }

// radii -> the attribute's units, in double; the object rounds to its real type (particles_diag.ipp:409-437)
inline void rng_bounds(int sel, double a, double b, double &lo, double &hi)
{
  if (sel == LCX_DIAG_SEL_DRY) { lo = std::pow(a, 3); hi = std::pow(b, 3); }
  else if (sel == LCX_DIAG_SEL_WET) { lo = std::pow(a, 2); hi = std::pow(b, 2); }
  else { lo = a; hi = b; }
}
// the power that moment k of a count raises its attribute to, in double (particles_diag.ipp:439-470)
inline double mom_power(int count, int k) { return count == LCX_DIAG_DRY_MOM ? k / 3. : count == LCX_DIAG_WET_MOM ? k / 2. : double(k); }

// the first fault of a list, named; true when there is none
inline bool validate(const lcx_diag_req_t *req, int n_req, std::string &err)
{
  if (n_req < 0) { err = "libcloudph++: diag_batch: n_req < 0"; return false; }
  if (n_req > 0 && !req) { err = "libcloudph++: diag_batch: req == NULL with n_req > 0"; return false; }
  for (int r = 0; r < n_req; ++r) {
    const lcx_diag_req_t &q = req[r];
    const std::string at = "libcloudph++: diag_batch: request " + std::to_string(r) + ": ";
    if (q.n_clauses < 1 || q.n_clauses > LCX_DIAG_MAX_CLAUSES) {
      err = at + "n_clauses = " + std::to_string(q.n_clauses) + " is outside 1 .. " + std::to_string(LCX_DIAG_MAX_CLAUSES);
      return false;
    }
    for (int c = 0; c < q.n_clauses; ++c)
      if (q.clause[c].sel < LCX_DIAG_SEL_ALL || q.clause[c].sel > LCX_DIAG_SEL_WATER) {
        err = at + "clause " + std::to_string(c) + ": unknown sel " + std::to_string(q.clause[c].sel);
        return false;
      }
    if (q.count < LCX_DIAG_SD_CONC || q.count > LCX_DIAG_KAPPA_MOM) { err = at + "unknown count " + std::to_string(q.count); return false; }
  }
  return true;
}

// one request as the kernel reads it: thresholds and power already in the object's real type
template <class T> struct dev_req {
  T lo[LCX_DIAG_MAX_CLAUSES], hi[LCX_DIAG_MAX_CLAUSES];
  T power;
  uint32_t row;                           // of the output
  uint8_t n_clauses, sel[LCX_DIAG_MAX_CLAUSES];
  uint8_t count, attr;                    // attr: of the moment
  uint8_t same_pow;                       // the request before it in the pass raises the same attribute to the same power
};
template <class T> struct dev_pass { dev_req<T> r[MAX_PASS]; };
static_assert(sizeof(dev_pass<double>) <= 3072, "the pass table is a kernel argument next to a dozen pointers: 4 KiB in all");

template <class T> struct pass {
  int n = 0;
  unsigned used = 0;                      // bit a: some request of the pass reads attribute a
  int src[MAX_PASS];                      // slot -> index in the caller's list
  dev_pass<T> tab;
};

inline int req_per_pass(size_t n_cell, size_t real_bytes)
{
  const size_t row = 2 * std::max<size_t>(n_cell, 1) * real_bytes;
  return int(std::max<size_t>(1, std::min<size_t>(size_t(MAX_PASS), SCRATCH_CAP / row)));
}
inline size_t scratch_bytes(size_t n_cell, size_t real_bytes) { return size_t(req_per_pass(n_cell, real_bytes)) * 2 * n_cell * real_bytes; }

// (attribute, power) of a request's pow; sd_conc has none and sorts first
template <class T> inline void pow_key(const lcx_diag_req_t &q, int &attr, T &power)
{
  if (q.count == LCX_DIAG_SD_CONC) { attr = -1; power = T(0); }
  else { attr = count_attr(q.count); power = T(mom_power(q.count, q.k)); }
}

// The whole (validated) list ordered by (attribute, power bits), stably, then cut into passes of rpp: requests that share a power
// are neighbours and, inside a pass, share its evaluation.  rows_by_slot: a pass writes row `slot` of a buffer of its own (host
// output), else row `index in the caller's list` (device output).
template <class T> inline std::vector<pass<T>> plan(const lcx_diag_req_t *req, int n_req, int rpp, bool rows_by_slot)
{
  rpp = std::max(1, std::min(rpp, MAX_PASS));
  std::vector<int> order(size_t(std::max(n_req, 0)));
  for (int r = 0; r < n_req; ++r) order[size_t(r)] = r;
  auto bits = [](T v) { uint64_t b = 0; std::memcpy(&b, &v, sizeof(T)); return b; };
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
    int aa, ab; T pa, pb;
    pow_key<T>(req[a], aa, pa); pow_key<T>(req[b], ab, pb);
    return aa != ab ? aa < ab : bits(pa) < bits(pb);
  });
  std::vector<pass<T>> passes;
  for (int i = 0; i < n_req; ++i) {
    if (i % rpp == 0) { passes.emplace_back(); std::memset(&passes.back().tab, 0, sizeof(dev_pass<T>)); }
    pass<T> &p = passes.back();
    const int slot = p.n++;
    const lcx_diag_req_t &q = req[order[size_t(i)]];
    dev_req<T> &d = p.tab.r[slot];
    p.src[slot] = order[size_t(i)];
    d.row = uint32_t(rows_by_slot ? slot : order[size_t(i)]);
    d.n_clauses = uint8_t(q.n_clauses);
    for (int c = 0; c < q.n_clauses; ++c) {
      double lo = 0, hi = 0;
      d.sel[c] = uint8_t(q.clause[c].sel);
      if (sel_is_range(q.clause[c].sel)) rng_bounds(q.clause[c].sel, q.clause[c].lo, q.clause[c].hi, lo, hi);
      d.lo[c] = T(lo); d.hi[c] = T(hi);
      if (q.clause[c].sel != LCX_DIAG_SEL_ALL) p.used |= 1u << sel_attr(q.clause[c].sel);
    }
    int attr; T power;
    pow_key<T>(q, attr, power);
    d.count = uint8_t(q.count); d.attr = uint8_t(attr < 0 ? 1 : attr); d.power = power;
    if (attr >= 0) p.used |= 1u << attr;
    if (slot > 0 && attr >= 0) {
      const dev_req<T> &b = p.tab.r[slot - 1];
      d.same_pow = uint8_t(b.count != LCX_DIAG_SD_CONC && b.attr == d.attr && bits(b.power) == bits(d.power));
    }
  }
  return passes;
}

} // namespace diag
} // namespace lcx
#endif
