// lcx_cond_plan.hpp -- what the condensation settles on the host: the route of a step_cond (cond_route_of), the kernel of a per-substep
// launch with what the launch needs beyond its name (cond_kernel_of), the five meanings of opts_init.dbg_cond_budget (cond_budget), the
// sizes of its launches and lists (cond_*_cap, cond_*_grid ...) and the form of the per-cell finish (cond_finish_of).  Results never depend
// on a measurement switch: every form of the fast arithmetic gives the same bits.
//
// No HIP include (include/lcx.h is plain C: enum lcx_cond_kernel, enum lcx_cond_finish, the LCX_DBG_* bits): lcx_core.hip's step_cond,
// cond_substep, cond_substeps_fused, launch_cellfinish and the two sites that defer a sort decide with it, and tools/cond_plan_check.cpp
// compiles it alone under the host sanitizers.
#ifndef LCX_COND_PLAN_HPP
#define LCX_COND_PLAN_HPP

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/lcx.h"

namespace lcx {

// the debug bits that the plan reads (include/lcx.h LCX_DBG_*) and the three options beside them, filled once from the object's options
struct cond_toggles {
  bool no_pre = false;             // NO_COND_PRE: the per-cell set-up per droplet instead (k_cond<T, true>)
  bool sorted_order = false;       // COND_SORTED_ORDER: the positional form, over the sorted order
  bool two_pass = false;           // COND_TOMS_TWO_PASS: round 2's kernels where cond_solver = 1 (toms_two_pass())
  bool no_fold = false;            // COND_NO_FOLD
  bool lean_r3 = false;            // COND_LEAN_R3
  bool fold = false;               // COND_FOLD
  bool wq = false, wq_cap128 = false, wq_pf = false, wq_pf2 = false;      // COND_WQ and its three variants
  bool budget = false;             // COND_BUDGET: the first pass's loop with a budget of trips, records, k_cond_lean_resume
  bool probe = false;              // COND_PROBE
  bool no_list = false;            // COND_NO_LIST
  bool finish_staged = false;      // FINISH_STAGED
  bool substep_variant = false;    // one of per_substep_variants is set
  bool strict_fp = false; int cond_solver = 0; bool exact_sstp_cond = false;

  // (a measurement switch that names one of the per-substep kernels gets that kernel)
  static constexpr unsigned per_substep_variants = LCX_DBG_COND_NO_FUSED_SUBSTEPS | LCX_DBG_COND_FOLD | LCX_DBG_COND_WQ | LCX_DBG_COND_BUDGET | LCX_DBG_COND_PROBE |
                                                   LCX_DBG_COND_LEAN_R3 | LCX_DBG_FINISH_STAGED | LCX_DBG_COND_NO_FOLD;
  cond_toggles() = default;
  cond_toggles(unsigned dbg_flags, bool strict, int solver, bool exact)
    : no_pre(dbg_flags & LCX_DBG_NO_COND_PRE), sorted_order(dbg_flags & LCX_DBG_COND_SORTED_ORDER), two_pass(dbg_flags & LCX_DBG_COND_TOMS_TWO_PASS),
      no_fold(dbg_flags & LCX_DBG_COND_NO_FOLD), lean_r3(dbg_flags & LCX_DBG_COND_LEAN_R3), fold(dbg_flags & LCX_DBG_COND_FOLD), wq(dbg_flags & LCX_DBG_COND_WQ),
      wq_cap128(dbg_flags & LCX_DBG_COND_WQ_CAP128), wq_pf(dbg_flags & LCX_DBG_COND_WQ_PF), wq_pf2(dbg_flags & LCX_DBG_COND_WQ_PF2), budget(dbg_flags & LCX_DBG_COND_BUDGET),
      probe(dbg_flags & LCX_DBG_COND_PROBE), no_list(dbg_flags & LCX_DBG_COND_NO_LIST), finish_staged(dbg_flags & LCX_DBG_FINISH_STAGED),
      substep_variant(dbg_flags & per_substep_variants), strict_fp(strict), cond_solver(solver), exact_sstp_cond(exact) {}

  bool toms() const { return cond_solver == 1; }
  bool toms_two_pass() const { return toms() && two_pass; }
  // the per-cell set-up hoisted (k_cell_cond_pre) and one scratch value per droplet, the change of n rw^3; else n rw^3 before and after
  bool fast(bool turb_cond) const { return !strict_fp && !turb_cond && !no_pre; }
  // the condensation kernel will be a storage-order one of the lean family: the step's re-sort may ride on it (carries_scatter)
  bool lean_storage() const { return !strict_fp && !no_pre && !sorted_order && !toms_two_pass() && !exact_sstp_cond; }
  // does a per-substep launch carry the scatter of a sort that was left to it?
  bool carries_scatter(bool sort_deferred, bool turb_cond, size_t npart) const { return sort_deferred && lean_storage() && !turb_cond && npart != 0; }
  int wq_cap() const { return wq_cap128 ? 128 : 96; }
  int wq_prefetch() const { return wq_pf2 ? 2 : wq_pf ? 1 : 0; }
};

// ---- the route of a step_cond: exact per-particle substepping, every substep in ONE launch (k_cond_substeps, round 6: fast arithmetic,
// sstp_cond > 1, the sorted order in place), or a cell pass, a kernel and a finish per substep ----
enum class cond_route { PER_PARTICLE, SUBSTEPS_FUSED, PER_SUBSTEP };
struct cond_route_plan { cond_route route; bool sort_ahead; };      // sort_ahead: hskpng_sort ahead of the route (else its first kernel carries the scatter)
inline cond_route_plan cond_route_of(const cond_toggles &t, int sstp_cond, int sstp_cond_act, bool sort_deferred, bool turb_cond, size_t npart)
{
  if (t.exact_sstp_cond && (sstp_cond > 1 || sstp_cond_act > 1)) return {cond_route::PER_PARTICLE, true};
  if (sstp_cond > 1 && t.lean_storage() && !turb_cond && npart != 0 && !t.substep_variant) return {cond_route::SUBSTEPS_FUSED, true};
  return {cond_route::PER_SUBSTEP, !t.carries_scatter(sort_deferred, turb_cond, npart)};
}

// ---- opts_init.dbg_cond_budget, a test / measurement value with five meanings, decoded once ----
struct cond_budget {
  static constexpr int FOLD_STAGE = 128;           // k_cond_lean_fold's LDS stage (lcx_kernels.hpp FOLD_CAP)
  static constexpr unsigned NO_BUDGET = 100u;      // a first pass without a budget of trips: the solver's own iteration limit
  static constexpr unsigned LIST_TRIPS = 2u;       // COND_BUDGET's default
  // two passes: a short iteration budget first, the droplets that need more in a dense second launch (k_cond_fast).  The second launch
  // costs what its slowest wave costs (~60 us) however few droplets it holds, and the first pass saves ~2.3 us per million droplets: one
  // pass below 2^25 droplets (a 16-plane slab of C3, 16.7e6 SDs: 0.96 ms in two passes, 0.91 in one).
  static constexpr unsigned TWO_PASS_FIRST = 6u; static constexpr size_t TWO_PASS_FROM = size_t(1) << 25;
  int x = 0;
  bool low_byte() const { return x > 0 && (x & 255); }
  // k_cond_lean_fold: slots of its stage in use (a test makes it small so that droplets stay behind)
  unsigned fold_stage() const { return unsigned(x > 0 ? std::min(x, FOLD_STAGE) : FOLD_STAGE); }
  // COND_BUDGET: the trips of the first pass's loop (x & 255) ...
  unsigned list_trips() const { return low_byte() ? unsigned(x & 255) : LIST_TRIPS; }
  // ... and the records per part: x >> 8, a test's own capacity; else 3 % of the part's droplets (bench.py's settled boxes leave 1 %)
  uint32_t records_per_part(size_t shard_cap) const { return x > 255 ? uint32_t(x >> 8) : uint32_t(std::max<size_t>(256, shard_cap * 3 / 100)); }
  // COND_WQ: batches of 64 slots per wave (x & 255: tests, measurements); else 8, fewer in a small box -- enough workgroups to fill the device first
  unsigned wq_batches(unsigned chunks) const
  {
    unsigned nb = 8u;
    while (nb > 1 && chunks / nb < 2048u) nb /= 2;
    return low_byte() ? unsigned(x & 255) : nb;
  }
  // COND_TOMS_TWO_PASS: the first pass's iterations (the parity tests force the two-pass form at their small sizes with it); 0: one pass
  unsigned two_pass_first(size_t npart) const { return x > 0 ? unsigned(x) : x < 0 ? 0u : npart >= TWO_PASS_FROM ? TWO_PASS_FIRST : 0u; }
};

// ---- the kernel of a per-substep launch (enum lcx_cond_kernel: what "raw_mode" reports) and what the launch needs beyond the name ----
enum class cond_budget_form { NONE, TWO, RUN_TIME };       // no budget; two trips as straight-line code; the run-time form of the loop
struct cond_kernel_plan {
  lcx_cond_kernel kernel;
  bool fast;                       // cond_toggles::fast: the cell pass leaves the set-up, the kernel one value per droplet, the finish takes deltas
  bool storage_order;              // over the storage (its cells from ijk, the scatter may ride on it) instead of the sorted order
  bool uni;                        // one hygroscopicity in the whole run and the kernel takes it as a scalar
  bool want_list;                  // leaves a list of droplets for the reference's iterates (k_cond_lean_listed)
  unsigned trips;                  // ... whose first pass gives every droplet's loop that many trips (cond_budget::NO_BUDGET: its own limit) ...
  cond_budget_form budget;         // ... and below that limit leaves records for k_cond_lean_resume, in this form of the loop
  bool probe;                      // the seven k_cond_probe launches go first (measurement only)
};
// the precedence of the rounds: each later one only where the earlier one's condition does not hold
inline cond_kernel_plan cond_kernel_of(const cond_toggles &t, const cond_budget &b, bool turb_cond, bool kpa_uniform)
{
  using BF = cond_budget_form;
  constexpr unsigned NB = cond_budget::NO_BUDGET;
  if (t.strict_fp) return {LCX_CK_STRICT, false, false, false, false, NB, BF::NONE, false};
  if (!t.fast(turb_cond)) return {LCX_CK_FAST_PER_DROPLET_SETUP, false, false, false, false, NB, BF::NONE, false};
  if (t.toms_two_pass()) return {LCX_CK_TOMS748_TWO_PASS, true, false, false, false, NB, BF::NONE, false};
  const bool list = !t.toms() && !t.no_list;
  // (the budget: measured and not adopted -- the first pass 3.0 -> 2.75 ms, its second pass 0.26 ms beside the ranking: the step as before)
  const unsigned trips = t.budget && !t.wq ? b.list_trips() : NB;
  const bool records = list && trips < NB;
  if (t.sorted_order) {
    if (t.toms()) return {LCX_CK_LEAN_TOMS748_SORTED, true, false, false, false, NB, BF::NONE, false};
    return {LCX_CK_LEAN_SORTED, true, false, false, list, trips, records ? BF::RUN_TIME : BF::NONE, false};
  }
  // (cond_solver = 1: the workgroup folded behind TOMS748's head -- this kernel is bound by instruction issue at half-empty waves, unlike
  // the lean solver's; COND_NO_FOLD: the plain kernel, the same bits)
  if (t.toms()) return {t.no_fold ? LCX_CK_LEAN_TOMS748 : LCX_CK_FOLD_TOMS748, true, true, kpa_uniform, false, NB, BF::NONE, false};
  if (t.lean_r3) return {LCX_CK_LEAN_R3, true, true, false, false, NB, BF::NONE, false};
  // (round 5, measured and kept behind a switch: the workgroup folded behind the solver's first loop trip -- the same bits, 6 % fewer vector
  // instructions per wave at a higher lane use, and not faster: the chip runs this kernel at its package power cap, where what a launch
  // costs is the lanes that compute, not the instructions that issue; see k_cond_lean_fold)
  if (t.fold) return {LCX_CK_FOLD_LEAN, true, true, kpa_uniform, false, NB, BF::NONE, false};
  // (round 6: a wave walks its batches and keeps the droplets whose first loop trip has not converged on a queue of its own in LDS,
  // k_cond_lean_wq: its queue takes the droplets that need more trips, so never a budget)
  if (t.wq) return {LCX_CK_LEAN_WQ, true, true, kpa_uniform, list, NB, BF::NONE, false};
  return {LCX_CK_LEAN, true, true, kpa_uniform, list, trips, !records ? BF::NONE : trips == 2u ? BF::TWO : BF::RUN_TIME, t.probe && kpa_uniform};
}

// ---- launch geometry: plain integers from the droplets, the cells, the workgroup (BS), the parts (DEFER_SHARDS) and the capacity ----
inline unsigned cond_blocks(size_t n, unsigned bs) { return unsigned((n + bs - 1) / bs); }
// the lean solver's list (cond_list), in `shards` parts with one counter each: a part's capacity for a launch of `blocks` workgroups of
// `per_block` droplets (part s holds at most the droplets of the workgroups b with b % shards == s)
inline size_t cond_list_shard_cap(size_t blocks, size_t per_block, unsigned shards) { return cond_blocks(blocks, shards) * per_block; }
// k_cond_lean_listed: the host does not know the counts -- workgroups for 1 % of the droplets (the settled boxes list 0.1 %, a swinging
// one 1 %) at a droplet per lane, more droplets by the stride; a workgroup that finds nothing leaves at once.  Per part:
inline unsigned cond_listed_per_part(size_t shard_cap, unsigned bs) { return unsigned(std::min<size_t>(2048, std::max<size_t>(8, shard_cap / 100 / bs + 1))); }
// k_cond_lean_resume: a lane per record
inline unsigned cond_resume_grid(uint32_t rec_cap, unsigned bs, unsigned shards) { return shards * ((rec_cap + bs - 1) / bs); }
// k_cond_lean_wq: a workgroup of `batches` chunks
inline unsigned cond_wq_grid(unsigned chunks, unsigned batches) { return (chunks + batches - 1) / batches; }
// the two-pass form: its parts (`rank` is free between the sorts; part s holds at most the positions of the workgroups b with b % shards
// == s), the first pass's budget -- none where the parts do not fit the scratch, tiny set-ups -- and the second launch's workgroups per part
inline size_t cond_two_pass_shard_cap(size_t npart, unsigned bs, unsigned shards) { return size_t(cond_blocks(cond_blocks(npart, bs), shards)) * bs; }
inline unsigned cond_two_pass_budget(const cond_budget &b, size_t npart, unsigned bs, unsigned shards, size_t capacity)
{ return size_t(shards) * cond_two_pass_shard_cap(npart, bs, shards) > capacity ? 0u : b.two_pass_first(npart); }
inline unsigned cond_two_pass_per_shard(size_t npart, unsigned bs, unsigned shards) { return std::max(1u, std::min(cond_blocks(npart / 8 + 1, bs), 256u * 64u) / shards); }
// k_cond_substeps: a workgroup owns a run of cells and their droplets -- bs / (droplets per cell) cells, `cells_max` at most, at least one
inline unsigned cond_substeps_cells_per_wg(size_t npart, size_t ncell, unsigned bs, unsigned cells_max)
{
  const unsigned per_cell = unsigned(std::max<size_t>(1, npart / std::max<size_t>(1, ncell)));
  return std::max(1u, std::min(cells_max, bs / per_cell));
}

// ---- the per-cell finish (enum lcx_cond_finish: "raw_cond_finish"): per-cell sums of n rw^3 before / after the substep + update_th_rv.
// Strict arithmetic: the ordered single-lane walk (the reference's summation order); fast: a whole wave per cell where cells are crowded,
// else eight lanes per cell -- straight from the deltas where they lie in the sorted order (no gather) unless FINISH_STAGED ----
constexpr size_t COND_FINISH_WAVE_CELLS = 4096, COND_FINISH_WAVE_PER_CELL = 192;
inline lcx_cond_finish cond_finish_of(bool strict_fp, bool delta, bool gather, bool staged, size_t ncell, size_t npart)
{
  if (strict_fp) return LCX_CF_ORDERED;
  if (ncell >= COND_FINISH_WAVE_CELLS && npart / ncell >= COND_FINISH_WAVE_PER_CELL) return LCX_CF_WAVE;
  return delta && !gather && !staged ? LCX_CF_DIRECT : LCX_CF_LANES8;
}

} // namespace lcx
#endif
