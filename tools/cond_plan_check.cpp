// The host side of the condensation's launches (csrc/lcx_cond_plan.hpp) in a program of its own: the kernel of a per-substep launch over
// every combination of the switches against the precedence of the rounds, each rule stated on its own; the rows of tests/test_hip_cond.py
// (what each of its objects must report); the route of a step_cond and who carries the scatter; the five meanings of dbg_cond_budget and the
// launch sizes at hand-computed values; the form of the per-cell finish with its thresholds on both sides.  No HIP include: the host
// compiler alone (tests/test_cond_plan_host.py builds it with -fsanitize=address,undefined).
#include <cstdio>
#include <cstdlib>

#include "../libcloudphxx_amd/csrc/lcx_cond_plan.hpp"

using namespace lcx;

static long checks = 0;
static void need(bool ok, const char *what, long at = -1)
{
  ++checks;
  if (!ok) { std::fprintf(stderr, "FAILED: %s (inputs %ld)\n", what, at); std::exit(1); }
}
static bool bit(unsigned m, int i) { return (m >> i) & 1u; }

// the switches that the plan reads, one bit of the enumeration each (the three variants of COND_WQ pick no kernel of enum lcx_cond_kernel)
static const unsigned FLAGS[] = {LCX_DBG_NO_COND_PRE, LCX_DBG_COND_SORTED_ORDER, LCX_DBG_COND_TOMS_TWO_PASS, LCX_DBG_COND_NO_FOLD, LCX_DBG_COND_LEAN_R3, LCX_DBG_COND_FOLD,
                                 LCX_DBG_COND_WQ, LCX_DBG_COND_BUDGET, LCX_DBG_COND_PROBE, LCX_DBG_COND_NO_LIST, LCX_DBG_COND_NO_FUSED_SUBSTEPS, LCX_DBG_FINISH_STAGED};
constexpr int N_FLAGS = sizeof(FLAGS) / sizeof(FLAGS[0]);
static unsigned flags_of(unsigned m) { unsigned f = 0; for (int i = 0; i < N_FLAGS; ++i) if (bit(m, i)) f |= FLAGS[i]; return f; }

// what an object reports after a step_cond: the route's own kernel (cond_perparticle, cond_substeps_fused), or the per-substep launch's
static int reported(const cond_toggles &t, const cond_budget &b, int sstp_cond, int sstp_cond_act, bool kpa_uniform)
{
  const cond_route_plan rt = cond_route_of(t, sstp_cond, sstp_cond_act, false, false, 1000);
  if (rt.route == cond_route::PER_PARTICLE) return LCX_CK_PER_PARTICLE;
  if (rt.route == cond_route::SUBSTEPS_FUSED) return LCX_CK_SUBSTEPS;
  return cond_kernel_of(t, b, false, kpa_uniform).kernel;
}

int main()
{
  using BF = cond_budget_form;
  // ---- 1. the kernel of a per-substep launch: every combination of the switches, strict, solver, turb_cond, kpa_uniform; five budgets ----
  const int budgets[] = {0, 1, 2, 3, 200};
  for (unsigned m = 0; m < (1u << (N_FLAGS + 4)); ++m)
    for (int bx : budgets) {
      const unsigned f = flags_of(m);
      const bool strict = bit(m, N_FLAGS), toms = bit(m, N_FLAGS + 1), turb = bit(m, N_FLAGS + 2), kpa = bit(m, N_FLAGS + 3);
      const bool no_pre = f & LCX_DBG_NO_COND_PRE, sorted = f & LCX_DBG_COND_SORTED_ORDER, two = f & LCX_DBG_COND_TOMS_TWO_PASS, no_fold = f & LCX_DBG_COND_NO_FOLD;
      const bool r3 = f & LCX_DBG_COND_LEAN_R3, fold = f & LCX_DBG_COND_FOLD, wq = f & LCX_DBG_COND_WQ, budget = f & LCX_DBG_COND_BUDGET, probe = f & LCX_DBG_COND_PROBE;
      const bool no_list = f & LCX_DBG_COND_NO_LIST;
      const cond_toggles t(f, strict, toms ? 1 : 0, false);
      const cond_budget b{bx};
      const cond_kernel_plan kp = cond_kernel_of(t, b, turb, kpa);
      const long at = long(m) * 1000 + bx;
      // the precedence, rule by rule: each names its kernel from the switches alone, and exactly one holds
      const bool per_droplet = !strict && (turb || no_pre), fast = !strict && !per_droplet, two_pass = fast && toms && two, lean = fast && !two_pass;
      const bool rule[12] = {false,
        /* STRICT */ strict,
        /* FAST_PER_DROPLET_SETUP */ per_droplet,
        /* LEAN */ lean && !sorted && !toms && !r3 && !fold && !wq,
        /* LEAN_SORTED */ lean && sorted && !toms,
        /* FOLD_TOMS748 */ lean && !sorted && toms && !no_fold,
        /* LEAN_TOMS748 */ lean && !sorted && toms && no_fold,
        /* LEAN_TOMS748_SORTED */ lean && sorted && toms,
        /* TOMS748_TWO_PASS */ two_pass,
        /* LEAN_R3 */ lean && !sorted && !toms && r3,
        /* FOLD_LEAN */ lean && !sorted && !toms && !r3 && fold,
        /* LEAN_WQ */ lean && !sorted && !toms && !r3 && !fold && wq};
      int holding = 0;
      for (int k = 1; k < 12; ++k) holding += rule[k];
      need(holding == 1, "exactly one form per combination", at);
      need(kp.kernel >= LCX_CK_STRICT && kp.kernel <= LCX_CK_LEAN_WQ && rule[kp.kernel], "the plan names the form whose rule holds", at);
      need((kp.kernel == LCX_CK_STRICT) == strict, "strict arithmetic comes first", at);
      if (!strict) need((kp.kernel == LCX_CK_FAST_PER_DROPLET_SETUP) == (turb || no_pre), "then the per-droplet set-up: turb_cond or NO_COND_PRE", at);
      if (two_pass) need(kp.kernel == LCX_CK_TOMS748_TWO_PASS, "then the two-pass form", at);
      if (kp.kernel == LCX_CK_LEAN_R3) need(!kp.uni && !kp.want_list, "LEAN_R3: the array form and no list even with one kappa", at);
      if (lean && !sorted && !toms && r3) need(kp.kernel == LCX_CK_LEAN_R3, "LEAN_R3 ahead of FOLD and WQ", at);
      if (lean && !sorted && !toms && !r3 && fold) need(kp.kernel == LCX_CK_FOLD_LEAN, "FOLD ahead of WQ", at);
      if (lean && sorted) need(kp.kernel == LCX_CK_LEAN_SORTED || kp.kernel == LCX_CK_LEAN_TOMS748_SORTED, "in sorted order: the two sorted forms, whatever else is set", at);
      // what the launch needs beyond the name
      need(kp.fast == fast, "fast: neither strict nor the per-droplet set-up", at);
      need(kp.storage_order == (lean && !sorted), "storage order: the lean family unless COND_SORTED_ORDER", at);
      need(kp.uni == (kpa && kp.storage_order && kp.kernel != LCX_CK_LEAN_R3), "scalar kappa: one kappa, storage order, not LEAN_R3", at);
      if (kp.want_list) need(!toms && !no_list, "a list only with solver 0 and without COND_NO_LIST", at);
      need(kp.want_list == (!no_list && (kp.kernel == LCX_CK_LEAN || kp.kernel == LCX_CK_LEAN_SORTED || kp.kernel == LCX_CK_LEAN_WQ)), "a list from k_cond_lean and k_cond_lean_wq alone", at);
      need(kp.probe == (kp.kernel == LCX_CK_LEAN && kpa && probe), "the probe only in the plain lean form with one kappa", at);
      if (kp.want_list) need(kp.trips == (budget && !wq ? (bx & 255 ? unsigned(bx & 255) : 2u) : 100u), "the list's trips: COND_BUDGET's unless COND_WQ, else the solver's own limit", at);
      need((kp.budget != BF::NONE) == (kp.want_list && kp.kernel != LCX_CK_LEAN_WQ && kp.trips < 100u), "records where a list, a budget below the solver's own limit", at);
      need((kp.budget == BF::TWO) == (kp.kernel == LCX_CK_LEAN && kp.want_list && kp.trips == 2u), "two trips as straight-line code: the plain lean form alone", at);
      // the kernel that is to carry a scatter is a storage-order one
      for (int exact = 0; exact < 2; ++exact) {
        const cond_toggles te(f, strict, toms ? 1 : 0, exact != 0);
        if (te.carries_scatter(true, turb, 7)) need(kp.storage_order && kp.fast, "a scatter rides on a storage-order kernel of the lean family only", at);
      }
    }
  // ---- 2. tests/test_hip_cond.py: what each of its objects must report (KERNELS, test_substeps, and exact per-particle substepping) ----
  {
    struct row { const char *name; bool strict; int solver; unsigned flags; int budget; int sstp; bool exact; int kernel; };
    const row rows[] = {
      {"strict", true, 0, 0, 0, 1, false, LCX_CK_STRICT},
      {"fast_per_droplet_setup", false, 0, LCX_DBG_NO_COND_PRE, 0, 1, false, LCX_CK_FAST_PER_DROPLET_SETUP},
      {"lean", false, 0, 0, 0, 1, false, LCX_CK_LEAN},
      {"lean_sorted", false, 0, LCX_DBG_COND_SORTED_ORDER, 0, 1, false, LCX_CK_LEAN_SORTED},
      {"fold_toms748", false, 1, 0, 0, 1, false, LCX_CK_FOLD_TOMS748},
      {"lean_toms748", false, 1, LCX_DBG_COND_NO_FOLD, 0, 1, false, LCX_CK_LEAN_TOMS748},
      {"lean_toms748_sorted", false, 1, LCX_DBG_COND_SORTED_ORDER, 0, 1, false, LCX_CK_LEAN_TOMS748_SORTED},
      {"toms748_two_pass_3", false, 1, LCX_DBG_COND_TOMS_TWO_PASS, 3, 1, false, LCX_CK_TOMS748_TWO_PASS},
      {"toms748_two_pass_all", false, 1, LCX_DBG_COND_TOMS_TWO_PASS, -1, 1, false, LCX_CK_TOMS748_TWO_PASS},
      {"lean_r3", false, 0, LCX_DBG_COND_LEAN_R3, 0, 1, false, LCX_CK_LEAN_R3},
      {"fold_lean", false, 0, LCX_DBG_COND_FOLD, 0, 1, false, LCX_CK_FOLD_LEAN},
      {"lean_wq", false, 0, LCX_DBG_COND_WQ, 0, 1, false, LCX_CK_LEAN_WQ},
      {"lean_wq_cap128", false, 0, LCX_DBG_COND_WQ | LCX_DBG_COND_WQ_CAP128, 0, 1, false, LCX_CK_LEAN_WQ},
      {"lean_resume_1", false, 0, LCX_DBG_COND_BUDGET, 1, 1, false, LCX_CK_LEAN},
      {"lean_resume_2", false, 0, LCX_DBG_COND_BUDGET, 2, 1, false, LCX_CK_LEAN},
      {"lean_finish_staged", false, 0, LCX_DBG_FINISH_STAGED, 0, 1, false, LCX_CK_LEAN},
      {"lean_sorted_finish_staged", false, 0, LCX_DBG_COND_SORTED_ORDER | LCX_DBG_FINISH_STAGED, 0, 1, false, LCX_CK_LEAN_SORTED},
      {"substeps fused, solver 0", false, 0, 0, 0, 4, false, LCX_CK_SUBSTEPS},
      {"substeps fused, solver 1", false, 1, 0, 0, 4, false, LCX_CK_SUBSTEPS},
      {"substeps one by one, solver 0", false, 0, LCX_DBG_COND_NO_FUSED_SUBSTEPS, 0, 4, false, LCX_CK_LEAN},
      {"substeps one by one, solver 1", false, 1, LCX_DBG_COND_NO_FUSED_SUBSTEPS, 0, 4, false, LCX_CK_FOLD_TOMS748},
      {"per particle", false, 0, 0, 0, 4, true, LCX_CK_PER_PARTICLE},
    };
    for (const row &r : rows)
      for (int kpa = 0; kpa < 2; ++kpa)
        need(reported(cond_toggles(r.flags, r.strict, r.solver, r.exact), cond_budget{r.budget}, r.sstp, 1, kpa != 0) == r.kernel, r.name);
    // the two resume rows take the two forms of the budget's loop, with records; the plain row neither
    const cond_toggles tb(LCX_DBG_COND_BUDGET, false, 0, false), t0(0, false, 0, false);
    need(cond_kernel_of(tb, cond_budget{1}, false, false).budget == BF::RUN_TIME && cond_kernel_of(tb, cond_budget{1}, false, false).trips == 1u, "lean_resume_1: one trip, the run-time form");
    need(cond_kernel_of(tb, cond_budget{2}, false, true).budget == BF::TWO, "lean_resume_2: two trips as straight-line code");
    need(cond_kernel_of(t0, cond_budget{0}, false, true).budget == BF::NONE && cond_kernel_of(t0, cond_budget{0}, false, true).want_list, "lean: a list and no budget");
    need(cond_toggles(LCX_DBG_COND_WQ | LCX_DBG_COND_WQ_CAP128, false, 0, false).wq_cap() == 128 && cond_toggles(LCX_DBG_COND_WQ, false, 0, false).wq_cap() == 96, "the queue: 96 entries, 128 with CAP128");
    need(cond_toggles(LCX_DBG_COND_WQ_PF, false, 0, false).wq_prefetch() == 1 && cond_toggles(LCX_DBG_COND_WQ_PF | LCX_DBG_COND_WQ_PF2, false, 0, false).wq_prefetch() == 2 && t0.wq_prefetch() == 0,
         "the prefetch: 0, PF 1, PF2 2");
  }
  // ---- 3. the route of a step_cond and who carries the scatter: every combination of their inputs ----
  for (unsigned m = 0; m < (1u << (N_FLAGS + 8)); ++m) {
    const unsigned f = flags_of(m);
    const bool strict = bit(m, N_FLAGS), toms = bit(m, N_FLAGS + 1), exact = bit(m, N_FLAGS + 2), deferred = bit(m, N_FLAGS + 3), turb = bit(m, N_FLAGS + 4);
    const int sstp = bit(m, N_FLAGS + 5) ? 3 : 1, sstp_act = bit(m, N_FLAGS + 6) ? 2 : 1;
    const size_t npart = bit(m, N_FLAGS + 7) ? 5 : 0;
    const cond_toggles t(f, strict, toms ? 1 : 0, exact);
    const cond_route_plan rt = cond_route_of(t, sstp, sstp_act, deferred, turb, npart);
    const bool lean_storage = !strict && !(f & LCX_DBG_NO_COND_PRE) && !(f & LCX_DBG_COND_SORTED_ORDER) && !(toms && (f & LCX_DBG_COND_TOMS_TWO_PASS)) && !exact;
    need(t.lean_storage() == lean_storage, "lean_storage: fast, per-cell set-up, storage order, not two-pass, not exact_sstp_cond", m);
    need(t.toms_two_pass() == (toms && (f & LCX_DBG_COND_TOMS_TWO_PASS)), "toms_two_pass: solver 1 with the switch", m);
    const bool carried = t.carries_scatter(deferred, turb, npart);
    need(carried == (deferred && lean_storage && !turb && npart != 0), "carries_scatter: a deferred sort, lean storage, no turb_cond, droplets", m);
    need((rt.route == cond_route::PER_PARTICLE) == (exact && (sstp > 1 || sstp_act > 1)), "PER_PARTICLE iff exact_sstp_cond with substeps", m);
    const bool masked = f & (LCX_DBG_COND_NO_FUSED_SUBSTEPS | LCX_DBG_COND_FOLD | LCX_DBG_COND_WQ | LCX_DBG_COND_BUDGET | LCX_DBG_COND_PROBE | LCX_DBG_COND_LEAN_R3 | LCX_DBG_FINISH_STAGED |
                             LCX_DBG_COND_NO_FOLD);
    if (rt.route == cond_route::SUBSTEPS_FUSED) need(!masked && !turb && npart != 0 && sstp > 1 && lean_storage, "SUBSTEPS_FUSED never with a switch of the mask, turb_cond or no droplets", m);
    if (rt.route != cond_route::PER_PARTICLE) need((rt.route == cond_route::SUBSTEPS_FUSED) == (sstp > 1 && lean_storage && !turb && npart != 0 && !masked), "SUBSTEPS_FUSED wherever all of it holds", m);
    need(rt.sort_ahead == !(rt.route == cond_route::PER_SUBSTEP && carried), "the sort is made ahead exactly when the scatter is not carried", m);
    if (!rt.sort_ahead) need(cond_kernel_of(t, cond_budget{}, turb, false).storage_order, "a sort left to the kernel: a storage-order kernel takes it", m);
  }
  // ---- 4a. dbg_cond_budget: {x, fold stage, trips, records of a part of 1000 / of 10000, batches at 16384 chunks, first pass below / from 2^25} ----
  {
    const size_t big = size_t(1) << 25;
    const long rows[][8] = {
      {0, 128, 2, 256, 300, 8, 0, 6}, {-5, 128, 2, 256, 300, 8, 0, 0}, {1, 1, 1, 256, 300, 1, 1, 1}, {2, 2, 2, 256, 300, 2, 2, 2}, {255, 128, 255, 256, 300, 255, 255, 255},
      {256, 128, 2, 1, 1, 8, 256, 256}, {256 + 3, 128, 3, 1, 1, 3, 259, 259}, {(4 << 8) | 3, 128, 3, 4, 4, 3, 1027, 1027}, {200, 128, 200, 256, 300, 200, 200, 200}};
    for (const auto &r : rows) {
      const cond_budget b{int(r[0])};
      need(b.fold_stage() == unsigned(r[1]), "the fold kernel's stage: min(x, FOLD_CAP), FOLD_CAP where x <= 0", r[0]);
      need(b.list_trips() == unsigned(r[2]), "COND_BUDGET's trips: x & 255, else 2", r[0]);
      need(b.records_per_part(1000) == uint32_t(r[3]) && b.records_per_part(10000) == uint32_t(r[4]), "records per part: x >> 8, else 3 % with a floor of 256", r[0]);
      need(b.wq_batches(16384) == unsigned(r[5]), "COND_WQ's batches: x & 255, else 8 at 16384 chunks", r[0]);
      need(b.two_pass_first(big - 1) == unsigned(r[6]) && b.two_pass_first(big) == unsigned(r[7]), "the two-pass budget: x, none below 0, 6 from 2^25 droplets at 0", r[0]);
    }
    const cond_budget none{};
    need(none.wq_batches(16383) == 4 && none.wq_batches(4096) == 2 && none.wq_batches(4095) == 1 && none.wq_batches(0) == 1, "batches of a small box: 2048 workgroups first");
  }
  // ---- 4b. launch geometry at BS = 256 and 64 parts, by hand ----
  {
    const unsigned BS = 256, SH = 64;
    const size_t big = size_t(1) << 25;
    const size_t np[] = {0, 1, 255, 256, 257, big - 1, big};
    const unsigned blocks[] = {0, 1, 1, 1, 2, 131072, 131072};
    const size_t list_cap[] = {0, 256, 256, 256, 256, 524288, 524288};                 // ceil(blocks / 64) * 256
    const unsigned per_part[] = {8, 8, 8, 8, 8, 21, 21};                               // cap / 100 / 256 + 1, at least 8
    const uint32_t rec_cap[] = {256, 256, 256, 256, 256, 15728, 15728};                // 3 % of the part, at least 256
    const unsigned n_resume[] = {64, 64, 64, 64, 64, 3968, 3968};                      // 64 * ceil(rec_cap / 256)
    const unsigned per_shard[] = {1, 1, 1, 1, 1, 256, 256};                            // min(blocks(n / 8 + 1), 16384) / 64, at least 1
    const unsigned cells_1[] = {64, 64, 1, 1, 1, 1, 1};                                // one cell: 256 / (droplets per cell), 64 at most, 1 at least
    for (int i = 0; i < 7; ++i) {
      need(cond_blocks(np[i], BS) == blocks[i], "workgroups of 256", i);
      need(cond_list_shard_cap(blocks[i], BS, SH) == list_cap[i] && cond_two_pass_shard_cap(np[i], BS, SH) == list_cap[i], "a part's capacity, the list's and the two-pass form's", i);
      need(cond_listed_per_part(list_cap[i], BS) == per_part[i], "the listed pass's workgroups per part", i);
      need(cond_budget{}.records_per_part(list_cap[i]) == rec_cap[i] && cond_resume_grid(rec_cap[i], BS, SH) == n_resume[i], "rec_cap and the resume pass's grid", i);
      need(cond_two_pass_per_shard(np[i], BS, SH) == per_shard[i], "the two-pass form's second launch", i);
      need(cond_substeps_cells_per_wg(np[i], 1, BS, 64) == cells_1[i], "cells per workgroup of the fused substeps, one cell", i);
    }
    need(cond_list_shard_cap(16384, size_t(BS) * 8, SH) == 256 * 2048, "the work queue's parts: 256 workgroups of 2048 droplets each");
    need(cond_listed_per_part(52400000, BS) == 2047 && cond_listed_per_part(52428800, BS) == 2048 && cond_listed_per_part(size_t(1) << 40, BS) == 2048, "2048 workgroups per part at most");
    need(cond_resume_grid(1, BS, SH) == 64 && cond_resume_grid(257, BS, SH) == 128 && cond_resume_grid(0, BS, SH) == 0, "a lane per record");
    need(cond_wq_grid(131072, 8) == 16384 && cond_wq_grid(5, 4) == 2 && cond_wq_grid(0, 1) == 0, "the work queue's grid");
    need(cond_two_pass_per_shard(262144, BS, SH) == 2, "129 workgroups in 64 parts: 2 each");
    // a capacity that is just too small for the parts drops the budget
    need(cond_two_pass_budget(cond_budget{}, big, BS, SH, big) == 6 && cond_two_pass_budget(cond_budget{}, big, BS, SH, big - 1) == 0, "2^25 droplets: 64 parts of 2^19 fit 2^25, not 2^25 - 1");
    need(cond_two_pass_budget(cond_budget{3}, 257, BS, SH, 16384) == 3 && cond_two_pass_budget(cond_budget{3}, 257, BS, SH, 16383) == 0, "257 droplets: 64 parts of 256 need 16384");
    need(cond_two_pass_budget(cond_budget{-1}, 257, BS, SH, 16384) == 0 && cond_two_pass_budget(cond_budget{}, big - 1, BS, SH, big) == 0, "no budget asked for, or below 2^25: one pass");
    // the fused substeps over 1, 4095 and 4096 cells
    const size_t cells[] = {1, 4095, 4096};
    for (size_t nc : cells) {
      need(cond_substeps_cells_per_wg(191 * nc, nc, BS, 64) == 1 && cond_substeps_cells_per_wg(192 * nc, nc, BS, 64) == 1, "191 and 192 per cell: one cell per workgroup", long(nc));
      need(cond_substeps_cells_per_wg(5 * nc, nc, BS, 64) == 51 && cond_substeps_cells_per_wg(4 * nc, nc, BS, 64) == 64 && cond_substeps_cells_per_wg(3 * nc, nc, BS, 64) == 64, "5, 4, 3 per cell: 51, 64, 64", long(nc));
      need(cond_substeps_cells_per_wg(0, nc, BS, 64) == 64 && cond_substeps_cells_per_wg(257 * nc, nc, BS, 64) == 1, "no droplets: 64; more than a workgroup's per cell: 1", long(nc));
    }
    need(cond_substeps_cells_per_wg(100, 0, BS, 64) == 2, "no cells counts as one");
  }
  // ---- 5. the per-cell finish: every combination of its inputs, 4096 cells and 192 per cell from both sides ----
  {
    const size_t cells[] = {1, 4095, 4096};
    for (unsigned m = 0; m < 16; ++m)
      for (size_t nc : cells)
        for (int k = 0; k < 3; ++k) {
          const bool strict = bit(m, 0), delta = bit(m, 1), gather = bit(m, 2), staged = bit(m, 3);
          const size_t npart = k == 0 ? 191 * nc : k == 1 ? 192 * nc - 1 : 192 * nc;           // (192 n - 1: 191 per cell in whole numbers)
          const lcx_cond_finish f = cond_finish_of(strict, delta, gather, staged, nc, npart);
          const long at = long(m) * 100000 + long(nc) * 10 + k;
          const bool crowded = nc >= 4096 && k == 2;
          need(f != LCX_CF_NONE, "a launch has a form", at);
          need((f == LCX_CF_ORDERED) == strict, "ORDERED iff strict arithmetic", at);
          need((f == LCX_CF_WAVE) == (!strict && crowded), "WAVE iff fast, at least 4096 cells, at least 192 per cell", at);
          need((f == LCX_CF_DIRECT) == (!strict && !crowded && delta && !gather && !staged), "DIRECT iff deltas in the sorted order, no gather, not staged", at);
          need((f == LCX_CF_LANES8) == (!strict && !crowded && !(delta && !gather && !staged)), "LANES8: the rest of the fast arithmetic", at);
        }
    need(cond_finish_of(false, true, false, false, 0, 0) == LCX_CF_DIRECT, "no cells: nothing is divided");
  }
  std::printf("ok: %ld checks\n", checks);
  return 0;
}
