// lcx_coal_plan.hpp -- what the coalescence settles on the host: which form its launch takes (coal_form_of), the two pause rules that switch
// the bound and the exit off where they do not pay (coal_adapt), and whether the draws made ahead are this launch's (coal_prevote_key).
// Results never depend on any of it: every form gives the same bits.
//
// No HIP include: lcx_core.hip's coal(), launch_umin(), step_async and its two polls decide with it, and tools/coal_plan_check.cpp compiles
// it alone under the host sanitizers.
#ifndef LCX_COAL_PLAN_HPP
#define LCX_COAL_PLAN_HPP

#include <cstdint>

namespace lcx {

// PAIRS: k_coal on an order that somebody has ranked.  The others rank for themselves (k_coal_ranked, round 7): plain; with the pair bound
// (SKIP, round 8); its workgroups leaving ahead of the ranking (EXIT, round 9); handed the tiles' flags of the cells' vote (TILES, round 10);
// and k_coal_cells, a wave per kept cell of the vote's list in place of the tiles (round 11).
enum class coal_form { PAIRS, RANKED, RANKED_SKIP, RANKED_EXIT, RANKED_TILES, CELLS };

// the debug bits that the plan reads (include/lcx.h LCX_DBG2_*), filled once from the object's flags
struct coal_toggles {
  bool counted = false;            // COAL_SKIP_COUNT: exact counters instead of the sample; never the list form
  bool no_rank_exit = false;       // NO_COAL_RANK_EXIT: no EXIT form, hence neither vote nor list
  bool rank_exit_always = false;   // COAL_RANK_EXIT_ALWAYS: the EXIT form whatever the last counters showed
  bool no_prevote = false;         // NO_COAL_PREVOTE: no draws ahead, hence neither TILES nor CELLS
  bool no_cell_list = false;       // NO_COAL_CELL_LIST: the vote leaves no list, hence never CELLS
  bool cell_list_always = false;   // COAL_CELL_LIST_ALWAYS: CELLS in every launch that is handed the flags
};

// The adaptive state: what the last counters that reached the host said, and for how long it holds.
struct coal_adapt {
  // the bound pays only where it skips: a sample of the launch's counters comes back to the host without a wait (a copy and an event, polled by
  // the next step_async); below COAL_SKIP_MIN_SHARE^-1 of the pairs skipped, COAL_SKIP_PAUSE steps run without maxima and without bound, then
  // one step probes again.  Results do not depend on it: a launch with the bound and one without give the same bits.
  static constexpr int COAL_SKIP_PAUSE = 32; static constexpr unsigned long long COAL_SKIP_MIN_SHARE = 200;      // (0.5 %)
  // Likewise the workgroups' exit ahead of the ranking (k_coal_ranked<.., SKIP, EXIT>): a workgroup that ranks after all pays for the vote and
  // for id loads one level later -- +0.17 ms on a launch of the 128^3 x 64 box in which none leaves, against -0.53 ms where all do, so the exit
  // breaks even at 0.17 / (0.17 + 0.53) = 0.24 of the workgroups leaving (EXPERIMENTS.md 7.10).  Below COAL_EXIT_MIN_PERCENT of them in a
  // launch's counters (or the sample of them) the next COAL_EXIT_PAUSE bound launches take round 8's form, then one probes again.  The same
  // bits either way.  (Which launch the flags are handed to, the tiles' or the kept cells': COAL_CELLS_MAX_PERCENT, with its figures, below.)
  static constexpr int COAL_EXIT_PAUSE = 32; static constexpr unsigned long long COAL_EXIT_MIN_PERCENT = 24;
  // The launch that is handed the flags is k_coal_cells where the last polled vote kept at most COAL_CELLS_MAX_PERCENT of the cells that hold a
  // pair, else k_coal_ranked<.., TILES>; the first launch of an object and the first after a restore know no vote and take the tiles.
  // COAL_CELLS_MAX_PERCENT, the break-even of the two launches (EXPERIMENTS.md 7.17; kernel trace, 64^3 x 64, f64, 32 768 tiles, us per launch):
  //   box (steps 2-8)            cells kept   tiles flagged on   k_coal_cells   k_coal_ranked<.., TILES>
  //   stratocumulus              0.1 %        1 %                13             38
  //   sparse (--dt 0.05)         16-19 %      91-95 %            148-168        280-284
  //   mixed (--dt 0.02)          50 %         52 %               412-425        197-202
  //   coal-stress --dt 0.045     100 %        100 %              804-824        348-358
  // The list form costs 10 us + 3.1 ns per kept cell; the tiles cost 1.07 ns per tile (the walk over the flags: 35 us here, 0.22 ms at 128^3) +
  // 9.6 ns per tile flagged on.  How many tiles a kept cell flags depends on how the kept cells lie: scattered (sparse) each flags a tile of its
  // own and the list form wins at 19 % and beyond; side by side (mixed: eight kept cells per kept tile) the lines cross at
  // 10 + 800 x = 38 + 330 x, x = 6 % of the cells.  The threshold is the lower of the two, so that no layout pays.
  static constexpr unsigned long long COAL_CELLS_MAX_PERCENT = 6;

  int skip_pause = 0, exit_pause = 0;                  // steps without a bound, bound launches without the EXIT form, still to go
  bool known = false;                                  // the last polled vote: has one arrived, ...
  unsigned long long kept = 0, with_pair = 0;          // ... the cells it kept, the cells that hold a pair

  // THE two pause rules, fed by whatever counted: a launch's sample or exact counters (pairs skipped of pairs examined, workgroups that left
  // of workgroups launched), or the vote's exact counts.  A zero denominator says nothing (a launch in round 8's form counts no workgroups).
  void feed(unsigned long long skipped, unsigned long long examined, unsigned long long left, unsigned long long launched)
  {
    if (examined && skipped * COAL_SKIP_MIN_SHARE < examined) skip_pause = COAL_SKIP_PAUSE;
    if (launched && left * 100 < launched * COAL_EXIT_MIN_PERCENT) exit_pause = COAL_EXIT_PAUSE;
  }
  void vote(unsigned long long kept_, unsigned long long with_pair_) { known = true; kept = kept_; with_pair = with_pair_; }
  // a step_async begins: is the bound paused in it?  (Counts the pause down; a step without coalescence leaves it alone.)
  bool bound_step(bool opts_coal)
  {
    const bool paused = opts_coal && skip_pause > 0;
    if (paused) --skip_pause;
    return paused;
  }
  // does a bound launch take the EXIT form?  launch_umin() asks ahead of the velocity pass, coal() at the launch: one rule, so the draws
  // made ahead are never wasted
  bool exit_form(const coal_toggles &t) const { return !t.no_rank_exit && (exit_pause == 0 || t.rank_exit_always); }
  // ... and are draws made ahead for it (k_coal_umin)?
  bool prevote_wanted(const coal_toggles &t) const { return exit_form(t) && !t.no_prevote; }
  // a bound launch has taken its form: one not in the EXIT form counts the pause down
  void exit_launch_done(bool exits) { if (!exits && exit_pause > 0) --exit_pause; }
  // the list form where the flags are handed over?
  bool list_wanted(const coal_toggles &t) const { return t.cell_list_always || (known && kept * 100 <= with_pair * COAL_CELLS_MAX_PERCENT); }
  bool operator==(const coal_adapt &b) const
  {
    return skip_pause == b.skip_pause && exit_pause == b.exit_pause && known == b.known && kept == b.kept && with_pair == b.with_pair;
  }
};

// What the draws ahead of the velocity pass (k_coal_umin) were made for; a launch may take them only if it is about to use exactly these.
struct coal_prevote_key {
  uint64_t call = 0, seed = 0, cells = 0, npart = 0;   // the generator's call number and seed, the cells' version, the droplets
  bool operator==(const coal_prevote_key &b) const { return call == b.call && seed == b.seed && cells == b.cells && npart == b.npart; }
};

struct coal_plan_in {
  bool first_substep = false;      // the step's first coalescence substep
  bool order_owed = false;         // its order is still owed and the kernel can rank it (coal_ranks_owed_order())
  bool replayed = false;           // the draws are a replayed stream's (rs.arr): k_coal reads them by id
  bool bound_armed = false;        // step_async's own velocity pass has just left the cells' maxima
  bool n_max_stale = false;        // the largest multiplicity is out of date: no bound without it
  bool exits = false;              // coal_adapt::exit_form
  bool prevote_usable = false;     // draws were made ahead and their key is this launch's
  bool listed = false;             // the vote leaves a list of the kept cells
  bool counted = false;            // coal_toggles::counted
  bool list_wanted = false;        // coal_adapt::list_wanted
};
// the part of it that the toggles and the adaptive state settle; the caller adds what it knows of the step, the order and the draws
inline coal_plan_in coal_plan_in_of(const coal_adapt &a, const coal_toggles &t)
{
  coal_plan_in in;
  in.exits = a.exit_form(t); in.listed = !t.no_cell_list; in.counted = t.counted; in.list_wanted = a.list_wanted(t);
  return in;
}
// the form, with the precedence of the rounds: each later one only where the earlier one's condition holds
inline coal_form coal_form_of(const coal_plan_in &in)
{
  if (!(in.first_substep && in.order_owed && !in.replayed)) return coal_form::PAIRS;
  if (!(in.bound_armed && !in.n_max_stale)) return coal_form::RANKED;
  if (!in.exits) return coal_form::RANKED_SKIP;
  if (!in.prevote_usable) return coal_form::RANKED_EXIT;
  return in.listed && !in.counted && in.list_wanted ? coal_form::CELLS : coal_form::RANKED_TILES;
}

} // namespace lcx
#endif
