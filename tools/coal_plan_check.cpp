// The host side of the coalescence's launch (csrc/lcx_coal_plan.hpp) in a program of its own: the form over every combination of the plan's
// inputs against the rules of DESIGN.md 4.2, each stated on its own; what each debug toggle forces; the two pause sequences step by step
// and launch by launch, their thresholds on both sides; the list's threshold; the key of the draws made ahead.  No HIP include: the host
// compiler alone (tests/test_coal_plan_host.py builds it with -fsanitize=address,undefined).
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../libcloudphxx_amd/csrc/lcx_coal_plan.hpp"

using namespace lcx;

static int checks = 0;
static void need(bool ok, const std::string &what)
{
  ++checks;
  if (!ok) { std::fprintf(stderr, "FAILED: %s\n", what.c_str()); std::exit(1); }
}
static bool bit(unsigned m, int i) { return (m >> i) & 1u; }

int main()
{
  using F = coal_form;
  // ---- the form over every combination of its ten inputs ----
  for (unsigned m = 0; m < (1u << 10); ++m) {
    coal_plan_in in;
    in.first_substep = bit(m, 0); in.order_owed = bit(m, 1); in.replayed = bit(m, 2); in.bound_armed = bit(m, 3); in.n_max_stale = bit(m, 4);
    in.exits = bit(m, 5); in.prevote_usable = bit(m, 6); in.listed = bit(m, 7); in.counted = bit(m, 8); in.list_wanted = bit(m, 9);
    const F f = coal_form_of(in);
    const std::string at = " (inputs " + std::to_string(m) + ")";
    need((f == F::PAIRS) == !(in.first_substep && in.order_owed && !in.replayed), "PAIRS iff not (first substep, order owed, own draws)" + at);
    const bool bound = f != F::PAIRS && f != F::RANKED;
    if (!(in.bound_armed && !in.n_max_stale)) need(!bound, "no bound without armed maxima and a current n_max" + at);
    if (f == F::PAIRS) continue;
    need(bound == (in.bound_armed && !in.n_max_stale), "a launch that ranks takes the bound wherever it is there" + at);
    if (f == F::CELLS) need(in.prevote_usable && in.listed && !in.counted && in.list_wanted, "CELLS only with the draws, a list, uncounted, wanted" + at);
    if (!bound) continue;
    need((f == F::RANKED_TILES) == (in.prevote_usable && in.exits && f != F::CELLS), "TILES iff the draws, the exit, not CELLS" + at);
    need((f == F::RANKED_EXIT) == (in.exits && !in.prevote_usable), "EXIT iff the exit without the draws" + at);
    need((f == F::RANKED_SKIP) == !in.exits, "SKIP iff no exit" + at);
    need((f == F::CELLS) == (in.exits && in.prevote_usable && in.listed && !in.counted && in.list_wanted), "CELLS wherever all of it holds" + at);
  }
  // ---- what each toggle forces, over every combination of the six, four adaptive states and draws made or not ----
  for (unsigned m = 0; m < (1u << 6); ++m)
    for (int state = 0; state < 4; ++state)
      for (int want_bound = 0; want_bound < 2; ++want_bound) {
        coal_toggles t;
        t.counted = bit(m, 0); t.no_rank_exit = bit(m, 1); t.rank_exit_always = bit(m, 2); t.no_prevote = bit(m, 3); t.no_cell_list = bit(m, 4); t.cell_list_always = bit(m, 5);
        coal_adapt a;
        if (state == 1) a.exit_pause = 7;
        if (state == 2) a.vote(1, 100);                      // (a sparse vote: the list is wanted)
        if (state == 3) a.vote(50, 100);                     // (a crowded one)
        coal_plan_in in = coal_plan_in_of(a, t);
        in.first_substep = in.order_owed = true; in.bound_armed = want_bound;
        in.prevote_usable = want_bound && a.prevote_wanted(t);          // (launch_umin, and the key matches)
        const F f = coal_form_of(in);
        const std::string at = " (toggles " + std::to_string(m) + ", state " + std::to_string(state) + ")";
        const bool exit_forms = f == F::RANKED_EXIT || f == F::RANKED_TILES || f == F::CELLS, flag_forms = f == F::RANKED_TILES || f == F::CELLS;
        if (!want_bound) { need(f == F::RANKED, "no bound asked for: the plain form" + at); continue; }
        if (t.no_rank_exit) need(f == F::RANKED_SKIP, "NO_COAL_RANK_EXIT: round 8's form" + at);
        if (t.rank_exit_always && !t.no_rank_exit) need(exit_forms, "COAL_RANK_EXIT_ALWAYS: an EXIT form, paused or not" + at);
        if (!t.no_rank_exit && !t.rank_exit_always) need(exit_forms == (state != 1), "the EXIT forms unless paused" + at);
        if (t.no_prevote) need(!flag_forms, "NO_COAL_PREVOTE: no flags" + at);
        if (!t.no_prevote && exit_forms) need(flag_forms, "the draws are made wherever the exit is taken" + at);
        if (t.no_cell_list || t.counted) need(f != F::CELLS, "NO_COAL_CELL_LIST, COAL_SKIP_COUNT: never the list form" + at);
        if (flag_forms && !t.no_cell_list && !t.counted) need((f == F::CELLS) == (t.cell_list_always || state == 2), "the list form: forced, or a sparse vote" + at);
      }
  const coal_toggles none;
  // ---- the bound's pause: just under the threshold, COAL_SKIP_PAUSE steps paused, the next one probes ----
  {
    const unsigned long long S = coal_adapt::COAL_SKIP_MIN_SHARE;
    coal_adapt a;
    a.feed(5, 5 * S, 0, 0);                                  // exactly ON the threshold: 5 * S < 5 * S is false
    need(a.skip_pause == 0 && a.exit_pause == 0, "skipped * SHARE == examined does not pause");
    a.feed(0, 0, 0, 0);
    need(a == coal_adapt{}, "examined == 0 and launched == 0 change nothing");
    a.feed(5, 5 * S + 1, 0, 0);                              // just under
    need(a.skip_pause == coal_adapt::COAL_SKIP_PAUSE && a.exit_pause == 0, "just under the share: the bound pauses, the exit does not");
    need(!a.bound_step(false) && a.skip_pause == coal_adapt::COAL_SKIP_PAUSE, "a step without coalescence is not paused and counts nothing down");
    for (int i = 0; i < coal_adapt::COAL_SKIP_PAUSE; ++i) need(a.bound_step(true), "paused step " + std::to_string(i));
    need(!a.bound_step(true) && a.skip_pause == 0, "the step behind the pause probes");
    a.feed(0, 7, 0, 0);                                      // none skipped at all
    need(a.skip_pause == coal_adapt::COAL_SKIP_PAUSE, "nothing skipped pauses");
    a.feed(0, 0, 0, 0);
    need(a.skip_pause == coal_adapt::COAL_SKIP_PAUSE, "examined == 0 leaves a running pause alone");
  }
  // ---- the exit's pause: just under the threshold, COAL_EXIT_PAUSE bound launches not in the EXIT form, the next one is ----
  {
    const unsigned long long P = coal_adapt::COAL_EXIT_MIN_PERCENT;
    coal_toggles always; always.rank_exit_always = true;
    coal_toggles never; never.no_rank_exit = true;
    coal_adapt a;
    need(a.exit_form(none) && a.prevote_wanted(none), "a fresh object takes the EXIT form and draws ahead");
    a.feed(0, 0, P, 100);                                    // exactly ON: P * 100 < 100 * P is false
    need(a.exit_pause == 0 && a.skip_pause == 0, "left * 100 == launched * PERCENT does not pause");
    a.feed(0, 0, 2 * P - 1, 200);                            // just under ((2 P - 1) * 100 < 200 P)
    need(a.exit_pause == coal_adapt::COAL_EXIT_PAUSE && a.skip_pause == 0, "just under the percentage: the exit pauses, the bound does not");
    for (int i = 0; i < coal_adapt::COAL_EXIT_PAUSE; ++i) {
      need(a.exit_form(always) && a.exit_pause == coal_adapt::COAL_EXIT_PAUSE - i, "COAL_RANK_EXIT_ALWAYS overrides a running pause without clearing it");
      need(!a.exit_form(never), "NO_COAL_RANK_EXIT: never");
      const bool exits = a.exit_form(none);
      need(!exits && !a.prevote_wanted(none), "paused launch " + std::to_string(i) + ": round 8's form, no draws ahead");
      a.exit_launch_done(exits);
    }
    need(a.exit_form(none) && a.exit_pause == 0, "the launch behind the pause probes");
    a.exit_launch_done(true);
    need(a.exit_pause == 0, "a launch in the EXIT form counts nothing down");
    a.feed(0, 0, 0, 9);
    const int before = a.exit_pause;
    a.exit_launch_done(true);                                // (COAL_RANK_EXIT_ALWAYS: launches in the EXIT form leave the pause as it is)
    need(before == coal_adapt::COAL_EXIT_PAUSE && a.exit_pause == before, "none left pauses; an EXIT launch under the pause does not count it down");
    a.feed(0, 0, 0, 0);
    need(a.exit_pause == before, "launched == 0 leaves a running pause alone");
    a.feed(1, 1, 1, 1);
    need(a.exit_pause == before && a.skip_pause == 0, "good counters do not end a pause early");
  }
  // ---- the list's threshold ----
  {
    const unsigned long long C = coal_adapt::COAL_CELLS_MAX_PERCENT;
    coal_toggles forced; forced.cell_list_always = true;
    coal_adapt a;
    need(!a.list_wanted(none), "no vote known: the tiles");
    need(a.list_wanted(forced), "COAL_CELL_LIST_ALWAYS: wanted with no vote known");
    a.vote(C, 100);
    need(a.known && a.list_wanted(none), "exactly COAL_CELLS_MAX_PERCENT of the cells with a pair: the list");
    a.vote(C + 1, 100);
    need(!a.list_wanted(none) && a.list_wanted(forced), "one cell above: the tiles, unless forced");
    a.vote(0, 0);
    need(a.list_wanted(none), "a vote of no cell at all: the list (nothing to launch over)");
  }
  // ---- the reset of a restore ----
  {
    coal_adapt a;
    a.feed(0, 1, 0, 1); a.vote(3, 4);
    need(!(a == coal_adapt{}) && a.skip_pause > 0 && a.exit_pause > 0 && a.known, "a state that differs from a fresh one in every member");
    a = coal_adapt{};
    coal_adapt fresh;
    need(a == fresh && a.skip_pause == 0 && a.exit_pause == 0 && !a.known && a.kept == 0 && a.with_pair == 0, "value-initialised: a fresh object's");
  }
  // ---- the key of the draws made ahead ----
  {
    const coal_prevote_key k{11, 22, 33, 44};
    need(k == coal_prevote_key{11, 22, 33, 44}, "the same call, seed, cells and droplets: usable");
    need(!(k == coal_prevote_key{12, 22, 33, 44}), "another call");
    need(!(k == coal_prevote_key{11, 23, 33, 44}), "another seed");
    need(!(k == coal_prevote_key{11, 22, 34, 44}), "another version of the cells");
    need(!(k == coal_prevote_key{11, 22, 33, 45}), "another number of droplets");
    need(!(k == coal_prevote_key{}), "a key never made");
  }
  std::printf("ok: %d checks\n", checks);
  return 0;
}
