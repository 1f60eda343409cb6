// The floor under the cell maxima of the coalescence bound (csrc/lcx_coal_prevote.hpp coal_cmax_floor) in a program of its own
// (tests/test_coal_floor_host.py builds it with -fsanitize=address,undefined and runs it): over a grid of time steps, largest multiplicities,
// cell volumes and scale factors the bound at the floor is <= eps and the bound one grid step above it is > eps, the floor never grows with the
// multiplicity or the time step, and (CMAX_FLOOR, CMAX_FLOOR) comes back where no radius qualifies.  And the vote's sub-lists as
// k_coal_cells reads them (coal_list_place_of, coal_sublist_cap): every global index below the total has one place, below its sub-list's length.
// Prints "ok: ..." and returns 0, or says what differs and returns 1.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <vector>

#include "../libcloudphxx_amd/csrc/lcx_coal_prevote.hpp"

using namespace lcx;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++fails; std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// a running maximum over the nodes of a table that ends at 300 um: 0 .. 100 um by 1, then by 10 (kernel_index)
template <class T> static std::vector<T> table(const double r_max)
{
  std::vector<T> e(size_t(kernel_index(n_t(r_max))) + 1);                       // (a vector so that the sanitizer watches the indices)
  for (size_t i = 0; i < e.size(); ++i) { const double x = double(i) / 40; e[i] = T(x < 1 ? 0.003 + x * x : 1.003); }
  return e;
}

// the grid index of a pair of floor words: the k with coal_floor_at(k) == w, 0 for (CMAX_FLOOR, CMAX_FLOOR)
static int grid_index(const coal_floor_words w, const int k_end)
{
  if (w.r_bits == CMAX_FLOOR && w.v_bits == CMAX_FLOOR) return 0;
  for (int k = 1; k < k_end; ++k) { const coal_floor_words g = coal_floor_at(k); if (g.r_bits == w.r_bits && g.v_bits == w.v_bits) return k; }
  return -1;
}

template <class T> static int check_floor(const char *name)
{
  const double r_max = 300;
  const std::vector<T> emax = table<T>(r_max);
  const int n_emax = int(emax.size()), k_end = int((r_max - 11.) / COAL_FLOOR_STEP_UM);
  const double dts[] = {0.01, 0.045, 0.25, 1, 4, 30}, n_maxs[] = {1, 1e3, 2.4e8, 1e9, 1e11, 1e14, 1e19};
  const double dvs[] = {1, 64000, 1e6}, scls[] = {1, 7, 63, 255};
  const double epss[] = {1. / 65536, 1. / 8192, 1. / 64};
  int n = 0, none = 0, some = 0;
  for (double eps : epss) for (double dv : dvs) for (double scl : scls) {
    for (double dt : dts) {
      int k_prev = 1 << 30;
      for (double n_max : n_maxs) {                      // (growing: the floor may only shrink)
        const coal_floor_words w = coal_cmax_floor<T>(T(dt), T(dv), T(scl), T(n_max), T(r_max), emax.data(), n_emax, T(eps));
        const int k = grid_index(w, k_end);
        CHECK(k >= 0, "%s: the floor (%08x, %08x) is no point of the grid", name, w.r_bits, w.v_bits);
        CHECK(w.r_bits >= CMAX_FLOOR && w.v_bits >= CMAX_FLOOR, "%s: a word below CMAX_FLOOR", name);
        if (k > 0) {
          const T b = coal_bound<T>(w.r_bits, w.v_bits, T(dv), T(scl), T(dt), T(n_max), T(r_max), emax.data(), n_emax);
          CHECK(b <= T(eps), "%s: dt %g n_max %g dv %g scl %g: the bound at the floor is %g above %g", name, dt, n_max, dv, scl, double(b), eps);
          ++some;
        } else ++none;
        if (k >= 0 && k + 1 < k_end) {                   // (one step above: over eps, or past the radii that the table bounds)
          const coal_floor_words up = coal_floor_at(k + 1);
          const T b = coal_bound<T>(up.r_bits, up.v_bits, T(dv), T(scl), T(dt), T(n_max), T(r_max), emax.data(), n_emax);
          const bool past_table = double(std::sqrt(u32_as_float(up.r_bits))) * 1e6 * (1 + 1. / 1024) >= r_max - 11.;   // (only there may the bound be NaN)
          CHECK(b > T(eps) || (past_table && std::isnan(double(b))), "%s: dt %g n_max %g dv %g scl %g: the bound one step above the floor is %g, not above %g", name, dt, n_max, dv, scl, double(b), eps);
          CHECK(up.r_bits > w.r_bits && up.v_bits > w.v_bits, "%s: the grid does not rise at step %d", name, k);
        }
        CHECK(k <= k_prev, "%s: the floor grows with n_max (dt %g dv %g scl %g: step %d after %d)", name, dt, dv, scl, k, k_prev);
        k_prev = k; ++n;
      }
    }
    for (double n_max : n_maxs) {                        // (and with the time step)
      int k_prev = 1 << 30;
      for (double dt : dts) {
        const int k = grid_index(coal_cmax_floor<T>(T(dt), T(dv), T(scl), T(n_max), T(r_max), emax.data(), n_emax, T(eps)), k_end);
        CHECK(k <= k_prev, "%s: the floor grows with dt (n_max %g dv %g scl %g: step %d after %d)", name, n_max, dv, scl, k, k_prev);
        k_prev = k;
      }
    }
  }
  CHECK(none > 0 && some > 0, "%s: %d cases without a floor, %d with one: the grid of cases covers one of them only", name, none, some);
  // no table, no tolerance: no floor
  const coal_floor_words a = coal_cmax_floor<T>(T(1), T(64000), T(63), T(1e6), T(r_max), emax.data(), 0, T(1. / 8192));
  const coal_floor_words b = coal_cmax_floor<T>(T(1), T(64000), T(63), T(1e6), T(r_max), emax.data(), n_emax, T(0));
  CHECK(a.r_bits == CMAX_FLOOR && a.v_bits == CMAX_FLOOR && b.r_bits == CMAX_FLOOR && b.v_bits == CMAX_FLOOR, "%s: a floor without a table or with eps = 0", name);
  // above the floor: either word, strictly; all ones always
  const coal_floor_words f = coal_floor_at(29);
  CHECK(!coal_above_floor(f.r_bits, f.v_bits, f) && coal_above_floor(f.r_bits + 1, CMAX_FLOOR, f) && coal_above_floor(CMAX_FLOOR, f.v_bits + 1, f) &&
        !coal_above_floor(CMAX_FLOOR, CMAX_FLOOR, f) && coal_above_floor(CMAX_POISON, CMAX_POISON, f), "%s: coal_above_floor", name);
  // float_bits_up rounds up and never below CMAX_FLOOR
  const double x = 5.3e-11;
  CHECK(double(u32_as_float(float_bits_up(x))) >= x && double(u32_as_float(float_bits_up(x) - 1)) < x, "%s: float_bits_up(%g)", name, x);
  CHECK(float_bits_up(1e-300) == CMAX_FLOOR, "%s: float_bits_up of a number below FLT_MIN", name);
  return n;
}

// The vote's sub-lists as k_coal_cells reads them: every global index below the total maps to exactly one (sub-list, offset), the offset below
// that sub-list's length; and over the waves of every grid of coal_cells_grid every index is taken exactly once.
static int check_sublists()
{
  std::vector<std::vector<uint32_t>> cases;
  uint64_t x = 88172645463325252ull;
  auto rnd = [&x] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  for (int t = 0; t < 24; ++t) {                         // random lengths, every third one zero, small and large
    std::vector<uint32_t> len(COAL_SUBLISTS);
    for (auto &l : len) l = rnd() % 3 == 0 ? 0u : uint32_t(rnd() % (t < 12 ? 5 : 700));
    cases.push_back(len);
  }
  for (uint32_t total : {0u, 1u, 2u, 65536u})            // one sub-list holds everything: the first, a middle one, the last
    for (int at : {0, 31, COAL_SUBLISTS - 1}) { std::vector<uint32_t> len(COAL_SUBLISTS, 0u); len[at] = total; cases.push_back(len); }
  { std::vector<uint32_t> len(COAL_SUBLISTS, 1024u); cases.push_back(len); }                             // 2^16 spread evenly
  { std::vector<uint32_t> len(COAL_SUBLISTS, 0u); len[0] = 1; len[COAL_SUBLISTS - 1] = 1; cases.push_back(len); }      // a total of 2 at the two ends
  int n = 0;
  for (const auto &len : cases) {
    std::vector<uint32_t> prefix(COAL_SUBLISTS + 1, 0u);
    for (int s = 0; s < COAL_SUBLISTS; ++s) prefix[s + 1] = prefix[s] + len[s];
    const uint32_t total = prefix[COAL_SUBLISTS];
    std::vector<std::vector<int>> seen(COAL_SUBLISTS);
    for (int s = 0; s < COAL_SUBLISTS; ++s) seen[s].assign(len[s], 0);      // (vectors so that the sanitizer watches the indices)
    for (uint32_t li = 0; li < total; ++li) {
      const coal_list_place p = coal_list_place_of(prefix.data(), li);
      CHECK(p.sub < uint32_t(COAL_SUBLISTS) && p.off < len[p.sub], "index %u of %u maps to (%u, %u), length %u", li, total, p.sub, p.off, p.sub < uint32_t(COAL_SUBLISTS) ? len[p.sub] : 0u);
      if (p.sub < uint32_t(COAL_SUBLISTS) && p.off < len[p.sub]) ++seen[p.sub][p.off];
      CHECK(prefix[p.sub] + p.off == li, "index %u maps to (%u, %u), which is index %u", li, p.sub, p.off, prefix[p.sub] + p.off);
    }
    uint64_t once = 0;
    for (const auto &sv : seen) for (int v : sv) once += v == 1;
    CHECK(once == total, "%" PRIu64 " of %u places taken exactly once", once, total);
    // the waves of a grid share the indices out; through the mapping every place is visited once
    for (uint64_t n_cell : {uint64_t(1), uint64_t(4096), uint64_t(1) << 21}) {
      const uint64_t n_wg = coal_cells_grid(n_cell, 4, 2048);
      std::vector<int> taken(total, 0);
      for (uint64_t wg = 0; wg < n_wg; ++wg) for (uint64_t w = 0; w < 4; ++w) {
        const coal_list_share sh = coal_list_share_of(wg, n_wg, w, 4);
        for (uint64_t li = sh.first; li < total; li += sh.step) { const coal_list_place p = coal_list_place_of(prefix.data(), uint32_t(li)); ++taken[prefix[p.sub] + p.off]; }
      }
      uint64_t t1 = 0;
      for (int v : taken) t1 += v == 1;
      CHECK(t1 == total, "grid of %" PRIu64 " workgroups: %" PRIu64 " of %u entries taken by exactly one wave", n_wg, t1, total);
    }
    ++n;
  }
  // a sub-list has room for every cell that its waves can keep
  for (uint64_t n_cell : {uint64_t(1), uint64_t(27), uint64_t(64), uint64_t(65), uint64_t(4096), uint64_t(4097), uint64_t(13824), uint64_t(1) << 21}) {
    const uint64_t cap = coal_sublist_cap(n_cell, 64), waves = (n_cell + 63) / 64;
    for (uint64_t s = 0; s < uint64_t(COAL_SUBLISTS); ++s) {
      uint64_t mine = 0;
      for (uint64_t w = s; w < waves; w += COAL_SUBLISTS) ++mine;
      CHECK(mine * 64 <= cap, "n_cell %" PRIu64 ": sub-list %" PRIu64 " can receive %" PRIu64 " cells, room for %" PRIu64, n_cell, s, mine * 64, cap);
    }
  }
  return n;
}

int main()
{
  const int n = check_floor<float>("float") + check_floor<double>("double"), s = check_sublists();
  if (fails) { std::printf("%d checks failed\n", fails); return 1; }
  std::printf("ok: %d floors, %d vectors of sub-list lengths\n", n, s);
  return 0;
}
