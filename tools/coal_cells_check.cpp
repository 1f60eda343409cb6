// What k_coal_cells shares with the host (csrc/lcx_coal_prevote.hpp) in a program of its own (tests/test_coal_cells_host.py builds it with
// -fsanitize=address,undefined and runs it): how the vote's list is shared out among the waves of a grid that does not grow with it, the
// grid's size, and a cell's pairs -- their number, their positions, and that the smallest of their draws is the one the vote compared.
// Prints "ok: ..." and returns 0, or says what differs and returns 1.
#include <cinttypes>
#include <cstdio>
#include <limits>
#include <vector>

#include "../libcloudphxx_amd/csrc/lcx_coal_prevote.hpp"

using namespace lcx;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++fails; std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// every entry below the count is taken by exactly one wave, none at or above it, whatever the grid
static int check_shares()
{
  const uint64_t counts[] = {0, 1, 3, 4, 5, 63, 64, 255, 256, 257, 8191, 8192, 8193, 36000};
  const uint64_t grids[] = {1, 2, 3, 7, 512, 2048}, waves[] = {1, 4};
  int n = 0;
  for (uint64_t count : counts)
    for (uint64_t n_wg : grids)
      for (uint64_t per : waves) {
        std::vector<int> seen(count, 0);                // (a vector so that the sanitizer watches the indices)
        for (uint64_t wg = 0; wg < n_wg; ++wg)
          for (uint64_t w = 0; w < per; ++w) {
            const coal_list_share s = coal_list_share_of(wg, n_wg, w, per);
            CHECK(s.step == n_wg * per && s.step > 0, "the step of %" PRIu64 " x %" PRIu64, n_wg, per);
            for (uint64_t li = s.first; li < count; li += s.step) ++seen[li];
          }
        uint64_t once = 0;
        for (int v : seen) once += v == 1;
        CHECK(once == count, "count %" PRIu64 ", %" PRIu64 " workgroups of %" PRIu64 ": %" PRIu64 " entries taken exactly once", count, n_wg, per, once);
        ++n;
      }
  return n;
}

static int check_grid()
{
  CHECK(coal_cells_grid(0, 4, 2048) == 1, "no cell: one workgroup");
  CHECK(coal_cells_grid(1, 4, 2048) == 1 && coal_cells_grid(4, 4, 2048) == 1 && coal_cells_grid(5, 4, 2048) == 2, "a wave per cell, rounded up");
  CHECK(coal_cells_grid(4096, 4, 2048) == 1024 && coal_cells_grid(8192, 4, 2048) == 2048 && coal_cells_grid(8193, 4, 2048) == 2048, "the cap");
  CHECK(coal_cells_grid(uint64_t(1) << 40, 4, 2048) == 2048 && coal_cells_grid(2097152, 4, 1) == 1, "the grid does not grow with the box");
  return 4;
}

template <class T> static int check_pairs(const char *name)
{
  const uint64_t call = 7, seed = 44;
  const uint32_t counts[] = {0, 1, 2, 3, 63, 64, 65, 129, 255, 256, 257, 600};
  const uint64_t offs[] = {0, 1, 1000, 1001, (uint64_t(1) << 32) - 130, (uint64_t(1) << 32) - 129, (uint64_t(1) << 32) + 10};
  int n = 0;
  for (uint64_t off : offs)
    for (uint32_t cnt : counts) {
      const uint64_t end = off + cnt, np = coal_cell_pairs(off, end);
      CHECK(np == cnt / 2, "%s: %u droplets hold %" PRIu64 " pairs", name, cnt, np);
      // the positions: even in-cell offsets, both members inside the cell, consecutive pairs disjoint; the kernel's windows of 256 ranks with two
      // pairs per lane visit every pair once
      std::vector<int> seen(np, 0);
      T smallest = std::numeric_limits<T>::infinity();
      for (uint64_t base = 0; base < 2 * np; base += 256)
        for (uint64_t lane = 0; lane < 64; ++lane)
          for (uint64_t k = 0; k < 2; ++k) {
            const uint64_t j = base / 2 + lane + k * 64;
            if (!(j < np)) continue;
            ++seen[j];
            const uint64_t p = coal_pair_pos(off, j);
            CHECK(((p - off) & 1) == 0 && p >= off && p + 1 < end, "%s: pair %" PRIu64 " of [%" PRIu64 ", %" PRIu64 ") at %" PRIu64, name, j, off, end, p);
            CHECK(2 * (j - base / 2) + 1 < 256, "%s: rank %" PRIu64 " outside its window", name, 2 * j + 1);
            const T u = philox::u01<T>(p, call, seed);
            if (u < smallest) smallest = u;
          }
      for (uint64_t j = 0; j < np; ++j) CHECK(seen[j] == 1, "%s: pair %" PRIu64 " of %u droplets visited %d times", name, j, cnt, seen[j]);
      CHECK(smallest == coal_cell_umin<T>(off, end, call, seed), "%s off %" PRIu64 " cnt %u: the kernel's draws and the vote's differ", name, off, cnt);
      ++n;
    }
  CHECK(coal_cell_pairs(100, 36) == 0, "%s: end < off counts as an empty cell", name);
  return n;
}

int main()
{
  const int s = check_shares(), g = check_grid(), p = check_pairs<float>("float") + check_pairs<double>("double");
  if (fails) { std::printf("%d checks failed\n", fails); return 1; }
  std::printf("ok: %d shares of a list, %d grids, %d cells' pairs\n", s, g, p);
  return 0;
}
