// The host side of csrc/lcx_coal_prevote.hpp in a program of its own (tests/test_coal_prevote_host.py builds it with
// -fsanitize=address,undefined and runs it): a cell's smallest draw against a brute-force minimum, the tile range of a cell's stretch, and the
// bound's NaN cases.  Prints "ok: ..." and returns 0, or says what differs and returns 1.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../libcloudphxx_amd/csrc/lcx_coal_prevote.hpp"

using namespace lcx;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++fails; std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

template <class T> static int check_umin(const char *name)
{
  const uint64_t call = 7, seed = 44;
  const uint32_t counts[] = {0, 1, 2, 3, 63, 64, 65, 255, 256};
  const uint64_t offs[] = {0, 1, 1000, 1001, (uint64_t(1) << 32) - 600, (uint64_t(1) << 32) - 599, (uint64_t(1) << 32) + 10};
  int n = 0;
  for (uint64_t off : offs)
    for (uint32_t cnt : counts) {
      const uint64_t end = off + cnt;
      // brute force: every pair position of the cell, as a vector so that the sanitizer watches the indices
      std::vector<T> u;
      for (uint64_t p = off; p + 1 < end; p += 2) u.push_back(philox::u01<T>(p, call, seed));
      T want = std::numeric_limits<T>::infinity();
      for (size_t i = 0; i < u.size(); ++i) if (u[i] < want) want = u[i];
      const T got = coal_cell_umin<T>(off, end, call, seed);
      CHECK(got == want, "%s off %" PRIu64 " cnt %u: %.17g against %.17g", name, off, cnt, double(got), double(want));
      CHECK(u.size() == cnt / 2, "%s pairs of %u", name, cnt);
      if (cnt < 2) CHECK(std::isinf(double(got)) && got > 0, "%s: a cell without a pair gives +inf", name);
      else CHECK(got >= T(0) && got < T(1), "%s: a draw lies in [0, 1)", name);
      // eight lanes that split the cell between them find the same minimum
      T split = std::numeric_limits<T>::infinity();
      for (uint64_t l = 0; l < 8; ++l) { const T s = coal_cell_umin<T>(off, end, call, seed, l, 8); if (s < split) split = s; }
      CHECK(split == want, "%s off %" PRIu64 " cnt %u: eight lanes give %.17g against %.17g", name, off, cnt, double(split), double(want));
      ++n;
    }
  // the position travels whole: above 2^32 the draw is not the one of the position's low word, and another call number is another draw
  const uint64_t hi = (uint64_t(1) << 32) + 10;
  CHECK(coal_cell_umin<T>(hi, hi + 2, call, seed) == philox::u01<T>(hi, call, seed), "%s: one pair at 2^32 + 10", name);
  CHECK(coal_cell_umin<T>(hi, hi + 2, call, seed) != coal_cell_umin<T>(10, 12, call, seed), "%s: the high word of the position is dropped", name);
  CHECK(coal_cell_umin<T>(0, 64, call, seed) != coal_cell_umin<T>(0, 64, call + 1, seed), "%s: the call number is ignored", name);
  // bounds that do not belong together end the loop at once
  CHECK(std::isinf(double(coal_cell_umin<T>(100, 36, call, seed))), "%s: end < off counts as an empty cell", name);
  // a cell that straddles 2^32: the pair at 2^32 - 2 and the one at 2^32
  const uint64_t lo = (uint64_t(1) << 32) - 2;
  const T a = philox::u01<T>(lo, call, seed), b = philox::u01<T>(lo + 2, call, seed);
  CHECK(coal_cell_umin<T>(lo, lo + 4, call, seed) == (a < b ? a : b), "%s: a cell across 2^32", name);
  return n;
}

static int check_tiles()
{
  const uint64_t TILE = 512;
  struct { uint64_t off, end, first, last; bool empty; const char *what; } cases[] = {
    {10, 74, 0, 0, false, "inside one tile"},
    {448, 512, 0, 0, false, "ending on a tile boundary"},
    {512, 576, 1, 1, false, "beginning on a tile boundary"},
    {480, 544, 0, 1, false, "straddling a boundary"},
    {3 * 512 - 1, 3 * 512 + 1, 2, 3, false, "its only pair starts at the odd position 512 k - 1"},
    {500, 500 + 1100, 0, 3, false, "longer than two tiles"},
    {700, 700, 1, 0, true, "empty"},
    {(uint64_t(1) << 32) - 20, (uint64_t(1) << 32) + 44, ((uint64_t(1) << 32) - 20) / 512, (uint64_t(1) << 32) / 512, false, "across 2^32"},
  };
  int n = 0;
  for (auto &c : cases) {
    const coal_tile_range r = coal_cell_tiles(c.off, c.end, TILE);
    if (c.empty) CHECK(r.first > r.last, "%s: [%" PRIu64 ", %" PRIu64 "]", c.what, r.first, r.last);
    else CHECK(r.first == c.first && r.last == c.last, "%s: [%" PRIu64 ", %" PRIu64 "]", c.what, r.first, r.last);
    // every pair of the cell is examined by a lane inside the range: the lane at p for an even position p, at p - 1 for an odd one
    for (uint64_t p = c.off; p + 1 < c.end; p += 2) {
      const uint64_t lane_pos = p & ~uint64_t(1);
      CHECK(lane_pos / TILE >= r.first && lane_pos / TILE <= r.last, "%s: the pair at %" PRIu64 " is examined outside the range", c.what, p);
    }
    ++n;
  }
  return n;
}

template <class T> static int check_bound(const char *name)
{
  const T emax[4] = {T(0.1), T(0.2), T(0.3), T(0.4)};
  const T r_max = T(300), dv = T(64000), dt = T(1), n_max = T(1e6);
  auto bits = [](float f) { return __builtin_bit_cast(uint32_t, f); };
  const T scl = coal_scale_of<T>(64);
  CHECK(scl == T(63), "%s: the scale factor of 64 droplets is %g", name, double(scl));
  CHECK(coal_scale_of<T>(1) == T(0) && coal_scale_of<T>(0) == T(0), "%s: no pair, no scale", name);
  CHECK(coal_scale_of<T>(3) == T(3), "%s: the scale factor of 3 droplets", name);
  const T b = coal_bound<T>(bits(1e-10f), bits(0.01f), dv, scl, dt, n_max, r_max, emax, 4);           // 10 um, 1 cm/s: the last node (index 10 capped to 3)
  const double want = 1. / 64000 * 63 * 1e6 * 3.141592653589793 * 4 * double(1e-10f) * double(0.01f) * 0.4 * (1 + 1. / 1024);
  CHECK(std::fabs(double(b) / want - 1) < 1e-5, "%s: the bound is %g against %g", name, double(b), want);
  CHECK(std::isnan(double(coal_bound<T>(0xFFFFFFFFu, bits(0.01f), dv, scl, dt, n_max, r_max, emax, 4))), "%s: a poisoned radius", name);
  CHECK(std::isnan(double(coal_bound<T>(bits(1e-10f), 0xFFFFFFFFu, dv, scl, dt, n_max, r_max, emax, 4))), "%s: a poisoned velocity", name);
  CHECK(std::isnan(double(coal_bound<T>(bits(1e-10f), bits(std::numeric_limits<float>::infinity()), dv, scl, dt, n_max, r_max, emax, 4))), "%s: an infinite velocity", name);
  CHECK(std::isnan(double(coal_bound<T>(bits(8.5e-8f), bits(0.01f), dv, scl, dt, n_max, r_max, emax, 4))), "%s: 291 um, within 11 um of the table's end", name);
  CHECK(coal_bound<T>(bits(1e-10f), bits(0.01f), dv, T(0), dt, n_max, r_max, emax, 4) == T(1e-30), "%s: a bound of zero is raised", name);
  return 9;
}

int main()
{
  const int n = check_umin<float>("float") + check_umin<double>("double"), t = check_tiles(), b = check_bound<float>("float") + check_bound<double>("double");
  if (fails) { std::printf("%d checks failed\n", fails); return 1; }
  std::printf("ok: %d cells' smallest draws, %d tile ranges, %d bound cases\n", n, t, b);
  return 0;
}
