// track_plan_check.cpp -- csrc/lcx_track_plan.hpp alone, for the host, under the sanitizers (tests/test_track_plan_host.py):
// the stride rule against a brute-force walk of the ranks, the sample buffer's offsets against a plain 3-D array, the validation's texts.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o track_plan_check tools/track_plan_check.cpp
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../libcloudphxx_amd/csrc/lcx_track_plan.hpp"

using namespace lcx::track;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static void rule(uint64_t Q, uint64_t room_, bool walk)
{
  const uint64_t st = stride(Q, room_), n = count(Q, st);
  if (Q == 0 || room_ == 0) { CHECK(st == 0 && n == 0); CHECK(!taken(0, st)); return; }
  CHECK(st >= 1 && n >= 1 && n <= room_);
  CHECK(st == 1 || (st - 1) * room_ < Q);                   // the smallest stride that fits: one less would take more than room
  CHECK((unsigned __int128)st * room_ >= Q);
  CHECK(n == (Q - 1) / st + 1);
  CHECK(taken(0, st) && index_of(0, st, 7) == 7);
  const uint64_t last = ((Q - 1) / st) * st;                // the last rank taken
  CHECK(taken(last, st) && index_of(last, st, 7) == 7 + n - 1);
  if (!walk) return;
  uint64_t k = 0;
  for (uint64_t q = 0; q < Q; ++q) if (taken(q, st)) { CHECK(index_of(q, st, 3) == 3 + k); ++k; }
  CHECK(k == n);
}

int main()
{
  // stride and count for Q in {0, 1, room - 1, room, room + 1, 2 room + 1, 2^32 - 1}
  for (uint64_t room_ : {uint64_t(1), uint64_t(2), uint64_t(5), uint64_t(64), uint64_t(1000), uint64_t(LCX_TRK_MAX)}) {
    for (uint64_t Q : {uint64_t(0), uint64_t(1), room_ - 1, room_, room_ + 1, 2 * room_ + 1}) rule(Q, room_, true);
    rule(0xFFFFFFFFull, room_, false);
  }
  rule(5, 0, true); rule(0, 0, true);
  rule(std::numeric_limits<uint64_t>::max(), 3, false);     // (no sum that wraps)
  CHECK(stride(10, 4) == 3 && count(10, 3) == 4);           // ranks 0, 3, 6, 9
  CHECK(stride(9, 4) == 3 && count(9, 3) == 3);             // ranks 0, 3, 6: fewer than room, never more
  CHECK(stride(4, 4) == 1 && count(4, 1) == 4 && stride(3, 4) == 1 && count(3, 1) == 3 && stride(5, 4) == 2 && count(5, 2) == 3);
  // room
  CHECK(room(10, 8, 3) == 5 && room(2, 8, 3) == 2 && room(2, 8, 8) == 0 && room(2, 8, 9) == 0 && room(0, 8, 0) == 0);
  CHECK(room(std::numeric_limits<uint64_t>::max(), LCX_TRK_MAX, 0) == uint64_t(LCX_TRK_MAX));
  // the buffer: [capacity][12][max_tracked], every element once, the last one the last
  {
    const size_t cap = 3, mx = 5;
    std::vector<int> hit(buf_elems(cap, mx), 0);
    CHECK(hit.size() == cap * 12 * mx);
    for (size_t s = 0; s < cap; ++s) for (int f = 0; f < LCX_TRK_FIELDS; ++f) for (size_t k = 0; k < mx; ++k) {
      const size_t off = buf_offset(s, f, k, mx);
      CHECK(off < hit.size());
      if (off < hit.size()) ++hit[off];
      CHECK(off == (s * 12 + size_t(f)) * mx + k);
    }
    for (int h : hit) CHECK(h == 1);
    CHECK(buf_offset(0, 0, 1, mx) - buf_offset(0, 0, 0, mx) == 1);          // field-major: neighbours in k are neighbours in memory
    CHECK(buf_offset(cap - 1, LCX_TRK_FIELDS - 1, mx - 1, mx) + 1 == buf_elems(cap, mx));
    CHECK(buf_elems(64, LCX_TRK_MAX) == size_t(64) * 12 * (size_t(1) << 20));
  }
  CHECK(LCX_TRK_FIELDS == 12 && LCX_TRK_N == 0 && LCX_TRK_CELL == 8 && LCX_TRK_RV == 11 && LCX_TRK_MAX == 1048576 && NONE == 0xFFFFFFFFu);
  // the validation
  {
    std::string err;
    lcx_diag_clause_t c[LCX_DIAG_MAX_CLAUSES + 1] = {};
    c[0].sel = LCX_DIAG_SEL_WET; c[0].lo = 1e-6; c[0].hi = 2e-6;
    const double box[6] = {0, 1, 0, 1, 0, 1};
    CHECK(validate(c, 1, nullptr, 1, err) && validate(c, 1, box, 7, err) && validate(c, LCX_DIAG_MAX_CLAUSES, box, 7, err));
    CHECK(!validate(c, 0, nullptr, 1, err) && err.find("n_clauses = 0 is outside 1 .. 4") != std::string::npos);
    CHECK(!validate(c, LCX_DIAG_MAX_CLAUSES + 1, nullptr, 1, err) && err.find("n_clauses = 5") != std::string::npos);
    CHECK(!validate(nullptr, 1, nullptr, 1, err) && err.find("clause == NULL") != std::string::npos);
    c[1].sel = 9;
    CHECK(!validate(c, 2, nullptr, 1, err) && err.find("clause 1: unknown sel 9") != std::string::npos);
    c[1].sel = -1;
    CHECK(!validate(c, 2, nullptr, 1, err) && err.find("unknown sel -1") != std::string::npos);
    CHECK(!validate(c, 1, nullptr, 0, err) && err.find("max_count == 0") != std::string::npos);
    double b2[6] = {0, 1, 2, 1, 0, 1};
    CHECK(!validate(c, 1, b2, 1, err) && err.find("lo > hi in pair 1") != std::string::npos);
    const bool no_y[3] = {true, false, true};
    CHECK(validate(c, 1, b2, 1, err, no_y));                 // (the pair of a dimension the object lacks is not read)
    b2[2] = 0; b2[5] = std::numeric_limits<double>::infinity();
    CHECK(!validate(c, 1, b2, 1, err) && err.find("bound 5 is not finite") != std::string::npos);
    b2[5] = 1; b2[0] = std::numeric_limits<double>::quiet_NaN();
    CHECK(!validate(c, 1, b2, 1, err) && err.find("bound 0 is not finite") != std::string::npos);
    b2[0] = 1;                                               // lo == hi: an empty box, allowed
    CHECK(validate(c, 1, b2, 1, err));
    CHECK(err.rfind("libcloudph++: track: ", 0) == 0);
  }
  if (fails) { std::printf("%d checks failed\n", fails); return 1; }
  std::printf("ok: stride rule, buffer offsets, validation\n");
  return 0;
}
