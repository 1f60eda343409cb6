// diag_batch_plan_check.cpp -- what lcx_diag_batch decides before a device is touched (libcloudphxx_amd/csrc/lcx_diag_plan.hpp) on
// its own, for a build under the host sanitizers (tests/test_diag_batch_api.py: g++ -fsanitize=address,undefined).  Drives the
// validation over malformed lists and the planner over large and random ones, float and double; every list lives in a heap block of
// exactly its size.  Every outcome must be the expected one; the sanitizers must have nothing to say.  Needs no GPU.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../libcloudphxx_amd/csrc/lcx_diag_plan.hpp"

using namespace lcx::diag;

static unsigned long long rng_state = 88172645463325252ull;
static unsigned rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return unsigned(rng_state >> 32); }

static lcx_diag_req_t good(int i)
{
  lcx_diag_req_t q;
  std::memset(&q, 0, sizeof q);
  q.n_clauses = 1 + int(rnd() % LCX_DIAG_MAX_CLAUSES);
  for (int c = 0; c < q.n_clauses; ++c) { q.clause[c].sel = int(rnd() % 5); q.clause[c].lo = 1e-9 * (1 + rnd() % 100); q.clause[c].hi = q.clause[c].lo * (1 + rnd() % 50); }
  q.count = int(rnd() % 4); q.k = int(rnd() % 5) - 1 + i % 2;
  return q;
}

#define FAIL(...) do { std::printf(__VA_ARGS__); std::printf("\n"); return 1; } while (0)

template <class T> static int check_plan(const std::vector<lcx_diag_req_t> &reqs, int rpp, bool by_slot, size_t &n_shared)
{
  const int n = int(reqs.size());
  const std::vector<pass<T>> P = plan<T>(reqs.data(), n, rpp, by_slot);
  const int cut = std::max(1, std::min(rpp, MAX_PASS));
  if (int(P.size()) != (n + cut - 1) / cut) FAIL("plan: %zu passes for %d requests at %d per pass", P.size(), n, cut);
  std::set<int> seen;
  for (const pass<T> &p : P) {
    if (p.n < 1 || p.n > cut) FAIL("plan: a pass of %d requests", p.n);
    unsigned used = 0;
    for (int s = 0; s < p.n; ++s) {
      const dev_req<T> &d = p.tab.r[s];
      const int src = p.src[s];
      if (src < 0 || src >= n || !seen.insert(src).second) FAIL("plan: request %d missing or twice", src);
      const lcx_diag_req_t &q = reqs[size_t(src)];
      if (d.row != uint32_t(by_slot ? s : src)) FAIL("plan: row %u of slot %d (request %d)", d.row, s, src);
      if (d.n_clauses != q.n_clauses || d.count != q.count) FAIL("plan: request %d altered", src);
      for (int c = 0; c < q.n_clauses; ++c) {
        double lo = 0, hi = 0;
        if (sel_is_range(q.clause[c].sel)) rng_bounds(q.clause[c].sel, q.clause[c].lo, q.clause[c].hi, lo, hi);
        if (d.sel[c] != q.clause[c].sel || d.lo[c] != T(lo) || d.hi[c] != T(hi)) FAIL("plan: clause %d of request %d altered", c, src);
        if (q.clause[c].sel != LCX_DIAG_SEL_ALL) used |= 1u << sel_attr(q.clause[c].sel);
      }
      if (q.count != LCX_DIAG_SD_CONC) {
        used |= 1u << count_attr(q.count);
        if (d.attr != count_attr(q.count) || d.power != T(mom_power(q.count, q.k))) FAIL("plan: power of request %d altered", src);
      }
      // same_pow exactly when the slot before is a moment of the same attribute and power
      const bool same = s > 0 && q.count != LCX_DIAG_SD_CONC && p.tab.r[s - 1].count != LCX_DIAG_SD_CONC && p.tab.r[s - 1].attr == d.attr &&
                        std::memcmp(&p.tab.r[s - 1].power, &d.power, sizeof(T)) == 0;
      if (bool(d.same_pow) != same) FAIL("plan: same_pow of slot %d is %d", s, int(d.same_pow));
      n_shared += same;
    }
    if (used != p.used) FAIL("plan: used attributes %u, expected %u", p.used, used);
  }
  if (int(seen.size()) != n) FAIL("plan: %zu of %d requests planned", seen.size(), n);
  return 0;
}

int main()
{
  std::string err;
  size_t n_cases = 0;
  // ---- validation: each malformed list is named, and nothing past the list's end is read
  if (!validate(nullptr, 0, err)) FAIL("an empty list must pass: %s", err.c_str());
  if (validate(nullptr, -1, err) || err.find("n_req < 0") == std::string::npos) FAIL("n_req < 0: %s", err.c_str());
  if (validate(nullptr, 3, err) || err.find("req == NULL") == std::string::npos) FAIL("null list: %s", err.c_str());
  for (int n = 1; n <= 70; ++n) {
    std::vector<lcx_diag_req_t> reqs;
    for (int i = 0; i < n; ++i) reqs.push_back(good(i));
    reqs.shrink_to_fit();
    if (!validate(reqs.data(), n, err)) FAIL("a good list of %d fails: %s", n, err.c_str());
    const int at = int(rnd() % unsigned(n));
    struct { int field, value; const char *needle; } bad[] = {
      {0, 0, "n_clauses = 0"}, {0, LCX_DIAG_MAX_CLAUSES + 1, "n_clauses = 5"}, {0, -7, "n_clauses = -7"}, {0, 1 << 30, "n_clauses"},
      {1, 5, "unknown sel 5"}, {1, -1, "unknown sel -1"}, {2, 4, "unknown count 4"}, {2, -1, "unknown count -1"}, {2, 1 << 20, "unknown count"}};
    for (const auto &b : bad) {
      std::vector<lcx_diag_req_t> r2(reqs);
      r2.shrink_to_fit();
      if (b.field == 0) r2[size_t(at)].n_clauses = b.value;
      else if (b.field == 1) r2[size_t(at)].clause[r2[size_t(at)].n_clauses - 1].sel = b.value;
      else r2[size_t(at)].count = b.value;
      if (validate(r2.data(), n, err)) FAIL("malformed request passes (%s)", b.needle);
      if (err.find(b.needle) == std::string::npos || err.find("request " + std::to_string(at) + ":") == std::string::npos) FAIL("wrong text for %s at %d: %s", b.needle, at, err.c_str());
      ++n_cases;
    }
  }
  // ---- pass size: never above the kernel's table, never below one, and within the cap whenever more than one request is granted
  for (size_t n_cell : {size_t(0), size_t(1), size_t(6), size_t(270), size_t(1) << 21, size_t(1) << 26, size_t(1) << 31, ~size_t(0) / 64})
    for (size_t rb : {size_t(4), size_t(8)}) {
      const int rpp = req_per_pass(n_cell, rb);
      if (rpp < 1 || rpp > MAX_PASS) FAIL("req_per_pass(%zu, %zu) = %d", n_cell, rb, rpp);
      if (rpp > 1 && scratch_bytes(n_cell, rb) > SCRATCH_CAP) FAIL("scratch above the cap at %zu cells", n_cell);
      ++n_cases;
    }
  // ---- plans: large and random lists, both real types, every pass size, both row rules
  size_t n_shared = 0;
  for (int n : {0, 1, 2, 31, 32, 33, 65, 1000, 20000}) {
    std::vector<lcx_diag_req_t> reqs;
    for (int i = 0; i < n; ++i) reqs.push_back(good(i));
    reqs.shrink_to_fit();
    for (int rpp : {-3, 1, 2, 7, 32, 1000}) {
      if (n > 1000 && rpp != 32 && rpp != 7) continue;
      for (bool by_slot : {false, true}) {
        if (check_plan<double>(reqs, rpp, by_slot, n_shared) || check_plan<float>(reqs, rpp, by_slot, n_shared)) return 1;
        n_cases += 2;
      }
    }
  }
  if (!n_shared) FAIL("no two requests ever shared a power: the ordering does nothing");
  std::printf("ok: %zu cases, %zu shared powers\n", n_cases, n_shared);
  return 0;
}
