// The host side of the particle dump (csrc/lcx_dump_plan.hpp) in a program of its own: every text of the validation, with arrays of exactly
// the length that the arguments name (a read beyond them is the address sanitizer's to find), and the rule of how many droplets are
// written -- lcx_track_plan.hpp's stride, count and taken with room = max_count -- walked over the ranks.  No HIP include: the host
// compiler alone (tests/test_dump_plan_host.py builds it with -fsanitize=address,undefined).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "../libcloudphxx_amd/csrc/lcx_dump_plan.hpp"

using namespace lcx;

static int checks = 0;
static void need(bool ok, const std::string &what)
{
  ++checks;
  if (!ok) { std::fprintf(stderr, "FAILED: %s\n", what.c_str()); std::exit(1); }
}
static void refused(const std::vector<lcx_diag_clause_t> &c, int nc, const double *box, const std::vector<int> &f, int nf, const std::string &text,
                    const bool *pair = nullptr, bool chem = true, bool ict = true, bool null_clause = false, bool null_field = false)
{
  std::string err;
  const bool ok = dump::validate(null_clause ? nullptr : c.data(), nc, box, null_field ? nullptr : f.data(), nf, err, pair, chem, ict);
  need(!ok && err == "libcloudph++: dump: " + text, text + " (got: " + err + ")");
}

int main()
{
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  std::vector<lcx_diag_clause_t> one{{LCX_DIAG_SEL_ALL, 0, 0}}, two{{LCX_DIAG_SEL_WET, 1e-6, 2e-6}, {LCX_DIAG_SEL_WATER, 0, 0}};
  std::vector<int> all;
  for (int f = 0; f < LCX_DMP_FIELDS; ++f) all.push_back(f);
  std::string err;
  need(dump::validate(one.data(), 1, nullptr, all.data(), LCX_DMP_FIELDS, err), "every field once");
  const double box[6] = {0, 1, 0, 0, -1, 5};
  need(dump::validate(two.data(), 2, box, std::vector<int>{LCX_DMP_SLOT}.data(), 1, err), "a box with an empty pair");
  refused(one, 0, nullptr, all, 1, "n_clauses = 0 is outside 1 .. " + std::to_string(LCX_DIAG_MAX_CLAUSES));
  refused(one, LCX_DIAG_MAX_CLAUSES + 1, nullptr, all, 1, "n_clauses = " + std::to_string(LCX_DIAG_MAX_CLAUSES + 1) + " is outside 1 .. " + std::to_string(LCX_DIAG_MAX_CLAUSES));
  refused(one, 1, nullptr, all, 1, "clause == NULL", nullptr, true, true, true);
  std::vector<lcx_diag_clause_t> bad{{LCX_DIAG_SEL_ALL, 0, 0}, {9, 0, 0}};
  refused(bad, 2, nullptr, all, 1, "clause 1: unknown sel 9");
  const double b1[6] = {0, 1, 2, 1, 0, 1}, b2[6] = {0, 1, 0, 1, 0, inf}, b3[6] = {nan, 1, 0, 1, 0, 1};
  refused(one, 1, b1, all, 1, "box: lo > hi in pair 1");
  refused(one, 1, b2, all, 1, "box: bound 5 is not finite");
  refused(one, 1, b3, all, 1, "box: bound 0 is not finite");
  const bool no_y[3] = {true, false, true};
  need(dump::validate(one.data(), 1, b1, all.data(), 1, err, no_y), "the pair of a dimension that is not read may hold anything");
  refused(one, 1, nullptr, all, 0, "n_fields = 0 is outside 1 .. " + std::to_string(int(LCX_DMP_FIELDS)));
  refused(one, 1, nullptr, all, LCX_DMP_FIELDS + 1, "n_fields = " + std::to_string(LCX_DMP_FIELDS + 1) + " is outside 1 .. " + std::to_string(int(LCX_DMP_FIELDS)));
  refused(one, 1, nullptr, all, 2, "field == NULL", nullptr, true, true, false, true);
  refused(one, 1, nullptr, {0, LCX_DMP_FIELDS}, 2, "field 1: unknown field " + std::to_string(int(LCX_DMP_FIELDS)));
  refused(one, 1, nullptr, {-3}, 1, "field 0: unknown field -3");
  refused(one, 1, nullptr, {LCX_DMP_RW2, LCX_DMP_N, LCX_DMP_RW2}, 3, "field 2: field " + std::to_string(int(LCX_DMP_RW2)) + " is given twice");
  for (int f = LCX_DMP_CHEM_HNO3; f <= LCX_DMP_CHEM_H; ++f)
    refused(one, 1, nullptr, {LCX_DMP_N, f}, 2, "field 1: a chemistry field, but opts_init.chem_switch is off", nullptr, false, true);
  refused(one, 1, nullptr, {LCX_DMP_INCLOUD_TIME}, 1, "field 0: incloud_time, but opts_init.diag_incloud_time is off", nullptr, true, false);
  need(dump::validate(one.data(), 1, nullptr, all.data(), LCX_DMP_INCLOUD_TIME, err, nullptr, false, false), "the fields below the optional ones need no option");
  // where the output goes
  double x = 0;
  need(dump::validate_out(nullptr, 0, 0, err), "out == NULL: the call only counts");
  need(!dump::validate_out(&x, 8, 0, err) && err == "libcloudph++: dump: max_count == 0", "max_count == 0");
  need(!dump::validate_out(&x, 7, 8, err) && err == "libcloudph++: dump: field_stride (7) < max_count (8)", "field_stride < max_count");
  need(dump::validate_out(&x, 8, 8, err), "field_stride == max_count");
  // how many are written: the ranks taken are written at consecutive indices below max_count, and one stride less would not fit
  for (uint64_t room : std::vector<uint64_t>{1, 2, 3, 7, 64, 1000})
    for (uint64_t Q : std::vector<uint64_t>{0, 1, room - 1, room, room + 1, 2 * room + 1, 135 * room + 1}) {
      const uint64_t s = track::stride(Q, room), w = track::count(Q, s);
      uint64_t next = 0;
      for (uint64_t q = 0; q < Q; ++q) if (track::taken(q, s)) { need(q / s == next, "consecutive indices"); ++next; }
      need(next == w && w <= room && (Q == 0) == (s == 0), "n_written = ceil(Q / stride) <= max_count");
      if (s > 1) need(track::count(Q, s - 1) > room, "the smallest stride that fits");
      if (Q && Q <= room) need(s == 1 && w == Q, "everything fits: stride 1");
    }
  std::printf("ok: %d checks\n", checks);
  return 0;
}
