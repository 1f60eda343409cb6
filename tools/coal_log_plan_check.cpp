// The host side of the collision log (csrc/lcx_coal_log_plan.hpp) in a program of its own: every text of the validation, the layout of
// the list at its edges (the largest capacity whose bytes size_t holds, and the one above), and the rule of how many events are held and
// whether a read's room fits them, walked over seen, capacity and cap_events around their boundaries.  No HIP include: the host compiler
// alone (tests/test_coal_log_plan_host.py builds it with -fsanitize=address,undefined).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "../libcloudphxx_amd/csrc/lcx_coal_log_plan.hpp"

using namespace lcx;

static int checks = 0;
static void need(bool ok, const std::string &what)
{
  ++checks;
  if (!ok) { std::fprintf(stderr, "FAILED: %s\n", what.c_str()); std::exit(1); }
}
static void refused(size_t capacity, double r_min, const std::string &text)
{
  std::string err;
  need(!coal_log::validate(capacity, r_min, err) && err == "libcloudph++: coal_log: " + text, text + " (got: " + err + ")");
}

int main()
{
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  const size_t top = std::numeric_limits<size_t>::max();
  std::string err;
  // capacity and r_min
  need(coal_log::validate(1, 0., err) && coal_log::validate(1u << 20, 25e-6, err), "a capacity and a radius");
  need(coal_log::validate(coal_log::max_capacity(), 0., err), "the largest capacity");
  refused(0, 0., "capacity == 0");
  refused(0, -1., "capacity == 0");                                    // (the first fault is the one named)
  for (size_t c : std::vector<size_t>{coal_log::max_capacity() + 1, top})
    refused(c, 0., "capacity = " + std::to_string(c) + ": a list of " + std::to_string(int(LCX_CLG_FIELDS)) + " rows has more bytes than size_t holds");
  for (double r : std::vector<double>{-1e-300, -1., -inf, inf, nan}) refused(8, r, "r_min must be non-negative and finite");
  // the layout: rows of `capacity` words one behind the other, the last word of the last row is the last of the bytes
  static_assert(LCX_CLG_FIELDS == 14 && coal_log::WORD == 8, "fourteen rows of 8-byte words");
  for (size_t cap : std::vector<size_t>{1, 5, 64, 65, 1u << 20, coal_log::max_capacity()}) {
    need(coal_log::row(0, cap) == 0, "the first row begins the list");
    for (int f = 1; f < LCX_CLG_FIELDS; ++f) need(coal_log::row(f, cap) - coal_log::row(f - 1, cap) == cap, "rows are a capacity apart");
    need(coal_log::words(cap) == coal_log::row(LCX_CLG_FIELDS - 1, cap) + cap, "the last row ends the list");
    need(coal_log::bytes(cap) / coal_log::WORD == coal_log::words(cap) && coal_log::bytes(cap) / cap == size_t(LCX_CLG_FIELDS) * coal_log::WORD, "bytes without a wrap");
  }
  need(coal_log::max_capacity() + 1 > top / (size_t(LCX_CLG_FIELDS) * coal_log::WORD), "one more would wrap");
  for (int f = 0; f < LCX_CLG_FIELDS; ++f) need(coal_log::is_integer(f) == (f <= LCX_CLG_N_R), "the integer rows come first");
  // held = min(seen, capacity); a read fits exactly when cap_events >= held
  const unsigned long long big = std::numeric_limits<unsigned long long>::max();
  for (size_t cap : std::vector<size_t>{1, 5, 64, 1000, top})
    for (unsigned long long seen : std::vector<unsigned long long>{0, 1, cap - 1, cap, (unsigned long long)cap + 1, 2ull * cap + 1, big}) {
      const unsigned long long held = coal_log::held(seen, cap);
      need(held <= seen && held <= cap && (held == seen || held == cap), "held = min(seen, capacity)");
      for (size_t room : std::vector<size_t>{0, 1, size_t(held) - 1, size_t(held), size_t(held) + 1, top}) {
        const bool fits = coal_log::fits(seen, cap, room);
        need(fits == (room >= held), "a read fits exactly when cap_events >= held");
        std::string e;
        need(coal_log::validate_room(seen, cap, room, e) == fits, "the room's validation is the kernels' rule");
        if (!fits) need(e == "libcloudph++: coal_log: cap_events (" + std::to_string(room) + ") < held (" + std::to_string(held) + ")", "cap_events < held (got: " + e + ")");
      }
    }
  // where a read's output goes
  double x = 0;
  need(!coal_log::validate_out(nullptr, 8, 8, err) && err == "libcloudph++: coal_log: out == NULL", "out == NULL");
  need(!coal_log::validate_out(&x, 7, 8, err) && err == "libcloudph++: coal_log: field_stride (7) < cap_events (8)", "field_stride < cap_events");
  need(coal_log::validate_out(&x, 8, 8, err) && coal_log::validate_out(&x, 0, 0, err), "field_stride == cap_events");
  need(coal_log::not_enabled("read") == "libcloudph++: coal_log: read while the log is not enabled (lcx_coal_log_enable)", "not enabled");
  need(coal_log::alloc_failed(112, "out of memory") == "libcloudph++: coal_log: the device allocation of 112 bytes failed (out of memory)", "the bytes asked for");
  std::printf("ok: %d checks\n", checks);
  return 0;
}
