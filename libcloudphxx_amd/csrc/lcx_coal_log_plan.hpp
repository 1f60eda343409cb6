// lcx_coal_log_plan.hpp -- what the collision log (include/lcx_coal_log.h) settles on the host: the validation that lcx_coal_log_check and
// lcx_coal_log_enable share, the layout of the list (its bytes for a capacity, where a field's row begins, which rows hold integers) and
// the rule of how many events are held and written.
//
// No HIP include: lcx_core.hip validates and sizes with it, lcx_kernels.hpp's coal_log_event and k_coal_log_f64 index with the same
// constexpr functions, and tools/coal_log_plan_check.cpp compiles it alone under the host sanitizers.
#ifndef LCX_COAL_LOG_PLAN_HPP
#define LCX_COAL_LOG_PLAN_HPP

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <string>

#include "../../include/lcx_coal_log.h"

namespace lcx {
namespace coal_log {

constexpr size_t WORD = 8;                                                       // every element of the list: a u64 or a double
// the list is [LCX_CLG_FIELDS][capacity] words, field-major: a wave's events land in consecutive words of each row
constexpr size_t row(int field, size_t capacity) { return size_t(field) * capacity; }
constexpr size_t words(size_t capacity) { return size_t(LCX_CLG_FIELDS) * capacity; }
constexpr size_t bytes(size_t capacity) { return words(capacity) * WORD; }
constexpr size_t max_capacity() { return std::numeric_limits<size_t>::max() / (size_t(LCX_CLG_FIELDS) * WORD); }
// rows below RW2_D hold unsigned 64-bit integers, the others doubles (the object's real type, widened exactly)
constexpr bool is_integer(int field) { return field < LCX_CLG_RW2_D; }
// how many events the list holds after `seen` were logged: those beyond the capacity were dropped
constexpr unsigned long long held(unsigned long long seen, size_t capacity) { return seen < capacity ? seen : (unsigned long long)capacity; }
// whether a read with room for cap_events per row writes (it writes all held events or none)
constexpr bool fits(unsigned long long seen, size_t capacity, size_t cap_events) { return held(seen, capacity) <= cap_events; }

inline const std::string &at() { static const std::string s = "libcloudph++: coal_log: "; return s; }

// the first fault of capacity and r_min, named; true when there is none
inline bool validate(size_t capacity, double r_min, std::string &err)
{
  if (capacity == 0) { err = at() + "capacity == 0"; return false; }
  if (capacity > max_capacity()) {
    err = at() + "capacity = " + std::to_string(capacity) + ": a list of " + std::to_string(int(LCX_CLG_FIELDS)) + " rows has more bytes than size_t holds";
    return false;
  }
  if (!(r_min >= 0) || !std::isfinite(r_min)) { err = at() + "r_min must be non-negative and finite"; return false; }
  return true;
}
// ... of where a read's output goes, before anything is launched
inline bool validate_out(const void *out, size_t field_stride, size_t cap_events, std::string &err)
{
  if (!out) { err = at() + "out == NULL"; return false; }
  if (field_stride < cap_events) { err = at() + "field_stride (" + std::to_string(field_stride) + ") < cap_events (" + std::to_string(cap_events) + ")"; return false; }
  return true;
}
// ... and of the room, once the cursor is known (the kernels have applied the same rule and written nothing)
inline bool validate_room(unsigned long long seen, size_t capacity, size_t cap_events, std::string &err)
{
  if (fits(seen, capacity, cap_events)) return true;
  err = at() + "cap_events (" + std::to_string(cap_events) + ") < held (" + std::to_string(held(seen, capacity)) + ")";
  return false;
}
inline std::string not_enabled(const char *what) { return at() + what + " while the log is not enabled (lcx_coal_log_enable)"; }
inline std::string alloc_failed(size_t n_bytes, const char *why) { return at() + "the device allocation of " + std::to_string(n_bytes) + " bytes failed (" + why + ")"; }

} // namespace coal_log
} // namespace lcx
#endif
