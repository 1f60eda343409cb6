// lcx_dump_plan.hpp -- what the particle dump (include/lcx_dump.h) settles on the host: the validation of its arguments and the kinds of
// source that a field is gathered from.  The integer rule of how many droplets are written is lcx_track_plan.hpp's (track::stride,
// track::count, track::taken), unchanged, with room = max_count.
//
// No HIP include: lcx_core.hip validates with it, lcx_dump_check is the same function without an object, lcx_kernels.hpp's k_dump_gather
// reads the descriptors that lcx_core.hip fills, and tools/dump_plan_check.cpp compiles it alone under the host sanitizers.
#ifndef LCX_DUMP_PLAN_HPP
#define LCX_DUMP_PLAN_HPP

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/lcx_dump.h"
#include "lcx_track_plan.hpp"

namespace lcx {
namespace dump {

// where a field's value comes from: a u64 column (n), the cell index column, the slot itself, a column of the object's real type, a cell
// array of the real type read through the cell index (NaN where that is no cell), or nothing (a constant 0: a position the object lacks,
// the mark of an object that does not track)
enum kind_t { K_U64, K_IJK, K_SLOT, K_REAL, K_CELL, K_ZERO };
struct field_desc { int kind; const void *p; };

inline bool is_chem(int f) { return f >= LCX_DMP_CHEM_HNO3 && f <= LCX_DMP_CHEM_H; }

// the first fault of a dump's selection and field list, named; true when there is none.  read_pair[d]: whether the pair of dimension d of
// `box` is read (NULL: all three); has_chem / has_ict: whether the object has the optional columns (lcx_dump_check: taken as given)
inline bool validate(const lcx_diag_clause_t *clause, int n_clauses, const double *box, const int *field, int n_fields, std::string &err,
                     const bool read_pair[3] = nullptr, bool has_chem = true, bool has_ict = true)
{
  const std::string at = "libcloudph++: dump: ";
  if (n_clauses < 1 || n_clauses > LCX_DIAG_MAX_CLAUSES) {
    err = at + "n_clauses = " + std::to_string(n_clauses) + " is outside 1 .. " + std::to_string(LCX_DIAG_MAX_CLAUSES);
    return false;
  }
  if (!clause) { err = at + "clause == NULL"; return false; }
  for (int c = 0; c < n_clauses; ++c)
    if (clause[c].sel < LCX_DIAG_SEL_ALL || clause[c].sel > LCX_DIAG_SEL_WATER) {
      err = at + "clause " + std::to_string(c) + ": unknown sel " + std::to_string(clause[c].sel);
      return false;
    }
  if (box)
    for (int d = 0; d < 3; ++d) {
      if (read_pair && !read_pair[d]) continue;
      const double lo = box[2 * d], hi = box[2 * d + 1];
      if (!std::isfinite(lo) || !std::isfinite(hi)) { err = at + "box: bound " + std::to_string(!std::isfinite(lo) ? 2 * d : 2 * d + 1) + " is not finite"; return false; }
      if (lo > hi) { err = at + "box: lo > hi in pair " + std::to_string(d); return false; }
    }
  if (n_fields < 1 || n_fields > LCX_DMP_FIELDS) {
    err = at + "n_fields = " + std::to_string(n_fields) + " is outside 1 .. " + std::to_string(int(LCX_DMP_FIELDS));
    return false;
  }
  if (!field) { err = at + "field == NULL"; return false; }
  bool seen[LCX_DMP_FIELDS] = {};
  for (int f = 0; f < n_fields; ++f) {
    const int id = field[f];
    if (id < 0 || id >= LCX_DMP_FIELDS) { err = at + "field " + std::to_string(f) + ": unknown field " + std::to_string(id); return false; }
    if (seen[id]) { err = at + "field " + std::to_string(f) + ": field " + std::to_string(id) + " is given twice"; return false; }
    seen[id] = true;
  }
  for (int f = 0; f < n_fields; ++f) {
    if (is_chem(field[f]) && !has_chem) { err = at + "field " + std::to_string(f) + ": a chemistry field, but opts_init.chem_switch is off"; return false; }
    if (field[f] == LCX_DMP_INCLOUD_TIME && !has_ict) { err = at + "field " + std::to_string(f) + ": incloud_time, but opts_init.diag_incloud_time is off"; return false; }
  }
  return true;
}
// ... and of where the output goes
inline bool validate_out(const void *out, size_t field_stride, size_t max_count, std::string &err)
{
  const std::string at = "libcloudph++: dump: ";
  if (!out) return true;                                 // (the call only counts: neither number is read)
  if (max_count == 0) { err = at + "max_count == 0"; return false; }
  if (field_stride < max_count) { err = at + "field_stride (" + std::to_string(field_stride) + ") < max_count (" + std::to_string(max_count) + ")"; return false; }
  return true;
}

} // namespace dump
} // namespace lcx
#endif
