// lcx_track_plan.hpp -- what tracked super-droplets (include/lcx_track.h) settle in integers, on both sides: the stride rule of a
// selection, the indexing of the sample buffer, and the validation of a selection's arguments.
//
// No HIP include: lcx_core.hip plans with it, lcx_kernels.hpp's k_track_assign and k_track_sample apply the same two functions per lane,
// lcx_track_check is its validation, and tools/track_plan_check.cpp compiles it alone under the host sanitizers.
#ifndef LCX_TRACK_PLAN_HPP
#define LCX_TRACK_PLAN_HPP

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/lcx_track.h"

#if defined(__HIPCC__)
#define LCX_TRK_HD __host__ __device__ inline
#else
#define LCX_TRK_HD inline
#endif

namespace lcx {
namespace track {

constexpr uint32_t NONE = 0xFFFFFFFFu;                 // slot_of[k]: no storage slot carries mark k + 1

// how many more droplets a selection may take
LCX_TRK_HD uint64_t room(uint64_t max_count, uint64_t max_tracked, uint64_t n_tracked)
{
  const uint64_t left = max_tracked > n_tracked ? max_tracked - n_tracked : 0;
  return max_count < left ? max_count : left;
}
// Q qualifying droplets ranked q = 0 .. Q - 1 in storage order: those with q % stride == 0 are taken.  0: nothing is.
// (no Q + room - 1: that sum may wrap)
LCX_TRK_HD uint64_t stride(uint64_t Q, uint64_t room_) { return (Q == 0 || room_ == 0) ? 0 : Q / room_ + (Q % room_ != 0); }
// ... and that many are: ceil(Q / stride) <= room
LCX_TRK_HD uint64_t count(uint64_t Q, uint64_t stride_) { return stride_ == 0 ? 0 : Q / stride_ + (Q % stride_ != 0); }
LCX_TRK_HD bool taken(uint64_t q, uint64_t stride_) { return stride_ != 0 && q % stride_ == 0; }
// the track index of rank q behind n_tracked earlier ones
LCX_TRK_HD uint64_t index_of(uint64_t q, uint64_t stride_, uint64_t n_tracked) { return n_tracked + q / stride_; }

// the sample buffer: capacity x LCX_TRK_FIELDS x max_tracked doubles, field-major inside a sample
LCX_TRK_HD size_t buf_offset(size_t s, int f, size_t k, size_t max_tracked) { return (s * size_t(LCX_TRK_FIELDS) + size_t(f)) * max_tracked + k; }
LCX_TRK_HD size_t buf_elems(size_t capacity, size_t max_tracked) { return capacity * size_t(LCX_TRK_FIELDS) * max_tracked; }

// the first fault of a selection's arguments, named; true when there is none.  read_pair[d]: whether the pair of dimension d of `box` is read
// (NULL: all three, without an object: lcx_track_check)
inline bool validate(const lcx_diag_clause_t *clause, int n_clauses, const double *box, size_t max_count, std::string &err, const bool read_pair[3] = nullptr)
{
  const std::string at = "libcloudph++: track: ";
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
  if (max_count == 0) { err = at + "max_count == 0"; return false; }
  return true;
}

} // namespace track
} // namespace lcx
#endif
