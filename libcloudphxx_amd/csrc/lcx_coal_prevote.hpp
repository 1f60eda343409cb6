// lcx_coal_prevote.hpp -- what must be the same code on both sides of the coalescence's per-cell vote (round 10), host and device.
//
// k_coal_ranked<.., SKIP, EXIT> lets a workgroup leave where every pair of its 512 positions has `bound < 1 && u >= bound` (lcx_kernels.hpp,
// above coal_pair).  `bound` is made of the pair's CELL alone and `u` of the pair's position, the call number and the seed alone, so whether a
// cell holds a kept pair can be settled per cell ahead of the launch:  kept_c  iff  !(bound_c < 1 && umin_c >= bound_c),  umin_c the smallest
// draw of the cell's pairs (k_coal_umin, k_coal_cellvote).  The pieces here are the ones both sides evaluate: the bound (coal_skipped calls it),
// the cell's smallest draw, and which workgroups' tiles a cell's stretch of the sorted order overlaps.
// The header needs lcx_math.hpp alone and compiles for the host by itself (tools/coal_prevote_check.cpp).
#pragma once
#include <math.h>
#include "lcx_math.hpp"

namespace lcx {

LCX_HD float u32_as_float(uint32_t u) { return __builtin_bit_cast(float, u); }
LCX_HD int kernel_index(n_t R) { return R <= 100. ? int(R) : int(100 + (R - 100.) / 10.); }          // kernel_interpolation.hpp: the table's node of a radius in um

constexpr uint32_t COAL_BOUND_NAN = 0xFFFFFFFFu;       // (= CMAX_POISON: what the velocity pass leaves for a cell whose maxima cannot be trusted)

// scale_factor, coal.ipp:99-107, of a cell that holds nn droplets
template <class T> LCX_HD T coal_scale_of(const n_t nn) { return nn > 1 ? (T(nn * (nn - 1)) / 2) / (nn / 2) : T(0); }

// The upper bound on the collision probability of any pair of a cell (derivation above coal_pair): r_bits and v_bits are the bits of the cell's
// largest rw2 and vt as floats rounded up, dvc its volume, scl its scale factor.  NaN where no bound can be given: a poisoned cell (either word
// all ones), an infinite maximum, a NaN anywhere, or a cell whose largest radius is within 11 um of the table's end.
template <class T>
LCX_HD T coal_bound(const uint32_t r_bits, const uint32_t v_bits, const T dvc, const T scl, const T dt, const T n_max, const T r_max, const T *emax, const int n_emax)
{
  const T rm = T(u32_as_float(r_bits)), vm = T(u32_as_float(v_bits));
  T bound = T(u32_as_float(COAL_BOUND_NAN));                                   // NaN
  const T r_um = sqrt(rm) * T(1e6) * T(1 + 1. / 1024);
  if (r_um < r_max - T(11) && vm < T(3e38)) {                                  // (false for a NaN)
    const n_t x0 = r_um >= T(100) ? n_t(floor(r_um / 10) * 10) : n_t(floor(r_um));
    const int ie = kernel_index(x0);
    bound = dt / dvc * scl * n_max * T(cst<T>::pi * 4) * rm * vm * emax[ie < n_emax ? ie : n_emax - 1] * T(1 + 1. / 1024);
    if (bound < T(1e-30)) bound = T(1e-30);
  }
  return bound;
}

// The words of a cell's maxima (k_vterm_b77<.., CELLMAX> writes them, coal_bound reads them): the bits of a positive float rounded UP, never
// below CMAX_FLOOR (FLT_MIN: a recorded maximum is never zero or subnormal); all ones where the maxima cannot be trusted.
constexpr uint32_t CMAX_POISON = 0xFFFFFFFFu, CMAX_FLOOR = 0x00800000u;
template <class T>
LCX_HD uint32_t float_bits_up(T x)                                             // x > 0 (infinity included)
{
  const float f = float(x);
  uint32_t b = __builtin_bit_cast(uint32_t, f);
  if (T(f) < x) ++b;                                                          // rounded down: the next float up
  return b < CMAX_FLOOR ? CMAX_FLOOR : b;
}

// Round 12, THE FLOOR UNDER THE MAXIMA.  The bound is monotone in both maxima (emax[] is a running maximum), so any words >= the true maxima are
// sound: they only keep more cells.  Every cell's words start from (R_f^2, V_f) instead of zero, and a droplet at or below both has nothing to
// offer (k_vterm_b77<.., CELLMAX>: the narrow cloud spectrum leaves a few percent of the droplets above).  R_f is the largest radius of a grid
// of COAL_FLOOR_STEP_UM (a quarter of the efficiency table's finest spacing) up to which the bound of a reference cell (volume dvc, scale factor
// scl) from the floor alone stays <= eps; V_f is 1.5 x the formula's reference velocity there (any positive choice is sound: this one sets how
// tight the floor is -- the correction factor of beard77 stays below 1.5 up to 500 hPa).  Where no radius qualifies, and where the table gives
// no bound, (CMAX_FLOOR, CMAX_FLOOR): no floor at all.
// eps by measurement (EXPERIMENTS.md 7.21; 128^3 x 64, f64, ms per step over 200 steps, three runs by turns, the parent 6.931): 2^-13 6.818,
// 2^-14 6.756, 2^-16 6.758.  A higher floor leaves fewer droplets offering and keeps more cells, which the vote's one cursor and k_coal_cells
// pay for; 2^-14 of the two that tie, the one that keeps fewer droplets offering in the first hundred steps.
constexpr double COAL_FLOOR_EPS = 1. / 16384, COAL_FLOOR_EPS_HIGH = 1. / 64, COAL_FLOOR_STEP_UM = 0.25;
struct coal_floor_words { uint32_t r_bits, v_bits; };
LCX_HD coal_floor_words coal_floor_at(const int k)                             // the words of grid radius k (k >= 1)
{
  const double r = k * COAL_FLOOR_STEP_UM * 1e-6;
  return coal_floor_words{float_bits_up(r * r), float_bits_up(1.5 * vt_beard77_v0(r))};
}
template <class T>
LCX_HD coal_floor_words coal_cmax_floor(const T dt, const T dvc, const T scl, const T n_max, const T r_max, const T *emax, const int n_emax, const T eps)
{
  coal_floor_words best{CMAX_FLOOR, CMAX_FLOOR};
  if (n_emax <= 0 || !(eps > T(0))) return best;
  const int k_end = int((double(r_max) - 11.) / COAL_FLOOR_STEP_UM);            // (coal_bound gives none beyond)
  for (int k = 1; k < k_end; ++k) {
    const coal_floor_words w = coal_floor_at(k);
    if (!(coal_bound<T>(w.r_bits, w.v_bits, dvc, scl, dt, n_max, r_max, emax, n_emax) <= eps)) break;        // (a NaN ends it too)
    best = w;
  }
  return best;
}
// does a droplet's pair of words rise above the floor's in either word?  (CMAX_POISON does by construction.)
LCX_HD bool coal_above_floor(const uint32_t r, const uint32_t v, const coal_floor_words f) { return r > f.r_bits || v > f.v_bits; }

// The smallest draw of the pairs of the cell whose stretch of the sorted order is [off, end): a pair's draw is philox::u01<T>(p, call, seed) with
// p the position of its first member, off + 2 j for j < (end - off) / 2 (pairs sit at even in-cell offsets).  The position travels as 64 bits, as
// in philox::gen.  Fewer than two droplets: no pair, +inf.  (first, stride): the share of one of `stride` lanes that split a cell between them.
// end < off (bounds that do not belong together: the host's ordering rules that out, the loop does not rely on it) counts as an empty cell.
template <class T>
LCX_HD T coal_cell_umin(const uint64_t off, const uint64_t end, const uint64_t call, const uint64_t seed, const uint64_t first = 0, const uint64_t stride = 1)
{
  T m = T(__builtin_huge_valf());
  const uint64_t n_pairs = end > off ? (end - off) / 2 : 0;
  for (uint64_t j = first; j < n_pairs; j += stride) {
    const T u = philox::u01<T>(off + 2 * j, call, seed);
    if (u < m) m = u;
  }
  return m;
}

// The pairs of the cell [off, end) as k_coal_cells walks them: their number, and the position of pair j's first member (the same positions
// coal_cell_umin draws at, so the vote and the kernel look at the same draws).
LCX_HD uint64_t coal_cell_pairs(const uint64_t off, const uint64_t end) { return end > off ? (end - off) / 2 : 0; }
LCX_HD uint64_t coal_pair_pos(const uint64_t off, const uint64_t j) { return off + 2 * j; }

// The list of kept cells (k_coal_cellvote leaves it, k_coal_cells reads it) is shared out among the waves of a grid that does not grow with the
// list: wave `wave` of workgroup `wg` takes the entries first, first + step, ... below the count.  Every entry below the count is taken by exactly
// one wave whatever the grid (tools/coal_cells_check.cpp); the host sizes the grid with coal_cells_grid (at least one workgroup, at most `cap`).
struct coal_list_share { uint64_t first, step; };
LCX_HD coal_list_share coal_list_share_of(const uint64_t wg, const uint64_t n_wg, const uint64_t wave, const uint64_t waves_per_wg)
{
  return coal_list_share{wg * waves_per_wg + wave, n_wg * waves_per_wg};
}
LCX_HD uint64_t coal_cells_grid(const uint64_t n_cell, const uint64_t waves_per_wg, const uint64_t cap)
{
  const uint64_t want = (n_cell + waves_per_wg - 1) / waves_per_wg;
  return want < 1 ? 1 : want > cap ? cap : want;
}

// Round 12: THE LIST IN SUB-LISTS.  One cursor for the whole list made every wave of the vote that keeps a cell queue behind the others in the L2
// (12 ns each; EXPERIMENTS.md 7.17, 7.21): the list is COAL_SUBLISTS sub-lists with a cursor each, a wave of the vote appending to the sub-list of
// its number modulo COAL_SUBLISTS.  Sub-list s occupies the entries [s * cap, s * cap + length_s) of the list's storage, cap = coal_sublist_cap:
// room for every cell that the waves of one sub-list can keep (cells_per_wave each).  k_coal_cells still walks global indices li below the total:
// a wave reads the lengths once, keeps their prefix sums (prefix[0] = 0 ... prefix[COAL_SUBLISTS] = the total) and maps li to its place --
// the sub-list s with prefix[s] <= li < prefix[s + 1], hence a sub-list that is not empty and an offset below its length, an entry that the
// vote has written.  li must be below the total (tools/coal_floor_check.cpp walks every li of random, empty and one-sided length vectors).
constexpr int COAL_SUBLISTS = 64;
LCX_HD uint64_t coal_sublist_cap(const uint64_t n_cell, const uint64_t cells_per_wave)
{
  const uint64_t waves = (n_cell + cells_per_wave - 1) / cells_per_wave;
  return (waves + COAL_SUBLISTS - 1) / COAL_SUBLISTS * cells_per_wave;
}
struct coal_list_place { uint32_t sub, off; };
LCX_HD coal_list_place coal_list_place_of(const uint32_t *prefix, const uint32_t li)
{
  uint32_t lo = 0, hi = COAL_SUBLISTS;                                         // prefix[lo] <= li < prefix[hi] throughout
  while (hi - lo > 1) { const uint32_t mid = (lo + hi) / 2; if (prefix[mid] <= li) lo = mid; else hi = mid; }
  return coal_list_place{lo, li - prefix[lo]};
}

// Which tiles a kept cell must keep.  Tile k is the positions [k * tile, (k + 1) * tile) of the sorted order, one workgroup of k_coal_ranked
// (tile = COAL_RANKED_POS).  The pair that starts at position p is examined by the lane that looks at p (p even) or at p - 1 (p odd); `tile` is
// even, so p - 1 lies in p's tile, and every pair of the cell is examined in a tile that holds one of the cell's own positions: the tiles that
// [off, end) overlaps, [first, last].  (More than the pairs' own tiles where the cell's last droplet is unpaired: erring toward keeping.)
// An empty cell overlaps none: first > last.
struct coal_tile_range { uint64_t first, last; };
LCX_HD coal_tile_range coal_cell_tiles(const uint64_t off, const uint64_t end, const uint64_t tile)
{
  if (end <= off) return coal_tile_range{1, 0};
  return coal_tile_range{off / tile, (end - 1) / tile};
}

} // namespace lcx
