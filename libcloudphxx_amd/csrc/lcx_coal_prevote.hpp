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
