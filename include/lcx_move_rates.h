/*
 * lcx_move_rates.h -- companion of lcx.h: transport rates per cell.  What the one move of an lcx_step_async -- advection, sedimentation,
 * subsidence, the SGS velocities and the boundary conditions -- carries into and out of every cell, up and down through its levels and
 * onto the ground, relative to a short list of threshold radii, summed per cell by a pass of its own around the move (a copy of ijk and n
 * ahead of it, one tally kernel behind it); no instantiation of the move kernel knows of it.  The third member of the family of
 * lcx_coal_rates.h and lcx_cond_rates.h: with all three at one radius a cell's number of rain drops closes in integers over a full step.
 * A header of its own because lcx.h is the surface that the CPU oracle mirrors entry for entry (tests/test_abi.py), and the reference
 * keeps no such sums.  Off by default; an object that never enabled them, or disabled them, allocates nothing and launches what it
 * launched before.
 *
 * Thresholds.  K wet radii 0 <= r_1 < ... < r_K, finite, 1 <= K <= LCX_MVR_MAX_THR.  Each has lo_t = T(r_t^2), taken exactly as
 * lcx_diag_wet_rng(r_t, ...) takes its lower bound: the square in double, then rounded to the object's real type T.  "Above t" is
 * rw2 >= lo_t with rw2 as stored at the move, which does not change it.  r_1 = 0 is allowed and means every droplet.
 *
 * Per droplet (a storage slot of [0, nphys) ahead of the move).  m: its multiplicity ahead of the move; c0: its cell as stored ahead of
 * the move.  A slot with m == 0 or a dead cell adds nothing -- droplets that coalescence has just used up included.  Behind the move the
 * droplet is either REMOVED (the move set n = 0) or alive in cell c1: the cell that the step itself stores for it, not a recomputation
 * that could round differently.  k0, k1: the vertical indices of c0 and c1; an object without a z dimension has none and its vertical
 * rows stay zero.  A radius cubed is r^3 = x * sqrt(x) with x = double(rw2); every term is computed in double whatever the real type.
 *
 * Per cell and threshold t, LCX_MVR_PER_THR = 10 rows; the index of a row is 10 t + which (t from 0).  A droplet above t adds m to the
 * _N rows and m r^3 to the _M3 rows named here:
 *
 *   droplet                               rows
 *   alive, c1 == c0                       nothing
 *   alive, c1 != c0                       OUT at c0, IN at c1;  DOWN at c0 if k1 < k0;  UP at c0 if k1 > k0
 *   removed through the bottom            OUT and DOWN at c0;  PRECIP at the lowest cell (k = 0) of c0's column
 *     (stored z < z0, and no side wall or top had removed it first)
 *   removed through the top (z >= z1)     OUT and UP at c0
 *   removed by an open side wall          OUT at c0
 *
 * The removal rules come in the order of the move: side walls, then top, then bottom.  PRECIP is exactly what the puddle receives.
 * A periodic side wall makes the arrival appear in the cell on the other side.  With periodic_topbot_walls nothing is removed at the
 * top or the bottom and the vertical rows compare the stored indices, so a wrap reads as the opposite direction (a droplet that falls
 * through the bottom into the top level counts UP).
 *
 * Budgets, per cell, with N and M3 = sum m r^3 of "above t":
 *   over the move, change of N(>= t) = IN_N_t - OUT_N_t (exact), change of M3(>= t) = IN_M3_t - OUT_M3_t;
 *   over the domain, sum IN_N_t = sum OUT_N_t - (removed above t);
 *   with r_1 = 0, sum_c PRECIP_N_0 is the increase of diag_puddle's outprtcl_num and 4/3 pi sum_c PRECIP_M3_0 that of outliq_vol;
 *   with lcx_cond_rates.h and lcx_coal_rates.h at the same radius, the number of rain drops of a cell changes over
 *   lcx_step_sync + lcx_step_async by UP_N - DOWN_N + ACNV_NR - SELF_RAIN_N + IN_N - OUT_N, exactly (UP_N, DOWN_N: lcx_cond_rates.h).
 *
 * What is tallied.  The one move of every lcx_step_async, whichever kernel runs it (euler, implicit, pred_corr, turb_adve, subsidence,
 * open walls), and both ways the step can end: the fused move with re-indexing, and the plain sequence (opts.rcyc, a matching source, a
 * source or relaxation short of room).  `calls` counts the moves tallied since enable or the last reset.  Not tallied: single stages
 * through lcx_stage; the super-droplets that a source, relaxation or recycling creates or rewrites -- they are not arrivals.  A 0-D
 * object may enable; its rows stay zero.
 *
 * Number types.  The _N rows are exact unsigned 64-bit integers: they do not depend on the order in which droplets arrive.  The _M3
 * rows are sums in m^3, kept in double whatever the object's real type; lanes of a wave with one target are summed in a fixed order and
 * the sums are added with floating-point atomics, so their LAST BITS DEPEND ON THE ARRIVAL ORDER and may differ between two runs of
 * the same state: a cell's sum of K_c terms is within (K_c + 8) * 2^-52 * sum |term| of the exact sum.  Nothing else of the object's
 * state is touched: with the tally on, every attribute, th, rv, the puddle, the sorted order and every random number is what it is
 * with it off, bit for bit.
 *
 * Snapshots (lcx_state.h): the tally is not part of a snapshot and its format does not know it.  lcx_snapshot_save of an enabled object
 * works as before; an object restored by lcx_snapshot_load is disabled, whatever it was before the load.
 *
 * Errors (text through lcx_last_error, each "libcloudph++: move_rates: ..."): n_thr outside 1 .. LCX_MVR_MAX_THR; a threshold negative
 * or not finite, or the thresholds not strictly increasing; the rounded bounds lo_t not strictly increasing in the object's real type
 * (possible in float); a read or a diag call while not enabled; `row` out of range; stride < n_cell; out == NULL; lcx_diag_move_rate
 * before lcx_init; an lcx_create_multi object: "libcloudph++: move_rates on a multi-device object is not built"; and a single-device
 * object that is a slab with neighbours: "libcloudph++: move_rates on a decomposed domain is not built" -- emigrants and immigrants
 * would break every budget above.
 */
#ifndef LCX_MOVE_RATES_H
#define LCX_MOVE_RATES_H

#include "lcx.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { LCX_MVR_IN_N, LCX_MVR_IN_M3, LCX_MVR_OUT_N, LCX_MVR_OUT_M3, LCX_MVR_DOWN_N, LCX_MVR_DOWN_M3, LCX_MVR_UP_N, LCX_MVR_UP_M3,
       LCX_MVR_PRECIP_N, LCX_MVR_PRECIP_M3, LCX_MVR_PER_THR };
enum { LCX_MVR_MAX_THR = 4 };

/* before or after lcx_init; r_thr[n_thr] strictly increasing, the first may be 0; zeroes the rows (an enabled object: new thresholds, zeroed) */
int lcx_move_rates_enable(lcx_particles *, const double *r_thr, int n_thr);
/* frees the rows and the scratch columns; the object launches what it launched before */
int lcx_move_rates_disable(lcx_particles *);
/* r_thr: room for LCX_MVR_MAX_THR values, the first n_thr are written; calls: the moves tallied since enable or the last reset;
 * any pointer may be NULL */
int lcx_move_rates_info(lcx_particles *, int *enabled, int *n_thr, double *r_thr, unsigned long long *calls);
/* out[row * stride + c], row < 10 n_thr, c the cell index of lcx_outbuf, stride >= n_cell; the numbers as doubles (exact below 2^53).
 * out is a host pointer, or with out_on_device = 1 a pointer into the memory of the object's device.  Ordered on lcx_stream; the call
 * waits for the stream once, at the end, as lcx_diag_batch does.  reset != 0 zeroes the rows (and `calls`) behind the read. */
int lcx_move_rates_read(lcx_particles *, double *out, size_t stride, int out_on_device, int reset);
/* fills lcx_outbuf with row `row` as a diag_*_mom call would: in the object's real type, divided by the cell's volume and dry density
 * (a 0-D parcel is not divided, as there) */
int lcx_diag_move_rate(lcx_particles *, int row);

#ifdef __cplusplus
}
#endif
#endif
