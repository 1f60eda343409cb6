/*
 * lcx_cond_rates.h -- companion of lcx.h: condensation rates per cell.  What one lcx_step_cond does to the wet spectrum relative to a short
 * list of threshold radii -- growth and evaporation above a threshold, droplets and water crossing it either way -- summed per cell by a
 * pass of its own around the condensation (a copy of rw2 ahead of it, one tally kernel behind it); no condensation kernel knows of it.  A
 * header of its own because lcx.h is the surface that the CPU oracle mirrors entry for entry (tests/test_abi.py), and the reference keeps
 * no such sums.  Off by default; an object that never enabled them, or disabled them, allocates nothing and launches what it launched before.
 *
 * Thresholds.  K wet radii r_1 < ... < r_K, 1 <= K <= LCX_CDR_MAX_THR.  Each has lo_t = T(r_t^2), taken exactly as lcx_diag_wet_rng(r_t, ...)
 * takes its lower bound: the square in double, then rounded to the object's real type T.  "Above t" is rw2 >= lo_t, which is what
 * lcx_diag_wet_rng(r_t, huge) selects, so budgets taken from lcx_diag_wet_rng moments close against these sums.
 *
 * Per droplet.  n: the multiplicity.  rw2_0: rw2 as stored when lcx_step_cond begins its condensation; rw2_1: rw2 as stored after the last
 * substep (every substep of the call is covered, per-cell and per-particle).  A radius cubed is r^3 = x * sqrt(x) with x = double(rw2);
 * every term is computed in double whatever the real type.
 *
 * Per cell and threshold t, LCX_CDR_PER_THR = 5 rows:
 *
 *   droplet, before -> after    rows
 *   above -> above              ABOVE_DM3_t += n (r1^3 - r0^3)    (signed)
 *   below -> above              UP_N_t += n,    UP_M3_t += n r1^3
 *   above -> below              DOWN_N_t += n,  DOWN_M3_t += n r0^3
 *   below -> below              nothing
 *
 * and one more row per cell, TOTAL_DM3 += n (r1^3 - r0^3) over all droplets.  5 K + 1 rows: the index of a threshold's row is
 * 5 t + which (t from 0), the last row, 5 K, is TOTAL_DM3.
 *
 * Budgets, per cell, with N and M3 = sum n r^3 of "above t":
 *   change of N(>= t)  = UP_N_t - DOWN_N_t   (exact),
 *   change of M3(>= t) = ABOVE_DM3_t + UP_M3_t - DOWN_M3_t,
 *   M3(< t) changes by TOTAL_DM3 minus the change of M3(>= t);  a band [r_s, r_t) is the difference of two thresholds;
 *   -4/3 pi rho_w TOTAL_DM3 / (dv rhod) is the cell's change of rv by condensation.
 * With lcx_coal_rates.h at the same threshold the number of rain droplets of a cell changes over a step of condensation and coalescence
 * by UP_N - DOWN_N + ACNV_NR - SELF_RAIN_N, exactly.
 *
 * What is tallied.  The net of the call: a droplet that crosses up and down again within one call's substeps counts nothing.  A dead
 * slot (n == 0) adds nothing.  An lcx_step_cond with opts.cond == 0 tallies nothing and is not counted in `calls`.  Coalescence, sources,
 * relaxation, recycling and lcx_init change radii too and are not tallied here.
 *
 * Number types.  UP_N and DOWN_N are exact unsigned 64-bit integers: they do not depend on the order in which droplets arrive.  The M3
 * rows are sums in m^3, kept in double whatever the object's real type; runs of one cell's droplets are summed inside a wave in a fixed
 * order and the runs' sums are added with floating-point atomics, so their LAST BITS DEPEND ON THE ARRIVAL ORDER and may differ
 * between two runs of the same state: a cell's sum of K terms is within K * 2^-52 * sum |term| of the exact sum, not reproducible to
 * bits.  Nothing else of the object's state is touched: with the tally on, every attribute, th, rv, the sorted order and every random
 * number is what it is with it off, bit for bit.
 *
 * Snapshots (lcx_state.h): the tally is not part of a snapshot and its format does not know it.  lcx_snapshot_save of an enabled object
 * works as before; an object restored by lcx_snapshot_load is disabled, whatever it was before the load.
 *
 * Errors (text through lcx_last_error, each "libcloudph++: cond_rates: ..."): n_thr outside 1 .. LCX_CDR_MAX_THR; a threshold not positive
 * or not finite, or the thresholds not strictly increasing; the rounded bounds lo_t not strictly increasing in the object's real type
 * (possible in float); a read or a diag call while not enabled; `row` out of range; stride < n_cell; out == NULL; lcx_diag_cond_rate
 * before lcx_init; and an lcx_create_multi object: "libcloudph++: cond_rates on a multi-device object is not built".  A single-device
 * object with distmem neighbours tallies its own cells.
 */
#ifndef LCX_COND_RATES_H
#define LCX_COND_RATES_H

#include "lcx.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { LCX_CDR_ABOVE_DM3, LCX_CDR_UP_N, LCX_CDR_UP_M3, LCX_CDR_DOWN_N, LCX_CDR_DOWN_M3, LCX_CDR_PER_THR };
enum { LCX_CDR_MAX_THR = 4 };

/* before or after lcx_init; r_thr[n_thr] strictly increasing; zeroes the rows (an enabled object: new thresholds, zeroed) */
int lcx_cond_rates_enable(lcx_particles *, const double *r_thr, int n_thr);
/* frees the rows and the scratch column; the object launches what it launched before */
int lcx_cond_rates_disable(lcx_particles *);
/* r_thr: room for LCX_CDR_MAX_THR values, the first n_thr are written; calls: lcx_step_cond calls tallied since enable or the last reset;
 * any pointer may be NULL */
int lcx_cond_rates_info(lcx_particles *, int *enabled, int *n_thr, double *r_thr, unsigned long long *calls);
/* out[row * stride + c], row < 5 n_thr + 1, c the cell index of lcx_outbuf, stride >= n_cell; the numbers as doubles (exact below 2^53).
 * out is a host pointer, or with out_on_device = 1 a pointer into the memory of the object's device.  Ordered on lcx_stream; the call
 * waits for the stream once, at the end, as lcx_diag_batch does.  reset != 0 zeroes the rows (and `calls`) behind the read. */
int lcx_cond_rates_read(lcx_particles *, double *out, size_t stride, int out_on_device, int reset);
/* fills lcx_outbuf with row `row` as a diag_*_mom call would: in the object's real type, divided by the cell's volume and dry density
 * (a 0-D parcel is not divided, as there) */
int lcx_diag_cond_rate(lcx_particles *, int row);

#ifdef __cplusplus
}
#endif
#endif
