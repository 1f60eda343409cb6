/*
 * lcx_coal_rates.h -- companion of lcx.h: collision rates per cell.  What every collision event of the coalescence moves between cloud
 * water and rain water -- autoconversion, accretion, self-collection -- summed per cell inside the coalescence kernels.  A header of its
 * own because lcx.h is the surface that the CPU oracle mirrors entry for entry (tests/test_abi.py), and the reference keeps no such sums.
 * Off by default; an object that never enabled them, or disabled them, launches the kernels it launched before.
 *
 * Definitions.  A threshold wet radius r_thr separates cloud from rain: cloud is rw2 < lo, rain is rw2 >= lo, where lo is the lower bound
 * that lcx_diag_wet_rng(r_thr, ...) selects with (r_thr squared in double, rounded to the object's real type).  So "rain" is what
 * lcx_diag_wet_rng(r_thr, huge) selects, and budgets taken from lcx_diag_wet_rng moments close against these sums.
 *
 * An event is one pair of super-droplets with col_no > 0 collisions (after the cap n_big / n_small).  D, the donor, is the member with the
 * larger or equal multiplicity (on a tie the pair's first member); R, the receiver, is the other; m is R's multiplicity before the event.
 * col_no * m droplets of D vanish, and the m droplets of R become droplets of the radius that the kernel stores.  The product's class is
 * taken from that stored value.  rD, rR: the radii before the event.
 *
 *   D      R      product   accumulators
 *   cloud  cloud  cloud     SELF_CLOUD_N += col_no * m
 *   cloud  cloud  rain      ACNV_M3 += m * (col_no * rD^3 + rR^3),  ACNV_NC += (col_no + 1) * m,  ACNV_NR += m
 *   cloud  rain   rain      ACCR_M3 += col_no * m * rD^3,  ACCR_NC += col_no * m
 *   rain   cloud  rain      ACCR_M3 += m * rR^3,  ACCR_NC += m,  SELF_RAIN_N += (col_no - 1) * m
 *   rain   rain   rain      SELF_RAIN_N += col_no * m
 *
 * (A product is never smaller than a member: with a rain member it counts as rain.)  Per cell, with N and M3 = sum n r^3 of the two classes:
 *   change of N_cloud = -(SELF_CLOUD_N + ACNV_NC + ACCR_NC),   change of N_rain = ACNV_NR - SELF_RAIN_N   (exact),
 *   change of M3_rain = ACNV_M3 + ACCR_M3   (to the rounding of the stored radii).
 * Multiply an M3 by 4/3 pi rho_w for a mass.
 *
 * The five number accumulators are exact unsigned 64-bit integers: they do not depend on the order in which events arrive.  The two M3
 * accumulators are sums of n r^3 in m^3, kept in double whatever the object's real type, each term computed in double from the radii as
 * the object holds them; they are added with floating-point atomics, so their LAST BITS DEPEND ON THE ARRIVAL ORDER and may differ
 * between two runs of the same state: a cell's sum of K terms is within K * 2^-52 * sum |term| of the exact sum, not reproducible to
 * bits.  Nothing else of the object's state is touched: with the accumulators on, every attribute and every random number is what it is
 * with them off, bit for bit.
 *
 * Every coalescence launch of lcx_step_async (all sstp_coal substeps) and of the stage hooks is tallied: the generic kernel, the Onishi
 * kernel, the production kernel and the kernel that ranks each cell's order for itself, with its probability bound and its early exit
 * where it would have used them (they skip only pairs that cannot collide).  A pair without a collision adds nothing.
 *
 * Snapshots (lcx_state.h): the accumulators are not part of a snapshot and its format does not know them.  lcx_snapshot_save of an
 * enabled object works as before; an object restored by lcx_snapshot_load is disabled, whatever it was before the load.
 *
 * Errors (text through lcx_last_error, each "libcloudph++: coal_rates: ..."): r_thr <= 0 or not finite; a read or a diag call while the
 * accumulators are not enabled; `which` outside 0 .. LCX_CR_COUNT - 1; stride < n_cell; out == NULL; and an lcx_create_multi object:
 * "libcloudph++: coal_rates on a multi-device object is not built".  A single-device object with distmem neighbours tallies its own cells.
 */
#ifndef LCX_COAL_RATES_H
#define LCX_COAL_RATES_H

#include "lcx.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { LCX_CR_ACNV_M3, LCX_CR_ACNV_NC, LCX_CR_ACNV_NR, LCX_CR_ACCR_M3, LCX_CR_ACCR_NC, LCX_CR_SELF_CLOUD_N, LCX_CR_SELF_RAIN_N, LCX_CR_COUNT };

/* before or after lcx_init; allocates and zeroes the accumulators (an enabled object: sets the threshold anew and zeroes) */
int lcx_coal_rates_enable(lcx_particles *, double r_thr);
/* frees them; the object launches what it launched before */
int lcx_coal_rates_disable(lcx_particles *);
/* launches: coalescence launches tallied since enable or the last reset; any pointer may be NULL */
int lcx_coal_rates_info(lcx_particles *, int *enabled, double *r_thr, unsigned long long *launches);
/* out[w * stride + c], w < LCX_CR_COUNT, c the cell index of lcx_outbuf, stride >= n_cell; the numbers as doubles (exact below 2^53).  out
 * is a host pointer, or with out_on_device = 1 a pointer into the memory of the object's device.  Ordered on lcx_stream; the call waits
 * for the stream once, at the end, as lcx_diag_batch does.  reset != 0 zeroes the accumulators (and `launches`) behind the read. */
int lcx_coal_rates_read(lcx_particles *, double *out, size_t stride, int out_on_device, int reset);
/* fills lcx_outbuf with accumulator `which` as a diag_*_mom call would: in the object's real type, divided by the cell's volume and dry
 * density (a 0-D parcel is not divided, as there) */
int lcx_diag_coal_rate(lcx_particles *, int which);

#ifdef __cplusplus
}
#endif
#endif
