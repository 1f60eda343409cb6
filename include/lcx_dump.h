/*
 * lcx_dump.h -- companion of lcx.h: the particle dump.  One read-only call that writes chosen fields of every qualifying super-droplet,
 * in storage order and converted to double, densely into an array of the caller's -- on the host or on the object's device.  What the
 * per-cell sums of lcx_diag.h cannot give and lcx_get_attr gives only a whole column at a time, behind a compaction: the droplets
 * themselves, filtered and gathered on the device in one selection pass and one gather pass; the host waits for the count between the two
 * (4 bytes read back) and for the gather at the end.  A header of its own because lcx.h is the surface that the CPU oracle mirrors entry
 * for entry (tests/test_abi.py), and the reference has nothing like it.  An object that never calls it allocates and launches exactly what
 * it did before.
 *
 * Which droplets qualify.  A storage slot in [0, n_storage) qualifies when its n > 0, it satisfies every clause and it lies in the box:
 * clauses and box exactly as lcx_track_select (lcx_track.h) defines them -- ANDed clauses with the bounds of lcx_diag_*_rng, the square
 * (wet) or cube (dry) of the radii in double, rounded on the host to the object's real type, lo <= v < hi; LCX_DIAG_SEL_ALL and
 * LCX_DIAG_SEL_WATER as in lcx_diag.h; if box != NULL the stored position, converted to double, in [box[0], box[1]) x [box[2], box[3]) x
 * [box[4], box[5]) (the pair of a dimension the object lacks is not read).  The droplet's mark plays no part: tracked droplets qualify.
 * Q: the number of qualifying slots, ranked q = 0 .. Q - 1 in storage order.
 *
 * How many are written.  out == NULL: the call only counts, *n_qualifying = Q, *n_written = 0, *stride = 0.  Otherwise stride =
 * ceil(Q / max_count) (1 when everything fits; 0 when Q == 0), the droplets with q % stride == 0 are written at index q / stride, and
 * *n_written = ceil(Q / stride) <= max_count: the rule of a selection in lcx_track.h with room = max_count, applied by the same
 * functions on the host and on the device.  Spread over the whole storage, exact in integers and reproducible from the raw state.
 *
 * Where the values go.  out[f * field_stride + i] holds field field[f] of the i-th written droplet; field_stride >= max_count; elements
 * at and beyond n_written, and between the rows, are not written.  A field may be given once.  out is a host pointer, or with
 * out_on_device = 1 a pointer into the memory of the object's device.  Any of n_qualifying, n_written and stride may be NULL.
 *
 * What each field holds (every one a stored value converted to double; nothing is recomputed):
 *   N .. RV                the twelve of LCX_TRK_*, in their order and with their definitions for an alive droplet: the multiplicity,
 *                          the stored positions (0 for a dimension the object lacks), rw2, rd3, kappa and vt (with its invalid flag) as
 *                          lcx_get_state_real("raw_...") shows them, the slot's raw_ijk, and the cell arrays "T", "RH", "rv" at that
 *                          cell as they stand (NaN if CELL is no cell)
 *   SLOT                   the storage slot: the index into the raw_ state (ascending in the output)
 *   TRACK                  the mark column of lcx_track.h as stored (k + 1, or 0); 0 while tracking is not enabled
 *   INCLOUD_TIME           the column of opts_init.diag_incloud_time as stored
 *   CHEM_HNO3 .. CHEM_H    the eight chemical masses, in common::chem order, as stored (opts_init.chem_switch)
 *
 * What does not change: anything.  The call allocates no attribute column, neither compacts nor sorts nor finishes a sort that a step
 * left owed, advances no random stream and changes no lcx_mode: every attribute, th, rv, the puddle, the order, a snapshot and the
 * launches of the steps around it are what they are without it, bit for bit.  Legal any time after lcx_init, also between
 * lcx_step_sync and lcx_step_async, and under stream_ordered (it waits for the stream all the same: it returns counts).  Scratch: one bit
 * per storage slot and one word per 2048 slots, kept by the object; with host output a staging buffer of n_fields * n_written doubles
 * that lives for the call.  With out_on_device the kernel writes the caller's memory and nothing else is allocated.
 *
 * lcx_dump_check validates clauses, box and fields without an object: no handle, no device (all three pairs of a box are read; the
 * options that the optional fields need are taken as given).
 *
 * Errors (text through lcx_last_error; a failed call leaves the object as it was).  Each "libcloudph++: dump: ...":
 *   before init(); n_clauses outside 1 .. LCX_DIAG_MAX_CLAUSES; clause == NULL; an unknown sel; a box bound that is not finite; a box
 *   with lo > hi; n_fields outside 1 .. LCX_DMP_FIELDS; field == NULL; an unknown field; a field given twice; a chemistry field without
 *   chem_switch; INCLOUD_TIME without diag_incloud_time; out != NULL with max_count == 0; field_stride < max_count.
 * And one without the colon: an lcx_create_multi object, "libcloudph++: dump on a multi-device object is not built".  A single-device
 * object that is a slab with neighbours is allowed: the call only reads.
 */
#ifndef LCX_DUMP_H
#define LCX_DUMP_H

#include "lcx.h"
#include "lcx_diag.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { LCX_DMP_N, LCX_DMP_X, LCX_DMP_Y, LCX_DMP_Z, LCX_DMP_RW2, LCX_DMP_RD3, LCX_DMP_KAPPA, LCX_DMP_VT, LCX_DMP_CELL,
       LCX_DMP_T, LCX_DMP_RH, LCX_DMP_RV,            /* the twelve of LCX_TRK_*, same order, same definitions */
       LCX_DMP_SLOT,                                  /* the storage slot (index into the raw_ state) */
       LCX_DMP_TRACK,                                 /* the mark column as stored (k + 1, or 0); tracking not enabled: 0 */
       LCX_DMP_INCLOUD_TIME,                          /* needs opts_init.diag_incloud_time */
       LCX_DMP_CHEM_HNO3, LCX_DMP_CHEM_NH3, LCX_DMP_CHEM_CO2, LCX_DMP_CHEM_SO2, LCX_DMP_CHEM_H2O2, LCX_DMP_CHEM_O3,
       LCX_DMP_CHEM_S_VI, LCX_DMP_CHEM_H,             /* eight, common::chem order; need chem_switch */
       LCX_DMP_FIELDS };

/* validation of clauses, box and fields only: no handle, no device */
int lcx_dump_check(const lcx_diag_clause_t *clause, int n_clauses, const double *box, const int *field, int n_fields);
int lcx_dump(lcx_particles *, const lcx_diag_clause_t *clause, int n_clauses, const double *box /* 6 or NULL */,
             const int *field, int n_fields, double *out, size_t field_stride, size_t max_count, int out_on_device,
             size_t *n_qualifying, size_t *n_written, unsigned long long *stride);

#ifdef __cplusplus
}
#endif
#endif
