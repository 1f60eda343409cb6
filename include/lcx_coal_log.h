/*
 * lcx_coal_log.h -- companion of lcx.h: the collision log.  Every coalescence event of a run -- who collided with whom -- appended to one
 * list in the memory of the object's device by the coalescence kernels themselves, from the values they hold in registers at the event.
 * What the seven sums per cell of lcx_coal_rates.h are one reduction of: size-resolved collection rates, the kernel a run sampled, the
 * partners of a lucky droplet, the dry radii of both members.  A header of its own because lcx.h is the surface that the CPU oracle
 * mirrors entry for entry (tests/test_abi.py), and the reference keeps no such list.  Off by default; an object that never enabled it, or
 * disabled it, allocates and launches exactly what it did before.
 *
 * Definitions, exactly those of lcx_coal_rates.h.  An event is one pair of super-droplets with col_no > 0 collisions (after the cap
 * n_big / n_small) whose receiver has a multiplicity m > 0.  D, the donor, is the member with the larger or equal multiplicity (on a tie
 * the pair's first member); R, the receiver, is the other.  col_no * m droplets of D vanish, and the m droplets of R become droplets of
 * the radius that the kernel stores.
 *
 * Which events are logged.  All of them with r_min == 0; else those whose product's STORED rw2 is >= lo, where lo is the lower bound that
 * lcx_diag_wet_rng(r_min, ...) selects with (r_min squared in double, rounded to the object's real type): the events that made or grew
 * a droplet of at least r_min.
 *
 * Counters.  seen: logged events since enable or the last resetting read, those that found no room included.  held = min(seen, capacity):
 * the events in the list; an event beyond the capacity is dropped and written nowhere.  launches: coalescence launches since enable (all
 * sstp_coal substeps of lcx_step_async, and the stage hooks); a read never resets it.
 *
 * The list.  [LCX_CLG_FIELDS][capacity] words of 8 bytes, field-major.  The order of the events is unspecified and may differ between two
 * runs of the same state (it is the order in which waves arrive); the set is the same.  Within one launch a storage slot is a member of at
 * most one pair, so (LAUNCH, SLOT_R) is a key.  What each field holds -- every one a value the kernel had in a register at the event,
 * converted to double by the read (integers are exact below 2^53); nothing is recomputed:
 *   LAUNCH          the launch's index since enable, from 0
 *   CELL            the pair's cell (the index of lcx_outbuf; 0 in a 0-D parcel)
 *   SLOT_D, SLOT_R  the members' storage slots: the index into the raw_ state, what the particle dump's LCX_DMP_SLOT shows.  A slot names the
 *                   droplet until the storage is re-ordered (at the end of lcx_step_async at the earliest): a dump taken between
 *                   lcx_step_sync and lcx_step_async joins to that step's events by slot, with n and rw2 equal to N_*, RW2_* in the
 *                   events of the step's first coalescence launch.
 *   COL_NO          the collision count after the cap
 *   N_D, N_R        the multiplicities before the event (after it: N_D - COL_NO * N_R and N_R)
 *   RW2_D, RW2_R    the wet radii squared before the event
 *   RW2_NEW         the value stored for R
 *   RD3_D, RD3_R    the dry radii cubed before the event (after it R holds COL_NO * RD3_D + RD3_R in the object's real type)
 *   VT_D, VT_R      the terminal velocities as the pair read them
 *
 * What does not change: with the log on, every attribute, th, rv, every random number, every lcx_mode and raw_ counter and the launches
 * of a step are what they are with it off, bit for bit; so are the collision rates of lcx_coal_rates.h, on at the same time or not.
 * lcx_step_async gains no host wait: the kernels append with one atomic per wave and call site, and nobody reads the cursor until
 * lcx_coal_log_info or lcx_coal_log_read, which wait for the stream once each.
 *
 * Snapshots (lcx_state.h): the log is not part of a snapshot.  lcx_snapshot_save of an enabled object works as before; an object
 * restored by lcx_snapshot_load has the log disabled, whatever it was before the load.
 *
 * Errors (text through lcx_last_error, each "libcloudph++: coal_log: ..."; a failed call leaves the object as it was): capacity == 0, or
 * a capacity whose list has more bytes than size_t holds; r_min negative or not finite; a read while the log is not enabled;
 * out == NULL; field_stride < cap_events; cap_events < held; a device allocation that fails (the text names the bytes asked for).  And one
 * without the colon: an lcx_create_multi object, "libcloudph++: coal_log on a multi-device object is not built".  A single-device object
 * that is a slab with neighbours logs its own cells' events, with its own slots.
 */
#ifndef LCX_COAL_LOG_H
#define LCX_COAL_LOG_H

#include "lcx.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { LCX_CLG_LAUNCH, LCX_CLG_CELL, LCX_CLG_SLOT_D, LCX_CLG_SLOT_R, LCX_CLG_COL_NO, LCX_CLG_N_D, LCX_CLG_N_R,      /* integers */
       LCX_CLG_RW2_D, LCX_CLG_RW2_R, LCX_CLG_RW2_NEW, LCX_CLG_RD3_D, LCX_CLG_RD3_R, LCX_CLG_VT_D, LCX_CLG_VT_R,     /* of the real type */
       LCX_CLG_FIELDS };

/* validation of capacity and r_min only: no handle, no device */
int lcx_coal_log_check(size_t capacity, double r_min);
/* before or after lcx_init; allocates the list and its cursor and clears them (an enabled object: re-allocates, sets r_min anew, clears
 * the list, seen and launches) */
int lcx_coal_log_enable(lcx_particles *, size_t capacity, double r_min);
/* frees both; the object launches what it launched before.  No error if the log is not enabled */
int lcx_coal_log_disable(lcx_particles *);
/* any pointer may be NULL; a disabled log: all zero.  Waits for the stream once when held or seen is asked for of an enabled log */
int lcx_coal_log_info(lcx_particles *, int *enabled, size_t *capacity, double *r_min, unsigned long long *held, unsigned long long *seen,
                      unsigned long long *launches);
/* out[f * field_stride + i], f < LCX_CLG_FIELDS, i < held: field f of the i-th held event; cap_events >= held is the room of a row,
 * field_stride >= cap_events; elements at and beyond held, and between the rows, are not written.  out is a host pointer, or with
 * out_on_device = 1 a pointer into the memory of the object's device, which the kernel then writes directly (a host read copies
 * min(cap_events, capacity) elements of every row: ask lcx_coal_log_info for held first).  *n_written = held, *seen as of the read; either
 * may be NULL.  Ordered on lcx_stream; the call waits for the stream once, at the end.  reset != 0 clears held and seen behind the read,
 * on the stream; a read that fails resets nothing. */
int lcx_coal_log_read(lcx_particles *, double *out, size_t field_stride, size_t cap_events, int out_on_device, int reset,
                      size_t *n_written, unsigned long long *seen);

#ifdef __cplusplus
}
#endif
#endif
