/*
 * lcx_track.h -- companion of lcx.h: tracked super-droplets.  A caller marks a set of droplets once and then takes samples of them: for
 * every tracked droplet twelve doubles -- multiplicity, position, wet and dry size, kappa, terminal velocity, cell, and the cell's T, RH
 * and rv -- into a buffer on the device that is read out whenever the caller likes.  A droplet's history from step to step, which the
 * per-cell sums of lcx_diag.h and the three rates cannot give, at the cost of a gather of the tracked droplets only.  A header of its own
 * because lcx.h is the surface that the CPU oracle mirrors entry for entry (tests/test_abi.py), and the reference has nothing like it.
 * Off by default; an object that never enabled it, or disabled it, allocates and launches exactly what it did before.
 * WHY a tracked droplet changed between two samples -- condensation, collection, chemistry, how many collisions -- is lcx_track_budget.h.
 *
 * The mark.  lcx_track_enable appends ONE attribute column, "track", to both storage sets, zeroed: of the object's real type, it holds
 * k + 1 for the droplet with track index k and 0 for every other droplet (k + 1 <= LCX_TRK_MAX = 2^20 is exact in float).  It travels
 * with its droplet through everything that copies a droplet's attributes: compaction, re-ordering of the storage, the swap of the two
 * sets.  lcx_get_state_real("raw_track") shows it per storage slot (0 elements while not enabled).  Beside it: slot_of[max_tracked]
 * (32-bit), the storage slot of every index, and the sample buffer of capacity x LCX_TRK_FIELDS x max_tracked doubles with steps[capacity]
 * and time[capacity].  Before or after lcx_init; on an enabled object the call starts over (marks zeroed, buffer empty, counters 0, the
 * new sizes).  1 <= max_tracked <= LCX_TRK_MAX, capacity >= 1, every >= 0.  lcx_track_disable drops the column (the last one: nothing
 * else adds columns after construction) and every buffer.
 *
 * Who keeps a mark.  Coalescence never touches marks: both members of a pair keep theirs, also when equal multiplicities are split.  Every
 * NEW droplet has mark 0: what a source or relaxation appends, the RECEIVER of a recycling (opts.rcyc; the donor keeps its mark), and
 * every droplet of lcx_set_particles (which so empties the tracked set's slots, not its indices).  A track index is never reused: a
 * droplet that dies leaves its index absent for good.
 *
 * Selection (after lcx_init).  A droplet qualifies when its storage slot in [0, n_storage) has n > 0, its mark is 0, it satisfies every
 * clause -- ANDed, with the bounds of lcx_diag_*_rng: the square (wet) or cube (dry) of the radii in double, rounded to the object's real
 * type, lo <= v < hi; LCX_DIAG_SEL_ALL and LCX_DIAG_SEL_WATER as in lcx_diag.h -- and, if box != NULL, its stored position, converted to
 * double, lies in [box[0], box[1]) x [box[2], box[3]) x [box[4], box[5]) (x, y, z; the pair of a dimension the object lacks is not read).
 * Q: the number of qualifying droplets, ranked q = 0 .. Q - 1 in storage order; room = min(max_count, max_tracked - n_tracked).
 * room == 0 or Q == 0: nothing is selected.  Otherwise stride = ceil(Q / room), the droplets with q % stride == 0 get the indices
 * n_tracked, n_tracked + 1, ... in storage order, and *n_selected = ceil(Q / stride).  Deterministic, exact in integers, spread over the
 * whole storage and reproducible from the raw state (lcx_get_state_*("raw_...")).  The call waits for the stream: it returns a count.
 * lcx_track_select_slots marks the given storage slots (indices into the raw_ state) in the order given, skipping slots that are out of
 * range, dead (n == 0) or already marked (a slot given twice included), and stops when max_tracked is reached.
 *
 * A sample writes, for every k < n_tracked, buf[s][f][k].  Alive (a slot carries mark k + 1 and its n > 0):
 *   N                      the multiplicity (exact below 2^53)
 *   X, Y, Z                the stored positions; 0 for a dimension the object lacks
 *   RW2, RD3, KAPPA, VT    what lcx_get_state_real("raw_rw2" / "raw_rd3" / "raw_kappa" / "raw_vt") shows for the slot at that moment: the
 *                          stored value converted to double, vt with its invalid flag as stored, kappa as the column holds it
 *   CELL                   the slot's raw_ijk
 *   T, RH, RV              the cell arrays "T", "RH", "rv" at that cell as they stand (nothing is recomputed; NaN if CELL is no cell)
 * Otherwise (dead, compacted away, or selected after the sample was taken) N = 0 and the other eleven are NaN.
 * steps[s]: the lcx_step_async calls completed since enable; time[s]: the sum of their time steps (a per-call opts.dt under
 * variable_dt_switch counts with its own value).  lcx_track_sample takes one sample now, any time after lcx_init.  With every > 0 the
 * object also takes one as the LAST thing of every every-th lcx_step_async since enable, queued on the object's stream with no host wait
 * (also under stream_ordered).  A sample that finds the buffer full is not taken and adds 1 to `dropped`.  With n_tracked == 0 a sample
 * is taken and holds nothing.
 *
 * Cost of a sample.  The storage slot of every index is kept (slot_of) and found again -- one pass over the mark column, counted in
 * `scans` -- only behind what permutes or rewrites storage: enable, compaction, re-ordering, recycling, lcx_set_particles.  The move,
 * coalescence, condensation and appends leave it valid: between two permutations a sample is one launch that reads O(n_tracked) bytes.
 *
 * Reading.  lcx_track_read writes out[s * sample_stride + f * field_stride + k] for s < *n_samples, f < LCX_TRK_FIELDS, k < n_tracked,
 * n_tracked as of the read (a droplet selected after a sample is absent in it); field_stride >= n_tracked, sample_stride >=
 * LCX_TRK_FIELDS * field_stride, cap_samples >= the samples held; elements in between are not written.  out is a host pointer, or with
 * out_on_device = 1 a pointer into the memory of the object's device; steps and time are host arrays of cap_samples and either may be
 * NULL.  One stream wait, at the end.  reset != 0 empties the buffer and zeroes `dropped`; the tracked set stays.
 *
 * Nothing else changes.  With tracking enabled every attribute, th, rv, the puddle, the sorted order, every random number and the kernel
 * that each step chooses (lcx_mode) are what they are without it, bit for bit; an enabled object stays on the production coalescence path.
 *
 * Snapshots (lcx_state.h): the column is NOT written and the format does not know it -- the snapshot of a tracking object is the snapshot
 * of the same run without tracking, byte for byte (the two sections that keep what atomics left, `rank` and `big_list`, are copied in one
 * form, made on the device beside the object's own arrays, so that a snapshot is reproducible from run to run).  An object restored by lcx_snapshot_load is disabled, whatever it was before
 * the load.
 *
 * Errors (text through lcx_last_error; a failed call leaves the object as it was).  Each "libcloudph++: track: ...":
 *   max_tracked outside 1 .. LCX_TRK_MAX; capacity == 0; every < 0; no free attribute column (all MAX_EXT in use);
 *   select, select_slots, sample, read or disable while not enabled; select, select_slots or sample before init();
 *   n_clauses outside 1 .. LCX_DIAG_MAX_CLAUSES; clause == NULL; an unknown sel; a box bound that is not finite; a box with lo > hi;
 *   max_count == 0; slot == NULL with n > 0; field_stride < n_tracked; sample_stride < LCX_TRK_FIELDS * field_stride;
 *   cap_samples < the samples held; out == NULL with samples to write.
 * And two without the colon: an lcx_create_multi object, "libcloudph++: track on a multi-device object is not built"; a single-device
 * object that is a slab with neighbours, "libcloudph++: track on a decomposed domain is not built" -- the migration record would grow.
 */
#ifndef LCX_TRACK_H
#define LCX_TRACK_H

#include "lcx.h"
#include "lcx_diag.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { LCX_TRK_N, LCX_TRK_X, LCX_TRK_Y, LCX_TRK_Z, LCX_TRK_RW2, LCX_TRK_RD3, LCX_TRK_KAPPA, LCX_TRK_VT,
       LCX_TRK_CELL, LCX_TRK_T, LCX_TRK_RH, LCX_TRK_RV, LCX_TRK_FIELDS };
enum { LCX_TRK_MAX = 1 << 20 };   /* track indices + 1 are exact in float */

/* validation of a selection's arguments only: no handle, no device (all three pairs of a box are read) */
int lcx_track_check(const lcx_diag_clause_t *clause, int n_clauses, const double *box, size_t max_count);
int lcx_track_enable(lcx_particles *, size_t max_tracked, size_t capacity, int every);
int lcx_track_disable(lcx_particles *);
int lcx_track_select(lcx_particles *, const lcx_diag_clause_t *clause, int n_clauses, const double *box /* 6 or NULL */,
                     size_t max_count, size_t *n_selected);
int lcx_track_select_slots(lcx_particles *, const unsigned long long *slot, size_t n, size_t *n_selected);
int lcx_track_sample(lcx_particles *);
/* any pointer may be NULL; not enabled: enabled = 0 and every other value 0 */
int lcx_track_info(lcx_particles *, int *enabled, size_t *max_tracked, size_t *n_tracked, size_t *capacity, size_t *n_samples,
                   unsigned long long *dropped, int *every, unsigned long long *scans);
int lcx_track_read(lcx_particles *, double *out, size_t sample_stride, size_t field_stride,
                   unsigned long long *steps, double *time, size_t cap_samples, size_t *n_samples,
                   int out_on_device, int reset);

#ifdef __cplusplus
}
#endif
#endif
