/*
 * lcx_track_budget.h -- companion of lcx_track.h: for every tracked super-droplet, how much of its change came from condensation, from
 * collection and from chemistry, and in how many collisions.  lcx_track.h records WHAT a marked droplet is at each sample; two samples are
 * at least one condensation and sstp_coal coalescence passes apart, and the difference of rw2 between them cannot be split afterwards.
 * The budget splits it as it happens: the state of the marked droplets is gathered ahead of and behind each pass, in a pass of its own
 * over O(n_tracked) bytes -- no physics kernel gets a new argument or a new form, no atomics, bit-reproducible from run to run.
 * Off by default; with the budget off an object allocates and launches exactly what it does with tracking alone.
 *
 * Passes.  A condensation pass is the condensation of one lcx_step_cond with opts.cond, all substeps and whichever kernels run them.
 * A chemistry pass is the chemistry of one lcx_step_cond.  A coalescence pass is one coalescence substep of lcx_step_async; there are
 * sstp_coal of them per step, as the step has adjusted that number.  lcx_stage (the single-stage test hook) stays outside the budget.
 *
 * Participation.  Track index k < n_tracked takes part in a pass if, at the start of the pass, a storage slot carries mark k + 1 and
 * that slot has n > 0.  Its stored n, rw2, rd3 at the start are n0, w0, d0; the same droplet's stored values at the end are n1, w1, d1
 * (n1 = 0 where the droplet is dead or gone: nothing of it is read then, and nothing is added to the DR3 / DRD3 fields).
 * c(v) = x * sqrt(x) with x = (double)v.
 *
 * Accumulators.  Seven doubles per track index: zero at lcx_track_budget_enable, zero for an index from the moment it is selected, never
 * reset otherwise, and kept when the droplet dies or loses its mark.
 *   LCX_TRB_COND_DR3    condensation   c(w1) - c(w0) if w1 != w0
 *   LCX_TRB_COAL_DR3    coalescence    c(w1) - c(w0) if w1 != w0
 *   LCX_TRB_COAL_DRD3   coalescence    (double)d1 - (double)d0 if d1 != d0
 *   LCX_TRB_CHEM_DRD3   chemistry      (double)d1 - (double)d0 if d1 != d0
 *   LCX_TRB_COAL_DN     coalescence    n0 - n1 (exact below 2^53)
 *   LCX_TRB_COAL_GIVES  coalescence    1 if n1 < n0 (it was the donor of the collision)
 *   LCX_TRB_COAL_GAINS  coalescence    1 if n1 == n0 and (w1 != w0 or d1 != d0) (it was the receiver)
 * A droplet is in at most one pair per coalescence pass, so GAINS + GIVES is the number of collision events it took part in.
 *
 * Closure.  Nothing else writes the rw2 of a droplet that keeps its mark, and only coalescence and chemistry write its rd3.  For a
 * droplet alive at two samples s1 < s2, between the samples' rows: c(rw2) changes by the change of COND_DR3 + COAL_DR3, rd3 by the
 * change of COAL_DRD3 + CHEM_DRD3, and n falls by the change of COAL_DN -- exactly, while opts.rcyc is off: recycling halves a donor
 * outside the budget.
 *
 * lcx_track_budget_enable needs an enabled tracking; before or after lcx_init, before or after selections.  It allocates
 * [LCX_TRB_FIELDS][max_tracked] doubles of accumulators, the start values per INDEX (n, rw2, rd3: not per slot, so a permutation cannot
 * invalidate them) and [capacity][LCX_TRB_FIELDS][max_tracked] doubles of sample rows.  lcx_track_budget_disable, lcx_track_disable,
 * lcx_track_enable on an enabled object (which starts over) and lcx_snapshot_load switch it off and free everything; the budget is not
 * part of a snapshot.
 *
 * Sample rows.  Every sample taken while the budget is on (lcx_track_sample, and the automatic one of every every-th step) also copies
 * the accumulators of [0, n_tracked) into its row, on the stream, with no host wait.  An index selected after a sample reads NaN in that
 * sample's row.  lcx_track_read(reset = 1) empties the rows together with the samples; the accumulators stay.
 *
 * Cost.  With n_tracked > 0: two launches per condensation pass, two per chemistry pass, sstp_coal + 1 per lcx_step_async with
 * coalescence (one stores the start values, one behind each substep adds its differences and stores the next start values), one per
 * sample; a pass that finds the slot list stale finds the slots again first (`scans` of lcx_track_info).  With n_tracked == 0: none.
 * Everything is queued on the object's stream behind the pass it closes and ahead of the next; no host wait, also under stream_ordered.
 *
 * Nothing else changes: every attribute, th, rv, the puddle, the sorted order, every random number, lcx_mode and the snapshot are what
 * they are with tracking alone, bit for bit.
 *
 * Errors (text through lcx_last_error; a failed call leaves the object as it was).  Each "libcloudph++: track budget: ...":
 *   enable while tracking is not enabled; disable or read while the budget is not enabled; field_stride < n_tracked;
 *   now_stride < n_tracked; sample_stride < LCX_TRB_FIELDS * field_stride; cap_samples < the samples held; out == NULL and now == NULL.
 * A multi-device object and a slab with neighbours are refused with the texts of lcx_track.h.
 */
#ifndef LCX_TRACK_BUDGET_H
#define LCX_TRACK_BUDGET_H

#include "lcx_track.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { LCX_TRB_COND_DR3, LCX_TRB_COAL_DR3, LCX_TRB_COAL_DRD3, LCX_TRB_CHEM_DRD3,
       LCX_TRB_COAL_DN, LCX_TRB_COAL_GAINS, LCX_TRB_COAL_GIVES, LCX_TRB_FIELDS };

int lcx_track_budget_enable(lcx_particles *);
int lcx_track_budget_disable(lcx_particles *);
/* any pointer may be NULL; not enabled: everything 0 */
int lcx_track_budget_info(lcx_particles *, int *enabled, unsigned long long *cond_passes,
                          unsigned long long *chem_passes, unsigned long long *coal_passes);
/* out[s * sample_stride + f * field_stride + k]: the rows of the samples held;
   now[f * now_stride + k]: the accumulators as they stand.
   Either may be NULL.  Strides and cap_samples checked as lcx_track_read checks them.
   Host pointers, or device pointers with out_on_device = 1.  One stream wait, at the end.  No reset. */
int lcx_track_budget_read(lcx_particles *, double *out, size_t sample_stride, size_t field_stride,
                          size_t cap_samples, size_t *n_samples, double *now, size_t now_stride,
                          int out_on_device);

#ifdef __cplusplus
}
#endif
#endif
