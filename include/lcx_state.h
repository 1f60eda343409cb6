/*
 * lcx_state.h -- companion of lcx.h: checkpoint and restart.  A snapshot is ONE contiguous host buffer (a "blob") that holds
 * everything a particles object needs in order to go on; restored into a fresh object it continues bit for bit as the object that
 * was saved would have.  A header of its own because lcx.h is the surface that the CPU oracle mirrors entry for entry
 * (tests/test_abi.py), and the reference has no restart.
 *
 * When: where the next legal call is lcx_step_sync / lcx_sync_in, i.e. after lcx_init and after every lcx_step_async.  Refused, each
 * with its own text: between step_sync and step_async, while a neighbour exchange is pending, while replayed random numbers are
 * queued.  Taking a snapshot cannot be observed in the results of the object that took it.
 *
 * Restore: lcx_create with the same lcx_opts_init_t and real kind, then lcx_snapshot_load IN THE PLACE OF lcx_init.  It does what
 * init does without sampling (grid, kernel and efficiency tables, vt_0, w_LS, SGS_mix_len, aerosol_conc_factor, relaxation tables,
 * buffers) and loads the rest; the next call is lcx_step_sync, and lcx_init fails with its "just once" text.  The distributions and
 * the other callbacks stay the caller's and are not stored.  The caller keeps his own Eulerian fields and his own step counter.
 *
 * Not kept: the lcx_diag_* selection (select anew) and the lcx_outbuf contents; profiling and the like start fresh, among them the
 * coalescence bound's pause counter (skip_pause: whether a step collects the per-cell maxima -- results do not depend on it).
 *
 * Mismatch is an error, never undefined behaviour: the blob records the format version, lcx_version(), the real kind and every scalar
 * field of lcx_opts_init_t (pointers and callbacks left out; strict_fp, cond_solver, dbg_flags and dbg_flags2 included: bit identity
 * needs them).  lcx_snapshot_load compares them with the receiving object's and names the first field that differs (dev_id is
 * recorded and not compared: it says where the object runs).  A truncated blob, a wrong magic, an unknown version, a section that
 * overruns the blob and a header checksum that does not match fail, each with its own text, before anything of the object has
 * changed.  A section whose checksum does not match once it is on the device fails too, naming the section; the object is then
 * left as created and accepts another load.
 *
 * Scope: a single-device object without neighbours, float or double, with every option built for it.  An object with
 * bcond_lft / bcond_rgt = distmem and an lcx_create_multi object answer "libcloudph++: snapshot of a decomposed domain is not built".
 *
 * Layout (little-endian; csrc/lcx_snapshot_format.hpp holds the structs, the writer and the validating reader):
 *   header, 256 bytes   magic "LCXSNAP1", format version (1), header size, total bytes, real kind, numbers of options / scalars /
 *                       sections, offsets of the three blocks and of the data, the staging chunk size, the head's checksum,
 *                       lcx_version() of the writer
 *   options             named 64-bit values: every scalar field of lcx_opts_init_t (name[32], bits: integers sign-extended, doubles
 *                       by bit pattern)
 *   scalars             named 64-bit values: counts (n_part, n_storage, n_cell), order-of-work flags (sorted, sort_deferred,
 *                       rank_owed, ...), the salts of a deferred or owed shuffle (deferred_rs.*), counters (rng_call, src_stp_ctr,
 *                       rlx_stp_ctr, steps_since_reorder, tag_next), dt and the substep numbers as adjusted, the puddle sums
 *   section table       64 bytes per section: name[32], element type (0 unsigned, 1 real, 2 bytes), element size, count, offset,
 *                       checksum
 *   sections            each at a multiple of 64 bytes: the columns of the storage over its whole extent, dead slots included
 *                       (n, rd3, rw2, kappa, vt, x, y, z, sd.* for the per-droplet extras), ijk, rank, sorted_id, sorted_ijk,
 *                       cell_cnt, cell_start, the cell fields (cell.*), the Courant arrays, ambient.* gases, puddle accumulators
 * Checksum of a section, of the head and of lcx_snapshot_checksum_host: the sum modulo 2^64, over the 8-byte little-endian words w_i
 * of the data (i from 0, the tail padded with zeros), of mix(w_i + (i + 1) * 0x9E3779B97F4A7C15), where
 *   mix(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; return z ^ (z >> 31)
 * (the finaliser of splitmix64).  It depends on the position of every word and not on the order of summation: the device computes
 * each section's while the data is in its memory, at save and again after load.
 *
 * Copies go through two page-locked chunks of 32 MiB (recorded in the header), one in flight while the host moves the other: the
 * caller's buffer may be pageable, and nothing of the blob's size is allocated, page-locked or on the device.
 */
#ifndef LCX_STATE_H
#define LCX_STATE_H

#include "lcx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of a snapshot taken now */
int lcx_snapshot_size(lcx_particles *, size_t *bytes);
/* writes the blob into host_buf[0, cap); *written = its size */
int lcx_snapshot_save(lcx_particles *, void *host_buf, size_t cap, size_t *written);
/* in the place of lcx_init, into a fresh object */
int lcx_snapshot_load(lcx_particles *, const void *host_buf, size_t bytes);
/* host only, no device needed: validates header and section table and describes the blob as text (version, counts, one line per
 * section) in out[0, cap), zero-terminated */
int lcx_snapshot_describe(const void *host_buf, size_t bytes, char *out, size_t cap);
/* the checksum above on the host (needs no GPU) */
int lcx_snapshot_checksum_host(const void *data, size_t bytes, unsigned long long *out);
/* parity hook in the style of lcx_math_probe: the device's checksum of a host array (copied to the device, summed there) */
int lcx_snapshot_checksum_probe(const void *host_data, size_t bytes, unsigned long long *out);
/* measurement hook (tools/snapshot_cost.py): device time in ms of one checksum pass (both launches) over `bytes` bytes of device
 * memory, the mean of `reps` passes behind a warm-up */
int lcx_snapshot_checksum_time(size_t bytes, int reps, double *ms_per_pass);

#ifdef __cplusplus
}
#endif
#endif
