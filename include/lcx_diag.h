/*
 * lcx_diag.h -- companion of lcx.h: many selections and moments in one pass over the super-droplets.  A header of its own because
 * lcx.h is the surface that the CPU oracle mirrors entry for entry (tests/test_abi.py), and the reference has no such call: its
 * drivers write a spectrum as a loop of diag_*_rng, diag_*_mom, outbuf() per bin and moment.
 *
 * A request is one trip of that loop: a chain of selections and one counting call.  lcx_diag_batch answers a list of requests with
 * the bits that the chain of classic calls gives, reading the attributes once per pass and evaluating each distinct power once.
 *
 *   clauses   ANDed; they stand for "the first clause's call, then every further clause's _cons call":
 *               LCX_DIAG_SEL_ALL    lcx_diag_all
 *               LCX_DIAG_SEL_DRY    lcx_diag_dry_rng(lo, hi)   / lcx_diag_dry_rng_cons      lo, hi: radii, as those calls take them
 *               LCX_DIAG_SEL_WET    lcx_diag_wet_rng(lo, hi)   / lcx_diag_wet_rng_cons
 *               LCX_DIAG_SEL_KAPPA  lcx_diag_kappa_rng(lo, hi) / lcx_diag_kappa_rng_cons
 *               LCX_DIAG_SEL_WATER  lcx_diag_water             / lcx_diag_water_cons
 *   count     LCX_DIAG_SD_CONC    lcx_diag_sd_conc (k is not read)
 *             LCX_DIAG_DRY_MOM    lcx_diag_dry_mom(k)     LCX_DIAG_WET_MOM  lcx_diag_wet_mom(k)     LCX_DIAG_KAPPA_MOM  lcx_diag_kappa_mom(k)
 *   output    out[r * req_stride + c] in the object's real type, c the cell index of lcx_outbuf, req_stride >= n_cell; the elements
 *             between n_cell and req_stride are not written.  out is a host pointer, or with out_on_device = 1 a pointer into the
 *             memory of the object's device, which the kernel then writes directly.
 *
 * The classic selection, lcx_outbuf's contents and the order-of-calls state are left as they were.  The call returns with the result
 * in place (also with opts_init.stream_ordered) and waits for the stream once, at the end, with device and with host output.
 *
 * Passes: the list is cut into passes of at most *req_per_pass requests (lcx_diag_batch_info).  That number is
 * min(32, 512 MiB / (2 * n_cell * sizeof(real))), at least 1: 32 requests fit a kernel's argument block, and with host output a pass
 * needs a device result buffer and a page-locked staging area of req_per_pass * n_cell reals each -- *scratch_bytes is their sum, the
 * most the call ever allocates, whatever n_req is.  Device output allocates nothing.
 *
 * Errors (text through lcx_last_error): n_req < 0; a clause count outside 1 .. LCX_DIAG_MAX_CLAUSES; an unknown sel or count (the
 * classic selections and counts that are not listed above are refused by enumerator range); out == NULL with n_req > 0;
 * req_stride < n_cell; a multi-device object (lcx_create_multi): "libcloudph++: diag_batch on a multi-device object is not built".
 * Before lcx_init the call does what lcx_diag_all does there.  n_req == 0 succeeds and touches nothing.
 */
#ifndef LCX_DIAG_H
#define LCX_DIAG_H

#include "lcx.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { LCX_DIAG_SEL_ALL, LCX_DIAG_SEL_DRY, LCX_DIAG_SEL_WET, LCX_DIAG_SEL_KAPPA, LCX_DIAG_SEL_WATER };
enum { LCX_DIAG_SD_CONC, LCX_DIAG_DRY_MOM, LCX_DIAG_WET_MOM, LCX_DIAG_KAPPA_MOM };
#define LCX_DIAG_MAX_CLAUSES 4
typedef struct { int sel; double lo, hi; } lcx_diag_clause_t;   /* lo, hi: what diag_dry_rng / diag_wet_rng / diag_kappa_rng take */
typedef struct { int n_clauses; lcx_diag_clause_t clause[LCX_DIAG_MAX_CLAUSES]; int count; int k; } lcx_diag_req_t;

/* validation only: no handle, no device */
int lcx_diag_batch_check(const lcx_diag_req_t *req, int n_req);
/* requests per pass of this object, and the bytes that a call with host output allocates at most (see above) */
int lcx_diag_batch_info(lcx_particles *, int *req_per_pass, size_t *scratch_bytes);
int lcx_diag_batch(lcx_particles *, const lcx_diag_req_t *req, int n_req, void *out, size_t req_stride, int out_on_device);

#ifdef __cplusplus
}
#endif
#endif
