/*
 * lcx_rlx.h -- host-only companion of lcx.h for aerosol relaxation: the size bins that an object will use, computed without a
 * device.  It is a header of its own because lcx.h is the surface that the CPU oracle mirrors entry for entry
 * (tests/test_abi.py), and the oracle has no relaxation.
 */
#ifndef LCX_RLX_H
#define LCX_RLX_H

#include "lcx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* aerosol relaxation's size bins as an object created from these options in double lays them out (needs no GPU): for entry `spectrum`
 * of rlx_dry_distros, *n_bins = int(rlx_bins * its range of ln rd / the sum of all ranges), edges_rd3[0 .. *n_bins] the bin edges in
 * rd3 and centre_conc[0 .. *n_bins) the spectrum at each bin's centre times the bin's width in ln rd (the expected STP concentration
 * of the bin).  Either array may be NULL (to query *n_bins).  An object in float rounds the same expressions to float: its own
 * tables are lcx_get_state_real "raw_rlx_edges" / "raw_rlx_conc" (all spectra one after the other, n_bins + 1 edges each), and
 * lcx_get_state_u64 "raw_rlx_count" is the last firing's census, count[bin][level] (summed multiplicities). */
int lcx_rlx_layout(const lcx_opts_init_t *, int spectrum, double *edges_rd3, double *centre_conc, int *n_bins);

#ifdef __cplusplus
}
#endif
#endif
