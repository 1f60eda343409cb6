/*
 * lcx_chem.h -- aqueous chemistry of the super-droplets (opts_init.chem_switch; opts.chem_dsl / chem_dsc / chem_rct): the entries of
 * lcx.h that exchange Eulerian fields, with the reference's extra argument ambient_chem (particles.hpp:17-134,
 * std::map<chem_species_t, arrinfo_t>) as six arrays indexed by species, and diag_chem.  They live in a header of their own because
 * the CPU oracle, which mirrors every entry of lcx.h, has no chemistry.
 *
 * An object created with chem_switch takes these entries in the place of lcx_init / lcx_sync_in / lcx_step_cond / lcx_step_sync; the
 * plain ones fail with "chemistry was not switched off and ambient_chem is empty" (lcx_step_cond only with opts.chem_dsl, which writes
 * the gases back).  On an object without chemistry these entries fail with "chemistry was switched off and ambient_chem is not empty"
 * when any of the six arrays is given.  The arrays hold mixing ratios [kg of gas / kg of dry air] per cell, laid out like th and rv;
 * host or device arrays (lcx_arrinfo_t.on_device).  With opts.chem_dsl, step_cond / step_sync write the new values back after th and rv.
 */
#ifndef LCX_CHEM_H_INCLUDED
#define LCX_CHEM_H_INCLUDED

#include "lcx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* = common::chem::chem_species_t (common/chem.hpp:8-22): the first six are the gases and their dissolved forms (also the index into
 * ambient_chem and into lcx_diag_puddle's slots LCX_OUT_HNO3 ... LCX_OUT_H), S_VI and H exist in the droplets only */
enum lcx_chem_species {
  LCX_CHEM_HNO3 = 0, LCX_CHEM_NH3, LCX_CHEM_CO2, LCX_CHEM_SO2, LCX_CHEM_H2O2, LCX_CHEM_O3, LCX_CHEM_S_VI, LCX_CHEM_H,
  LCX_CHEM_GAS_N = LCX_CHEM_O3 + 1, LCX_CHEM_ALL = LCX_CHEM_H + 1
};

int lcx_init_chem(lcx_particles *, const lcx_arrinfo_t *th, const lcx_arrinfo_t *rv, const lcx_arrinfo_t *rhod,
                  const lcx_arrinfo_t *p, const lcx_arrinfo_t *courant_x, const lcx_arrinfo_t *courant_y,
                  const lcx_arrinfo_t *courant_z, const lcx_arrinfo_t *ambient_chem[6]);
int lcx_sync_in_chem(lcx_particles *, const lcx_arrinfo_t *th, const lcx_arrinfo_t *rv, const lcx_arrinfo_t *rhod,
                     const lcx_arrinfo_t *courant_x, const lcx_arrinfo_t *courant_y, const lcx_arrinfo_t *courant_z,
                     const lcx_arrinfo_t *diss_rate, const lcx_arrinfo_t *ambient_chem[6]);
int lcx_step_cond_chem(lcx_particles *, const lcx_opts_t *, const lcx_arrinfo_t *th, const lcx_arrinfo_t *rv,
                       const lcx_arrinfo_t *ambient_chem[6]);
int lcx_step_sync_chem(lcx_particles *, const lcx_opts_t *, const lcx_arrinfo_t *th, const lcx_arrinfo_t *rv,
                       const lcx_arrinfo_t *rhod, const lcx_arrinfo_t *courant_x, const lcx_arrinfo_t *courant_y,
                       const lcx_arrinfo_t *courant_z, const lcx_arrinfo_t *diss_rate, const lcx_arrinfo_t *ambient_chem[6]);
/* particles_diag.ipp:643-650: first moment of the mass of `species` over the current selection, per kg of dry air (outbuf) */
int lcx_diag_chem(lcx_particles *, int species);

#ifdef __cplusplus
}
#endif
#endif
