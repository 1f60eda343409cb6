// particles_proto_t<real_t> / particles_t<real_t, backend>: the reference's user-facing classes
// (reference: include/libcloudph++/lgrngn/particles.hpp:17-134, :136-246) re-implemented as a thin,
// header-only shim over the C ABI of the HIP library (include/lcx.h, liblcx_hip.so).
//
// Same virtuals, same default arguments, same exception type (std::runtime_error with the library's
// "libcloudph++: ..." message), same call-order rules (init once; then sync_in -> step_cond [= step_sync]
// -> step_async, diag_* in between), same ownership (caller owns every array; th / rv are written back at
// the end of step_cond; outbuf() points into library memory valid until the next outbuf()).
#pragma once
#include <algorithm>
#include "extincl.hpp"
#include "opts.hpp"
#include "opts_init.hpp"
#include "arrinfo.hpp"
#include "backend.hpp"
#include "../../lcx.h"
#include "../../lcx_chem.h"
#include "../../lcx_state.h"
#include "../../lcx_diag.h"
#include "../../lcx_coal_rates.h"
#include "../../lcx_cond_rates.h"
#include "../../lcx_move_rates.h"
#include "../../lcx_track.h"
#include "../../lcx_track_budget.h"
#include "../../lcx_dump.h"
#include "../../lcx_coal_log.h"

namespace libcloudphxx { namespace lgrngn {
  namespace chem = common::chem;

  template <typename real_t>
  struct particles_proto_t
  {
    typedef std::map<enum chem::chem_species_t, const arrinfo_t<real_t>> cchem_t;
    typedef std::map<enum chem::chem_species_t, arrinfo_t<real_t>> chem_t;
    typedef arrinfo_t<real_t> arr;

    virtual void init(const arr th, const arr rv, const arr rhod, const arr p = arr(), const arr courant_x = arr(),
                      const arr courant_y = arr(), const arr courant_z = arr(), const cchem_t ambient_chem = cchem_t()) { assert(false); }
    virtual void step_sync(const opts_t<real_t> &, arr th, arr rv, const arr rhod = arr(), const arr courant_x = arr(),
                           const arr courant_y = arr(), const arr courant_z = arr(), const arr diss_rate = arr(), chem_t ambient_chem = chem_t()) { assert(false); }
    virtual void sync_in(arr th, arr rv, const arr rhod = arr(), const arr courant_x = arr(), const arr courant_y = arr(),
                         const arr courant_z = arr(), const arr diss_rate = arr(), chem_t ambient_chem = chem_t()) { assert(false); }
    virtual void step_cond(const opts_t<real_t> &, arr th, arr rv, chem_t ambient_chem = chem_t()) { assert(false); }
    virtual void step_async(const opts_t<real_t> &) { assert(false); }

    virtual void diag_sd_conc() { assert(false); }
    virtual void diag_pressure() { assert(false); }
    virtual void diag_temperature() { assert(false); }
    virtual void diag_RH() { assert(false); }
    virtual void diag_all() { assert(false); }
    virtual void diag_water() { assert(false); }
    virtual void diag_dry_rng(const real_t &, const real_t &) { assert(false); }
    virtual void diag_wet_rng(const real_t &, const real_t &) { assert(false); }
    virtual void diag_kappa_rng(const real_t &, const real_t &) { assert(false); }
    virtual void diag_dry_rng_cons(const real_t &, const real_t &) { assert(false); }
    virtual void diag_wet_rng_cons(const real_t &, const real_t &) { assert(false); }
    virtual void diag_kappa_rng_cons(const real_t &, const real_t &) { assert(false); }
    virtual void diag_dry_mom(const int &) { assert(false); }
    virtual void diag_wet_mom(const int &) { assert(false); }
    virtual void diag_vel_div() { assert(false); }
    virtual void diag_kappa_mom(const int &) { assert(false); }
    virtual void diag_incloud_time_mom(const int &) { assert(false); }
    virtual void diag_up_mom(const int &) { assert(false); }
    virtual void diag_vp_mom(const int &) { assert(false); }
    virtual void diag_wp_mom(const int &) { assert(false); }
    virtual void diag_water_cons() { assert(false); }
    // diagnostics of the part outside this library (ice) are declared for source compatibility, never served; diag_chem is overridden below
    virtual void diag_chem(const enum common::chem::chem_species_t &) { assert(false); }
    virtual void diag_ice() { assert(false); }
    virtual void diag_ice_cons() { assert(false); }
    virtual void diag_ice_a_rng(const real_t &, const real_t &) { assert(false); }
    virtual void diag_ice_c_rng(const real_t &, const real_t &) { assert(false); }
    virtual void diag_ice_a_rng_cons(const real_t &, const real_t &) { assert(false); }
    virtual void diag_ice_c_rng_cons(const real_t &, const real_t &) { assert(false); }
    virtual void diag_ice_a_mom(const int &) { assert(false); }
    virtual void diag_ice_c_mom(const int &) { assert(false); }
    virtual void diag_ice_mix_ratio() { assert(false); }
    virtual void diag_precip_rate_ice_mass() { assert(false); }
    virtual void diag_max_rw() { assert(false); }
    virtual void diag_precip_rate() { assert(false); }
    virtual void diag_RH_ge_Sc() { assert(false); }
    virtual void diag_rw_ge_rc() { assert(false); }
    virtual void diag_wet_mass_dens(const real_t &, const real_t &) { assert(false); }
    virtual std::map<common::output_t, real_t> diag_puddle() { assert(false); return std::map<common::output_t, real_t>(); }
    virtual std::vector<real_t> get_attr(const std::string &) { assert(false); return std::vector<real_t>(); }
    virtual real_t *outbuf() { assert(false); return nullptr; }
    // checkpoint and restart (no reference counterpart; include/lcx_state.h): snapshot() after init() or step_async(), restore() on a fresh
    // object made from the same opts_init IN THE PLACE OF init().  The caller keeps his own Eulerian fields and step counter.
    virtual std::vector<unsigned char> snapshot() { assert(false); return std::vector<unsigned char>(); }
    virtual void restore(const void *, size_t) { assert(false); }

    opts_init_t<real_t> *opts_init = nullptr;        // points at the live internal copy (particles.hpp:129)
    virtual ~particles_proto_t() {}
  };

  // one request of particles_t<real_t, HIP>::diag_batch (an extension without a reference counterpart; include/lcx_diag.h): the chain
  // "first clause, every further clause with _cons" and the count that follows it.  sel: LCX_DIAG_SEL_*, lo / hi as diag_*_rng take
  // them; count: LCX_DIAG_SD_CONC or LCX_DIAG_*_MOM with k
  template <typename real_t>
  struct diag_req_t
  {
    struct clause_t { int sel; real_t lo, hi; };
    std::vector<clause_t> clauses;
    int count = LCX_DIAG_SD_CONC, k = 0;
    diag_req_t &all() { clauses.push_back(clause_t{LCX_DIAG_SEL_ALL, 0, 0}); return *this; }
    diag_req_t &water() { clauses.push_back(clause_t{LCX_DIAG_SEL_WATER, 0, 0}); return *this; }
    diag_req_t &dry_rng(real_t a, real_t b) { clauses.push_back(clause_t{LCX_DIAG_SEL_DRY, a, b}); return *this; }
    diag_req_t &wet_rng(real_t a, real_t b) { clauses.push_back(clause_t{LCX_DIAG_SEL_WET, a, b}); return *this; }
    diag_req_t &kappa_rng(real_t a, real_t b) { clauses.push_back(clause_t{LCX_DIAG_SEL_KAPPA, a, b}); return *this; }
    diag_req_t &sd_conc() { count = LCX_DIAG_SD_CONC; k = 0; return *this; }
    diag_req_t &dry_mom(int k_) { count = LCX_DIAG_DRY_MOM; k = k_; return *this; }
    diag_req_t &wet_mom(int k_) { count = LCX_DIAG_WET_MOM; k = k_; return *this; }
    diag_req_t &kappa_mom(int k_) { count = LCX_DIAG_KAPPA_MOM; k = k_; return *this; }
  };

  // the rows of one threshold of particles_t<real_t, HIP>::move_rates (an extension without a reference counterpart; include/lcx_move_rates.h
  // defines each of them)
  enum class move_rate_t : int
  {
    in_n = LCX_MVR_IN_N, in_m3 = LCX_MVR_IN_M3, out_n = LCX_MVR_OUT_N, out_m3 = LCX_MVR_OUT_M3, down_n = LCX_MVR_DOWN_N, down_m3 = LCX_MVR_DOWN_M3,
    up_n = LCX_MVR_UP_N, up_m3 = LCX_MVR_UP_M3, precip_n = LCX_MVR_PRECIP_N, precip_m3 = LCX_MVR_PRECIP_M3, per_thr = LCX_MVR_PER_THR
  };

  // the fields of one record of particles_t<real_t, HIP>::track (an extension without a reference counterpart; include/lcx_track.h defines each)
  enum track_field_t
  {
    trk_n = LCX_TRK_N, trk_x = LCX_TRK_X, trk_y = LCX_TRK_Y, trk_z = LCX_TRK_Z, trk_rw2 = LCX_TRK_RW2, trk_rd3 = LCX_TRK_RD3,
    trk_kappa = LCX_TRK_KAPPA, trk_vt = LCX_TRK_VT, trk_cell = LCX_TRK_CELL, trk_T = LCX_TRK_T, trk_RH = LCX_TRK_RH, trk_rv = LCX_TRK_RV,
    trk_fields = LCX_TRK_FIELDS
  };
  // what particles_t<real_t, HIP>::track reads: rec[(s * 12 + field) * n_tracked + k] for sample s and track index k
  struct track_record_t
  {
    size_t n_samples = 0, n_tracked = 0;
    std::vector<double> rec, time;
    std::vector<unsigned long long> steps;
    double at(size_t s, track_field_t f, size_t k) const { return rec[(s * size_t(LCX_TRK_FIELDS) + size_t(f)) * n_tracked + k]; }
  };
  // the fields of particles_t<real_t, HIP>::dump (an extension as well; include/lcx_dump.h defines each): the twelve of a track record, then
  // the storage slot, the track mark, the in-cloud time and the eight chemical masses
  enum dump_field_t
  {
    dmp_n = LCX_DMP_N, dmp_x = LCX_DMP_X, dmp_y = LCX_DMP_Y, dmp_z = LCX_DMP_Z, dmp_rw2 = LCX_DMP_RW2, dmp_rd3 = LCX_DMP_RD3,
    dmp_kappa = LCX_DMP_KAPPA, dmp_vt = LCX_DMP_VT, dmp_cell = LCX_DMP_CELL, dmp_T = LCX_DMP_T, dmp_RH = LCX_DMP_RH, dmp_rv = LCX_DMP_RV,
    dmp_slot = LCX_DMP_SLOT, dmp_track = LCX_DMP_TRACK, dmp_incloud_time = LCX_DMP_INCLOUD_TIME, dmp_chem_HNO3 = LCX_DMP_CHEM_HNO3,
    dmp_chem_NH3 = LCX_DMP_CHEM_NH3, dmp_chem_CO2 = LCX_DMP_CHEM_CO2, dmp_chem_SO2 = LCX_DMP_CHEM_SO2, dmp_chem_H2O2 = LCX_DMP_CHEM_H2O2,
    dmp_chem_O3 = LCX_DMP_CHEM_O3, dmp_chem_S_VI = LCX_DMP_CHEM_S_VI, dmp_chem_H = LCX_DMP_CHEM_H, dmp_fields = LCX_DMP_FIELDS
  };
  // the accumulators of particles_t<real_t, HIP>::track_budget (an extension as well; include/lcx_track_budget.h defines each)
  enum track_budget_field_t
  {
    trb_cond_dr3 = LCX_TRB_COND_DR3, trb_coal_dr3 = LCX_TRB_COAL_DR3, trb_coal_drd3 = LCX_TRB_COAL_DRD3, trb_chem_drd3 = LCX_TRB_CHEM_DRD3,
    trb_coal_dn = LCX_TRB_COAL_DN, trb_coal_gains = LCX_TRB_COAL_GAINS, trb_coal_gives = LCX_TRB_COAL_GIVES,
    trb_fields = LCX_TRB_FIELDS
  };
  // what track_budget reads: the rows of the samples held, rows[(s * 7 + field) * n_tracked + k], and the accumulators as they stand
  struct track_budget_t
  {
    size_t n_samples = 0, n_tracked = 0;
    std::vector<double> rows, acc;
    double at(size_t s, track_budget_field_t f, size_t k) const { return rows[(s * size_t(LCX_TRB_FIELDS) + size_t(f)) * n_tracked + k]; }
    double now(track_budget_field_t f, size_t k) const { return acc[size_t(f) * n_tracked + k]; }
  };

  // the rows of one threshold of particles_t<real_t, HIP>::cond_rates (an extension without a reference counterpart; include/lcx_cond_rates.h
  // defines each of them); total_dm3 names the row behind the last threshold's
  enum class cond_rate_t : int
  {
    above_dm3 = LCX_CDR_ABOVE_DM3, up_n = LCX_CDR_UP_N, up_m3 = LCX_CDR_UP_M3, down_n = LCX_CDR_DOWN_N, down_m3 = LCX_CDR_DOWN_M3,
    per_thr = LCX_CDR_PER_THR, total_dm3 = -1
  };

  // the accumulators of particles_t<real_t, HIP>::coal_rates (an extension without a reference counterpart; include/lcx_coal_rates.h
  // defines each of them)
  enum class coal_rate_t : int
  {
    acnv_m3 = LCX_CR_ACNV_M3, acnv_nc = LCX_CR_ACNV_NC, acnv_nr = LCX_CR_ACNV_NR, accr_m3 = LCX_CR_ACCR_M3, accr_nc = LCX_CR_ACCR_NC,
    self_cloud_n = LCX_CR_SELF_CLOUD_N, self_rain_n = LCX_CR_SELF_RAIN_N, count = LCX_CR_COUNT
  };

  // the rows of particles_t<real_t, HIP>::coal_log (an extension without a reference counterpart; include/lcx_coal_log.h defines each)
  enum class coal_log_field_t : int
  {
    launch = LCX_CLG_LAUNCH, cell = LCX_CLG_CELL, slot_d = LCX_CLG_SLOT_D, slot_r = LCX_CLG_SLOT_R, col_no = LCX_CLG_COL_NO, n_d = LCX_CLG_N_D,
    n_r = LCX_CLG_N_R, rw2_d = LCX_CLG_RW2_D, rw2_r = LCX_CLG_RW2_R, rw2_new = LCX_CLG_RW2_NEW, rd3_d = LCX_CLG_RD3_D, rd3_r = LCX_CLG_RD3_R,
    vt_d = LCX_CLG_VT_D, vt_r = LCX_CLG_VT_R, count = LCX_CLG_FIELDS
  };

  namespace detail
  {
    inline void lcx_check(int rc) { if (rc) throw std::runtime_error(lcx_last_error()); }

    template <typename real_t> inline double distro_trampoline(double lnrd, void *user)
    { return double(static_cast<common::unary_function<real_t> *>(user)->funval(real_t(lnrd))); }

    template <typename real_t> struct carr
    {
      lcx_arrinfo_t a; bool null;
      explicit carr(const arrinfo_t<real_t> &x) : null(x.is_null())
      { a.data = const_cast<void *>(static_cast<const void *>(x.data)); a.strides = x.strides; a.on_device = x.on_device ? 1 : 0; }
      const lcx_arrinfo_t *ptr() const { return null ? nullptr : &a; }
    };
    // the reference's ambient_chem map as the six pointers of include/lcx_chem.h (a species that the map lacks: a null entry)
    template <typename real_t> struct cchem
    {
      lcx_arrinfo_t a[6]; const lcx_arrinfo_t *p[6];
      template <class map_t> explicit cchem(const map_t &m)
      {
        for (int i = 0; i < 6; ++i) p[i] = nullptr;
        for (const auto &kv : m) {
          const int i = int(kv.first);
          if (i < 0 || i >= 6 || kv.second.is_null()) continue;
          a[i].data = const_cast<void *>(static_cast<const void *>(kv.second.data)); a[i].strides = kv.second.strides; a[i].on_device = kv.second.on_device ? 1 : 0;
          p[i] = &a[i];
        }
      }
    };
  }

  // generic declaration: only the HIP slots are implemented by this library
  template <typename real_t, backend_t backend> struct particles_t;

  template <typename real_t>
  struct particles_t<real_t, HIP> : particles_proto_t<real_t>
  {
    typedef particles_proto_t<real_t> parent_t;
    typedef arrinfo_t<real_t> arr;
    typedef typename parent_t::cchem_t cchem_t;
    typedef typename parent_t::chem_t chem_t;

    // pimpl kept public like in the reference (particles.hpp:229-230); it only holds the C handle and the options copy
    struct impl { lcx_particles *h = nullptr; opts_init_t<real_t> opts_init; std::vector<real_t> outbuf_copy; ~impl() { if (h) lcx_destroy(h); } };
    std::unique_ptr<impl> pimpl;

    // multi: the object spans opts_init.dev_count devices (lcx_create_multi) -- used by the multi_HIP specialisation below
    explicit particles_t(opts_init_t<real_t> oi, int n_x_tot = 0, bool multi = false) : pimpl(new impl)
    {
      pimpl->opts_init = oi;
      this->opts_init = &pimpl->opts_init;
      lcx_opts_init_t c;
      lcx_opts_init_default(&c);
      const opts_init_t<real_t> &o = pimpl->opts_init;
      c.nx = o.nx; c.ny = o.ny; c.nz = o.nz; c.dx = o.dx; c.dy = o.dy; c.dz = o.dz; c.dt = o.dt;
      c.sstp_cond = o.sstp_cond; c.sstp_coal = o.sstp_coal; c.sstp_cond_act = o.sstp_cond_act; c.sstp_chem = o.sstp_chem;
      c.x0 = o.x0; c.y0 = o.y0; c.z0 = o.z0; c.x1 = o.x1; c.y1 = o.y1; c.z1 = o.z1;
      c.sd_conc = o.sd_conc; c.sd_conc_large_tail = o.sd_conc_large_tail; c.aerosol_independent_of_rhod = o.aerosol_independent_of_rhod;
      c.variable_dt_switch = o.variable_dt_switch; c.sd_const_multi = o.sd_const_multi; c.n_sd_max = o.n_sd_max;
      c.kernel = int(o.kernel); c.terminal_velocity = int(o.terminal_velocity); c.adve_scheme = int(o.adve_scheme); c.RH_formula = int(o.RH_formula);
      std::vector<double> kp(o.kernel_parameters.begin(), o.kernel_parameters.end()), wls(o.w_LS.begin(), o.w_LS.end()),
                          acf(o.aerosol_conc_factor.begin(), o.aerosol_conc_factor.end()), sgs(o.SGS_mix_len.begin(), o.SGS_mix_len.end());
      c.SGS_mix_len = sgs.data(); c.n_SGS_mix_len = int(sgs.size());
      c.kernel_parameters = kp.data(); c.n_kernel_parameters = int(kp.size());
      c.w_LS = wls.data(); c.n_w_LS = int(wls.size());
      c.aerosol_conc_factor = acf.data(); c.n_aerosol_conc_factor = int(acf.size());
      c.chem_switch = o.chem_switch; c.coal_switch = o.coal_switch; c.sedi_switch = o.sedi_switch; c.subs_switch = o.subs_switch;
      c.rlx_switch = o.rlx_switch; c.turb_adve_switch = o.turb_adve_switch; c.turb_cond_switch = o.turb_cond_switch;
      c.turb_coal_switch = o.turb_coal_switch; c.ice_switch = o.ice_switch; c.exact_sstp_cond = o.exact_sstp_cond;
      c.sstp_cond_mix = o.sstp_cond_mix; c.adaptive_sstp_cond = o.adaptive_sstp_cond; c.time_dep_ice_nucl = o.time_dep_ice_nucl;
      c.RH_max = o.RH_max; c.sstp_cond_adapt_drw2_eps = o.sstp_cond_adapt_drw2_eps; c.sstp_cond_adapt_drw2_max = o.sstp_cond_adapt_drw2_max; c.rc2_T = o.rc2_T;
      c.rng_seed = o.rng_seed; c.rng_seed_init = o.rng_seed_init; c.rng_seed_init_switch = o.rng_seed_init_switch;
      c.dev_count = o.dev_count; c.dev_id = o.dev_id; c.rd_min = o.rd_min; c.rd_max = o.rd_max;
      c.no_ccn_at_init = o.no_ccn_at_init; c.open_side_walls = o.open_side_walls; c.periodic_topbot_walls = o.periodic_topbot_walls;
      c.src_type = int(o.src_type); c.th_dry = o.th_dry; c.const_p = o.const_p; c.diag_incloud_time = o.diag_incloud_time;
      c.n_x_tot = n_x_tot; c.strict_fp = o.strict_fp; c.cond_solver = o.cond_solver; c.reorder_every = o.reorder_every; c.stream_ordered = o.stream_ordered;
      c.dbg_flags = o.dbg_flags;
      c.dbg_flags2 = o.dbg_flags2;
      c.n_x_bfr = o.n_x_bfr; c.bcond_lft = o.bcond_lft; c.bcond_rgt = o.bcond_rgt;
      c.chem_rho = o.chem_rho;
      c.src_x0 = o.src_x0; c.src_y0 = o.src_y0; c.src_z0 = o.src_z0; c.src_x1 = o.src_x1; c.src_y1 = o.src_y1; c.src_z1 = o.src_z1;
      // std::map iterates in (kappa, rd_insol) order, which is the order the library expects
      std::vector<lcx_distro_t> dd;
      for (const auto &kv : pimpl->opts_init.dry_distros) {
        lcx_distro_t d{};
        d.kappa = kv.first.kappa; d.rd_insol = kv.first.rd_insol;
        d.fn = &detail::distro_trampoline<real_t>; d.user = kv.second.get();     // shared_ptr kept alive by pimpl->opts_init
        dd.push_back(d);
      }
      c.dry_distros = dd.data(); c.n_dry_distros = int(dd.size());
      std::vector<lcx_dry_size_t> ds;
      for (const auto &kv : o.dry_sizes) for (const auto &rc : kv.second)
        ds.push_back(lcx_dry_size_t{double(kv.first.kappa), double(kv.first.rd_insol), double(rc.first), double(rc.second.first), rc.second.second});
      c.dry_sizes = ds.data(); c.n_dry_sizes = int(ds.size());
      // aerosol relaxation: an unordered_map in the reference, sorted by kappa here (the order the library expects)
      c.rlx_bins = int(o.rlx_bins); c.rlx_sd_per_bin = o.rlx_sd_per_bin; c.rlx_timescale = o.rlx_timescale; c.supstp_rlx = o.supstp_rlx;
      std::vector<lcx_rlx_distro_t> rd;
      for (const auto &kv : pimpl->opts_init.rlx_dry_distros) {
        lcx_rlx_distro_t e{};
        e.distro.kappa = kv.first;
        e.distro.fn = &detail::distro_trampoline<real_t>; e.distro.user = std::get<0>(kv.second).get();   // shared_ptr kept alive by pimpl->opts_init
        e.kappa_min = std::get<1>(kv.second).first; e.kappa_max = std::get<1>(kv.second).second;
        e.z_min = std::get<2>(kv.second).first; e.z_max = std::get<2>(kv.second).second;
        rd.push_back(e);
      }
      std::sort(rd.begin(), rd.end(), [](const lcx_rlx_distro_t &a, const lcx_rlx_distro_t &b) { return a.distro.kappa < b.distro.kappa; });
      c.rlx_dry_distros = rd.empty() ? nullptr : rd.data(); c.n_rlx_dry_distros = int(rd.size());
      detail::lcx_check(multi ? lcx_create_multi(&c, int(sizeof(real_t)), &pimpl->h) : lcx_create(&c, int(sizeof(real_t)), &pimpl->h));
    }
    ~particles_t() override {}

    void init(const arr th, const arr rv, const arr rhod, const arr p = arr(), const arr courant_x = arr(), const arr courant_y = arr(),
              const arr courant_z = arr(), const cchem_t ambient_chem = cchem_t()) override
    {
      detail::carr<real_t> a(th), b(rv), c(rhod), d(p), e(courant_x), f(courant_y), g(courant_z);
      if (ambient_chem.empty()) { detail::lcx_check(lcx_init(pimpl->h, a.ptr(), b.ptr(), c.ptr(), d.ptr(), e.ptr(), f.ptr(), g.ptr())); return; }
      detail::cchem<real_t> ch(ambient_chem);
      detail::lcx_check(lcx_init_chem(pimpl->h, a.ptr(), b.ptr(), c.ptr(), d.ptr(), e.ptr(), f.ptr(), g.ptr(), ch.p));
    }
    void sync_in(arr th, arr rv, const arr rhod = arr(), const arr courant_x = arr(), const arr courant_y = arr(), const arr courant_z = arr(),
                 const arr diss_rate = arr(), chem_t ambient_chem = chem_t()) override
    {
      detail::carr<real_t> a(th), b(rv), c(rhod), e(courant_x), f(courant_y), g(courant_z), d(diss_rate);
      if (ambient_chem.empty()) { detail::lcx_check(lcx_sync_in(pimpl->h, a.ptr(), b.ptr(), c.ptr(), e.ptr(), f.ptr(), g.ptr(), d.ptr())); return; }
      detail::cchem<real_t> ch(ambient_chem);
      detail::lcx_check(lcx_sync_in_chem(pimpl->h, a.ptr(), b.ptr(), c.ptr(), e.ptr(), f.ptr(), g.ptr(), d.ptr(), ch.p));
    }
    void step_cond(const opts_t<real_t> &opts, arr th, arr rv, chem_t ambient_chem = chem_t()) override
    {
      const lcx_opts_t oc = conv(opts);
      detail::carr<real_t> a(th), b(rv);
      if (ambient_chem.empty()) { detail::lcx_check(lcx_step_cond(pimpl->h, &oc, a.ptr(), b.ptr())); return; }
      detail::cchem<real_t> ch(ambient_chem);
      detail::lcx_check(lcx_step_cond_chem(pimpl->h, &oc, a.ptr(), b.ptr(), ch.p));
    }
    void step_sync(const opts_t<real_t> &opts, arr th, arr rv, const arr rhod = arr(), const arr courant_x = arr(), const arr courant_y = arr(),
                   const arr courant_z = arr(), const arr diss_rate = arr(), chem_t ambient_chem = chem_t()) override
    {
      sync_in(th, rv, rhod, courant_x, courant_y, courant_z, diss_rate, ambient_chem);
      step_cond(opts, th, rv, ambient_chem);
    }
    void step_async(const opts_t<real_t> &opts) override
    {
      lcx_opts_t oc = conv(opts);
      // the aerosol source's spectra: arrays in std::map order that live until the call returns
      std::vector<lcx_src_distro_t> sd;
      for (const auto &kv : opts.src_dry_distros) {
        lcx_src_distro_t e{};
        e.distro.kappa = kv.first.kappa; e.distro.rd_insol = kv.first.rd_insol;
        e.distro.fn = &detail::distro_trampoline<real_t>; e.distro.user = std::get<0>(kv.second).get();
        e.sd_conc = (unsigned long long)(std::get<1>(kv.second)); e.supstp = std::get<2>(kv.second);
        sd.push_back(e);
      }
      std::vector<lcx_src_size_t> ss;
      for (const auto &kv : opts.src_dry_sizes) for (const auto &rc : kv.second)
        ss.push_back(lcx_src_size_t{double(kv.first.kappa), double(kv.first.rd_insol), double(rc.first), double(std::get<0>(rc.second)),
                                    std::get<1>(rc.second), std::get<2>(rc.second)});
      oc.src_dry_distros = sd.empty() ? nullptr : sd.data(); oc.n_src_dry_distros = int(sd.size());
      oc.src_dry_sizes = ss.empty() ? nullptr : ss.data(); oc.n_src_dry_sizes = int(ss.size());
      detail::lcx_check(lcx_step_async(pimpl->h, &oc));
    }

    void diag_chem(const enum common::chem::chem_species_t &c) override { detail::lcx_check(lcx_diag_chem(pimpl->h, int(c))); }
    void diag_sd_conc() override { detail::lcx_check(lcx_diag_sd_conc(pimpl->h)); }
    void diag_pressure() override { detail::lcx_check(lcx_diag_pressure(pimpl->h)); }
    void diag_temperature() override { detail::lcx_check(lcx_diag_temperature(pimpl->h)); }
    void diag_RH() override { detail::lcx_check(lcx_diag_RH(pimpl->h)); }
    void diag_all() override { detail::lcx_check(lcx_diag_all(pimpl->h)); }
    void diag_water() override { detail::lcx_check(lcx_diag_water(pimpl->h)); }
    void diag_dry_rng(const real_t &a, const real_t &b) override { detail::lcx_check(lcx_diag_dry_rng(pimpl->h, a, b)); }
    void diag_wet_rng(const real_t &a, const real_t &b) override { detail::lcx_check(lcx_diag_wet_rng(pimpl->h, a, b)); }
    void diag_kappa_rng(const real_t &a, const real_t &b) override { detail::lcx_check(lcx_diag_kappa_rng(pimpl->h, a, b)); }
    void diag_dry_rng_cons(const real_t &a, const real_t &b) override { detail::lcx_check(lcx_diag_dry_rng_cons(pimpl->h, a, b)); }
    void diag_wet_rng_cons(const real_t &a, const real_t &b) override { detail::lcx_check(lcx_diag_wet_rng_cons(pimpl->h, a, b)); }
    void diag_kappa_rng_cons(const real_t &a, const real_t &b) override { detail::lcx_check(lcx_diag_kappa_rng_cons(pimpl->h, a, b)); }
    void diag_dry_mom(const int &k) override { detail::lcx_check(lcx_diag_dry_mom(pimpl->h, k)); }
    void diag_wet_mom(const int &k) override { detail::lcx_check(lcx_diag_wet_mom(pimpl->h, k)); }
    void diag_vel_div() override { detail::lcx_check(lcx_diag_vel_div(pimpl->h)); }
    void diag_kappa_mom(const int &k) override { detail::lcx_check(lcx_diag_kappa_mom(pimpl->h, k)); }
    void diag_incloud_time_mom(const int &k) override { detail::lcx_check(lcx_diag_incloud_time_mom(pimpl->h, k)); }
    void diag_up_mom(const int &k) override { detail::lcx_check(lcx_diag_up_mom(pimpl->h, k)); }
    void diag_vp_mom(const int &k) override { detail::lcx_check(lcx_diag_vp_mom(pimpl->h, k)); }
    void diag_wp_mom(const int &k) override { detail::lcx_check(lcx_diag_wp_mom(pimpl->h, k)); }
    void diag_water_cons() override { detail::lcx_check(lcx_diag_water_cons(pimpl->h)); }
    void diag_max_rw() override { detail::lcx_check(lcx_diag_max_rw(pimpl->h)); }
    void diag_precip_rate() override { detail::lcx_check(lcx_diag_precip_rate(pimpl->h)); }
    void diag_RH_ge_Sc() override { detail::lcx_check(lcx_diag_RH_ge_Sc(pimpl->h)); }
    void diag_rw_ge_rc() override { detail::lcx_check(lcx_diag_rw_ge_rc(pimpl->h)); }
    void diag_wet_mass_dens(const real_t &rad, const real_t &sig0) override { detail::lcx_check(lcx_diag_wet_mass_dens(pimpl->h, rad, sig0)); }
    std::map<common::output_t, real_t> diag_puddle() override
    {
      double v[LCX_OUT_COUNT];
      detail::lcx_check(lcx_diag_puddle(pimpl->h, v));
      std::map<common::output_t, real_t> m;
      for (int i = 0; i < LCX_OUT_COUNT; ++i) m[static_cast<common::output_t>(i)] = real_t(v[i]);
      return m;
    }
    std::vector<real_t> get_attr(const std::string &name) override
    {
      size_t n = 0;
      detail::lcx_check(lcx_get_attr(pimpl->h, name.c_str(), nullptr, 0, &n));
      std::vector<real_t> out(n);
      detail::lcx_check(lcx_get_attr(pimpl->h, name.c_str(), out.data(), n, &n));
      return out;
    }
    real_t *outbuf() override
    {
      const void *p = nullptr; size_t n = 0;
      detail::lcx_check(lcx_outbuf(pimpl->h, &p, &n));
      return const_cast<real_t *>(static_cast<const real_t *>(p));
    }
    std::vector<unsigned char> snapshot() override
    {
      size_t n = 0;
      detail::lcx_check(lcx_snapshot_size(pimpl->h, &n));
      std::vector<unsigned char> blob(n);
      detail::lcx_check(lcx_snapshot_save(pimpl->h, blob.data(), blob.size(), &n));
      blob.resize(n);
      return blob;
    }
    void restore(const void *blob, size_t bytes) override { detail::lcx_check(lcx_snapshot_load(pimpl->h, blob, bytes)); }
    // EXTENSION, no reference counterpart (include/lcx_diag.h): out[r * stride + cell] = what reqs[r]'s selections, its count and
    // outbuf() give, bit for bit, from one pass over the super-droplets per diag_batch_info() requests; stride >= n_cell.  The
    // classic selection and outbuf() are left as they were.  Not virtual: particles_proto_t stays the reference's.
    void diag_batch(const std::vector<diag_req_t<real_t>> &reqs, real_t *out, size_t stride, bool on_device = false)
    {
      std::vector<lcx_diag_req_t> c(reqs.size());
      for (size_t r = 0; r < reqs.size(); ++r) {
        const size_t nc = reqs[r].clauses.size();
        c[r].n_clauses = nc > LCX_DIAG_MAX_CLAUSES ? LCX_DIAG_MAX_CLAUSES + 1 : int(nc);       // (too many: the library names the request)
        for (size_t i = 0; i < nc && i < LCX_DIAG_MAX_CLAUSES; ++i)
          c[r].clause[i] = lcx_diag_clause_t{reqs[r].clauses[i].sel, double(reqs[r].clauses[i].lo), double(reqs[r].clauses[i].hi)};
        c[r].count = reqs[r].count; c[r].k = reqs[r].k;
      }
      detail::lcx_check(lcx_diag_batch(pimpl->h, c.data(), int(c.size()), out, stride, on_device ? 1 : 0));
    }
    int diag_batch_info(size_t *scratch_bytes = nullptr)
    {
      int rpp = 0;
      detail::lcx_check(lcx_diag_batch_info(pimpl->h, &rpp, scratch_bytes));
      return rpp;
    }
    // EXTENSION, no reference counterpart (include/lcx_coal_rates.h): per-cell sums of what every collision event moves between cloud
    // (wet radius below r_thr) and rain -- autoconversion, accretion, self-collection -- filled inside the coalescence kernels while
    // enabled.  coal_rates: out[int(coal_rate_t) * n_cell + cell] (resized to count * n_cell), the numbers as doubles; reset zeroes the
    // accumulators behind the read.  diag_coal_rate fills outbuf() like a diag_*_mom call.  A snapshot does not hold them: a restored
    // object is disabled.  Not virtual: particles_proto_t stays the reference's.
    void coal_rates_enable(real_t r_thr) { detail::lcx_check(lcx_coal_rates_enable(pimpl->h, double(r_thr))); }
    void coal_rates_disable() { detail::lcx_check(lcx_coal_rates_disable(pimpl->h)); }
    void coal_rates(std::vector<double> &out, bool reset = false)
    {
      size_t n_cell = 0;
      detail::lcx_check(lcx_n_cell(pimpl->h, &n_cell));
      out.resize(size_t(LCX_CR_COUNT) * n_cell);
      detail::lcx_check(lcx_coal_rates_read(pimpl->h, out.data(), n_cell, 0, reset ? 1 : 0));
    }
    void diag_coal_rate(coal_rate_t which) { detail::lcx_check(lcx_diag_coal_rate(pimpl->h, int(which))); }
    // EXTENSION, no reference counterpart (include/lcx_cond_rates.h): per-cell tally of what step_cond's condensation does relative to up to
    // LCX_CDR_MAX_THR increasing threshold radii -- growth above a threshold, droplets and water crossing it up and down, and the total --
    // filled by a pass of its own around the condensation while enabled.  cond_rates: out[row * n_cell + cell] with row = 5 t + int(cond_rate_t)
    // and the total in row 5 K (resized to (5 K + 1) * n_cell), the numbers as doubles; reset zeroes the rows behind the read.  diag_cond_rate
    // fills outbuf() like a diag_*_mom call.  A snapshot does not hold them: a restored object is disabled.  Not virtual, as above.
    void cond_rates_enable(const std::vector<real_t> &r_thr)
    {
      std::vector<double> r(r_thr.begin(), r_thr.end());
      detail::lcx_check(lcx_cond_rates_enable(pimpl->h, r.data(), int(r.size())));
    }
    void cond_rates_disable() { detail::lcx_check(lcx_cond_rates_disable(pimpl->h)); }
    void cond_rates(std::vector<double> &out, bool reset = false)
    {
      size_t n_cell = 0; int n_thr = 0;
      detail::lcx_check(lcx_n_cell(pimpl->h, &n_cell));
      detail::lcx_check(lcx_cond_rates_info(pimpl->h, nullptr, &n_thr, nullptr, nullptr));
      out.resize(size_t(LCX_CDR_PER_THR * n_thr + 1) * n_cell);
      detail::lcx_check(lcx_cond_rates_read(pimpl->h, out.data(), n_cell, 0, reset ? 1 : 0));
    }
    void diag_cond_rate(cond_rate_t which, int t = 0)
    {
      int n_thr = 0;
      detail::lcx_check(lcx_cond_rates_info(pimpl->h, nullptr, &n_thr, nullptr, nullptr));
      detail::lcx_check(lcx_diag_cond_rate(pimpl->h, which == cond_rate_t::total_dm3 ? LCX_CDR_PER_THR * n_thr : LCX_CDR_PER_THR * t + int(which)));
    }
    // EXTENSION, no reference counterpart (include/lcx_move_rates.h): per-cell tally of what step_async's move carries into and out of a cell, down
    // and up through its levels and onto the ground, relative to up to LCX_MVR_MAX_THR increasing threshold radii (the first may be 0: every
    // droplet), filled by a pass of its own around the move while enabled.  move_rates: out[row * n_cell + cell] with row = 10 t + int(move_rate_t)
    // (resized to 10 K * n_cell), the numbers as doubles; reset zeroes the rows behind the read.  diag_move_rate fills outbuf() like a diag_*_mom
    // call.  A snapshot does not hold them: a restored object is disabled.  Not virtual, as above.
    void move_rates_enable(const std::vector<real_t> &r_thr)
    {
      std::vector<double> r(r_thr.begin(), r_thr.end());
      detail::lcx_check(lcx_move_rates_enable(pimpl->h, r.data(), int(r.size())));
    }
    void move_rates_disable() { detail::lcx_check(lcx_move_rates_disable(pimpl->h)); }
    unsigned long long move_rates_calls()
    {
      unsigned long long calls = 0;
      detail::lcx_check(lcx_move_rates_info(pimpl->h, nullptr, nullptr, nullptr, &calls));
      return calls;
    }
    void move_rates(std::vector<double> &out, bool reset = false)
    {
      size_t n_cell = 0; int n_thr = 0;
      detail::lcx_check(lcx_n_cell(pimpl->h, &n_cell));
      detail::lcx_check(lcx_move_rates_info(pimpl->h, nullptr, &n_thr, nullptr, nullptr));
      out.resize(size_t(LCX_MVR_PER_THR * n_thr) * n_cell);
      detail::lcx_check(lcx_move_rates_read(pimpl->h, out.data(), n_cell, 0, reset ? 1 : 0));
    }
    void diag_move_rate(move_rate_t which, int t = 0) { detail::lcx_check(lcx_diag_move_rate(pimpl->h, LCX_MVR_PER_THR * t + int(which))); }
    // EXTENSION, no reference counterpart (include/lcx_track.h): tracked super-droplets.  track_enable makes room for max_tracked droplets and
    // `capacity` samples (every > 0: every every-th step_async ends in a sample); track_select marks droplets that satisfy every clause of
    // `sel` (a diag_req_t's clauses, ANDed; its count is not read) and lie in box = {x0, x1, y0, y1, z0, z1} (empty: anywhere), at most
    // max_count of them, spread over the storage, and returns how many it took; track_sample takes one sample now; track reads the samples
    // held.  A snapshot does not hold the marks: a restored object is disabled.  Not virtual, as above.
    void track_enable(size_t max_tracked, size_t capacity = 64, int every = 0) { detail::lcx_check(lcx_track_enable(pimpl->h, max_tracked, capacity, every)); }
    void track_disable() { detail::lcx_check(lcx_track_disable(pimpl->h)); }
    size_t track_select(const diag_req_t<real_t> &sel, const std::vector<double> &box = std::vector<double>(), size_t max_count = size_t(LCX_TRK_MAX))
    {
      std::vector<lcx_diag_clause_t> c;
      for (const auto &cl : sel.clauses) c.push_back(lcx_diag_clause_t{cl.sel, double(cl.lo), double(cl.hi)});
      if (!box.empty() && box.size() != 6) throw std::runtime_error("libcloudph++: track: box must hold six bounds (x0, x1, y0, y1, z0, z1)");
      size_t got = 0;
      detail::lcx_check(lcx_track_select(pimpl->h, c.data(), int(c.size()), box.empty() ? nullptr : box.data(), max_count, &got));
      return got;
    }
    size_t track_select_slots(const std::vector<unsigned long long> &slots)
    {
      size_t got = 0;
      detail::lcx_check(lcx_track_select_slots(pimpl->h, slots.data(), slots.size(), &got));
      return got;
    }
    void track_sample() { detail::lcx_check(lcx_track_sample(pimpl->h)); }
    // enabled, max_tracked, n_tracked, capacity, n_samples, dropped, every, scans: any pointer may be null
    void track_info(int *enabled, size_t *max_tracked = nullptr, size_t *n_tracked = nullptr, size_t *capacity = nullptr, size_t *n_samples = nullptr,
                    unsigned long long *dropped = nullptr, int *every = nullptr, unsigned long long *scans = nullptr)
    { detail::lcx_check(lcx_track_info(pimpl->h, enabled, max_tracked, n_tracked, capacity, n_samples, dropped, every, scans)); }
    void track(track_record_t &out, bool reset = false)
    {
      detail::lcx_check(lcx_track_info(pimpl->h, nullptr, nullptr, &out.n_tracked, nullptr, &out.n_samples, nullptr, nullptr, nullptr));
      out.rec.assign(out.n_samples * size_t(LCX_TRK_FIELDS) * out.n_tracked, 0.);
      out.steps.assign(out.n_samples, 0ull); out.time.assign(out.n_samples, 0.);
      size_t got = 0;
      detail::lcx_check(lcx_track_read(pimpl->h, out.rec.data(), size_t(LCX_TRK_FIELDS) * out.n_tracked, out.n_tracked, out.steps.data(), out.time.data(),
                                       out.n_samples, &got, 0, reset ? 1 : 0));
    }
    // EXTENSION (include/lcx_track_budget.h): every tracked droplet's growth split into condensation, collection and chemistry, and its
    // collisions counted.  Needs track_enable; every sample taken while it is on also holds a row of the seven accumulators.
    void track_budget_enable() { detail::lcx_check(lcx_track_budget_enable(pimpl->h)); }
    void track_budget_disable() { detail::lcx_check(lcx_track_budget_disable(pimpl->h)); }
    void track_budget_info(int *enabled, unsigned long long *cond_passes = nullptr, unsigned long long *chem_passes = nullptr,
                           unsigned long long *coal_passes = nullptr)
    { detail::lcx_check(lcx_track_budget_info(pimpl->h, enabled, cond_passes, chem_passes, coal_passes)); }
    void track_budget(track_budget_t &out)
    {
      detail::lcx_check(lcx_track_info(pimpl->h, nullptr, nullptr, &out.n_tracked, nullptr, &out.n_samples, nullptr, nullptr, nullptr));
      out.rows.assign(std::max<size_t>(out.n_samples * size_t(LCX_TRB_FIELDS) * out.n_tracked, 1), 0.);
      out.acc.assign(std::max<size_t>(size_t(LCX_TRB_FIELDS) * out.n_tracked, 1), 0.);
      size_t got = 0;
      detail::lcx_check(lcx_track_budget_read(pimpl->h, out.rows.data(), size_t(LCX_TRB_FIELDS) * out.n_tracked, out.n_tracked, out.n_samples, &got,
                                              out.acc.data(), out.n_tracked, 0));
    }
    // EXTENSION (include/lcx_dump.h): the chosen fields of every droplet that satisfies every clause of `sel` (as track_select reads it) and
    // lies in box, in storage order and as doubles: one vector per field, each of n_written elements.  max_count == 0: everything (the call
    // counts first); otherwise at most max_count droplets, every stride-th of the n_qualifying.  The object is only read.
    std::vector<std::vector<double>> dump(const diag_req_t<real_t> &sel, const std::vector<double> &box, const std::vector<dump_field_t> &fields,
                                          size_t max_count = 0, size_t *n_qualifying = nullptr, unsigned long long *stride = nullptr)
    {
      std::vector<lcx_diag_clause_t> c;
      for (const auto &cl : sel.clauses) c.push_back(lcx_diag_clause_t{cl.sel, double(cl.lo), double(cl.hi)});
      if (!box.empty() && box.size() != 6) throw std::runtime_error("libcloudph++: dump: box must hold six bounds (x0, x1, y0, y1, z0, z1)");
      const double *b = box.empty() ? nullptr : box.data();
      std::vector<int> f(fields.begin(), fields.end());
      size_t Q = 0, written = 0;
      if (max_count == 0) {
        detail::lcx_check(lcx_dump(pimpl->h, c.data(), int(c.size()), b, f.data(), int(f.size()), nullptr, 0, 0, 0, &Q, nullptr, nullptr));
        max_count = std::max<size_t>(Q, 1);
      }
      std::vector<double> flat(f.size() * max_count);
      detail::lcx_check(lcx_dump(pimpl->h, c.data(), int(c.size()), b, f.data(), int(f.size()), flat.data(), max_count, max_count, 0, &Q, &written, stride));
      if (n_qualifying) *n_qualifying = Q;
      std::vector<std::vector<double>> out(f.size());
      for (size_t k = 0; k < f.size(); ++k) out[k].assign(flat.begin() + k * max_count, flat.begin() + k * max_count + written);
      return out;
    }
    // EXTENSION, no reference counterpart (include/lcx_coal_log.h): every coalescence event -- the two droplets, their sizes and
    // multiplicities before it, the collision count, the product -- appended to a list of `capacity` events on the device by the
    // coalescence kernels while enabled; r_min > 0 keeps the events whose product has a wet radius of at least r_min.  coal_log: one
    // vector per coal_log_field_t, each of `held` elements, in no particular order; reset empties the log behind the read.  A snapshot
    // does not hold it: a restored object has it disabled.  Not virtual: particles_proto_t stays the reference's.
    struct coal_log_info_t { bool enabled; size_t capacity; double r_min; unsigned long long held, seen, launches; };
    void coal_log_enable(size_t capacity, real_t r_min = 0) { detail::lcx_check(lcx_coal_log_enable(pimpl->h, capacity, double(r_min))); }
    void coal_log_disable() { detail::lcx_check(lcx_coal_log_disable(pimpl->h)); }
    coal_log_info_t coal_log_info()
    {
      int en = 0;
      coal_log_info_t i{};
      detail::lcx_check(lcx_coal_log_info(pimpl->h, &en, &i.capacity, &i.r_min, &i.held, &i.seen, &i.launches));
      i.enabled = en != 0;
      return i;
    }
    std::vector<std::vector<double>> coal_log(bool reset = false)
    {
      unsigned long long held = 0;
      detail::lcx_check(lcx_coal_log_info(pimpl->h, nullptr, nullptr, nullptr, &held, nullptr, nullptr));
      const size_t room = std::max<size_t>(size_t(held), 1);
      size_t written = 0;
      std::vector<double> flat(size_t(LCX_CLG_FIELDS) * room);
      detail::lcx_check(lcx_coal_log_read(pimpl->h, flat.data(), room, room, 0, reset ? 1 : 0, &written, nullptr));
      std::vector<std::vector<double>> out(LCX_CLG_FIELDS);
      for (size_t k = 0; k < size_t(LCX_CLG_FIELDS); ++k) out[k].assign(flat.begin() + k * room, flat.begin() + k * room + written);
      return out;
    }

  private:
    static lcx_opts_t conv(const opts_t<real_t> &o)
    {
      lcx_opts_t c;
      lcx_opts_default(&c);
      c.adve = o.adve; c.sedi = o.sedi; c.subs = o.subs; c.cond = o.cond; c.coal = o.coal; c.src = o.src; c.rlx = o.rlx; c.rcyc = o.rcyc;
      c.turb_adve = o.turb_adve; c.turb_cond = o.turb_cond; c.turb_coal = o.turb_coal; c.ice_nucl = o.ice_nucl;
      c.chem_dsl = o.chem_dsl; c.chem_dsc = o.chem_dsc; c.chem_rct = o.chem_rct; c.RH_max = o.RH_max; c.dt = o.dt;
      return c;
    }
  };

  // particles_t<real_t, multi_HIP>: one object over all (or opts_init.dev_count) devices of the process, the reference's
  // particles_t<real_t, multi_CUDA> (reference: lgrngn/particles.hpp:246-340, src/particles_multi_gpu_*.ipp).  Same virtuals;
  // arrays are the GLOBAL ones, outbuf() the global field, get_attr() throws (particles_multi_gpu_ctor.ipp:53-57), opts.rcyc is
  // refused (particles_multi_gpu_step.ipp:63-65).  The slabs, worker threads and the device-driven exchange live inside the
  // library (libcloudphxx_amd/csrc/lcx_multi.hpp).
  template <typename real_t>
  struct particles_t<real_t, multi_HIP> : particles_t<real_t, HIP>
  {
    explicit particles_t(opts_init_t<real_t> oi) : particles_t<real_t, HIP>(oi, 0, true)
    {
      int n = 0;
      detail::lcx_check(lcx_multi_dev_count(this->pimpl->h, &n));
      this->pimpl->opts_init.dev_count = n;              // the reference stores the actual count in the live copy
    }
  };
  // the reference's own backend names: a driver that instantiates or dynamic_casts to them gets the HIP objects
  template <typename real_t>
  struct particles_t<real_t, CUDA> : particles_t<real_t, HIP>
  { explicit particles_t(opts_init_t<real_t> oi, int n_x_tot = 0) : particles_t<real_t, HIP>(oi, n_x_tot) {} };
  template <typename real_t>
  struct particles_t<real_t, multi_CUDA> : particles_t<real_t, multi_HIP>
  { explicit particles_t(opts_init_t<real_t> oi) : particles_t<real_t, multi_HIP>(oi) {} };
} }
