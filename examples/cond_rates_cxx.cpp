// A cell's rain-water budget, term by term.  A small 2-D box of drizzling cloud runs a few steps of condensation and coalescence (no transport)
// with both tallies switched on at one threshold radius of 25 um: the condensation rates (include/lcx_cond_rates.h: growth of the rain drops,
// water carried across the threshold by droplets growing or shrinking past it) and the collision rates (include/lcx_coal_rates.h:
// autoconversion, accretion).  After each step both are read and reset, and for one cell the sum of the five terms is printed beside the
// change of the cell's rain water as the classic calls see it (diag_wet_rng(25 um, 1) + diag_wet_mom(3)), with the exact budget of the
// number of rain drops (tests/test_cond_rates_cxx.py).
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>
#include <libcloudph++/lgrngn/factory.hpp>

using namespace libcloudphxx::lgrngn;
typedef double real_t;

struct lognormal : libcloudphxx::common::unary_function<real_t>
{
  real_t mean_r, stdev, n_tot;
  lognormal(real_t m, real_t s, real_t n) : mean_r(m), stdev(s), n_tot(n) {}
  real_t funval(const real_t lnr) const override
  { return n_tot * std::exp(-std::pow((lnr - std::log(mean_r)), 2) / 2 / std::pow(std::log(stdev), 2)) / std::log(stdev) / std::sqrt(2 * M_PI); }
};

int main()
{
  const int nx = 4, nz = 4, n_cell = nx * nz, steps = 8, cell = 5;
  const real_t r_thr = 25e-6, rho_w = 1e3, dv = 10 * 10 * 1, rhod0 = 1.;
  opts_init_t<real_t> oi;
  // few, large condensation nuclei in very moist air: the droplets grow to tens of micrometres within the first steps
  oi.dry_distros.emplace(kappa_rd_insol_t<real_t>(.61, 0.), std::make_shared<lognormal>(.2e-6, 1.6, 10e6));
  oi.kernel = kernel_t::geometric; oi.terminal_velocity = vt_t::beard77fast;
  oi.dt = 2; oi.nx = nx; oi.nz = nz; oi.dx = oi.dz = 10; oi.x1 = nx * 10; oi.z1 = nz * 10; oi.sd_conc = 64; oi.n_sd_max = 64 * n_cell;
  particles_t<real_t, HIP> prtcls(oi);
  std::vector<real_t> th(n_cell, 300.), rv(n_cell, .0235), rhod(n_cell, rhod0), Cx((nx + 1) * nz, 0.), Cz(nx * (nz + 1), 0.);
  const std::vector<ptrdiff_t> s{nz, 1}, sz{nz + 1, 1};
  auto a = [&](std::vector<real_t> &v, const std::vector<ptrdiff_t> &st) { return arrinfo_t<real_t>(v.data(), st); };
  prtcls.init(a(th, s), a(rv, s), a(rhod, s), arrinfo_t<real_t>(), a(Cx, s), arrinfo_t<real_t>(), a(Cz, sz));
  prtcls.cond_rates_enable(std::vector<real_t>{r_thr});
  prtcls.coal_rates_enable(r_thr);

  opts_t<real_t> opts;
  opts.adve = opts.sedi = false;                            // the budget of a cell without its transport terms
  // the cell's rain as the classic calls see it: (number of drops, sum n r^3)
  auto rain = [&](double &n_rain, double &m3_rain) {
    prtcls.diag_wet_rng(r_thr, 1); prtcls.diag_wet_mom(0); n_rain = double(prtcls.outbuf()[cell]) * rhod0 * dv;
    prtcls.diag_wet_rng(r_thr, 1); prtcls.diag_wet_mom(3); m3_rain = double(prtcls.outbuf()[cell]) * rhod0 * dv;
  };
  std::vector<double> cd, cl;
  double n0, m0, n1, m1;
  rain(n0, m0);
  for (int step = 0; step < steps; ++step) {
    prtcls.step_sync(opts, a(th, s), a(rv, s), a(rhod, s));
    prtcls.step_async(opts);
    prtcls.cond_rates(cd, true);                            // this step's tally; the rows start the next step from zero
    prtcls.coal_rates(cl, true);
    rain(n1, m1);
    auto cdr = [&](cond_rate_t w) { return cd[size_t(w) * n_cell + cell]; };
    auto clr = [&](coal_rate_t w) { return cl[size_t(w) * n_cell + cell]; };
    const double to_mass = 4. / 3 * M_PI * rho_w;           // sum n r^3 -> kg
    const double growth = cdr(cond_rate_t::above_dm3), up = cdr(cond_rate_t::up_m3), down = cdr(cond_rate_t::down_m3);
    const double acnv = clr(coal_rate_t::acnv_m3), accr = clr(coal_rate_t::accr_m3);
    std::printf("step %d growth_kg %.6e up_kg %.6e down_kg %.6e acnv_kg %.6e accr_kg %.6e sum_kg %.9e seen_kg %.9e drops_tallied %.0f drops_seen %.0f\n",
                step + 1, to_mass * growth, to_mass * up, to_mass * down, to_mass * acnv, to_mass * accr,
                to_mass * (growth + up - down + acnv + accr), to_mass * (m1 - m0),
                cdr(cond_rate_t::up_n) - cdr(cond_rate_t::down_n) + clr(coal_rate_t::acnv_nr) - clr(coal_rate_t::self_rain_n), n1 - n0);
    n0 = n1; m0 = m1;
  }
  // the condensation's total as a specific quantity per cell, like a diag_*_mom result (here: nothing since the last reset)
  prtcls.diag_cond_rate(cond_rate_t::total_dm3);
  std::printf("outbuf_after_reset %.1f\n", double(prtcls.outbuf()[cell]));
  return 0;
}
