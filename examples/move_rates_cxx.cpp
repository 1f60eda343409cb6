// Transport, the third term of a cell's budget.  A small 2-D box of drizzling cloud in a sinking, drifting flow runs a few full steps
// (condensation, coalescence, advection, sedimentation) with the move rates on (include/lcx_move_rates.h) at two thresholds, 0 (every
// droplet) and 25 um (rain), and the condensation and collision rates at 25 um.  After each step all three are read and reset, and the
// example prints the two closures that the move rates add: at the ground, the precipitation map's sum beside the puddle's increase
// (particles, exactly; liquid volume); and for one cell the change of the number of rain drops as the classic calls see it
// (diag_wet_rng(25 um, 1) + diag_wet_mom(0)) beside condensation's crossings + collisions + arrivals - departures
// (tests/test_move_rates_cxx.py).
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
  const real_t r_thr = 25e-6, dv = 10 * 10 * 1, rhod0 = 1.;
  opts_init_t<real_t> oi;
  // few, large condensation nuclei in very moist air: the droplets grow to tens of micrometres within the first steps
  oi.dry_distros.emplace(kappa_rd_insol_t<real_t>(.61, 0.), std::make_shared<lognormal>(.2e-6, 1.6, 10e6));
  oi.kernel = kernel_t::geometric; oi.terminal_velocity = vt_t::beard77fast;
  oi.dt = 2; oi.nx = nx; oi.nz = nz; oi.dx = oi.dz = 10; oi.x1 = nx * 10; oi.z1 = nz * 10; oi.sd_conc = 64; oi.n_sd_max = 64 * n_cell;
  particles_t<real_t, HIP> prtcls(oi);
  // the air drifts to the right by 0.3 cells a step and sinks by 0.2
  std::vector<real_t> th(n_cell, 300.), rv(n_cell, .0235), rhod(n_cell, rhod0), Cx((nx + 1) * nz, .3), Cz(nx * (nz + 1), -.2);
  const std::vector<ptrdiff_t> s{nz, 1}, sz{nz + 1, 1};
  auto a = [&](std::vector<real_t> &v, const std::vector<ptrdiff_t> &st) { return arrinfo_t<real_t>(v.data(), st); };
  prtcls.init(a(th, s), a(rv, s), a(rhod, s), arrinfo_t<real_t>(), a(Cx, s), arrinfo_t<real_t>(), a(Cz, sz));
  prtcls.move_rates_enable(std::vector<real_t>{0., r_thr});
  prtcls.cond_rates_enable(std::vector<real_t>{r_thr});
  prtcls.coal_rates_enable(r_thr);

  opts_t<real_t> opts;                                      // everything on: condensation, coalescence, advection, sedimentation
  auto rain = [&]() { prtcls.diag_wet_rng(r_thr, 1); prtcls.diag_wet_mom(0); return double(prtcls.outbuf()[cell]) * rhod0 * dv; };
  using libcloudphxx::common::output_t;
  std::vector<double> mv, cd, cl;
  double n0 = rain();
  auto pud0 = prtcls.diag_puddle();
  for (int step = 0; step < steps; ++step) {
    prtcls.step_sync(opts, a(th, s), a(rv, s), a(rhod, s));
    prtcls.step_async(opts);
    prtcls.move_rates(mv, true);                            // this step's tally; the rows start the next step from zero
    prtcls.cond_rates(cd, true);
    prtcls.coal_rates(cl, true);
    const double n1 = rain();
    auto pud1 = prtcls.diag_puddle();
    auto mvr = [&](move_rate_t w, int t, int c) { return mv[size_t(int(move_rate_t::per_thr) * t + int(w)) * n_cell + c]; };
    auto cdr = [&](cond_rate_t w) { return cd[size_t(w) * n_cell + cell]; };
    auto clr = [&](coal_rate_t w) { return cl[size_t(w) * n_cell + cell]; };
    double precip_n = 0, precip_m3 = 0;
    for (int c = 0; c < n_cell; ++c) { precip_n += mvr(move_rate_t::precip_n, 0, c); precip_m3 += mvr(move_rate_t::precip_m3, 0, c); }
    const double in = mvr(move_rate_t::in_n, 1, cell), out = mvr(move_rate_t::out_n, 1, cell);
    std::printf("step %d precip_n %.0f puddle_n %.0f precip_vol %.9e puddle_vol %.9e rain_in %.0f rain_out %.0f drops_tallied %.0f drops_seen %.0f\n",
                step + 1, precip_n, double(pud1[output_t::outprtcl_num]) - double(pud0[output_t::outprtcl_num]),
                4. / 3 * M_PI * precip_m3, double(pud1[output_t::outliq_vol]) - double(pud0[output_t::outliq_vol]), in, out,
                cdr(cond_rate_t::up_n) - cdr(cond_rate_t::down_n) + clr(coal_rate_t::acnv_nr) - clr(coal_rate_t::self_rain_n) + in - out, n1 - n0);
    n0 = n1; pud0 = pud1;
  }
  std::printf("moves_tallied_since_reset %llu\n", prtcls.move_rates_calls());
  return 0;
}
