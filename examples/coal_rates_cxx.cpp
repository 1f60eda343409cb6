// How rain forms, read off the collisions themselves.  A 2-D box of drizzling cloud runs a few steps with the collision rates switched on
// (an extension of the concrete class, include/lcx_coal_rates.h): every collision event is classed by the threshold radius of 25 um as
// autoconversion (two cloud droplets make a rain drop), accretion (a rain drop collects cloud droplets) or self-collection, and summed per
// cell inside the coalescence kernels.  After each step the accumulators are read and reset, and the domain's autoconversion and accretion
// mass rates are printed -- what a bulk scheme parametrises (blk_1m / blk_2m: acnv, accr) -- with the numbers of droplets they took from
// the cloud (tests/test_coal_rates_cxx.py).
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
  const int nx = 6, nz = 5, n_cell = nx * nz, steps = 8;
  const real_t r_thr = 25e-6, rho_w = 1e3;
  opts_init_t<real_t> oi;
  // few, large condensation nuclei in very moist air: the droplets grow to tens of micrometres within the first steps
  oi.dry_distros.emplace(kappa_rd_insol_t<real_t>(.61, 0.), std::make_shared<lognormal>(.2e-6, 1.6, 10e6));
  oi.kernel = kernel_t::geometric; oi.terminal_velocity = vt_t::beard77fast;
  oi.dt = 2; oi.nx = nx; oi.nz = nz; oi.dx = oi.dz = 10; oi.x1 = nx * 10; oi.z1 = nz * 10; oi.sd_conc = 64; oi.n_sd_max = 64 * n_cell;
  particles_t<real_t, HIP> prtcls(oi);
  std::vector<real_t> th(n_cell, 300.), rv(n_cell, .0235), rhod(n_cell, 1.), Cx((nx + 1) * nz, .1), Cz(nx * (nz + 1), 0.);
  const std::vector<ptrdiff_t> s{nz, 1}, sz{nz + 1, 1};
  auto a = [&](std::vector<real_t> &v, const std::vector<ptrdiff_t> &st) { return arrinfo_t<real_t>(v.data(), st); };
  prtcls.init(a(th, s), a(rv, s), a(rhod, s), arrinfo_t<real_t>(), a(Cx, s), arrinfo_t<real_t>(), a(Cz, sz));
  prtcls.coal_rates_enable(r_thr);

  opts_t<real_t> opts;
  std::vector<double> acc;
  auto total = [&](coal_rate_t w) { double t = 0; for (int c = 0; c < n_cell; ++c) t += acc[size_t(w) * n_cell + c]; return t; };
  for (int step = 0; step < steps; ++step) {
    prtcls.step_sync(opts, a(th, s), a(rv, s), a(rhod, s));
    prtcls.step_async(opts);
    prtcls.coal_rates(acc, true);                           // this step's events; the accumulators start the next step from zero
    const double to_mass = 4. / 3 * M_PI * rho_w / oi.dt;   // sum n r^3 per step -> kg / s
    std::printf("step %d acnv_kg_per_s %.6e accr_kg_per_s %.6e acnv_droplets %.0f accr_droplets %.0f self_cloud %.0f self_rain %.0f\n", step + 1,
                to_mass * total(coal_rate_t::acnv_m3), to_mass * total(coal_rate_t::accr_m3), total(coal_rate_t::acnv_nc), total(coal_rate_t::accr_nc),
                total(coal_rate_t::self_cloud_n), total(coal_rate_t::self_rain_n));
  }
  // the same accumulator as a specific quantity per cell, like a diag_*_mom result (here: nothing since the last reset)
  prtcls.diag_coal_rate(coal_rate_t::accr_m3);
  std::printf("outbuf_after_reset %.1f\n", double(prtcls.outbuf()[0]));
  return 0;
}
