// Who collided with whom.  The drizzling 2-D box of coal_rates_cxx.cpp runs a few steps with the collision log switched on (an extension
// of the concrete class, include/lcx_coal_log.h) beside the collision rates, both at 25 um: the log holds every coalescence event -- the two
// droplets, their sizes and multiplicities before it, the collision count, the product --, the rates hold seven sums of them per cell.
// After each step both are read and reset; the example prints the number of events and counts autoconversion (two cloud droplets make a
// rain drop) from the log by the table of include/lcx_coal_rates.h, next to what the rates say (tests/test_coal_log_cxx.py).
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
  const real_t r_thr = 25e-6, lo = r_thr * r_thr;           // (double: the bound that the kernels compare rw2 with is the square itself)
  opts_init_t<real_t> oi;
  oi.dry_distros.emplace(kappa_rd_insol_t<real_t>(.61, 0.), std::make_shared<lognormal>(.2e-6, 1.6, 10e6));
  oi.kernel = kernel_t::geometric; oi.terminal_velocity = vt_t::beard77fast;
  oi.dt = 2; oi.nx = nx; oi.nz = nz; oi.dx = oi.dz = 10; oi.x1 = nx * 10; oi.z1 = nz * 10; oi.sd_conc = 64; oi.n_sd_max = 64 * n_cell;
  particles_t<real_t, HIP> prtcls(oi);
  std::vector<real_t> th(n_cell, 300.), rv(n_cell, .0235), rhod(n_cell, 1.), Cx((nx + 1) * nz, .1), Cz(nx * (nz + 1), 0.);
  const std::vector<ptrdiff_t> s{nz, 1}, sz{nz + 1, 1};
  auto a = [&](std::vector<real_t> &v, const std::vector<ptrdiff_t> &st) { return arrinfo_t<real_t>(v.data(), st); };
  prtcls.init(a(th, s), a(rv, s), a(rhod, s), arrinfo_t<real_t>(), a(Cx, s), arrinfo_t<real_t>(), a(Cz, sz));
  prtcls.coal_rates_enable(r_thr);
  prtcls.coal_log_enable(size_t(64) * n_cell);              // (a droplet is in one pair per launch at most: a step cannot log more)

  opts_t<real_t> opts;
  std::vector<double> acc;
  auto total = [&](coal_rate_t w) { double t = 0; for (int c = 0; c < n_cell; ++c) t += acc[size_t(w) * n_cell + c]; return t; };
  auto row = [](const std::vector<std::vector<double>> &ev, coal_log_field_t f) -> const std::vector<double> & { return ev[size_t(f)]; };
  for (int step = 0; step < steps; ++step) {
    prtcls.step_sync(opts, a(th, s), a(rv, s), a(rhod, s));
    prtcls.step_async(opts);
    const auto info = prtcls.coal_log_info();
    const auto ev = prtcls.coal_log(true);                  // this step's events; the log starts the next step empty
    prtcls.coal_rates(acc, true);
    double acnv_nr = 0, acnv_nc = 0, largest = 0;
    for (size_t i = 0; i < ev[0].size(); ++i) {
      const double m = row(ev, coal_log_field_t::n_r)[i], col_no = row(ev, coal_log_field_t::col_no)[i], rw2_new = row(ev, coal_log_field_t::rw2_new)[i];
      if (row(ev, coal_log_field_t::rw2_d)[i] < lo && row(ev, coal_log_field_t::rw2_r)[i] < lo && rw2_new >= lo) { acnv_nr += m; acnv_nc += (col_no + 1) * m; }
      largest = std::fmax(largest, std::sqrt(rw2_new));
    }
    std::printf("step %d events %zu seen %llu acnv_nr_log %.0f acnv_nr_rates %.0f acnv_nc_log %.0f acnv_nc_rates %.0f largest_product_um %.3f\n", step + 1,
                ev[0].size(), info.seen, acnv_nr, total(coal_rate_t::acnv_nr), acnv_nc, total(coal_rate_t::acnv_nc), largest * 1e6);
  }
  const auto end = prtcls.coal_log_info();
  std::printf("launches %llu held_after_reset %llu\n", end.launches, end.held);
  return 0;
}
