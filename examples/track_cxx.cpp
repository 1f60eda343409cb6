// One droplet's story.  A small 2-D box of drizzling cloud in a sinking, drifting flow (the box of move_rates_cxx.cpp) spins up for a few
// steps, then marks up to eight drizzle-sized droplets (wet radius >= 15 um) in the second level of the box -- near cloud base -- with
// track_select (include/lcx_track.h) and runs eight more steps with every = 1: each step ends in a sample of the marked droplets, queued
// behind the step with no host wait.  The samples are read once, at the end, and the example prints per step the radius, the height and
// the relative humidity that the first marked droplet saw, until it reaches the ground (tests/test_track_cxx.py).
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
  const int nx = 4, nz = 4, n_cell = nx * nz, spin_up = 4, steps = 8;
  opts_init_t<real_t> oi;
  // few, large condensation nuclei in very moist air: the droplets grow to tens of micrometres within the first steps
  oi.dry_distros.emplace(kappa_rd_insol_t<real_t>(.61, 0.), std::make_shared<lognormal>(.2e-6, 1.6, 10e6));
  oi.kernel = kernel_t::geometric; oi.terminal_velocity = vt_t::beard77fast;
  oi.dt = 2; oi.nx = nx; oi.nz = nz; oi.dx = oi.dz = 10; oi.x1 = nx * 10; oi.z1 = nz * 10; oi.sd_conc = 64; oi.n_sd_max = 64 * n_cell;
  particles_t<real_t, HIP> prtcls(oi);
  // the air drifts to the right by 0.3 cells a step and sinks by 0.2
  std::vector<real_t> th(n_cell, 300.), rv(n_cell, .0235), rhod(n_cell, 1.), Cx((nx + 1) * nz, .3), Cz(nx * (nz + 1), -.2);
  const std::vector<ptrdiff_t> s{nz, 1}, sz{nz + 1, 1};
  auto a = [&](std::vector<real_t> &v, const std::vector<ptrdiff_t> &st) { return arrinfo_t<real_t>(v.data(), st); };
  prtcls.init(a(th, s), a(rv, s), a(rhod, s), arrinfo_t<real_t>(), a(Cx, s), arrinfo_t<real_t>(), a(Cz, sz));

  opts_t<real_t> opts;                                      // everything on: condensation, coalescence, advection, sedimentation
  for (int step = 0; step < spin_up; ++step) { prtcls.step_sync(opts, a(th, s), a(rv, s), a(rhod, s)); prtcls.step_async(opts); }

  prtcls.track_enable(8, steps, 1);                         // eight droplets, eight samples, one at the end of every step
  const size_t got = prtcls.track_select(diag_req_t<real_t>().wet_rng(15e-6, 1), {0., oi.x1, 0., 0., oi.z1 / 4, oi.z1 / 2}, 8);
  std::printf("selected %zu\n", got);
  for (int step = 0; step < steps; ++step) { prtcls.step_sync(opts, a(th, s), a(rv, s), a(rhod, s)); prtcls.step_async(opts); }

  track_record_t rec;
  prtcls.track(rec);
  for (size_t i = 0; i < rec.n_samples && rec.n_tracked; ++i) {
    if (rec.at(i, trk_n, 0) == 0) { std::printf("step %llu time %g gone\n", rec.steps[i], rec.time[i]); continue; }
    std::printf("step %llu time %g n %.0f r_um %.6f z %.6f cell %.0f RH %.6f\n", rec.steps[i], rec.time[i], rec.at(i, trk_n, 0),
                1e6 * std::sqrt(rec.at(i, trk_rw2, 0)), rec.at(i, trk_z, 0), rec.at(i, trk_cell, 0), rec.at(i, trk_RH, 0));
  }
  unsigned long long scans = 0, dropped = 0;
  prtcls.track_info(nullptr, nullptr, nullptr, nullptr, nullptr, &dropped, nullptr, &scans);
  std::printf("samples %zu dropped %llu scans %llu\n", rec.n_samples, dropped, scans);
  return 0;
}
