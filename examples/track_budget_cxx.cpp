// Where one droplet's water came from.  The drizzling 2-D box of track_cxx.cpp spins up for a few steps, then marks up to thirty-two
// drizzle-sized droplets (wet radius >= 15 um) in the upper half of the box, switches the budget on (include/lcx_track_budget.h) and runs
// six more steps with every = 1.  After the last step it prints, for the first marked droplet that is still alive: its radius, the share
// of its r^3 growth since it was marked that came from condensation and the share that it collected, and the number of collisions it
// took part in (tests/test_track_budget_cxx.py).
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
  const int nx = 4, nz = 4, n_cell = nx * nz, spin_up = 4, steps = 6;
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

  prtcls.track_enable(32, steps, 1);                        // thirty-two droplets, six samples, one at the end of every step
  prtcls.track_budget_enable();
  const size_t got = prtcls.track_select(diag_req_t<real_t>().wet_rng(15e-6, 1), {0., oi.x1, 0., 0., oi.z1 / 2, oi.z1}, 32);
  std::printf("selected %zu\n", got);
  for (int step = 0; step < steps; ++step) { prtcls.step_sync(opts, a(th, s), a(rv, s), a(rhod, s)); prtcls.step_async(opts); }

  track_record_t rec;
  track_budget_t bud;
  prtcls.track(rec);
  prtcls.track_budget(bud);
  unsigned long long cond_passes = 0, coal_passes = 0;
  prtcls.track_budget_info(nullptr, &cond_passes, nullptr, &coal_passes);
  std::printf("samples %zu cond_passes %llu coal_passes %llu\n", bud.n_samples, cond_passes, coal_passes);
  const size_t last = rec.n_samples - 1;
  for (size_t k = 0; k < rec.n_tracked; ++k) {
    if (rec.at(last, trk_n, k) == 0) continue;
    const double cond = bud.now(trb_cond_dr3, k), coal = bud.now(trb_coal_dr3, k), all = cond + coal;
    // (closure: the first sample's r^3 plus what the rows say was added since is the last sample's r^3)
    const double w0 = rec.at(0, trk_rw2, k), grown = bud.at(last, trb_cond_dr3, k) + bud.at(last, trb_coal_dr3, k) - bud.at(0, trb_cond_dr3, k) - bud.at(0, trb_coal_dr3, k);
    std::printf("index %zu r_um %.9f r_um_from_budget %.9f\n", k, 1e6 * std::sqrt(rec.at(last, trk_rw2, k)), 1e6 * std::cbrt(w0 * std::sqrt(w0) + grown));
    std::printf("dr3_um3 %.6e from_condensation %.12f collected %.12f\n", 1e18 * all, cond / all, coal / all);
    std::printf("collisions %.0f gains %.0f gives %.0f\n", bud.now(trb_coal_gains, k) + bud.now(trb_coal_gives, k), bud.now(trb_coal_gains, k),
                bud.now(trb_coal_gives, k));
    return 0;
  }
  std::printf("no marked droplet is alive\n");
  return 0;
}
