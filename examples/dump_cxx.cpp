// The droplets themselves.  A small 2-D box of drizzling cloud in a sinking, drifting flow (the box of track_cxx.cpp) runs for a few steps;
// then one call of dump (include/lcx_dump.h) hands over the multiplicity, the position, the squared wet radius and the cell of every droplet
// above 25 um in the lowest two levels -- filtered and gathered on the device, with nothing compacted or sorted on the way.  The example
// prints their count and the sum of n r^3 over them, summed on the host, beside the same quantity from the per-cell diagnostics
// (diag_wet_rng + diag_wet_mom(3), summed over the cells of those two levels and scaled back by dv rhod): it checks itself
// (tests/test_dump_cxx.py).
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
  const int nx = 4, nz = 4, n_cell = nx * nz, steps = 6;
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

  opts_t<real_t> opts;                                      // everything on: condensation, coalescence, advection, sedimentation
  for (int step = 0; step < steps; ++step) { prtcls.step_sync(opts, a(th, s), a(rv, s), a(rhod, s)); prtcls.step_async(opts); }

  // the dump comes first: it reads the storage as the step left it
  size_t Q = 0; unsigned long long stride = 0;
  const auto d = prtcls.dump(diag_req_t<real_t>().wet_rng(r_thr, 1), {0., oi.x1, 0., 0., 0., 2 * oi.dz}, {dmp_n, dmp_x, dmp_z, dmp_rw2, dmp_cell}, 0, &Q, &stride);
  double sum_dump = 0;
  bool in_levels = true;
  for (size_t i = 0; i < d[0].size(); ++i) {
    sum_dump += d[0][i] * std::pow(d[3][i], 1.5);
    in_levels = in_levels && int(d[4][i]) % nz < 2 && d[2][i] < 2 * oi.dz && d[1][i] >= 0 && d[1][i] < oi.x1;
  }
  prtcls.diag_wet_rng(r_thr, 1); prtcls.diag_wet_mom(3);
  double sum_diag = 0;
  for (int i = 0; i < nx; ++i) for (int k = 0; k < 2; ++k) sum_diag += double(prtcls.outbuf()[i * nz + k]) * rhod0 * dv;
  std::printf("dumped %zu of %zu stride %llu in_levels %d\n", d[0].size(), Q, stride, int(in_levels));
  std::printf("sum_n_r3 dump %.17g diag %.17g\n", sum_dump, sum_diag);
  return 0;
}
