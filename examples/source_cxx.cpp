// The aerosol source through the reference's C++ interface: a 2 x 2 box in which only the lower row gets new
// super-droplets (opts_init.src_type = simple, opts.src_dry_distros), 100 steps with one firing every 50.  Prints
// the super-droplet count of the four cells (x-major: lower, upper, lower, upper); tests/test_sources_cxx.py checks it.
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
  opts_init_t<real_t> oi;
  const kappa_rd_insol_t<real_t> key(.61, 0.);
  oi.dry_distros.emplace(key, std::make_shared<lognormal>(.02e-6, 1.4, 60e6));
  oi.coal_switch = oi.sedi_switch = false;
  oi.dt = 1; oi.nx = 2; oi.nz = 2; oi.dx = oi.dz = 1; oi.x1 = 2; oi.z1 = 2;
  oi.sd_conc = 1024; oi.n_sd_max = 6144;
  oi.src_type = src_t::simple;
  oi.src_x0 = 0; oi.src_x1 = 2; oi.src_z0 = 0; oi.src_z1 = 1;
  std::unique_ptr<particles_proto_t<real_t>> prtcls(factory<real_t>(HIP, oi));
  std::vector<real_t> th(4, 300.), rv(4, .01), rhod(4, 1.);
  const std::vector<ptrdiff_t> s{2, 1};
  prtcls->init(arrinfo_t<real_t>(th.data(), s), arrinfo_t<real_t>(rv.data(), s), arrinfo_t<real_t>(rhod.data(), s));
  opts_t<real_t> opts;
  opts.adve = opts.sedi = opts.cond = opts.coal = false;
  opts.src = true;
  opts.src_dry_distros.emplace(key, std::make_tuple(std::make_shared<lognormal>(.05e-6, 1.4, 60e4), 512, 50));
  for (int step = 0; step < 100; ++step) {
    prtcls->step_sync(opts, arrinfo_t<real_t>(th.data(), s), arrinfo_t<real_t>(rv.data(), s), arrinfo_t<real_t>(rhod.data(), s));
    prtcls->step_async(opts);
  }
  prtcls->diag_all(); prtcls->diag_sd_conc();
  const real_t *out = prtcls->outbuf();
  std::printf("%g %g %g %g\n", out[0], out[1], out[2], out[3]);
  return 0;
}
