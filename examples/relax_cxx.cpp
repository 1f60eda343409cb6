// Aerosol relaxation through the reference's C++ interface: a 2 x 2 box whose lower row is relaxed towards twice the initial
// spectrum (opts_init.rlx_switch, rlx_dry_distros, opts.rlx) with a time scale of twice the run: two steps, one firing.  Prints the
// super-droplet count of the four cells (x-major: lower, upper, lower, upper) and the lower-over-upper ratio of the 0th and 1st
// wet moments (1.5 expected); tests/test_relaxation_cxx.py checks them.
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
  const real_t kappa = .61;
  oi.dry_distros.emplace(kappa_rd_insol_t<real_t>(kappa, 0.), std::make_shared<lognormal>(.02e-6, 1.4, 60e6));
  oi.coal_switch = oi.sedi_switch = false;
  oi.dt = 1; oi.nx = 2; oi.nz = 2; oi.dx = oi.dz = 1; oi.x1 = 2; oi.z1 = 2;
  oi.aerosol_independent_of_rhod = true;
  oi.sd_conc = 1024; oi.n_sd_max = 8192;
  oi.rlx_switch = true;
  oi.rlx_bins = 1024; oi.rlx_sd_per_bin = 1; oi.rlx_timescale = 4; oi.supstp_rlx = 2;
  oi.rlx_dry_distros.emplace(kappa, std::make_tuple(std::make_shared<lognormal>(.02e-6, 1.4, 120e6), std::make_pair(real_t(0), real_t(2)),
                                                    std::make_pair(real_t(0), oi.dz)));
  std::unique_ptr<particles_proto_t<real_t>> prtcls(factory<real_t>(HIP, oi));
  std::vector<real_t> th(4, 300.), rv(4, .01), rhod(4, 1.);
  const std::vector<ptrdiff_t> s{2, 1};
  prtcls->init(arrinfo_t<real_t>(th.data(), s), arrinfo_t<real_t>(rv.data(), s), arrinfo_t<real_t>(rhod.data(), s));
  opts_t<real_t> opts;
  opts.adve = opts.sedi = opts.cond = opts.coal = false;
  opts.rlx = true;
  for (int step = 0; step < 2; ++step) {
    prtcls->step_sync(opts, arrinfo_t<real_t>(th.data(), s), arrinfo_t<real_t>(rv.data(), s), arrinfo_t<real_t>(rhod.data(), s));
    prtcls->step_async(opts);
  }
  prtcls->diag_all(); prtcls->diag_sd_conc();
  const real_t *out = prtcls->outbuf();
  std::printf("%g %g %g %g", out[0], out[1], out[2], out[3]);
  for (int k = 0; k < 2; ++k) {
    prtcls->diag_all(); prtcls->diag_wet_mom(k);
    out = prtcls->outbuf();
    std::printf(" %.6f", (out[0] + out[2]) / (out[1] + out[3]));
  }
  std::printf("\n");
  return 0;
}
