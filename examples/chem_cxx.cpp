// Aqueous chemistry through the reference's C++ interface: a 0-D parcel of 64 super-droplets at slight supersaturation with the trace
// gases of the kinematic chemistry case, ten steps of condensation with dissolution, dissociation and oxidation (opts_init.chem_switch,
// chem_rho, sstp_chem = 2; opts.chem_dsl / chem_dsc / chem_rct; ambient_chem in init and step_sync).  Prints the first moments of
// S_VI, H and SO2 (diag_chem) and the mixing ratios of SO2, H2O2 and O3 left in the air; tests/test_chemistry_cxx.py reproduces them
// through the Python mirror.
#include <cmath>
#include <cstdio>
#include <map>
#include <memory>
#include <vector>
#include <libcloudph++/lgrngn/factory.hpp>

using namespace libcloudphxx::lgrngn;
namespace chem = libcloudphxx::common::chem;
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
  oi.dry_distros.emplace(kappa_rd_insol_t<real_t>(.61, 0.), std::make_shared<lognormal>(.04e-6, 1.4, 60e6));
  oi.coal_switch = oi.sedi_switch = false;
  oi.dt = 1; oi.sd_conc = 64; oi.n_sd_max = 64;
  oi.chem_switch = true; oi.chem_rho = 1.8e3; oi.sstp_chem = 2;
  std::unique_ptr<particles_proto_t<real_t>> prtcls(factory<real_t>(HIP, oi));
  std::vector<real_t> th(1, 289.), rv(1, .0064), rhod(1, 1.1);
  // volume mixing ratios of the kinematic chemistry case, as mass mixing ratios (x M_gas / M_d)
  const real_t M_d = 0.02897;
  std::vector<real_t> gas = {.1e-9 * 63e-3 / M_d, .1e-9 * 17e-3 / M_d, 360e-6 * 44e-3 / M_d, .2e-9 * 64e-3 / M_d, .4e-9 * 34e-3 / M_d, 25e-9 * 48e-3 / M_d};
  const std::vector<ptrdiff_t> s{1};
  particles_proto_t<real_t>::cchem_t amb_c;
  particles_proto_t<real_t>::chem_t amb;
  for (int g = 0; g < chem::chem_gas_n; ++g) {
    amb_c.emplace(chem::chem_species_t(g), arrinfo_t<real_t>(&gas[g], s));
    amb.emplace(chem::chem_species_t(g), arrinfo_t<real_t>(&gas[g], s));
  }
  prtcls->init(arrinfo_t<real_t>(th.data(), s), arrinfo_t<real_t>(rv.data(), s), arrinfo_t<real_t>(rhod.data(), s), arrinfo_t<real_t>(),
               arrinfo_t<real_t>(), arrinfo_t<real_t>(), arrinfo_t<real_t>(), amb_c);
  opts_t<real_t> opts;
  opts.adve = opts.sedi = opts.coal = false;
  opts.cond = true;
  opts.chem_dsl = opts.chem_dsc = opts.chem_rct = true;
  for (int step = 0; step < 10; ++step) {
    prtcls->step_sync(opts, arrinfo_t<real_t>(th.data(), s), arrinfo_t<real_t>(rv.data(), s), arrinfo_t<real_t>(rhod.data(), s), arrinfo_t<real_t>(),
                      arrinfo_t<real_t>(), arrinfo_t<real_t>(), arrinfo_t<real_t>(), amb);
    prtcls->step_async(opts);
  }
  for (chem::chem_species_t sp : {chem::S_VI, chem::H, chem::SO2}) {
    prtcls->diag_all(); prtcls->diag_chem(sp);
    std::printf("%.17g ", prtcls->outbuf()[0]);
  }
  std::printf("%.17g %.17g %.17g\n", gas[chem::SO2], gas[chem::H2O2], gas[chem::O3]);
  return 0;
}
