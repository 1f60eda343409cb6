// The output of a spectrum in one call.  The reference's kinematic driver writes its spectra as a loop over bins -- diag_dry_rng /
// diag_wet_rng, then diag_*_mom, then outbuf(), per bin and moment (kin_cloud_2d_lgrngn.hpp, diag()).  Here a 2-D box runs a few steps,
// the loop writes 39 dry bins, 24 wet bins, the cloud and rain ranges' wet moments 0-3 and sd_conc, and one diag_batch() call
// (an extension of the concrete class, include/lcx_diag.h) asks for the same list.  The printed line says how many of the
// requests x cells values agree bit for bit: all of them (tests/test_diag_batch_cxx.py).
#include <cmath>
#include <cstdio>
#include <cstring>
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
  const int nx = 6, nz = 5, n_cell = nx * nz;
  opts_init_t<real_t> oi;
  oi.dry_distros.emplace(kappa_rd_insol_t<real_t>(.61, 0.), std::make_shared<lognormal>(.04e-6 / 2, 1.4, 60e6));
  oi.kernel = kernel_t::geometric; oi.terminal_velocity = vt_t::beard77fast;
  oi.dt = 1; oi.nx = nx; oi.nz = nz; oi.dx = oi.dz = 10; oi.x1 = nx * 10; oi.z1 = nz * 10; oi.sd_conc = 32; oi.n_sd_max = 32 * n_cell;
  particles_t<real_t, HIP> prtcls(oi);
  std::vector<real_t> th(n_cell, 300.), rv(n_cell, .0225), rhod(n_cell, 1.), Cx((nx + 1) * nz, .1), Cz(nx * (nz + 1), 0.);
  const std::vector<ptrdiff_t> s{nz, 1}, sz{nz + 1, 1};
  auto a = [&](std::vector<real_t> &v, const std::vector<ptrdiff_t> &st) { return arrinfo_t<real_t>(v.data(), st); };
  prtcls.init(a(th, s), a(rv, s), a(rhod, s), arrinfo_t<real_t>(), a(Cx, s), arrinfo_t<real_t>(), a(Cz, sz));
  opts_t<real_t> opts;
  for (int step = 0; step < 5; ++step) { prtcls.step_sync(opts, a(th, s), a(rv, s), a(rhod, s)); prtcls.step_async(opts); }

  // the request list: the driver's bins (paper_GMD_2015/fig_a: 40 dry edges at a tenth of a decade, 25 wet at a fifth) and ranges
  std::vector<diag_req_t<real_t>> reqs;
  for (int i = 0; i < 39; ++i) reqs.push_back(diag_req_t<real_t>().dry_rng(1e-6 * std::pow(10, -3 + i * .1), 1e-6 * std::pow(10, -3 + (i + 1) * .1)).dry_mom(0));
  for (int i = 0; i < 24; ++i) reqs.push_back(diag_req_t<real_t>().wet_rng(1e-6 * std::pow(10, -3 + i * .2), 1e-6 * std::pow(10, -3 + (i + 1) * .2)).wet_mom(0));
  for (int k = 0; k < 4; ++k) reqs.push_back(diag_req_t<real_t>().wet_rng(.5e-6, 25e-6).wet_mom(k));
  for (int k = 0; k < 4; ++k) reqs.push_back(diag_req_t<real_t>().wet_rng(25e-6, 1).wet_mom(k));
  reqs.push_back(diag_req_t<real_t>().all().sd_conc());

  // one call
  std::vector<real_t> batch(reqs.size() * n_cell, -1);
  prtcls.diag_batch(reqs, batch.data(), n_cell);

  // the loop
  std::vector<real_t> loop;
  for (const auto &r : reqs) {
    const auto &c = r.clauses[0];
    if (c.sel == LCX_DIAG_SEL_ALL) prtcls.diag_all();
    else if (c.sel == LCX_DIAG_SEL_DRY) prtcls.diag_dry_rng(c.lo, c.hi);
    else prtcls.diag_wet_rng(c.lo, c.hi);
    if (r.count == LCX_DIAG_SD_CONC) prtcls.diag_sd_conc();
    else if (r.count == LCX_DIAG_DRY_MOM) prtcls.diag_dry_mom(r.k);
    else prtcls.diag_wet_mom(r.k);
    const real_t *out = prtcls.outbuf();
    loop.insert(loop.end(), out, out + n_cell);
  }

  size_t same = 0, nonzero = 0;
  for (size_t i = 0; i < loop.size(); ++i) { same += std::memcmp(&loop[i], &batch[i], sizeof(real_t)) == 0; nonzero += batch[i] != 0; }
  std::printf("diag_batch requests %zu cells %d per_pass %d values %zu identical %zu nonzero %zu\n", reqs.size(), n_cell, prtcls.diag_batch_info(),
              loop.size(), same, nonzero);
  return same == loop.size() ? 0 : 1;
}
