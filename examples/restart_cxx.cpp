// Stop a run and continue it, through the reference's C++ interface plus snapshot() / restore() (include/lcx_state.h): the 0-D parcel
// of parcel_cxx.cpp runs 20 steps, writes its snapshot to a file, a NEW object reads the file back in the place of init() and runs 20
// more steps.  Beside it an uninterrupted parcel runs 40 steps.  The two printed lines -- final rv and wet third moment -- are equal
// as text (tests/test_restart_cxx.py).  What the caller keeps himself: his own fields (th, rv here) and his step counter.
#include <cmath>
#include <cstdio>
#include <memory>
#include <string>
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

static opts_init_t<real_t> parcel_opts()
{
  opts_init_t<real_t> oi;
  oi.dry_distros.emplace(kappa_rd_insol_t<real_t>(.61, 0.), std::make_shared<lognormal>(.04e-6 / 2, 1.4, 60e6));
  oi.sedi_switch = false;
  oi.kernel = kernel_t::geometric; oi.terminal_velocity = vt_t::beard77fast;
  oi.RH_max = 0.999; oi.dt = 1; oi.sd_conc = 100; oi.n_sd_max = 100;
  return oi;
}

struct parcel
{
  std::unique_ptr<particles_proto_t<real_t>> prtcls;
  real_t th = 300, rv = 0.02, rhod = 1;
  const ptrdiff_t strides[1] = {1};
  opts_t<real_t> opts;
  parcel() : prtcls(factory<real_t>(HIP, parcel_opts())) { opts.adve = opts.sedi = false; }
  arrinfo_t<real_t> a(real_t &x) { return arrinfo_t<real_t>(&x, strides); }
  void init() { prtcls->init(a(th), a(rv), a(rhod)); }
  void run(int steps)
  {
    for (int step = 0; step < steps; ++step) { prtcls->step_sync(opts, a(th), a(rv), a(rhod)); prtcls->step_async(opts); }
  }
  void print(const char *what)
  {
    prtcls->diag_all(); prtcls->diag_wet_mom(3);
    std::printf("%s rv %.17g wet_mom3 %.17g\n", what, rv, prtcls->outbuf()[0]);
  }
};

int main(int argc, char **argv)
{
  const std::string path = argc > 1 ? argv[1] : "restart_cxx.snapshot";
  real_t th_kept, rv_kept;
  {
    parcel p;
    p.init();
    p.run(20);
    const std::vector<unsigned char> blob = p.prtcls->snapshot();
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(blob.data(), 1, blob.size(), f) != blob.size()) { std::perror("writing the snapshot"); return 1; }
    std::fclose(f);
    th_kept = p.th; rv_kept = p.rv;          // the caller's own fields: his to keep
  }
  {
    parcel q;                                // a new object from the same options; restore() in the place of init()
    std::vector<unsigned char> blob;
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) { std::perror("reading the snapshot"); return 1; }
    unsigned char buf[4096]; size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) blob.insert(blob.end(), buf, buf + n);
    std::fclose(f);
    std::remove(path.c_str());
    q.prtcls->restore(blob.data(), blob.size());
    q.th = th_kept; q.rv = rv_kept;
    q.run(20);
    q.print("final");
  }
  {
    parcel u;
    u.init();
    u.run(40);
    u.print("final");
  }
  return 0;
}
