// lcx_math.hpp -- device/host formula library of the lgrngn hot path (HIP, gfx950).
//
// Templated on real_t (float | double).  Expressions keep the operator order of the reference
// formulas they implement (cited per function, paths relative to the reference checkout) and the
// library is compiled with -ffp-contract=off, so that +,-,*,/,sqrt results are IEEE-identical to the
// reference's CPU backends; only libm calls (exp, log, pow, cbrt) may differ in the last ulp.
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cstdint>
#include <type_traits>

#define LCX_HD __host__ __device__ __forceinline__

namespace lcx {

using n_t = unsigned long long;   // src/impl/particles_impl.ipp:29

template <class T> struct lim;
template <> struct lim<float>  { static constexpr float  eps = FLT_EPSILON, max = FLT_MAX, min = FLT_MIN; };
template <> struct lim<double> { static constexpr double eps = DBL_EPSILON, max = DBL_MAX, min = DBL_MIN; };

// std::min / std::max semantics (first argument wins on ties / NaN in the second)
template <class T> LCX_HD T mn(T a, T b) { return b < a ? b : a; }
template <class T> LCX_HD T mx(T a, T b) { return a < b ? b : a; }

// ---- constants: common/moist_air.hpp:26-112, const_cp.hpp:22-26, earth.hpp:16-22, theta_std.hpp:20
template <class T> struct cst {
  static constexpr T c_pd = T(1005), c_pv = T(1850), c_pw = T(4218);
  static constexpr T M_d = T(0.02897);
  static constexpr T M_v = T(1 * 1e-3) + T(17 * 1e-3);       // molar_mass.hpp:23-24, moist_air.hpp:36
  static constexpr T kaBoNA = T(8.3144621);
  static constexpr T R_d = kaBoNA / M_d, R_v = kaBoNA / M_v, eps = M_v / M_d;
  static constexpr T rho_w = T(1e3), D_0 = T(2.26e-5), K_0 = T(2.4e-2);
  static constexpr T p_tri = T(611.73), T_tri = T(273.16), l_tri = T(2.5e6);
  static constexpr T p_1000 = T(100000), g = T(9.81), p_stp = T(101325), T_stp = T(273.15 + 15);
  static constexpr T rho_stp = p_stp / T_stp / R_d;
  static constexpr T pi = T(3.141592653589793238462643383279502884L);
};

// theta_dry.hpp:24-55
template <class T> LCX_HD T theta_dry_T(T th, T rhod)
{
  using c = cst<T>;
  return pow(th * pow(rhod * c::R_d / c::p_1000, c::R_d / c::c_pd), c::c_pd / (c::c_pd - c::R_d));
}
template <class T> LCX_HD T theta_dry_p(T rhod, T r, T Tk) { using c = cst<T>; return rhod * (c::R_d + r * c::R_v) * Tk; }
// theta_std.hpp:35-41
template <class T> LCX_HD T exner(T p) { using c = cst<T>; return pow(p / c::p_1000, c::R_d / c::c_pd); }
// const_cp.hpp:82-86
template <class T> LCX_HD T l_v(T Tk) { using c = cst<T>; return c::l_tri + (c::c_pv - c::c_pw) * (Tk - c::T_tri); }
// theta_dry.hpp:60-65
template <class T> LCX_HD T d_th_d_rv(T Tk, T th) { return -th / Tk * l_v(Tk) / cst<T>::c_pd; }
// moist_air.hpp:77-83
template <class T> LCX_HD T p_v(T p, T r) { return p * r / (r + cst<T>::eps); }
// const_cp.hpp:34-43
template <class T> LCX_HD T p_vs(T Tk)
{
  using c = cst<T>;
  return c::p_tri * exp(
    (c::l_tri + (c::c_pw - c::c_pv) * c::T_tri) / c::R_v * (T(1) / c::T_tri - T(1) / Tk)
    - (c::c_pw - c::c_pv) / c::R_v * log(Tk / c::T_tri));
}
// const_cp.hpp:58-64
template <class T> LCX_HD T r_vs(T Tk, T p) { return cst<T>::eps / (p / p_vs(Tk) - 1); }
// tetens.hpp:12-37
template <class T> LCX_HD T tet_p_vs(T Tk)
{
  const T Tc = T(Tk - 273.15);
  return T(T(6.1078e2) * exp((T(17.27) * Tc) / (Tc + T(237.3))));
}
template <class T> LCX_HD T tet_r_vs(T Tk, T p)
{
  const T Tc = Tk - T(273.15);
  return T(T(380) / (p * exp(T(-17.2693882) * Tc / (Tk - T(35.86))) - T(610.9)));
}
// hskpng_Tpr.ipp:64-97,146-165
template <class T> LCX_HD T RH_of(int formula, T p, T rv, T Tk)
{
  switch (formula) {
    case 0: return p_v(p, rv) / p_vs(Tk);
    case 1: return rv / r_vs(Tk, p);
    case 2: return p_v(p, rv) / tet_p_vs(Tk);
    default: return rv / tet_r_vs(Tk, p);
  }
}
// vterm.hpp:22-31
template <class T> LCX_HD T visc(T Tk)
{
  const T tt = Tk / cst<T>::T_tri;
  return T(1.72 * 1e-5) * (T(393) / (Tk + T(120))) * T(tt * sqrt(tt));
}
// mean_free_path.hpp:16-51
template <class T> LCX_HD T lambda_D_of(T Tk) { using c = cst<T>; return T(2) * c::D_0 / T(sqrt(T(2) * T(c::R_v * Tk))); }
template <class T> LCX_HD T lambda_K_of(T Tk, T p) { using c = cst<T>; return T(.8) * (c::K_0 * Tk / p) / T(sqrt(T(2) * T(c::R_d * Tk))); }
// kelvin_term.hpp:25-50
template <class T> LCX_HD T sg_surf(T Tk) { return T(0.07275) * (T(1.) - T(0.002) * (Tk - T(291.))); }
template <class T> LCX_HD T kelvin_A(T Tk) { using c = cst<T>; return T(2) * sg_surf(Tk) / c::R_v / Tk / c::rho_w; }
// kappa_koehler.hpp:31-54
template <class T> LCX_HD T rw3_eq_nokelvin(T rd3, T kappa, T RH) { return rd3 * (1 - RH * (1 - kappa)) / (1 - RH); }
template <class T> LCX_HD T a_w(T rw3, T rd3, T kappa) { return (rw3 - rd3) / (rw3 - rd3 * (T(1) - kappa)); }
// transition_regime.hpp:15-20
template <class T> LCX_HD T trans_beta(T Kn) { return (1 + Kn) / (1 + T(1.71) * Kn + T(1.33) * Kn * Kn); }

// ---------------------------------------------------------------------------------------------
// TOMS 748 bracketing root finder in the form the reference vendors it
// (common/detail/toms748.hpp:60-454): same steps, same safeguards, same termination test, because
// the returned value is the midpoint of the LAST bracket and therefore depends on the iteration path.
// F: functor with T operator()(T) const.
template <class T> LCX_HD T eps_tolerance(unsigned bits)
{                                                                  // toms748.hpp:267-282
  return mx(T(ldexpf(1.0f, 1 - int(bits))), T(4 * lim<T>::eps));
}
template <class T> LCX_HD bool tol_reached(T eps, T a, T b) { return fabs(a - b) <= eps * mn(fabs(a), fabs(b)); }

// Fast arithmetic only (functors that declare `fast_div`, i.e. the collected growth rate): the interpolation steps divide
// ~20 times per loop iteration, a quarter of the condensation kernel's instructions as IEEE sequences (v_div_scale x2,
// v_rcp_f64, 6 FMA, v_div_fmas, v_div_fixup).  A reciprocal refined by two Newton steps (<= 1 ulp, math probe 4) times the
// numerator is half of that, and denominators shared between quotients are inverted once.  Quotients differ from the IEEE
// ones by <= 2 ulp, i.e. like the growth rate itself in this mode; the strict mode keeps the IEEE divisions.
// fast_div level of a functor: 0 none (IEEE divisions), 1 reciprocal + two Newton steps, 2 reciprocal + one Newton step
template <class F, class = void> struct fastdiv { static constexpr int value = 0; };
template <class F> struct fastdiv<F, std::void_t<decltype(F::fast_div)>> { static constexpr int value = int(F::fast_div); };
LCX_HD double rcp_refined(double y)
{
#if defined(__HIP_DEVICE_COMPILE__)
  const double r0 = __builtin_amdgcn_rcp(y);
  const double r1 = __builtin_fma(__builtin_fma(-y, r0, 1.0), r0, r0);
  return __builtin_fma(__builtin_fma(-y, r1, 1.0), r1, r1);
#else
  return 1.0 / y;
#endif
}
LCX_HD float rcp_refined(float y) { return 1.f / y; }
// one Newton step on the hardware reciprocal (v_rcp_f64 delivers ~2^-25: one step squares that -- measured <= 11 ulp, math
// probe 6).  Used for the interpolated abscissae of the fast-mode root finder only, never for a function value.
LCX_HD double rcp_newton1(double y)
{
#if defined(__HIP_DEVICE_COMPILE__)
  const double r0 = __builtin_amdgcn_rcp(y);
  return __builtin_fma(__builtin_fma(-y, r0, 1.0), r0, r0);
#else
  return 1.0 / y;
#endif
}
LCX_HD float rcp_newton1(float y) { return 1.f / y; }
template <int FD, class T> LCX_HD T rcp_fd(T y) { if constexpr (FD == 2) return rcp_newton1(y); else return rcp_refined(y); }
// The correctly rounded quotient without the scaling that the compiler's f64 division carries (v_div_scale twice, v_div_fmas,
// v_div_fixup around the very same reciprocal refinement): for finite, non-zero operands whose exponents are nowhere near the ends of
// the range -- every quantity of the growth rate, 1e-30 ... 1e30 -- the scaled and the unscaled sequence are the same eight operations
// on the same numbers, so the bits are those of `n / d` (tools/strict_checksum.py before and after).  Eight instructions instead of
// eleven, fourteen divisions per evaluation of the strict growth rate.  (A cell without any vapour, RH_eff = rho_v = 0, gives
// -inf / inf = NaN in the reference's expression as well: no case in which `/` has an answer and this has none.)
LCX_HD double div_unscaled(double n, double d)
{
#if defined(__HIP_DEVICE_COMPILE__)
  double r = __builtin_amdgcn_rcp(d);
  double e = __builtin_fma(-d, r, 1.0);
  r = __builtin_fma(r, e, r);
  e = __builtin_fma(-d, r, 1.0);
  r = __builtin_fma(r, e, r);
  const double q = n * r;
  const double rem = __builtin_fma(-d, q, n);
  return __builtin_fma(rem, r, q);
#else
  return n / d;
#endif
}
LCX_HD float div_unscaled(float n, float d) { return n / d; }
template <int FD, class T> LCX_HD T dvd(T x, T y)
{
  if constexpr (FD != 0) return x * rcp_fd<FD>(y);
  else return div_unscaled(x, y);            // (strict: the bits of x / y, see above -- the root finder's own quotients)
}

namespace t748 {
template <class T> struct st { T a, b, fa, fb, d, fd; };

// (Measured and dropped in fast arithmetic: the interpolation steps through selects instead of branches -- quotient formed
// unconditionally, the quadratic step's secant fallback computed next to its Newton iterations: 6.78 ms against 6.63.)
template <int FD = 0, class T> LCX_HD T safe_div(T num, T den, T r)
{                                                                  // :124-138
  if constexpr (FD != 0 && sizeof(T) == 8) {
    // fast arithmetic in double precision: the reference's guard is against a quotient beyond the largest number; with squared radii of
    // 1e-18 ... 1e-6 m^2 and function values of the same units that needs a denominator that IS zero -- the one case kept (round 5: five
    // instructions per quotient less, five quotients per quadratic step; the condensation launch of cond_solver = 1 5.67 -> 5.60 ms on
    // one box).  Single precision keeps the guard: its range, 1e-38 ... 3e38, IS within reach of these quotients (the float C2 run
    // produced NaNs without it).
    return den == 0 ? r : dvd<FD>(num, den);
  }
  if (fabs(den) < 1 && fabs(den * lim<T>::max) <= fabs(num)) return r;
  return dvd<FD>(num, den);
}
template <int FD = 0, class T> LCX_HD T secant(T a, T b, T fa, T fb)
{                                                                  // :140-160
  const T tol = lim<T>::eps * 5;
  const T c = a - dvd<FD>(fa, T(fb - fa)) * (b - a);
  if (c <= a + fabs(a) * tol || c >= b - fabs(b) * tol) return (a + b) / 2;
  return c;
}
template <int FD = 0, class T> LCX_HD T quadratic(T a, T b, T d, T fa, T fb, T fd, unsigned count)
{                                                                  // :162-222
  T B = safe_div<FD>(T(fb - fa), T(b - a), lim<T>::max);
  T A = safe_div<FD>(T(fd - fb), T(d - b), lim<T>::max);
  A = safe_div<FD>(T(A - B), T(d - a), T(0));
  if (A == 0) return secant<FD>(a, b, fa, fb);
  T c = copysign(T(1), A * fa) > 0 ? a : b;
  for (unsigned i = 1; i <= count; ++i)
    c -= safe_div<FD>(T(fa + (B + A * (c - b)) * (c - a)), T(B + A * (2 * c - a - b)), T(1 + c - a));
  if (c <= a || c >= b) c = secant<FD>(a, b, fa, fb);
  return c;
}
template <int FD = 0, class T> LCX_HD T cubic(T a, T b, T d, T e, T fa, T fb, T fd, T fe)
{                                                                  // :224-262
  if constexpr (FD != 0) {                                         // six distinct denominators among the nine quotients
    const T r_ed = rcp_fd<FD>(T(fe - fd)), r_db = rcp_fd<FD>(T(fd - fb)), r_ba = rcp_fd<FD>(T(fb - fa)),
            r_eb = rcp_fd<FD>(T(fe - fb)), r_da = rcp_fd<FD>(T(fd - fa)), r_ea = rcp_fd<FD>(T(fe - fa));
    const T q11 = (d - e) * fd * r_ed;
    const T q21 = (b - d) * fb * r_db;
    const T q31 = (a - b) * fa * r_ba;
    const T d21 = (b - d) * fd * r_db;
    const T d31 = (a - b) * fb * r_ba;
    const T q22 = (d21 - q11) * fb * r_eb;
    const T q32 = (d31 - q21) * fa * r_da;
    const T d32 = (d31 - q21) * fd * r_da;
    const T q33 = (d32 - q22) * fa * r_ea;
    T c = q31 + q32 + q33 + a;
    if (c <= a || c >= b) c = quadratic<FD>(a, b, d, fa, fb, fd, 3);
    return c;
  }
  const T q11 = (d - e) * fd / (fe - fd);
  const T q21 = (b - d) * fb / (fd - fb);
  const T q31 = (a - b) * fa / (fb - fa);
  const T d21 = (b - d) * fd / (fd - fb);
  const T d31 = (a - b) * fb / (fb - fa);
  const T q22 = (d21 - q11) * fb / (fe - fb);
  const T q32 = (d31 - q21) * fa / (fd - fa);
  const T d32 = (d31 - q21) * fd / (fd - fa);
  const T q33 = (d32 - q22) * fa / (fe - fa);
  T c = q31 + q32 + q33 + a;
  if (c <= a || c >= b) c = quadratic(a, b, d, fa, fb, fd, 3);
  return c;
}
template <class T, class F> LCX_HD void bracket(const F &f, st<T> &s, T c)
{                                                                  // :60-122
  if constexpr (fastdiv<F>::value != 0) {
    // fast arithmetic: the same decisions as below through selects -- every `if` in divergent code is an exec-mask save / branch /
    // restore (a few dozen cycles of a wave that has only three others to hide behind), and these bodies are single assignments
    const T tol = lim<T>::eps * 2;
    const T w = s.b - s.a;
    T cc = c;
    cc = (c >= s.b - fabs(s.b) * tol) ? s.b - fabs(s.a) * tol : cc;
    cc = (c <= s.a + fabs(s.a) * tol) ? s.a + fabs(s.a) * tol : cc;
    cc = (w < 2 * tol * s.a) ? s.a + w / 2 : cc;
    const T fc = f(cc);
    const bool zero = fc == 0, neg = !zero && copysign(T(1), s.fa * fc) < 0, pos = !zero && !neg;
    const T a0 = s.a, fa0 = s.fa, b0 = s.b, fb0 = s.fb;
    s.d = zero ? T(0) : neg ? b0 : a0;
    s.fd = zero ? T(0) : neg ? fb0 : fa0;
    s.a = neg ? a0 : cc;
    s.fa = zero ? T(0) : pos ? fc : fa0;
    s.b = neg ? cc : b0;
    s.fb = neg ? fc : fb0;
    return;
  }
  const T tol = lim<T>::eps * 2;
  if ((s.b - s.a) < 2 * tol * s.a) c = s.a + (s.b - s.a) / 2;
  else if (c <= s.a + fabs(s.a) * tol) c = s.a + fabs(s.a) * tol;
  else if (c >= s.b - fabs(s.b) * tol) c = s.b - fabs(s.a) * tol;
  const T fc = f(c);
  if (fc == 0) { s.a = c; s.fa = 0; s.d = 0; s.fd = 0; return; }
  if (copysign(T(1), s.fa * fc) < 0) { s.d = s.b; s.fd = s.fb; s.b = c; s.fb = fc; }
  else                               { s.d = s.a; s.fd = s.fa; s.a = c; s.fa = fc; }
}
template <class T> LCX_HD bool prof(const st<T> &s, T fe)
{
  const T md = lim<T>::min * 32;
  return fabs(s.fa - s.fb) < md || fabs(s.fa - s.fd) < md || fabs(s.fa - fe) < md ||
         fabs(s.fb - s.fd) < md || fabs(s.fb - fe) < md || fabs(s.fd - fe) < md;
}
} // namespace t748

// toms748.hpp:289-431 in two halves that a kernel may run on different lanes (same operations on the same values, hence
// the same result): toms748_head = the entry checks plus the secant and the first quadratic step; toms748_tail = the
// main loop and the final midpoint.  `carry` is everything the loop needs.
template <class T> struct toms_carry { t748::st<T> s; T e, fe; unsigned count; };
template <class T, class F>
LCX_HD bool toms748_head(const F &f, T ax, T bx, T fax, T fbx, T eps, unsigned max_iter, toms_carry<T> &k, T &root)
{                                                                  // returns true when `root` is final
  using namespace t748;
  constexpr int FD = fastdiv<F>::value;
  k.count = max_iter;
  k.s = st<T>{ax, bx, fax, fbx, T(0), T(0)};
  st<T> &s = k.s;
  T c;
  if (tol_reached(eps, s.a, s.b) || s.fa == 0 || s.fb == 0) {
    if (s.fa == 0) s.b = s.a; else if (s.fb == 0) s.a = s.b;
    root = (s.a + s.b) / 2;
    return true;
  }
  k.fe = k.e = s.fd = 1e5f;
  if (s.fa != 0) {
    c = secant<FD>(s.a, s.b, s.fa, s.fb);
    bracket(f, s, c);
    --k.count;
    if (k.count && s.fa != 0 && !tol_reached(eps, s.a, s.b)) {
      c = quadratic<FD>(s.a, s.b, s.d, s.fa, s.fb, s.fd, 2);
      k.e = s.d; k.fe = s.fd;
      bracket(f, s, c);
      --k.count;
    }
  }
  if (k.count && s.fa != 0 && !tol_reached(eps, s.a, s.b)) return false;       // the loop has work to do
  if (s.fa == 0) s.b = s.a; else if (s.fb == 0) s.a = s.b;
  root = (s.a + s.b) / 2;
  return true;
}
template <class T, class F>
LCX_HD T toms748_tail(const F &f, toms_carry<T> k, T eps, unsigned *iters_left = nullptr)
{
  using namespace t748;
  constexpr int FD = fastdiv<F>::value;
  st<T> &s = k.s;
  T c, u, fu, w0, &e = k.e, &fe = k.fe;
  unsigned &count = k.count;
  const T mu = 0.5f;
  while (count && s.fa != 0 && !tol_reached(eps, s.a, s.b)) {
    w0 = s.b - s.a;                                // (b0 - a0 of the reference: only the width is used below)
    c = prof(s, fe) ? quadratic<FD>(s.a, s.b, s.d, s.fa, s.fb, s.fd, 2) : cubic<FD>(s.a, s.b, s.d, e, s.fa, s.fb, s.fd, fe);
    e = s.d; fe = s.fd;
    bracket(f, s, c);
    if (0 == --count || s.fa == 0 || tol_reached(eps, s.a, s.b)) break;
    c = prof(s, fe) ? quadratic<FD>(s.a, s.b, s.d, s.fa, s.fb, s.fd, 3) : cubic<FD>(s.a, s.b, s.d, e, s.fa, s.fb, s.fd, fe);
    bracket(f, s, c);
    if (0 == --count || s.fa == 0 || tol_reached(eps, s.a, s.b)) break;
    if (fabs(s.fa) < fabs(s.fb)) { u = s.a; fu = s.fa; } else { u = s.b; fu = s.fb; }
    c = u - 2 * dvd<FD>(fu, T(s.fb - s.fa)) * (s.b - s.a);
    if (fabs(c - u) > (s.b - s.a) / 2) c = s.a + (s.b - s.a) / 2;
    e = s.d; fe = s.fd;
    bracket(f, s, c);
    if (0 == --count || s.fa == 0 || tol_reached(eps, s.a, s.b)) break;
    if ((s.b - s.a) < mu * w0) continue;
    e = s.d; fe = s.fd;
    bracket(f, s, T(s.a + (s.b - s.a) / 2));
    --count;
  }
  if (iters_left) *iters_left = count;
  if (s.fa == 0) s.b = s.a; else if (s.fb == 0) s.a = s.b;
  return (s.a + s.b) / 2;
}
template <class T, class F>
LCX_HD T toms748_solve(const F &f, T ax, T bx, T fax, T fbx, T eps, unsigned max_iter)
{                                                                  // toms748.hpp:289-431
  toms_carry<T> k;
  T root;
  if (toms748_head(f, ax, bx, fax, fbx, eps, max_iter, k, root)) return root;
  return toms748_tail(f, k, eps);
}

// ---- equilibrium wet radius at init: kappa_koehler.hpp:58-146, init_wet.ipp:17-38
template <class T> struct rw3_eq_minfun {
  T RH, rd3, kappa, A;   // A = kelvin::A(T): hoisted (same value every evaluation)
  LCX_HD T operator()(T rw3) const { return RH - a_w(rw3, rd3, kappa) * exp(A / T(cbrt(rw3))); }
};
template <class T> LCX_HD T rw3_eq(T rd3, T kappa, T RH, T Tk)
{
  if (kappa == 0) return rd3;
  const rw3_eq_minfun<T> f{RH, rd3, kappa, kelvin_A(Tk)};
  const T a = rd3, b = rw3_eq_nokelvin(rd3, kappa, RH);
  return toms748_solve(f, a, b, f(a), f(b), eps_tolerance<T>(sizeof(T) * 8 / 4), 100u);
}

// ---- critical radius: kappa_koehler.hpp:88-166 (evaluated in double whatever real_t), particles_diag.ipp:41-62
struct rw3_cr_minfun {
  double rd3, kappa, A;
  LCX_HD double operator()(double rw3) const
  { return A * (rd3 - rw3) * ((kappa - 1) * rd3 + rw3) + 3 * kappa * rd3 * rw3 * cbrt(rw3); }
};
template <class T> LCX_HD T rc2_of(T rd3, T kappa, T Tk)
{
  const rw3_cr_minfun f{double(rd3), double(kappa), kelvin_A(double(Tk))};
  const double a = 1e0 * double(rd3), b = 1e8 * double(rd3);
  const T rw3 = T(toms748_solve(f, a, b, f(a), f(b), eps_tolerance<double>(sizeof(double) * 8 / 4), 100u));
  return pow(rw3, T(2. / 3));
}

template <class T> LCX_HD T rw3_cr_of(T rd3, T kappa, T Tk)
{
  const rw3_cr_minfun f{double(rd3), double(kappa), kelvin_A(double(Tk))};
  const double a = 1e0 * double(rd3), b = 1e8 * double(rd3);
  return T(toms748_solve(f, a, b, f(a), f(b), eps_tolerance<double>(sizeof(double) * 8 / 4), 100u));
}
// critical supersaturation, kappa_koehler.hpp:168-189
template <class T> LCX_HD T S_cr(T rd3, T kappa, T Tk)
{
  const T rw3 = rw3_cr_of(rd3, kappa, Tk);
  return a_w(rw3, rd3, kappa) * exp(kelvin_A(Tk) / T(cbrt(rw3)));
}

// Constant tables in a kernel that LOOPS over batches of droplets (k_cond_lean_wq).  Left alone, the compiler hoists the loop-invariant
// scalar loads of every table of every inlined growth-rate evaluation in front of the loop and holds them in scalar registers through
// it -- 66 of the 102 there are; the kernel's pointers then live in lanes of a vector register (v_readlane: vector issue slots).  A table
// pointer that went through an empty asm statement (lcx_tab<true>) is a new value as far as the compiler can tell, so its loads stay inside
// the loop's trip.  WHERE inside matters as much: a coefficient that is loaded in the basic block that uses it reaches the Horner step
// through two v_mov_b32 and a v_fmac_f64; loaded in a DOMINATING block it is the scalar operand of a v_fma_f64 (measured: the kernel
// issued 612 vector instructions per 64 droplets either way until its tables were loaded at the top of the trip -- lcx_tab_touch -- and
// handed down to the evaluations as pointers, cond_fun_fast::t_expk / t_cbrt).
#if defined(__HIP_DEVICE_COMPILE__)
template <bool FRESH> __device__ __forceinline__ const double *lcx_tab(const double *p)
{
  if constexpr (FRESH) {
    const double __attribute__((address_space(4))) *q = (const double __attribute__((address_space(4))) *)p;
    asm volatile("" : "+s"(q));
    return (const double *)q;
  }
  return p;
}
// the loads of c[0 .. N-1], here and now (later loads of the same addresses are these)
template <int N> __device__ __forceinline__ void lcx_tab_touch(const double *c)
{
  static_assert(N == 5 || N == 14, "the tables of the growth rate");
  if constexpr (N == 5) asm volatile("" :: "s"(c[0]), "s"(c[1]), "s"(c[2]), "s"(c[3]), "s"(c[4]));
  else asm volatile("" :: "s"(c[0]), "s"(c[1]), "s"(c[2]), "s"(c[3]), "s"(c[4]), "s"(c[5]), "s"(c[6]), "s"(c[7]), "s"(c[8]), "s"(c[9]), "s"(c[10]),
                    "s"(c[11]), "s"(c[12]), "s"(c[13]));
}
#endif
// ---- condensational growth: condensation/common/particles_impl_cond_common.ipp:80-338,
//      maxwell-mason.hpp:15-47, ventil.hpp:16-80
// Everything that does not depend on the trial radius is evaluated ONCE per super-droplet
// (the reference recomputes it in every drw2_dt call); each hoisted quantity is the same
// expression, so the values entering the formulas are bit-identical.
// The device library's exp(double), operation for operation (range reduction by ln 2 in two parts, the degree-11 Horner scheme, its two
// closing steps, ldexp, the overflow / underflow selects -- read off the library's code for gfx950), with its coefficients in CONSTANT
// memory: a literal 64-bit coefficient costs two v_mov_b32 per use (an fp64 instruction takes no 64-bit literal), 29 moves in front of
// every inlined copy of the strict growth rate and two dozen vector registers held through it; through the scalar cache they arrive as
// SGPR operands.  The same bits as exp() for every argument (tests/test_hip_parity.py::test_fast_math_accuracy, math probe 9 against 3).
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __constant__ unsigned long long lcx_explib_c[13] = {
  0x3ff71547652b82feull, 0xbfe62e42fefa39efull, 0xbc7abc9e3b39803full, 0x3e5ade156a5dcb37ull, 0x3e928af3fca7ab0cull, 0x3ec71dee623fde64ull,
  0x3efa01997c89e6b0ull, 0x3f2a01a014761f6eull, 0x3f56c16c1852b7b0ull, 0x3f81111111122322ull, 0x3fa55555555502a1ull, 0x3fc5555555555511ull,
  0x3fe000000000000bull};
#endif
LCX_HD double exp_lib(double x)
{
  // (gfx950 only: the transcription is of THIS target's device library; on another target -- or should a ROCm update change ocml's exp,
  // which tests/test_hip_parity.py::test_fast_math_accuracy, math probe 9 against 3, reports -- the library's own exp is the fallback)
#if defined(__HIP_DEVICE_COMPILE__) && defined(__gfx950__)
  const double *c = reinterpret_cast<const double *>(lcx_explib_c);
  const double dn = __builtin_rint(x * c[0]);
  double f = __builtin_fma(c[1], dn, x);
  f = __builtin_fma(c[2], dn, f);
  double p = __builtin_fma(c[3], f, c[4]);
  p = __builtin_fma(f, p, c[5]);
  p = __builtin_fma(f, p, c[6]);
  p = __builtin_fma(f, p, c[7]);
  p = __builtin_fma(f, p, c[8]);
  p = __builtin_fma(f, p, c[9]);
  p = __builtin_fma(f, p, c[10]);
  p = __builtin_fma(f, p, c[11]);
  p = __builtin_fma(f, p, c[12]);
  p = __builtin_fma(f, p, 1.0);
  p = __builtin_fma(f, p, 1.0);
  double z = __builtin_ldexp(p, int(dn));
  if (x > 1024.0) z = __builtin_inf();
  if (x < -1075.0) z = 0.0;
  return z;
#else
  return exp(x);
#endif
}
LCX_HD float exp_lib(float x) { return exp(x); }
// The library's pow as a REAL call (strict arithmetic only): Re^0.077 sits in a branch that only drops above ~50 um take, and the
// library routine is ~220 instructions and two dozen 64-bit literals in each of the twenty places where the strict growth rate is
// inlined -- half of the kernel's code.  Out of line it is there once; the same routine, the same bits.
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __attribute__((noinline)) inline double pow_outlined(double x, double y) { return pow(x, y); }
__device__ __attribute__((noinline)) inline float pow_outlined(float x, float y) { return pow(x, y); }
#else
inline double pow_outlined(double x, double y) { return pow(x, y); }
inline float pow_outlined(float x, float y) { return pow(x, y); }
#endif
template <class T> struct cond_fun {
  T rw2_old, dt, rd3, kpa;
  T vt, rhod, eta;
  T Sc, Pr;           // Sc = eta/rhod/D_0, Pr = c_pd*eta/K_0
  T lambda_D, lambda_K;
  T rho_v, Tk, RH_eff, lv, A;
  T lv_term;          // (lv / R_v / T - 1)

  LCX_HD T Nu(T X, T Re) const
  {                                                                // ventil.hpp:30-44
    // max(1, pow(Re, .077)) == 1 for Re <= 1 (pow is monotone, pow(1,.)=1; NaN for Re<0 loses in std::max)
    const T m = (Re > T(1)) ? mx(T(1), T(pow_outlined(Re, T(.077)))) : T(1);
    return T(1) + T(cbrt(T(1) + Re * X)) * m;
  }
  LCX_HD T drw2_dt(T rw2) const
  {
    using c = cst<T>;
    const T rw = sqrt(rw2);
    const T rw3 = rw * rw * rw;
    // (every `/` of the reference's expression, in its order, as div_unscaled)
    auto dv_ = [](T n_, T d_) { return div_unscaled(n_, d_); };
    auto beta = [&](T Kn) { return dv_(T(1) + Kn, T(1) + T(1.71) * Kn + T(1.33) * Kn * Kn); };      // trans_beta
    const T Re = dv_(vt * (T(2) * rw) * rhod, eta);
    const T D = c::D_0 * beta(dv_(lambda_D, rw)) * (Nu(Sc, Re) / 2);
    const T K = c::K_0 * beta(dv_(lambda_K, rw)) * (Nu(Pr, Re) / 2);
    const T aw = dv_(rw3 - rd3, rw3 - rd3 * (T(1) - kpa));                                             // a_w
    const T klv = exp_lib(dv_(A, rw));
    return T(2) * dv_(dv_(T(1) - dv_(aw * klv, RH_eff), c::rho_w),
                      dv_(dv_(T(1), D), rho_v) + dv_(dv_(dv_(lv, K), RH_eff), Tk) * lv_term);
  }
  LCX_HD T operator()(T rw2) const { return rw2_old + dt * drw2_dt(rw2) - rw2; }
};

// ---- lean fp64 elementary functions for the collected growth rate (fast mode only).
// The library cbrt/exp cost ~34/~54 VALU instructions each and make up 85 % of one growth-rate evaluation; their
// arguments here are confined (cbrt of 1 + Re*Sc >= 1, exp of the Kelvin term A/r_w in (0, a few)), so a single
// precision hardware seed (v_log_f32 / v_exp_f32 / v_rcp_f32) refined in double does the same job in ~15/~20.
// Both are accurate to <= 1 ulp on their domain (tests/test_hip_parity.py::test_fast_math_accuracy) and fall back
// to the library call outside it.
LCX_HD double cbrt_seeded_core(double x)            // 0.125 <= x < 1e30 is the caller's business
{
#if defined(__HIP_DEVICE_COMPILE__)
  const float xf = float(x);
  const float y0 = __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(xf) * (1.f / 3.f));
  const double inv = double(__builtin_amdgcn_rcpf(3.f * y0 * y0));
  double y = double(y0);
  y = __builtin_fma(-inv, __builtin_fma(y * y, y, -x), y);
  y = __builtin_fma(-inv, __builtin_fma(y * y, y, -x), y);
  return y;
#else
  return cbrt(x);
#endif
}
LCX_HD float cbrt_seeded_core(float x) { return cbrt(x); }
// cube root of ANY finite argument without a library fallback: |x| scaled into the seeded domain by an exact power of 8, the sign
// put back.  The ventilation factors' 1 + Re Sc goes below 1 and through zero for a droplet whose terminal velocity carries the
// reference's "invalid" flag vt = -1 (a droplet that coalesced in the previous step_async keeps it through the next condensation,
// particles_step.ipp:386-392: the last coalescence substep is not followed by hskpng_vterm_invalid), i.e. Re < 0.
LCX_HD double cbrt_signed_core(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
  const double a = fabs(x);
  const bool small = a < 0.125;
  const double r = cbrt_seeded_core(small ? a * 0x1p90 : a) * (small ? 0x1p-30 : 1.0);
  return a < 0x1p-92 ? 0.0 : copysign(r, x);          // (|1 + Re Sc| < 2e-28: the seed would underflow; the root is < 6e-10 of the factor's 1)
#else
  return cbrt(x);
#endif
}
LCX_HD float cbrt_signed_core(float x) { return cbrt(x); }
LCX_HD double cbrt_seeded(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
  if (!(x >= 0.125 && x < 1e30)) return cbrt(x);
  const float xf = float(x);
  const float y0 = __builtin_amdgcn_exp2f(__builtin_amdgcn_logf(xf) * (1.f / 3.f));      // ~1e-6 relative
  const double inv = double(__builtin_amdgcn_rcpf(3.f * y0 * y0));                       // 1 / (3 y^2), ~1e-7
  double y = double(y0);
  y = __builtin_fma(-inv, __builtin_fma(y * y, y, -x), y);                               // Newton, error -> ~1e-13
  y = __builtin_fma(-inv, __builtin_fma(y * y, y, -x), y);                               //          -> rounding
  return y;
#else
  return cbrt(x);
#endif
}
LCX_HD float cbrt_seeded(float x) { return cbrt(x); }

LCX_HD double exp_reduced_core(double x)            // |x| < 700 is the caller's business
{
  const double k = __builtin_rint(x * 1.4426950408889634);
  double r = __builtin_fma(-k, 6.93147180369123816490e-01, x);                           // ln2 hi / lo (fdlibm split)
  r = __builtin_fma(-k, 1.90821492927058770002e-10, r);
  double p = 1.6059043836821613e-10;                                                     // 1/13!
  p = __builtin_fma(p, r, 2.08767569878681e-09);
  p = __builtin_fma(p, r, 2.505210838544172e-08);
  p = __builtin_fma(p, r, 2.755731922398589e-07);
  p = __builtin_fma(p, r, 2.7557319223985893e-06);
  p = __builtin_fma(p, r, 2.48015873015873e-05);
  p = __builtin_fma(p, r, 1.984126984126984e-04);
  p = __builtin_fma(p, r, 1.3888888888888889e-03);
  p = __builtin_fma(p, r, 8.333333333333333e-03);
  p = __builtin_fma(p, r, 4.1666666666666664e-02);
  p = __builtin_fma(p, r, 1.6666666666666666e-01);
  p = __builtin_fma(p, r, 0.5);
  p = __builtin_fma(p, r, 1.0);
  p = __builtin_fma(p, r, 1.0);
  return __builtin_ldexp(p, int(k));
}
// exp of the Kelvin term A / r_w (0 < x < ~2; anything finite below 700 works): the same reduction and the same degree-13 polynomial as
// exp_reduced_core, evaluated as two interleaved Horner chains in r^2 (even and odd coefficients) -- half the dependent length -- and
// without the range check, whose library fallback would end the caller's scheduling region.  <= 1 ulp like exp_reduced (math probe 8).
// (the polynomial's coefficients sit in constant memory: gfx950's VOP3 takes no 64-bit literal, and a literal addend of a Horner step is
// materialised with two v_mov_b32 per step in front of a v_fmac -- read through the scalar cache they arrive in SGPRs, which a v_fma
// takes as they are: see DESIGN.md for what that saves)
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __constant__ double lcx_expk_c[14] = {
  1.4426950408889634, 6.93147180369123816490e-01, 1.90821492927058770002e-10,
  2.08767569878681e-09, 1.6059043836821613e-10, 2.755731922398589e-07, 2.505210838544172e-08, 2.48015873015873e-05, 2.7557319223985893e-06,
  1.3888888888888889e-03, 1.984126984126984e-04, 4.1666666666666664e-02, 8.333333333333333e-03, 1.6666666666666666e-01};
#endif
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ double exp_kelvin_c(double x, const double *c)         // (c: lcx_expk_c, or its image behind lcx_tab<true>)
{
  const double k = __builtin_rint(x * c[0]);
  double r = __builtin_fma(-k, c[1], x);
  r = __builtin_fma(-k, c[2], r);
  const double r2 = r * r;
  double pe = c[3];                                          // 1/12!
  double po = c[4];                                          // 1/13!
  pe = __builtin_fma(pe, r2, c[5]);                          // 1/10!
  po = __builtin_fma(po, r2, c[6]);                          // 1/11!
  pe = __builtin_fma(pe, r2, c[7]);                          // 1/8!
  po = __builtin_fma(po, r2, c[8]);                          // 1/9!
  pe = __builtin_fma(pe, r2, c[9]);                          // 1/6!
  po = __builtin_fma(po, r2, c[10]);                         // 1/7!
  pe = __builtin_fma(pe, r2, c[11]);                         // 1/4!
  po = __builtin_fma(po, r2, c[12]);                         // 1/5!
  pe = __builtin_fma(pe, r2, 0.5);                           // 1/2!
  po = __builtin_fma(po, r2, c[13]);                         // 1/3!
  // 1 + r + r^2 (pe + r po)
  const double p = __builtin_fma(r2, __builtin_fma(po, r, pe), r) + 1.0;
  return __builtin_ldexp(p, int(k));
}
#endif
LCX_HD double exp_kelvin(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return exp_kelvin_c(x, lcx_expk_c);
#else
  return exp(x);
#endif
}
LCX_HD float exp_kelvin(float x) { return exp(x); }
// 1 / sqrt(x) for a positive NORMAL x: the operations of the device library's rsqrt (hardware seed, one refinement step in e = 1 - x y^2
// with the second-order term) without its test for a seed that is zero, infinite or NaN -- the same bits for every argument the
// condensation kernel has (a squared radius, or a bracket end not below the dry radius), four instructions fewer per evaluation
LCX_HD double rsqrt_pos(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
  const double y0 = __builtin_amdgcn_rsq(x);
  const double e = __builtin_fma(y0 * -x, y0, 1.0);
  return __builtin_fma(y0 * e, __builtin_fma(e, 0.375, 0.5), y0);
#else
  return 1.0 / sqrt(x);
#endif
}
LCX_HD float rsqrt_pos(float x) { return rsqrt(x); }
LCX_HD double exp_reduced(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
  if (!(x > -700. && x < 700.)) return exp(x);
  return exp_reduced_core(x);
#else
  return exp(x);
#endif
}
LCX_HD float exp_reduced(float x) { return exp(x); }

// natural logarithm of a positive normal double for the fast-arithmetic terminal-velocity pass (only the index of a
// ln(r)-uniform table is taken from it): mantissa in [sqrt(1/2), sqrt(2)), log m = 2 atanh((m-1)/(m+1)) as an odd series.
// <= 2 ulp (math probe 5); the library call costs about twice as many instructions.
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __constant__ double lcx_logl_c[14] = {1.0 / 23.0, 1.0 / 21.0, 1.0 / 19.0, 1.0 / 17.0, 1.0 / 15.0, 1.0 / 13.0, 1.0 / 11.0, 1.0 / 9.0, 1.0 / 7.0, 1.0 / 5.0,
                                                 1.0 / 3.0, 0.70710678118654752, 6.93147180369123816490e-01, 1.90821492927058770002e-10};
template <bool FRESH = false> LCX_HD double log_lean_core(double x)               // positive normal x is the caller's business
{
  const double *c = lcx_tab<FRESH>(lcx_logl_c);                      // (coefficients through the scalar cache, see exp_kelvin)
  int e = __builtin_amdgcn_frexp_exp(x);
  double m = __builtin_amdgcn_frexp_mant(x);                     // [0.5, 1)
  if (m < c[11]) { m = m + m; e -= 1; }
  const double s = (m - 1.0) * rcp_refined(m + 1.0);
  const double z = s * s;
  double p = c[0];
  p = __builtin_fma(p, z, c[1]);
  p = __builtin_fma(p, z, c[2]);
  p = __builtin_fma(p, z, c[3]);
  p = __builtin_fma(p, z, c[4]);
  p = __builtin_fma(p, z, c[5]);
  p = __builtin_fma(p, z, c[6]);
  p = __builtin_fma(p, z, c[7]);
  p = __builtin_fma(p, z, c[8]);
  p = __builtin_fma(p, z, c[9]);
  p = __builtin_fma(p, z, c[10]);
  const double two_s = s + s;
  const double lm = __builtin_fma(two_s * z, p, two_s);
  const double ed = double(e);
  return __builtin_fma(ed, c[12], __builtin_fma(ed, c[13], lm));
}
#endif
LCX_HD double log_lean(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
  if (!(x >= 2.3e-308 && x < 1.7e308)) return log(x);
  return log_lean_core(x);
#else
  return log(x);
#endif
}
LCX_HD float log_lean(float x) { return log(x); }

// x^y for x > 1 and a small positive exponent (the ventilation factor's Re^0.077 of drops above ~50 um): exp(y ln x) from the two
// lean functions above, <= 2 ulp here because |y ln x| stays below a few units; the library pow is ~10x the instructions and
// two dozen scalar constants, all of it inlined into every copy of the growth rate.
LCX_HD double pow_lean(double x, double y)
{
#if defined(__HIP_DEVICE_COMPILE__)
  if (!(x < 1e300)) return pow(x, y);               // (x > 1 is the caller's; inf / NaN take the library's way)
  return exp_reduced_core(y * log_lean_core(x));
#else
  return pow(x, y);
#endif
}
LCX_HD float pow_lean(float x, float y) { return pow(x, y); }
// the same without the library fallback (1 < x < 1e300 is the caller's business): the growth rate's Re^0.077 sits in a rarely taken
// branch of every inlined copy, where the library pow is ~220 instructions of code each -- a third of the condensation kernel
LCX_HD double pow_core(double x, double y)
{
#if defined(__HIP_DEVICE_COMPILE__)
  return exp_kelvin(y * log_lean_core(x));
#else
  return pow(x, y);
#endif
}
LCX_HD float pow_core(float x, float y) { return pow(x, y); }

// The same growth rate as cond_fun, algebraically collected into ONE rational expression (one IEEE division
// instead of fifteen) with FMA contraction allowed.  Selected by opts_init.strict_fp = 0.  It is the counterpart
// of how the reference itself is built for production (-Ofast: reassociation + contraction, CMakeLists.txt:124):
// values differ from the strict form by a few ulp per evaluation, i.e. far inside the root finder's 2^-15
// tolerance; the parity tests hold it to the same bars as the strict form.
//   r dr/dt = (da RH - na klv) nD Sh nK Nu / ( da RH rho_w (c1 dD nK Nu + c2 dK nD Sh) )
// with beta(Kn) = n/d, a_w = na/da, c1 = 2/(D_0 rho_v), c2 = 2 l_v (l_v/(R_v T) - 1)/(K_0 RH T).
// droplet-independent part of the collected growth rate's set-up
// (two_rho_eta = 2 rhod / eta: the cell's part of the Reynolds number, for the production kernels' form of the growth rate -- OPT bit 3)
template <class T> struct cond_cell_fast { T Sc, Pr, lambda_D, lambda_K, A, RH_eff, c1, c2_rho, RH_rho_w, rhod, eta, two_rho_eta; };
// cbrt(1 + x): for |x| below 2^-8 (Re Sc of droplets up to ~8 um) the Taylor series to x^5 (next term 0.023 x^6 < 1e-16)
template <bool SERIES, class T> LCX_HD T cbrt1p(T x)
{
  if constexpr (SERIES && sizeof(T) == 8) {
    if (fabs(x) < T(0x1p-8))
      return T(1) + x * (T(1. / 3) + x * (T(-1. / 9) + x * (T(5. / 81) + x * (T(-10. / 243) + x * T(22. / 729)))));
  }
  return cbrt_seeded(T(1) + x);
}
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __constant__ double lcx_cbrt1p_c[5] = {1. / 3, -1. / 9, 5. / 81, -10. / 243, 22. / 729};
#endif
// OPT (measurement / tuning switches, all inside the fast arithmetic's few-ulp envelope): bit 0 the root finder's reciprocals
// with one Newton step instead of two; bit 1 the ventilation factors' cube roots by series for small arguments; bit 2 (the lean
// kernel, with bit 1): the same values from fewer instructions -- the reciprocal square root without the library's seed test (rsqrt_pos),
// the series' range test as one v_max_f64.  (Measured and dropped: the Kelvin exponential without its range reduction where that is
// the identity, A / r_w < 0.34 -- the same bits from five instructions fewer per evaluation, but the fallback's second code path costs
// 23 VGPRs, 102 instead of 79: four waves per SIMD instead of six.)
// Bit 3 (round 5, the production kernels): the same rational expression from six instructions fewer per evaluation, inside the mode's
// few-ulp envelope but NOT the same bits as without it -- Re Sc and Re Pr from per-droplet products c_Re Sc, c_Re Pr (Sc, Pr then hold those
// products); 1 + (1 + x p(x)) of the common branch as 2 + x p(x); the quotient's reciprocal with one Newton step instead of two
// (v_rcp_f64 delivers 2^-25: <= 11 ulp after one step, lcx_math.hpp rcp_newton1 -- a relative 2e-15 of a growth rate that the root
// finder resolves to 3e-5); 2 dt folded into one factor of the root finder's function; and the Reynolds number's 2 rhod / eta taken per
// cell (one product per droplet instead of an IEEE division).
// The launch is priced in lanes that compute (the package power cap, see k_cond_lean_fold): every fp64 operation less is time.
// (Measured and dropped once more, round 5: the Kelvin exponential without its range reduction for A / r_w < 0.34 -- six instructions
// that are the identity for every droplet above 3 nm -- with exp_kelvin as the fallback of the lanes outside: inlined, 78 -> 100 vector
// registers; as an out-of-line call 82, five waves per SIMD and the call's register traffic: 3.16 ms against 2.77 on one box.)
template <class T, int OPT = 0> struct cond_fun_fast {      // (OPT = 0: the form the per-particle kernels and turb_cond use)
  static constexpr int fast_div = (OPT & 1) ? 2 : 1;      // the root finder may use refined reciprocals (t748 above)
  static constexpr bool trim = (OPT & 8) != 0 && sizeof(T) == 8;
  static constexpr bool fresh = (OPT & 16) != 0;         // (a kernel that loops over batches of droplets: see lcx_tab)
  T rw2_old, dt, rd3, rd3_1mk, c_Re, Sc, Pr, lambda_D, lambda_K, A, RH_eff, c1, c2_rho, RH_rho_w;
  const double *t_expk = nullptr, *t_cbrt = nullptr;     // (fresh: the tables' images that the kernel loaded at the top of its trip)
  LCX_HD void setup(const cond_fun<T> &f)
  {
    using c = cst<T>;
    rw2_old = f.rw2_old; dt = f.dt; rd3 = f.rd3; rd3_1mk = f.rd3 * (T(1) - f.kpa);
    c_Re = f.vt * T(2) * f.rhod / f.eta;
    Sc = f.Sc; Pr = f.Pr; lambda_D = f.lambda_D; lambda_K = f.lambda_K; A = f.A; RH_eff = f.RH_eff;
    c1 = T(2) / (c::D_0 * f.rho_v);
    c2_rho = T(2) * f.lv * f.lv_term / (c::K_0 * f.RH_eff * f.Tk);
    RH_rho_w = f.RH_eff * c::rho_w;
  }
  // the same set-up split into its per-cell part (k_cond_cellpre, once per cell and substep) and the droplet's own part:
  // identical expressions, so the values are bit-identical to setup()
  LCX_HD void setup_cell(const cond_cell_fast<T> &cc, T rw2_old_, T dt_, T rd3_, T kpa, T vt)
  {
    rw2_old = rw2_old_; dt = dt_; rd3 = rd3_; rd3_1mk = rd3_ * (T(1) - kpa);
    // (bit 3: the cell's 2 rhod / eta comes with the cell's constants -- one product per droplet instead of an IEEE division)
    if constexpr (trim) c_Re = vt * cc.two_rho_eta; else c_Re = vt * T(2) * cc.rhod / cc.eta;
    Sc = cc.Sc; Pr = cc.Pr; lambda_D = cc.lambda_D; lambda_K = cc.lambda_K; A = cc.A; RH_eff = cc.RH_eff;
    c1 = cc.c1; c2_rho = cc.c2_rho; RH_rho_w = cc.RH_rho_w;
    if constexpr (trim) { Sc = c_Re * Sc; Pr = c_Re * Pr; }
  }
  LCX_HD T drw2_dt(T rw2) const { return T(2) * half_drw2_dt(rw2); }
  LCX_HD T half_drw2_dt(T rw2) const         // r dr/dt
  {
#pragma clang fp contract(fast)
    T irw;                            // one v_rsq + Newton step; rw = rw2 / sqrt(rw2) to ~1 ulp
    if constexpr ((OPT & 4) != 0) irw = rsqrt_pos(rw2); else irw = rsqrt(rw2);
    const T rw = rw2 * irw;
    const T Re = c_Re * rw;
    const T KnD = lambda_D * irw, KnK = lambda_K * irw;
    const T nD = T(1) + KnD, dD = T(1) + KnD * (T(1.71) + T(1.33) * KnD);
    const T nK = T(1) + KnK, dK = T(1) + KnK * (T(1.71) + T(1.33) * KnK);
    // rw^3 - rd^3 (1 - kappa) and rw^3 - rd^3 as ONE fused operation each, written out: left to `contract(fast)` the compiler fuses the
    // product rw2 * rw into the subtractions only while nobody else uses it, so that a caller that also wants rw^3 (k_cond_lean's change of
    // the third moment) would change the last bit of every evaluation
    const T na = T(fma(rw2, rw, -rd3)), da = T(fma(rw2, rw, -rd3_1mk));
    T Sh, Nu, klv;
    if constexpr (trim) {
      // Round 5, the production form: the series of the common droplet and the cube roots of the bigger one behind the two sides of ONE
      // branch (round 2 computed the series for everybody and repaired Sh and Nu behind it: what a launch costs is the lanes that compute,
      // and on drizzle -- bench.py's coal-stress leg -- every lane took both), and the cube roots without the handling of a negative or
      // tiny argument unless a lane has one (1 + Re Sc >= 1 for every droplet whose terminal velocity is valid): the same bits as
      // cbrt_signed_core there.
#if defined(__HIP_DEVICE_COMPILE__)
      const T xS = rw * Sc, xN = rw * Pr;                // (Sc, Pr hold c_Re Sc, c_Re Pr)
      const double *q = fresh ? t_cbrt : lcx_cbrt1p_c;  // (coefficients through the scalar cache, see exp_kelvin)
      if constexpr (fresh) klv = exp_kelvin_c(A * irw, t_expk); else klv = exp_kelvin(A * irw);
      if (T(__builtin_fmax(fabs(xS), fabs(xN))) < T(0x1p-8)) {
        Sh = T(2) + xS * (T(q[0]) + xS * (T(q[1]) + xS * (T(q[2]) + xS * (T(q[3]) + xS * T(q[4])))));
        Nu = T(2) + xN * (T(q[0]) + xN * (T(q[1]) + xN * (T(q[2]) + xN * (T(q[3]) + xN * T(q[4])))));
      } else {
        const T aS = T(1) + xS, aN = T(1) + xN;
        T cS, cN;
        if (aS >= T(0.125) && aN >= T(0.125)) { cS = cbrt_seeded_core(aS); cN = cbrt_seeded_core(aN); }
        else { cS = cbrt_signed_core(aS); cN = cbrt_signed_core(aN); }      // (a droplet whose vt is flagged invalid, -1: see below)
        T m = T(1);
        if (Re > T(1)) {
          if constexpr (fresh) m = mx(T(1), T(exp_kelvin_c(T(.077) * log_lean_core<true>(Re), t_expk))); else m = mx(T(1), T(pow_core(Re, T(.077))));
        }
        Sh = T(1) + cS * m; Nu = T(1) + cN * m;
      }
#else
      const T m = (Re > T(1)) ? mx(T(1), T(pow(Re, T(.077)))) : T(1);
      Sh = T(1) + cbrt1p<false>(Re * (Sc / c_Re)) * m;
      Nu = T(1) + cbrt1p<false>(Re * (Pr / c_Re)) * m;
      klv = exp_reduced(A * irw);
#endif
    } else if constexpr ((OPT & 2) != 0 && sizeof(T) == 8) {
      // ONE straight-line block for the common droplet (Re Sc < 2^-8: below ~8 um): the two cube-root series, the Knudsen terms and the
      // Kelvin exponential are independent chains that the scheduler interleaves -- at four waves per SIMD the kernel runs at the
      // latency of its dependent fp64 chains, and every branch (even one that the whole wave skips) ends a scheduling region.  Bigger
      // droplets repair Sh and Nu behind it in one rarely taken branch.  (cond on C3: 7.0 -> 6.7 ms with the two cube roots behind one
      // branch instead of two; -> see DESIGN.md for this form.)
      const T xS = Re * Sc, xN = Re * Pr;
#if defined(__HIP_DEVICE_COMPILE__)
      const double *q = lcx_cbrt1p_c;                  // (coefficients through the scalar cache, see exp_kelvin)
      T cS = T(1) + xS * (T(q[0]) + xS * (T(q[1]) + xS * (T(q[2]) + xS * (T(q[3]) + xS * T(q[4])))));
      T cN = T(1) + xN * (T(q[0]) + xN * (T(q[1]) + xN * (T(q[2]) + xN * (T(q[3]) + xN * T(q[4])))));
#else
      T cS = T(1) + xS * (T(1. / 3) + xS * (T(-1. / 9) + xS * (T(5. / 81) + xS * (T(-10. / 243) + xS * T(22. / 729)))));
      T cN = T(1) + xN * (T(1. / 3) + xN * (T(-1. / 9) + xN * (T(5. / 81) + xN * (T(-10. / 243) + xN * T(22. / 729)))));
#endif
      klv = exp_kelvin(A * irw);
      Sh = T(1) + cS; Nu = T(1) + cN;
      bool big;
      if constexpr ((OPT & 4) != 0) big = !(T(__builtin_fmax(fabs(xS), fabs(xN))) < T(0x1p-8)); else big = !(mx(fabs(xS), fabs(xN)) < T(0x1p-8));
      if (big) {
        // (no range check, whose library fallback is code in every copy: |1 + Re Sc| is below 1e30 for anything that is a droplet, and
        // the signed form takes the negative Reynolds number of a droplet whose vt is flagged invalid (-1) -- the series above is for
        // |Re Sc| < 2^-8 only: round 2 tested `Re Sc < 2^-8`, sent those droplets through the series at Re Sc ~ -0.7 and got their
        // growth wrong by up to 20 % (5 of 2.1e6 droplets per step at 512 SDs per cell, tests/test_hip_configs.py C5))
        cS = cbrt_signed_core(T(1) + xS); cN = cbrt_signed_core(T(1) + xN);
        const T m = (Re > T(1)) ? mx(T(1), T(pow_core(Re, T(.077)))) : T(1);
        Sh = T(1) + cS * m; Nu = T(1) + cN * m;
      }
    } else {
      const T m = (Re > T(1)) ? mx(T(1), T(pow(Re, T(.077)))) : T(1);
      Sh = T(1) + cbrt1p<false>(Re * Sc) * m;
      Nu = T(1) + cbrt1p<false>(Re * Pr) * m;
      klv = exp_reduced(A * irw);
    }
    const T nDSh = nD * Sh, nKNu = nK * Nu;
    const T num = (da * RH_eff - na * klv) * (nDSh * nKNu);
    const T den = (da * RH_rho_w) * (c1 * dD * nKNu + c2_rho * dK * nDSh);
    if constexpr (trim) return dvd<2>(num, den);
    return dvd<1>(num, den);
  }
  LCX_HD T operator()(T rw2) const
  {
#pragma clang fp contract(fast)
    // (dt is uniform: 2 dt is formed once, in a scalar register pair; the fused operation written out, see na / da above)
    if constexpr (trim) return T(fma(T(dt + dt), half_drw2_dt(rw2), rw2_old)) - rw2;
    return rw2_old + dt * drw2_dt(rw2) - rw2;
  }
};

// NOTE (measured on MI355X, 128^3 x 64 SDs, fp64): three forms of this routine were timed --
//   nested calls as below (growth rate inlined at ~10 sites, 128 VGPRs, 4 waves/SIMD)        17.1 ms
//   one-loop state machine with a single evaluation site (160 VGPRs, 3 waves/SIMD)            18.3 ms
//   persistent lanes refilled from an LDS-staged chunk (mean instead of max iterations/wave)  22.0 ms
// The kernel is bound by fp64 VALU issue (~500 instructions per evaluation, ~15 IEEE divisions), not by
// divergence or instruction fetch, so the plain form with the lowest register count wins.
// Later, with the lean growth rate (10.7 ms): the root finder split at its loop entry (toms748_head / toms748_tail below)
// with the ~40 % of droplets that enter the loop compacted onto fewer lanes -- in one kernel through LDS 12.0 ms, as
// two kernels through HBM 5.5 + 7..8.8 ms.  Dense waves of "hard" droplets pay the maximum over 64 of them, which costs
// more than the idle lanes it removes.  The growth rate as a real (noinline) function instead of ~20 inlined copies
// (80 KB of code): 16.3 ms against 8.6 -- the call ABI's register shuffling costs far more than the instruction cache gains.
// (the lean solvers' early out of a clamped bracket, see lean2_head: kappa RH far above the rounding of rd2^(3/2) - rd3)
template <class F> LCX_HD bool lean_clamped_sign_change(const F &f) { return (f.rd3 - f.rd3_1mk) * f.RH_eff > decltype(f.rd3)(1e-12) * f.rd3; }
// cond_common.ipp:197-337 up to and including the first two root-finder steps.  Returns true when `result` is final.
template <class T, class F>
LCX_HD bool advance_rw2_head_with(const F &f, T rw2_old, T rd3, T dt, T eps, T cond_mlt, unsigned n_iter, toms_carry<T> &k, T &result,
                                  T *rd2_lazy = nullptr)
{
  const T drw2 = dt * f.drw2_dt(rw2_old);
  if (drw2 == 0) { result = rw2_old; return true; }
  // rd2_lazy (fast arithmetic, a caller that runs head and tail on the same lane): the squared dry radius only ever clamps, and a droplet
  // that grows from a wet radius above its dry one has neither clamp bind -- it skips the cube root (see lean2_head; the same bits);
  // *rd2_lazy = 0 then stands for "below everything" in the tail as well
  T rd2 = T(0);
  if (!(rd2_lazy && fastdiv<F>::value != 0 && drw2 > 0 && rw2_old * rw2_old * rw2_old > rd3 * rd3 * T(1.000001))) {
    T rd;
    if constexpr (fastdiv<F>::value != 0) rd = cbrt_seeded(T(rd3 * T(0x1p90))) * T(0x1p-30); else rd = cbrt(rd3);   // exact scaling into the seeded domain
    rd2 = rd * rd;
  }
  if (rd2_lazy) *rd2_lazy = rd2;
  const T a_un = rw2_old + mn(T(0), cond_mlt * drw2);
  const T a = mx(rd2, a_un),
          b = rw2_old + mx(T(0), cond_mlt * drw2);
  if (a == b) { result = rw2_old; return true; }
  if constexpr (fastdiv<F>::value != 0) {
    // Fast arithmetic: a bracket that already meets the root finder's tolerance (a droplet near equilibrium) is answered with its
    // midpoint WITHOUT the function value at its far end.  The reference evaluates f there first and then returns either that very
    // midpoint (toms748's entry check, toms748.hpp:296-305) or rw2_old + drw2 (no sign change) -- the same number, the midpoint of
    // [rw2_old, rw2_old + 2 drw2], to the last bit or the one before it.  Round 5: also when the dry radius clamps the lower end -- at
    // the dry radius the water activity is zero, the droplet would grow there, the reference finds the sign change and returns this
    // very midpoint (see lean2_head; near-dry particles of no hygroscopicity: 60 % of bench.py's coal-stress box).
    if (tol_reached(eps, a, b) && (a == a_un || lean_clamped_sign_change(f))) { result = (a + b) / 2; return true; }
  }
  T fa, fb;
  // the reference takes f(rw2_old) == drw2 at the near end of the bracket (cond_common.ipp:296-305)
  if constexpr (fastdiv<F>::value != 0) {
    // ONE evaluation site for the far end: growing and evaporating droplets of a wave (the haze of a subsaturated cell hovers around
    // drw2 = 0) would otherwise run the two inlined copies one after the other
    const bool grows = drw2 > 0;
    const T f_far = f(grows ? b : a);
    fa = grows ? drw2 : f_far; fb = grows ? f_far : drw2;
  } else {
    if (drw2 > 0) { fa = drw2; fb = f(b); }
    else          { fa = f(a); fb = drw2; }
  }
  T rw2_new;
  if (fa * fb > 0) rw2_new = rw2_old + drw2;
  else if (!toms748_head(f, a, b, fa, fb, eps, n_iter, k, rw2_new)) return false;
  if (rw2_new < rd2) rw2_new = rd2;
  result = rw2_new;
  return true;
}
template <class T, class F>
LCX_HD T advance_rw2_tail_with(const F &f, T rd3, T eps, const toms_carry<T> &k, unsigned *iters_left = nullptr, const T *rd2_known = nullptr)
{
  T rw2_new = toms748_tail(f, k, eps, iters_left);
  T rd2;
  if (rd2_known) rd2 = *rd2_known;                  // (the head's, see rd2_lazy there)
  else {
    T rd;
    if constexpr (fastdiv<F>::value != 0) rd = cbrt_seeded(T(rd3 * T(0x1p90))) * T(0x1p-30); else rd = cbrt(rd3);   // exact scaling into the seeded domain
    rd2 = rd * rd;
  }
  if (rw2_new < rd2) rw2_new = rd2;
  return rw2_new;
}
// iters_left (optional): the root finder's remaining iteration budget on return -- 0 says that n_iter ran out (the answer is then
// NOT the reference's unless n_iter is its 100; k_cond_fast uses a short budget to set the slowest droplets aside, see there)
template <class T, class F>
LCX_HD T advance_rw2_with(const F &f, T rw2_old, T rd3, T dt, T eps, T cond_mlt, unsigned n_iter, unsigned *iters_left = nullptr)
{                                                                  // cond_common.ipp:197-337
  toms_carry<T> k;
  k.count = n_iter;
  T r, rd2;
  if (advance_rw2_head_with(f, rw2_old, rd3, dt, eps, cond_mlt, n_iter, k, r, &rd2)) { if (iters_left) *iters_left = k.count; return r; }
  return advance_rw2_tail_with(f, rd3, eps, k, iters_left, &rd2);
}
// ---- Fast arithmetic's own root finder (opts_init.strict_fp == 0).  TOMS748 was written to spend few FUNCTION EVALUATIONS; here an
// evaluation is ~75 fp64 operations and the algorithm's own interpolation (a cubic through four points: six reciprocals and thirty
// products per update), its six-value bracket state and its branches were MORE than half of the condensation kernel's instructions (profiles/
// r02h_k_cond_fast_instruction_mix.txt: 360 of 759 fp64 instructions per wave in the growth rate, the rest in the root finder, next to 574
// moves / selects / compares).  It also has to pull BOTH ends of its bracket inside the tolerance, although the tolerance is relative
// to rw2 and the function is all but linear over the bracket for every droplet whose radius changes by less than a per cent in a step
// (cloud droplets): the secant through the two ends is then already the answer.
// This solver keeps the reference's bracket and its early outs (cond_common.ipp:197-305), then iterates the secant on a bracket that always
// holds a sign change (regula falsi with the Anderson-Bjorck scaling of the retained end, order ~1.7) and stops when the ITERATE has
// converged: |c_new - c| <= eps c, or the bracket is inside the tolerance.  The root it returns solves the same backward-Euler equation
// to the same tolerance, eps = 2^-15 (config.hpp:39): it lies within that of the reference's answer (the midpoint of TOMS748's last
// bracket), which is SURVEY 8a's bar for rw2 (rtol 1e-4), not bit for bit.  The strict arithmetic (the API default) keeps TOMS748.
// the lean solvers' stopping rule (see lean2_loop): two successive iterates within the tolerance of each other are believed only when
// the function value has at least halved on its side of the root (superlinear convergence gives orders of magnitude per step; a
// secant that crawls along a step of f does not).  Double precision only: in single precision the function values next to the root
// are rounding noise (RH - klv cancels to three digits of the 24-bit significand) and do not halve -- the float build's loop ran to its
// iteration limit on that noise, its condensation launch 2.1 -> 6.1 ms.  (lean2_loop has its own rule for float, see there: the plain
// rule below, kept for advance_rw2_lean_with, left 3 of 6144 crafted droplets two tolerances from the root: in float that function,
// i.e. LCX_DBG_COND_LEAN_R3, is neither the same bits as lean2_* any more nor held to the tolerance by a test.)
// (Tried: "or within an eighth of the tolerance" instead of the precision test -- the crawl's ratio can be 0.99, and 748 of 3e5 random
// droplets of kappa = 1e-10 were off again.)
template <class T> LCX_HD bool lean_converged(T d, T lim, T fc, T fs)
{
  if constexpr (sizeof(T) == 4) return d <= lim;
  else return d <= lim && fabs(fc) <= T(0.5) * fabs(fs);
}
template <class T, class F>
LCX_HD T advance_rw2_lean_with(const F &f, T rw2_old, T rd3, T dt, T eps, T cond_mlt, unsigned n_iter)
{
  constexpr int FD = fastdiv<F>::value;
  const T drw2 = dt * f.drw2_dt(rw2_old);
  if (drw2 == 0) return rw2_old;
  T rd;
  if constexpr (FD != 0) rd = cbrt_seeded(T(rd3 * T(0x1p90))) * T(0x1p-30); else rd = cbrt(rd3);
  const T rd2 = rd * rd;
  const T a_un = rw2_old + mn(T(0), cond_mlt * drw2);
  T a = mx(rd2, a_un), b = rw2_old + mx(T(0), cond_mlt * drw2);
  if (a == b) return rw2_old;
  if (tol_reached(eps, a, b) && (a == a_un || lean_clamped_sign_change(f))) return (a + b) / 2;      // (see lean2_head)
  const bool grows = drw2 > 0;
  const T f_far = f(grows ? b : a);
  T fa = grows ? drw2 : f_far, fb = grows ? f_far : drw2;          // f(rw2_old) == drw2 (cond_common.ipp:296-305)
  T r;
  if (fa * fb > 0) r = rw2_old + drw2;
  else if (fa == 0) r = a;
  else if (fb == 0) r = b;
  else {
    // (x1, f1): the latest point, (x0, f0): the retained end of the bracket (opposite sign)
    T x0 = a, f0 = fa, x1 = b, f1 = fb;
    T c = x1 - f1 * dvd<FD>(T(x1 - x0), T(f1 - f0));
    r = c;
    for (unsigned it = 0; it < n_iter; ++it) {
      if (!(c > mn(x0, x1) && c < mx(x0, x1))) c = x0 + (x1 - x0) / 2;          // (rounding at the very end of a search)
      const T fc = f(c);
      if (fc == 0) { r = c; break; }
      const T fs = ((fc < 0) != (f1 < 0)) ? f0 : f1;                             // the previous value on fc's side of the root (see lean2_loop)
      if ((fc < 0) != (f1 < 0)) { x0 = x1; f0 = f1; }                            // the root is between the last two points
      else { T m = T(1) - dvd<FD>(fc, f1); if (!(m > 0)) m = T(0.5); f0 = f0 * m; }     // same side twice: Anderson-Bjorck
      x1 = c; f1 = fc;
      const T c_new = x1 - f1 * dvd<FD>(T(x1 - x0), T(f1 - f0));
      r = c_new;
      if (lean_converged(T(fabs(c_new - c)), T(eps * mn(fabs(c_new), fabs(c))), fc, fs) || tol_reached(eps, x0, x1)) break;
      c = c_new;
    }
    if (!(r > mn(a, b) && r < mx(a, b))) r = x1;                                  // (never leave the reference's bracket)
  }
  if (r < rd2) r = rd2;
  return r;
}
// The same solver with its bookkeeping pared down (round 4): the SAME operations on the droplet's numbers in the same order -- the
// answer is the one of advance_rw2_lean_with bit for bit IN DOUBLE (tools/cond_solver_probe.hip: 4e6 random droplets on the device; tests/
// test_hip_parity.py: the kernels) except that an iterate that rounding puts ON an end of its bracket is evaluated where it is instead of
// being moved to the midpoint (a far end that is a root to twelve digits: never seen) -- but the loop body is straight-line code
// (selects instead of the three divergent branches that mixed waves always took both ways), the exact-zero test is left to the
// arithmetic (f(c) = 0 gives c_new = c and ends the loop through the convergence test with the same answer), and minima / maxima of
// positive numbers are single instructions.  In three parts, so that a kernel can stop a droplet's loop after a few evaluations and
// have another lane take it up where it stands (k_cond_lean):
//   lean2_head   the reference's bracket and early outs (cond_common.ipp:197-305), the far end's evaluation, the first secant point
//   lean2_loop   up to `budget` evaluations; false: the budget ran out, s.c is the next point to evaluate
//   lean2_tail   the two clamps
template <class T> struct lean_state { T x0, f0, x1, f1, c, a, b; };      // (x1, f1): the latest point, (x0, f0): the retained end (opposite sign)
// suspicious (optional): set when the bracket may hold SEVERAL roots -- the caller then hands the droplet to the reference's own iterates
// (k_cond_lean) and the function returns at once.  Seen at production size only (tests/test_hip_reverse_replay.py, 2^24 droplets): a
// droplet that can evaporate down to its dry core within the step (the bracket reaches from beyond four dry radii to within four dry
// radii of the core: a 0.8 um droplet on a 5 nm core) has a root where it has shrunk to half its radius AND roots next to the core, where the Kelvin term takes
// over; the growing counterpart is a bracket that spans more than a factor of four in radius in supersaturated air.  Each solver's
// iterates pick one root; TOMS748's choice is the reference's.  About 0.1 % of the droplets of bench.py's settled boxes.
template <class T, class F>
LCX_HD bool lean2_head(const F &f, T rw2_old, T rd3, T dt, T eps, T cond_mlt, lean_state<T> &s, T &r, T &rd2, bool *suspicious = nullptr, bool ask = true)
{
  constexpr int FD = fastdiv<F>::value;
  const T drw2 = dt * f.drw2_dt(rw2_old);
  r = rw2_old;
  if (drw2 == 0) return true;
  // The squared dry radius only ever CLAMPS: the lower end of the bracket and the answer.  A droplet that grows from a wet radius
  // above its dry one (rw2_old^3 > rd3^2 with a margin far above the cube root's rounding) has neither clamp bind -- its bracket starts
  // at rw2_old, every answer lies above that -- and skips the cube root (round 5: four fifths of the droplets of a cloudy box; the same
  // bits, rd2 = 0 stands for "below everything")
  rd2 = T(0);
  if (!(drw2 > 0 && rw2_old * rw2_old * rw2_old > rd3 * rd3 * T(1.000001))) {
    T rd;
    if constexpr (FD != 0) rd = cbrt_seeded(T(rd3 * T(0x1p90))) * T(0x1p-30); else rd = cbrt(rd3);
    rd2 = rd * rd;
  }
  const T a_un = rw2_old + mn(T(0), cond_mlt * drw2);
  const T a = mx(rd2, a_un), b = rw2_old + mx(T(0), cond_mlt * drw2);
  if (a == b) return true;
  // A bracket already inside the tolerance is answered with its midpoint.  Round 5: also one whose lower end the dry radius clamps -- at
  // the dry radius the water activity is zero (rounding aside: 2e-16 of rd^3 against kappa rd^3 RH), so the droplet would grow there,
  // f(a) > 0 > f(rw2_old): the reference evaluates f(a), finds the sign change and returns this very midpoint (toms748's entry check,
  // toms748.hpp:305-313).  Rounds 3-4 evaluated f(a) and iterated inside the tolerance (three evaluations, and an answer that could
  // end ON the dry radius, half a tolerance away).  Near-dry particles of almost no hygroscopicity in subsaturated air are 60 % of
  // bench.py's coal-stress box (kappa = 1e-10, the reference's coalescence tests' set-up): its condensation launch 5.85 -> 4.95 ms.
  if (tol_reached(eps, a, b) && (a == a_un || lean_clamped_sign_change(f))) { r = (a + b) / 2; return true; }
  const bool grows = drw2 > 0;
  if (suspicious && ask) {      // (`ask`: a run-time switch beside the pointer -- a pointer that is selected at run time keeps the flag in memory)
    // (evaporating: the bracket reaches from beyond four dry radii down to within four dry radii of the core -- clamped by it or not)
    const bool several = grows ? (f.RH_eff > T(1) && b > T(16) * rw2_old) : (a < T(16) * rd2 && rw2_old > T(16) * rd2);
    *suspicious = several;
    if (several) return true;
  }
  const T f_far = f(grows ? b : a);
  const T fa = grows ? drw2 : f_far, fb = grows ? f_far : drw2;     // f(rw2_old) == drw2 (cond_common.ipp:296-305)
  bool final = true;
  if (fa * fb > 0) r = rw2_old + drw2;
  else if (fa == 0) r = a;
  else if (fb == 0) r = b;
  else {
    s.x0 = a; s.f0 = fa; s.x1 = b; s.f1 = fb; s.a = a; s.b = b;
    s.c = s.x1 - s.f1 * dvd<FD>(T(s.x1 - s.x0), T(s.f1 - s.f0));
    r = s.c;
    final = false;
  }
  if (final && r < rd2) r = rd2;
  return final;
}
template <class T, class F>
LCX_HD bool lean2_loop(const F &f, T eps, unsigned budget, lean_state<T> &s, T &r)
{
  constexpr int FD = fastdiv<F>::value;
  T x0 = s.x0, f0 = s.f0, x1 = s.x1, f1 = s.f1, c = s.c;
  bool done = false;
  for (unsigned it = 0; it < budget; ++it) {
    const T fc = f(c);
    const bool opp = (fc < 0) != (f1 < 0);                          // the root is between the last two points
    // Round 5: the iterate's convergence is believed only while the function values fall -- |f(c)| at most half of the previous value on
    // its side of the root.  Superlinear convergence gives orders of magnitude per step (the common droplet's confirming evaluation
    // finds 1e-3 of the ends' values); a particle of almost no hygroscopicity next to its dry radius has a STEP for f (zero water
    // activity within kappa of the dry radius, full evaporation rate just above), on which the secant crawls at a fixed ratio and two
    // successive iterates can be within the tolerance of each other a hundred tolerances from the root -- rounds 3-4 stopped there
    // (tests/test_hip_parity.py test_cond_step_with_near_dry_particles: 18 of 6144 such particles off by up to 7e-4; of 3e5 random
    // droplets with kappa = 1e-10 ... 1e-8, 1-3 % off by up to 0.2 against TOMS748 on the same function, none with this rule); now the
    // loop goes on to the bracket's own width.  In the bench's boxes 1.8 % of the droplets -- stiff haze, whose iterate converges in x
    // before its function value has halved -- take one evaluation more and end within 2e-10 of their old answer (tools/solver_lab.py
    // solve_lean2(guard=True): 3.129 -> 3.147 evaluations per droplet).  What remains between this solver and TOMS748 is the droplet
    // that ACTIVATES within the step (several roots in the bracket, each solver's iterates pick one: 0.03 % of a random population
    // spanning 0.9 <= RH <= 1.02, none in the parity tests' boxes) -- opts_init.cond_solver = 1 is there for the reference's choice.
    const T fs = opp ? f0 : f1;
    // same side twice: Anderson-Bjorck scaling of the retained end.  Round 5: behind a branch again -- nine droplets in ten do not take
    // it, and what a launch costs is the lanes that compute (the package's power cap), not the instructions that a wave issues
    T f0s = f0;
    if (!opp) {
      T m = T(1) - dvd<FD>(fc, f1);
      m = m > 0 ? m : T(0.5);
      f0s = f0 * m;
    }
    f0 = opp ? f1 : f0s;
    x0 = opp ? x1 : x0;
    x1 = c; f1 = fc;
    const T c_new = x1 - f1 * dvd<FD>(T(x1 - x0), T(f1 - f0));
    r = c_new;
    if constexpr (sizeof(T) == 4) {
      // Single precision (tests/test_hip_cond.py): the tolerance is 2^-7, and two iterates that close say little.  The plain rule stopped
      // the crawl described above two tolerances from the root (kappa = 1e-4 next to the dry radius), the double's rule as well where the
      // ventilation factor has its cusp (a negative Reynolds number: the value halves across the cusp, the root is a per cent further on)
      // -- 3 of 6144 crafted droplets -- and alone it never ends on a function that is rounding noise.  So here only the BRACKET ends the
      // loop, and iterates that agree are confirmed: the next evaluation is a probe beyond the iterate, towards the retained end, just far
      // enough that a sign change there puts the whole bracket inside the tolerance.  On noise the probe finds the sign change (it lies
      // half a per cent away, the noise 1e-4); on a crawl it does not and the loop goes on.  One evaluation more per droplet.
      const T d = fabs(c_new - c), lim = eps * T(__builtin_fmin(fabs(c_new), fabs(c)));
      done = fabs(x0 - x1) <= eps * T(__builtin_fmin(fabs(x0), fabs(x1)));
      c = c_new;
      (void)fs;
      const T off = T(0.875) * (lim - d);
      if (!done && off >= T(0.125) * lim) {
        const T t = x0 > c_new ? c_new + off : c_new - off;
        if (x0 > c_new ? t < x0 : t > x0) c = t;
        else done = true;                                    // (the retained end is nearer than that: the bracket is inside the tolerance)
      }
    } else {
      done = lean_converged(T(fabs(c_new - c)), T(eps * T(__builtin_fmin(fabs(c_new), fabs(c)))), fc, fs) ||
             fabs(x0 - x1) <= eps * T(__builtin_fmin(fabs(x0), fabs(x1)));
      c = c_new;
    }
    if (done) break;
  }
  s.x0 = x0; s.f0 = f0; s.x1 = x1; s.f1 = f1; s.c = c;
  return done;
}
template <class T>
LCX_HD T lean2_tail(const lean_state<T> &s, T r, T rd2)
{
  if (!(r > T(__builtin_fmin(s.a, s.b)) && r < T(__builtin_fmax(s.a, s.b)))) r = s.x1;       // (never leave the reference's bracket)
  if (r < rd2) r = rd2;
  return r;
}
template <class T, class F>
LCX_HD T advance_rw2_lean2_with(const F &f, T rw2_old, T rd3, T dt, T eps, T cond_mlt, unsigned n_iter, bool *suspicious = nullptr, bool ask = true)
{
  lean_state<T> s;
  T r, rd2 = 0;
  if (lean2_head(f, rw2_old, rd3, dt, eps, cond_mlt, s, r, rd2, suspicious, ask)) return r;
  lean2_loop(f, eps, n_iter, s, r);       // (a budget that runs out leaves the last iterate in r, as the plain loop does)
  return lean2_tail(s, r, rd2);
}
// per-cell part of with_cond_fun + cond_fun_fast::setup (same expressions, same order)
template <class T>
LCX_HD cond_cell_fast<T> make_cond_cell_fast(T rhod, T rv, T Tk, T eta, T lambda_D, T lambda_K, T RH, T RH_max)
{
  using c = cst<T>;
  cond_cell_fast<T> cc;
  cc.Sc = eta / rhod / c::D_0;
  cc.Pr = c::c_pd * eta / c::K_0;
  cc.lambda_D = lambda_D; cc.lambda_K = lambda_K;
  const T rho_v = rhod * rv;
  cc.RH_eff = RH > RH_max ? RH_max : RH;
  const T lv = l_v(Tk);
  cc.A = kelvin_A(Tk);
  const T lv_term = lv / c::R_v / Tk - T(1);
  cc.c1 = T(2) / (c::D_0 * rho_v);
  cc.c2_rho = T(2) * lv * lv_term / (c::K_0 * cc.RH_eff * Tk);
  cc.RH_rho_w = cc.RH_eff * c::rho_w;
  cc.rhod = rhod; cc.eta = eta; cc.two_rho_eta = T(2) * rhod / eta;
  return cc;
}
// builds the growth-rate functor (strict or collected form) and hands it to `body`
template <class T, bool FAST, class Body>
LCX_HD auto with_cond_fun(T rw2_old, T dt, T rhod, T rv, T Tk, T eta, T rd3, T kpa, T vt, T lambda_D, T lambda_K, T RH, T RH_max, const Body &body)
{
  using c = cst<T>;
  cond_fun<T> f;
  f.rw2_old = rw2_old; f.dt = dt; f.rd3 = rd3; f.kpa = kpa; f.vt = vt; f.rhod = rhod; f.eta = eta;
  f.Sc = eta / rhod / c::D_0;
  f.Pr = c::c_pd * eta / c::K_0;
  f.lambda_D = lambda_D; f.lambda_K = lambda_K;
  f.rho_v = rhod * rv; f.Tk = Tk; f.RH_eff = RH > RH_max ? RH_max : RH;
  f.lv = l_v(Tk);
  f.A = kelvin_A(Tk);
  f.lv_term = f.lv / c::R_v / Tk - T(1);
  if constexpr (FAST) { cond_fun_fast<T> ff; ff.setup(f); return body(ff); }
  else return body(f);
}
template <class T, bool FAST = false>
LCX_HD T advance_rw2(T rw2_old, T dt, T rhod, T rv, T Tk, T eta, T rd3, T kpa, T vt,
                     T lambda_D, T lambda_K, T RH, T RH_max, T eps, T cond_mlt, unsigned n_iter)
{                                                                  // cond_common.ipp:187-337
  if (rw2_old <= 0) return rw2_old;
  return with_cond_fun<T, FAST>(rw2_old, dt, rhod, rv, Tk, eta, rd3, kpa, vt, lambda_D, lambda_K, RH, RH_max,
                                [&](const auto &fn) { return advance_rw2_with(fn, rw2_old, rd3, dt, eps, cond_mlt, n_iter); });
}

// ---- terminal velocities: common/vterm.hpp:33-220 (khvorostyanov and beard77_v0 in double whatever real_t)
LCX_HD double vt_khvorostyanov(double r, double rhoa, double eta, bool spherical)
{
  using c = cst<double>;
  const double X = double(32. / 3) * (c::rho_w - rhoa) / rhoa * c::g * r * r * r / eta / eta * rhoa * rhoa;
  const double sX = sqrt(X);
  const double b = double(.0902 / 2) * sX / ((sqrt(double(1) + double(.0902) * sX) - double(1)) * (sqrt(double(1) + double(.0902) * sX)));
  const double pow_hlpr = sqrt(double(1) + double(.0902) * sX) - double(1);
  const double a = double(9.06 * 9.06 / 4) * pow_hlpr * pow_hlpr / pow(X, b);
  double Av;
  if (spherical)
    Av = a * pow(eta / rhoa * double(1e4), double(1) - double(2) * b) * pow(double(4. / 3) * c::rho_w / rhoa * c::g * double(1e2), b);
  else {
    const double lambda_half = 2.35e-3;
    const double ksi = exp(-r / lambda_half) + (double(1) - exp(-r / lambda_half)) / (double(1) + r / lambda_half);
    const double alfa = c::pi / double(6) * c::rho_w * ksi;
    Av = a * pow(eta / rhoa * double(1e4), double(1) - double(2) * b) * pow(double(2.546479) * alfa / rhoa * c::g * double(1e2), b);
  }
  const double Bv = double(3) * b - double(1);
  return (Av * double(pow(double(2 * 1e2) * r, Bv))) / double(1e2);
}
LCX_HD double vt_beard77_v0(double r)
{
  const double m_s[4] = {0.105035e2, 0.108750e1, -0.133245, -0.659969e-2};
  const double m_l[8] = {0.65639e1, -0.10391e1, -0.14001e1, -0.82736e0, -0.34277e0, -0.83072e-1, -0.10583e-1, -0.54208e-3};
  const double x = log(2 * 100 * r);
  double y = 0;
  if (r <= 20e-6) for (int i = 0; i < 4; ++i) y += m_s[i] * pow(x, double(i));
  else            for (int i = 0; i < 8; ++i) y += m_l[i] * pow(x, double(i));
  return exp(y) / 100.;
}
// The part of vt_beard77_fact that depends on the cell only (evaluated once per cell by k_vterm_cellpre, the very same
// expressions): l of the small-droplet branch, eta_0 / eta, eps_c of the large-droplet branch
template <class T> struct beard77_cell { T l, e0e, eps_c; };
template <class T> LCX_HD beard77_cell<T> vt_beard77_cellpart(T p, T rhoa, T eta)
{
  using c = cst<T>;
  const T eta_0 = T(1.818e-5), l_0 = T(6.62e-8);
  beard77_cell<T> b;
  b.l = l_0 * (eta / eta_0) * sqrt(c::p_stp / p * c::rho_stp / rhoa);
  b.e0e = eta_0 / eta;
  b.eps_c = sqrt(c::rho_stp / rhoa) - 1;
  return b;
}
template <class T> LCX_HD T vt_beard77_fact_pre(T r, const beard77_cell<T> &b)
{
  if (r <= T(20e-6)) {
    const T l_0 = T(6.62e-8);
    return b.e0e * (1 + T(1.255) * (b.l / r)) / (1 + T(1.255) * (l_0 / r));
  } else {
    const T eps_s = b.e0e - 1;
    return T(1.104) * eps_s + ((T(1.058) * b.eps_c - T(1.104) * eps_s) * (T(5.52) + log(2 * 100 * r)) / T(5.01)) + 1;
  }
}
// the same with the droplet radius entering as 1/r (fast arithmetic: reciprocal square root instead of sqrt and two divisions)
template <class T> LCX_HD T vt_beard77_fact_pre_small_fast(T inv_r, const beard77_cell<T> &b)
{
  const T l_0 = T(6.62e-8);
  return dvd<1>(T(b.e0e * (1 + T(1.255) * (b.l * inv_r))), T(1 + T(1.255) * (l_0 * inv_r)));
}
template <class T> LCX_HD T vt_beard77_fact(T r, T p, T rhoa, T eta)
{
  using c = cst<T>;
  const T eta_0 = T(1.818e-5);
  if (r <= T(20e-6)) {
    const T l_0 = T(6.62e-8);
    const T l = l_0 * (eta / eta_0) * sqrt(c::p_stp / p * c::rho_stp / rhoa);
    return (eta_0 / eta) * (1 + T(1.255) * (l / r)) / (1 + T(1.255) * (l_0 / r));
  } else {
    const T eps_s = (eta_0 / eta) - 1;
    const T eps_c = sqrt(c::rho_stp / rhoa) - 1;
    return T(1.104) * eps_s + ((T(1.058) * eps_c - T(1.104) * eps_s) * (T(5.52) + log(2 * 100 * r)) / T(5.01)) + 1;
  }
}
template <class T> LCX_HD T vt_beard76(T r, T Tk, T p, T rhoa, T eta)
{
  using c = cst<T>;
  if (r <= T(9.5e-6)) {
    const T l = T(6.62e-8) * (eta / T(1.818e-5)) * (c::p_stp / p) * sqrt(Tk / T(293.15));
    const T C_ac = T(1.) + T(1.255) * l / r;
    return (c::rho_w - rhoa) * c::g / (T(4.5) * eta) * C_ac * r * r;
  } else if (r <= T(5.035e-4)) {
    const double b[7] = {-0.318657e1, 0.992696, -0.153193e-2, -0.987059e-3, -0.578878e-3, 0.855176e-4, -0.327815e-5};
    const T l = T(6.62e-8) * (eta / T(1.818e-5)) * (c::p_stp / p) * sqrt(Tk / T(293.15));
    const T C_ac = T(1.) + T(1.255) * l / r;
    const T log_N_Da = log(T(32. / 3.) * r * r * r * rhoa * (c::rho_w - rhoa) * c::g / eta / eta);
    T Y = 0.;
    for (int i = 0; i < 7; ++i) Y = T(double(Y) + b[i] * pow(double(log_N_Da), double(i)));
    const T N_Re = T(C_ac * exp(double(Y)));
    return eta * N_Re / rhoa / T(2.) / r;
  } else {
    const T b[6] = {T(-0.500015e1), T(0.523778e1), T(-0.204914e1), T(0.475294), T(-0.542819e-1), T(0.238449e-2)};
    const T sg = sg_surf(Tk);
    const T Bo = T(16. / 3.) * r * r * (c::rho_w - rhoa) * c::g / sg;
    const T N_p = sg * sg * sg * rhoa * rhoa / eta / eta / eta / eta / c::g / (c::rho_w - rhoa);
    const T X = log(Bo * pow(N_p, T(1. / 6.)));
    T Y = 0.;
    for (int i = 0; i < 6; ++i) Y = Y + b[i] * pow(X, T(i));
    const T N_Re = pow(N_p, T(1. / 6.)) * exp(Y);
    return eta * N_Re / rhoa / T(2.) / r;
  }
}

// ---- Philox4x32-10 counter-based generator (Salmon et al. 2011): stateless, so every kernel draws
//      the number it needs from (call counter, element index) with no HBM traffic.
struct philox {
  static LCX_HD void round(uint32_t (&c)[4], uint32_t (&k)[2])
  {
    const uint64_t p0 = uint64_t(0xD2511F53u) * c[0], p1 = uint64_t(0xCD9E8D57u) * c[2];
    const uint32_t n0 = uint32_t(p1 >> 32) ^ c[1] ^ k[0], n2 = uint32_t(p0 >> 32) ^ c[3] ^ k[1];
    c[1] = uint32_t(p1); c[3] = uint32_t(p0); c[0] = n0; c[2] = n2;
    k[0] += 0x9E3779B9u; k[1] += 0xBB67AE85u;
  }
  static LCX_HD void gen(uint64_t idx, uint64_t call, uint64_t seed, uint32_t (&out)[4])
  {
    uint32_t c[4] = {uint32_t(idx), uint32_t(idx >> 32), uint32_t(call), uint32_t(call >> 32)};
    uint32_t k[2] = {uint32_t(seed), uint32_t(seed >> 32)};
    for (int i = 0; i < 10; ++i) round(c, k);
    for (int i = 0; i < 4; ++i) out[i] = c[i];
  }
  // uniform in [0,1) with 53 (double) / 24 (float) random bits
  template <class T> static LCX_HD T u01(uint64_t idx, uint64_t call, uint64_t seed)
  {
    uint32_t r[4]; gen(idx, call, seed, r);
    if (sizeof(T) == 8) return T(double((uint64_t(r[0]) << 21) ^ (uint64_t(r[1]) >> 11)) * (1.0 / 9007199254740992.0));
    return T(float(r[0] >> 8) * (1.0f / 16777216.0f));
  }
  // standard normal: Box-Muller from two uniforms of one Philox block
  template <class T> static LCX_HD T normal(uint64_t idx, uint64_t call, uint64_t seed)
  {
    uint32_t r[4]; gen(idx, call, seed, r);
    const double u1 = (double((uint64_t(r[0]) << 21) ^ (uint64_t(r[1]) >> 11)) + 1.0) * (1.0 / 9007199254740992.0);     // (0, 1]
    const double u2 = double((uint64_t(r[2]) << 21) ^ (uint64_t(r[3]) >> 11)) * (1.0 / 9007199254740992.0);
    return T(sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925286766559 * u2));
  }
  static LCX_HD uint32_t un(uint64_t idx, uint64_t call, uint64_t seed)
  {
    uint32_t r[4]; gen(idx, call, seed, r);
    return r[0];
  }
};

} // namespace lcx
