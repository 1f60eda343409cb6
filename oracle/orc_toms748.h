/*
 * orc_toms748.h -- TEST INFRASTRUCTURE (oracle), not product code.
 *
 * TOMS 748 (Alefeld, Potra, Shi 1995), the variant vendored by the reference:
 * include/libcloudph++/common/detail/toms748.hpp:60-454, as a plain-C template.  orc_physics.h includes it once per floating
 * type it needs a root finder in, with
 *   T7R            the type
 *   T7(name)       the name of `name` in this instance
 *   T7_EPS, T7_MAX, T7_MIN   std::numeric_limits<T7R>::epsilon(), max(), min()
 * defined, and T7(dmin), T7(dmax) (std::min, std::max of T7R) declared.  No include guard: that is the point.
 */
typedef T7R (*T7(orc_fn))(T7R x, void *ctx);

static inline int T7(orc_tol_reached)(T7R eps, T7R a, T7R b)
{                                                   /* toms748.hpp:267-282 */
  return fabs(a - b) <= eps * T7(dmin)(fabs(a), fabs(b));
}
static inline T7R T7(orc_eps_tolerance)(unsigned bits)
{
  return T7(dmax)((T7R)ldexpf(1.0f, 1 - (int)bits), 4 * T7_EPS);
}
static inline T7R T7(t748_safe_div)(T7R num, T7R denom, T7R r)
{                                                   /* toms748.hpp:124-138 */
  if (fabs(denom) < 1 && fabs(denom * T7_MAX) <= fabs(num)) return r;
  return num / denom;
}
static inline T7R T7(t748_secant)(T7R a, T7R b, T7R fa, T7R fb)
{                                                   /* toms748.hpp:140-160 */
  const T7R tol = T7_EPS * 5;
  const T7R c = a - (fa / (fb - fa)) * (b - a);
  if (c <= a + fabs(a) * tol || c >= b - fabs(b) * tol) return (a + b) / 2;
  return c;
}
static inline T7R T7(t748_quadratic)(T7R a, T7R b, T7R d, T7R fa, T7R fb, T7R fd, unsigned count)
{                                                   /* toms748.hpp:162-222 */
  T7R B = T7(t748_safe_div)(fb - fa, b - a, T7_MAX);
  T7R A = T7(t748_safe_div)(fd - fb, d - b, T7_MAX);
  A = T7(t748_safe_div)(A - B, d - a, 0.);
  if (A == 0) return T7(t748_secant)(a, b, fa, fb);
  T7R c = copysign(1., A * fa) > 0 ? a : b;
  for (unsigned i = 1; i <= count; ++i)
    c -= T7(t748_safe_div)(fa + (B + A * (c - b)) * (c - a), B + A * (2 * c - a - b), 1 + c - a);
  if (c <= a || c >= b) c = T7(t748_secant)(a, b, fa, fb);
  return c;
}
static inline T7R T7(t748_cubic)(T7R a, T7R b, T7R d, T7R e, T7R fa, T7R fb, T7R fd, T7R fe)
{                                                   /* toms748.hpp:224-262 */
  const T7R q11 = (d - e) * fd / (fe - fd);
  const T7R q21 = (b - d) * fb / (fd - fb);
  const T7R q31 = (a - b) * fa / (fb - fa);
  const T7R d21 = (b - d) * fd / (fd - fb);
  const T7R d31 = (a - b) * fb / (fb - fa);
  const T7R q22 = (d21 - q11) * fb / (fe - fb);
  const T7R q32 = (d31 - q21) * fa / (fd - fa);
  const T7R d32 = (d31 - q21) * fd / (fd - fa);
  const T7R q33 = (d32 - q22) * fa / (fe - fa);
  T7R c = q31 + q32 + q33 + a;
  if (c <= a || c >= b) c = T7(t748_quadratic)(a, b, d, fa, fb, fd, 3);
  return c;
}
typedef struct { T7R a, b, fa, fb, d, fd; } T7(t748_state);
static inline void T7(t748_bracket)(T7(orc_fn) f, void *ctx, T7(t748_state) *s, T7R c)
{                                                   /* toms748.hpp:60-122 */
  const T7R tol = T7_EPS * 2;
  if ((s->b - s->a) < 2 * tol * s->a) c = s->a + (s->b - s->a) / 2;
  else if (c <= s->a + fabs(s->a) * tol) c = s->a + fabs(s->a) * tol;
  else if (c >= s->b - fabs(s->b) * tol) c = s->b - fabs(s->a) * tol;
  const T7R fc = f(c, ctx);
  if (fc == 0) { s->a = c; s->fa = 0; s->d = 0; s->fd = 0; return; }
  if (copysign(1., s->fa * fc) < 0) { s->d = s->b; s->fd = s->fb; s->b = c; s->fb = fc; }
  else                              { s->d = s->a; s->fd = s->fa; s->a = c; s->fa = fc; }
}
static inline int T7(t748_prof)(const T7(t748_state) *s, T7R fe)
{
  const T7R md = T7_MIN * 32;
  return fabs(s->fa - s->fb) < md || fabs(s->fa - s->fd) < md || fabs(s->fa - fe) < md ||
         fabs(s->fb - s->fd) < md || fabs(s->fb - fe) < md || fabs(s->fd - fe) < md;
}
static inline T7R T7(orc_toms748)(T7(orc_fn) f, void *ctx, T7R ax, T7R bx, T7R fax, T7R fbx,
                                 T7R eps, uintmax_t *max_iter)
{                                                   /* toms748.hpp:289-431 */
  uintmax_t count = *max_iter;
  T7(t748_state) s = {ax, bx, fax, fbx, 0, 0};
  T7R c, u, fu, a0, b0, e, fe;
  const T7R mu = 0.5;
  if (T7(orc_tol_reached)(eps, s.a, s.b) || s.fa == 0 || s.fb == 0) {
    *max_iter = 0;
    if (s.fa == 0) s.b = s.a; else if (s.fb == 0) s.a = s.b;
    return (s.a + s.b) / 2;
  }
  fe = e = s.fd = 1e5f;
  if (s.fa != 0) {
    c = T7(t748_secant)(s.a, s.b, s.fa, s.fb);
    T7(t748_bracket)(f, ctx, &s, c);
    --count;
    if (count && s.fa != 0 && !T7(orc_tol_reached)(eps, s.a, s.b)) {
      c = T7(t748_quadratic)(s.a, s.b, s.d, s.fa, s.fb, s.fd, 2);
      e = s.d; fe = s.fd;
      T7(t748_bracket)(f, ctx, &s, c);
      --count;
    }
  }
  while (count && s.fa != 0 && !T7(orc_tol_reached)(eps, s.a, s.b)) {
    a0 = s.a; b0 = s.b;
    c = T7(t748_prof)(&s, fe) ? T7(t748_quadratic)(s.a, s.b, s.d, s.fa, s.fb, s.fd, 2)
                          : T7(t748_cubic)(s.a, s.b, s.d, e, s.fa, s.fb, s.fd, fe);
    e = s.d; fe = s.fd;
    T7(t748_bracket)(f, ctx, &s, c);
    if (0 == --count || s.fa == 0 || T7(orc_tol_reached)(eps, s.a, s.b)) break;
    c = T7(t748_prof)(&s, fe) ? T7(t748_quadratic)(s.a, s.b, s.d, s.fa, s.fb, s.fd, 3)
                          : T7(t748_cubic)(s.a, s.b, s.d, e, s.fa, s.fb, s.fd, fe);
    T7(t748_bracket)(f, ctx, &s, c);
    if (0 == --count || s.fa == 0 || T7(orc_tol_reached)(eps, s.a, s.b)) break;
    if (fabs(s.fa) < fabs(s.fb)) { u = s.a; fu = s.fa; } else { u = s.b; fu = s.fb; }
    c = u - 2 * (fu / (s.fb - s.fa)) * (s.b - s.a);
    if (fabs(c - u) > (s.b - s.a) / 2) c = s.a + (s.b - s.a) / 2;
    e = s.d; fe = s.fd;
    T7(t748_bracket)(f, ctx, &s, c);
    if (0 == --count || s.fa == 0 || T7(orc_tol_reached)(eps, s.a, s.b)) break;
    if ((s.b - s.a) < mu * (b0 - a0)) continue;
    e = s.d; fe = s.fd;
    T7(t748_bracket)(f, ctx, &s, s.a + (s.b - s.a) / 2);
    --count;
  }
  *max_iter -= count;
  if (s.fa == 0) s.b = s.a; else if (s.fb == 0) s.a = s.b;
  return (s.a + s.b) / 2;
}
