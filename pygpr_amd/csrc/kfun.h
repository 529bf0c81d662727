// Device helpers shared by the covariance / gradient tile kernels (kbuild.hip: VALU bodies; kmfma.hip: matrix-pipe bodies).
// pg_exp: the direct-difference VALU bodies (kind_eval below; xgrad.hip).  pg_exp_tab: the VALU build's fast body (fp64 squared exponential)
// and every fp64 matrix-pipe body, whose Matern forms take their root from pg_sqrt_pos (the fp32 ones use the hardware's own, kmfma.hip).
#pragma once
#include "common.h"

// exp for the covariance kernels: branch-free, 2^k * P13(r) with r = x - k ln2 (two-term reduction) and the
// Taylor polynomial to degree 13 on |r| <= ln2/2 (truncation 4e-18 relative); <= 2 ulp, subnormal results via
// v_ldexp_f64.  Arguments are <= 0 here; anything below -800 gives 0.
__device__ __forceinline__ double pg_exp(double x) {
    x = (x < -800.0) ? -800.0 : x;      // not fmax: a NaN argument (NaN coordinate or hyper-parameter) must stay NaN
    const double kf = __builtin_rint(x * 1.44269504088896338700e+00);
    double r = __builtin_fma(-kf, 6.93147180369123816490e-01, x);
    r = __builtin_fma(-kf, 1.90821492927058770002e-10, r);
    double p = 1.6059043836821613e-10;                  // 1/13!
    p = __builtin_fma(p, r, 2.08767569878681e-09);      // 1/12!
    p = __builtin_fma(p, r, 2.505210838544172e-08);     // 1/11!
    p = __builtin_fma(p, r, 2.755731922398589e-07);     // 1/10!
    p = __builtin_fma(p, r, 2.7557319223985893e-06);    // 1/9!
    p = __builtin_fma(p, r, 2.48015873015873e-05);      // 1/8!
    p = __builtin_fma(p, r, 1.984126984126984e-04);     // 1/7!
    p = __builtin_fma(p, r, 1.388888888888889e-03);     // 1/6!
    p = __builtin_fma(p, r, 8.333333333333333e-03);     // 1/5!
    p = __builtin_fma(p, r, 4.1666666666666664e-02);    // 1/4!
    p = __builtin_fma(p, r, 1.6666666666666666e-01);    // 1/3!
    p = __builtin_fma(p, r, 0.5);
    p = __builtin_fma(p, r, 1.0);
    p = __builtin_fma(p, r, 1.0);
    return ldexp(p, (int)kf);
}
__device__ __forceinline__ float pg_exp(float x) { return expf(x); }

// The covariance build's own exponential (round 3): the build is bound by fp64 VALU issue, and the degree-13 chain above is half of an
// element's instructions.  Here x = (32 e + j) ln2 / 32 + r with |r| <= ln2 / 64: 2^(j/32) comes from a 32-entry table in LDS
// (32 doubles cover the 64 banks once: no conflicts between distinct entries), exp(r) from the Taylor polynomial to degree 6
// (truncation r^7 / 7! < 3.5e-18), 2^e from v_ldexp_f64: 13 fp64 operations instead of 21, <= 2 ulp.  `tab` may carry a factor
// (the component's sigma^2) -- the product costs nothing then.
static __device__ const double pg_exp2_32[32] = {
    1.00000000000000000e+00, 1.02189714865411663e+00, 1.04427378242741375e+00, 1.06714040067682370e+00,
    1.09050773266525769e+00, 1.11438674259589243e+00, 1.13878863475669156e+00, 1.16372485877757748e+00,
    1.18920711500272103e+00, 1.21524735998046896e+00, 1.24185781207348400e+00, 1.26905095719173322e+00,
    1.29683955465100964e+00, 1.32523664315974132e+00, 1.35425554693689265e+00, 1.38390988196383202e+00,
    1.41421356237309515e+00, 1.44518080697704665e+00, 1.47682614593949935e+00, 1.50916442759342284e+00,
    1.54221082540794074e+00, 1.57598084510788650e+00, 1.61049033194925428e+00, 1.64575547815396495e+00,
    1.68179283050742900e+00, 1.71861929812247793e+00, 1.75625216037329945e+00, 1.79470907500310717e+00,
    1.83400808640934243e+00, 1.87416763411029996e+00, 1.91520656139714740e+00, 1.95714412417540018e+00};
__device__ __forceinline__ double pg_exp_tab(double x, const double* tab) {
    x = (x < -800.0) ? -800.0 : x;      // (a NaN argument stays NaN)
    const double kf = __builtin_rint(x * 4.61662413084468283841e+01);              // 32 / ln2
    double r = __builtin_fma(-kf, 2.16608493865351192653e-02, x);                   // ln2 / 32, upper 32 bits: kf * hi is exact
    r = __builtin_fma(-kf, 5.96317165397058656257e-12, r);
    const int k = (int)kf;
    double p = 1.3888888888888889e-03;                  // 1/6!
    p = __builtin_fma(p, r, 8.3333333333333332e-03);    // 1/5!
    p = __builtin_fma(p, r, 4.1666666666666664e-02);    // 1/4!
    p = __builtin_fma(p, r, 1.6666666666666666e-01);    // 1/3!
    p = __builtin_fma(p, r, 0.5);
    p = __builtin_fma(p, r, 1.0);
    p = __builtin_fma(p, r, 1.0);
    return ldexp(p * tab[k & 31], k >> 5);
}

// sqrt(x) for x >= 0 in the Matern kernels' radial distance (a NaN stays a NaN): v_rsq_f64 refined by one Newton step on 1/sqrt and one on
// the root itself (both quadratic: <= 1 ulp whatever the instruction's own precision) -- nine fp64 operations where the IEEE expansion
// of sqrt() with its range scaling is about twenty.  Arguments below 1e-280 (a point against itself) return about 1e-140: every term
// the kernels form from r then rounds exactly as with r = 0; arguments above 1e300 (points an overflow apart) are taken as 1e300 -- the
// reciprocal root of infinity is 0 and would turn the result into a NaN where the covariance is simply 0.
__device__ __forceinline__ double pg_sqrt_pos(double x) {
    x = (x < 1.0e-280) ? 1.0e-280 : x;
    x = (x > 1.0e300) ? 1.0e300 : x;
    double y = __builtin_amdgcn_rsq(x);
    const double t = __builtin_fma(-0.5 * x * y, y, 0.5);
    y = __builtin_fma(y, t, y);
    double r = x * y;
    r = __builtin_fma(__builtin_fma(-r, r, x), 0.5 * y, r);
    return r;
}

// sin(pi t) and cos(pi t) for the periodic kernel: branch-free, r = t - rint(t) (exact: |r| <= 1/2, odd in t, so sin^2 is exactly
// even in the difference it came from), then the Taylor polynomials of sin(pi r) = r S(r^2) and cos(pi r) = C(r^2) with the powers of
// pi folded into the coefficients -- no product pi * r is ever rounded.  fp64: S to r^21 and C to r^22, truncation (pi/2)^23 / 23! =
// 1.3e-18 and (pi/2)^24 / 24! = 8e-20; fp32: S to r^13 and C to r^14 (7e-10, 7e-11).  No other argument reduction is needed, so the
// n^2 d evaluations of a build never meet the device library's large-argument path.  A NaN stays a NaN, an infinite t (a period of 0)
// becomes one (inf - inf).  Measured against a 50-digit evaluation over t in [-40, 40]: DESIGN.md 4.9b.
#define PG_PI 3.14159265358979323846
__device__ __forceinline__ void pg_sincospi(double t, double* s, double* c) {
    const double r = t - __builtin_rint(t);
    const double z = r * r;
    double p = 5.392664662608129e-10;                    // pi^21 / 21!
    p = __builtin_fma(p, z, -2.2948428997269873e-08);    // -pi^19 / 19!
    p = __builtin_fma(p, z, 7.952054001475513e-07);      // pi^17 / 17!
    p = __builtin_fma(p, z, -2.1915353447830217e-05);    // -pi^15 / 15!
    p = __builtin_fma(p, z, 4.6630280576761255e-04);     // pi^13 / 13!
    p = __builtin_fma(p, z, -7.3704309457143504e-03);    // -pi^11 / 11!
    p = __builtin_fma(p, z, 8.214588661112823e-02);      // pi^9 / 9!
    p = __builtin_fma(p, z, -5.992645293207921e-01);     // -pi^7 / 7!
    p = __builtin_fma(p, z, 2.5501640398773455);         // pi^5 / 5!
    p = __builtin_fma(p, z, -5.16771278004997);          // -pi^3 / 3!
    p = __builtin_fma(p, z, 3.141592653589793);          // pi
    *s = r * p;
    double q = -7.700707130601354e-11;                   // -pi^22 / 22!
    q = __builtin_fma(q, z, 3.604730797462501e-09);      // pi^20 / 20!
    q = __builtin_fma(q, z, -1.3878952462213771e-07);    // -pi^18 / 18!
    q = __builtin_fma(q, z, 4.303069587032947e-06);      // pi^16 / 16!
    q = __builtin_fma(q, z, -1.046381049248457e-04);     // -pi^14 / 14!
    q = __builtin_fma(q, z, 1.9295743094039231e-03);     // pi^12 / 12!
    q = __builtin_fma(q, z, -2.580689139001406e-02);     // -pi^10 / 10!
    q = __builtin_fma(q, z, 2.353306303588932e-01);      // pi^8 / 8!
    q = __builtin_fma(q, z, -1.3352627688545895);        // -pi^6 / 6!
    q = __builtin_fma(q, z, 4.0587121264167685);         // pi^4 / 4!
    q = __builtin_fma(q, z, -4.934802200544679);         // -pi^2 / 2!
    *c = __builtin_fma(q, z, 1.0);
}
__device__ __forceinline__ void pg_sincospi(float t, float* s, float* c) {
    const float r = t - __builtin_rintf(t);
    const float z = r * r;
    float p = 4.6630280576761255e-04f;                   // pi^13 / 13!
    p = __builtin_fmaf(p, z, -7.3704309457143504e-03f);
    p = __builtin_fmaf(p, z, 8.214588661112823e-02f);
    p = __builtin_fmaf(p, z, -5.992645293207921e-01f);
    p = __builtin_fmaf(p, z, 2.5501640398773455f);
    p = __builtin_fmaf(p, z, -5.16771278004997f);
    p = __builtin_fmaf(p, z, 3.141592653589793f);
    *s = r * p;
    float q = -1.046381049248457e-04f;                   // -pi^14 / 14!
    q = __builtin_fmaf(q, z, 1.9295743094039231e-03f);
    q = __builtin_fmaf(q, z, -2.580689139001406e-02f);
    q = __builtin_fmaf(q, z, 2.353306303588932e-01f);
    q = __builtin_fmaf(q, z, -1.3352627688545895f);
    q = __builtin_fmaf(q, z, 4.0587121264167685f);
    q = __builtin_fmaf(q, z, -4.934802200544679f);
    *c = __builtin_fmaf(q, z, 1.0f);
}

// Half the factor `coef` of the length-scale derivative dK/dl_k = coef base l_k D_k^2, per stationary kind (base: see kind_eval).  The
// periodic kind has sin^2(pi D_k / p_k) where the others have D_k^2: dK/dl_k = -2 K l_k s_k^2, the squared exponential's factor.
__device__ __forceinline__ double kind_hcoef(int kind) {
    if (kind == PG_KIND_RBF || kind == PG_KIND_RQ || kind == PG_KIND_PERIODIC) return -1.0;
    if (kind == PG_KIND_MATERN52) return 0.5 * -(5.0 / 3.0);
    if (kind == PG_KIND_MATERN32) return -1.5;
    return -0.5;                               // PG_KIND_MATERN12
}

// Hyper-parameters of one stationary child of this kind at dimension d: [sigma, l_1..l_d], and for the rational quadratic its shape
// alpha behind them (at off + d + 1), for the periodic kind its d periods there (off + d + 1 .. off + 2 d).  Everything that walks a
// child's block asks here instead of assuming d + 1.
__host__ __device__ constexpr int kind_nparam(int kind, int d) {
    return kind == PG_KIND_PERIODIC ? 2 * d + 1 : (kind == PG_KIND_RQ ? d + 2 : d + 1);
}
// The periodic kind's terms of one coordinate pair from t = D_k / p_k:  s2 = sin^2(pi t)  (the scaled distance is sum_k l_k^2 s2_k and
// K = sigma^2 exp(-sq): the squared exponential's radial function),  s2w = sin(2 pi t) = 2 sin cos  (the period and test-point derivatives:
// dK/dp_k = K l_k^2 s2w pi t / p_k,  dK/dx*_k = -K l_k^2 s2w pi / p_k).  The phase comes from the DIFFERENCE: the warped-point form
// (the squared exponential on (l/2) [cos, sin](2 pi x / p)) takes the phase of the coordinate and loses |x| / p ulps.
template <typename T> __device__ __forceinline__ void per_terms(T t, T& s2, T& s2w) {
    T s, c;
    pg_sincospi(t, &s, &c);
    s2 = s * s;
    s2w = (T)2 * s * c;
}
template <typename T> __device__ __forceinline__ T per_sin2(T t) {
    T s2, s2w;
    per_terms(t, s2, s2w);
    return s2;
}
// The squared shape a = alpha^2 of component c (0 for the kinds without one: their blocks end at l_d and hp[off + d + 1] is not theirs)
__device__ __forceinline__ double kind_shape2(const pg_covspec& spec, const double* hp, int c, int d) {
    if (spec.kind[c] != PG_KIND_RQ) return 0.0;
    const double al = hp[spec.off[c] + d + 1];
    return al * al;
}

// 1 / u for u >= 1 (a NaN stays a NaN): v_rcp_f64 and two Newton steps, <= 1 ulp -- five fp64 operations where the IEEE division
// with its scaling is about fifteen.
__device__ __forceinline__ double pg_rcp_ge1(double u) {
    double y = __builtin_amdgcn_rcp(u);
    y = __builtin_fma(y, __builtin_fma(-u, y, 1.0), y);
    y = __builtin_fma(y, __builtin_fma(-u, y, 1.0), y);
    return y;
}
__device__ __forceinline__ float pg_rcp_ge1(float u) { return 1.0f / u; }

// Rational quadratic from the scaled squared distance sq, the squared shape a = alpha^2 and ia = 1 / a:  t = sq / a,
//   lg = log1p(t),  ex = exp(-a lg) = (1 + t)^-a  (no sigma^2: the caller's exponential may carry it),  iu = 1 / (1 + t),
//   fs = t / (1 + t) - log1p(t)  the factor of the shape derivative, dK/dalpha = 2 alpha K fs (0 at sq = 0, -t^2 / 2 + O(t^3) near it).
// The logarithm is the device library's log1p: exact to an ulp for the small t of a large shape, where K tends to the squared
// exponential and log(1 + t) would lose every digit of t.  t beyond 1e300 (points an overflow apart) is taken as 1e300: K is 0 there
// either way, and 1 / (1 + inf) would turn `base` into a NaN.  Select, not fmin: a NaN coordinate or hyper-parameter stays NaN.
// alpha = 0 gives NaN (0 * inf) and is not worked around.
template <typename T> struct RqTerms { T arg, iu, fs; };      // arg = -a lg: the exponential's argument
template <typename T> __device__ __forceinline__ RqTerms<T> rq_terms(T sq, T a, T ia) {
    T t = sq * ia;
    const T big = sizeof(T) == 8 ? (T)1.0e300 : (T)1.0e30f;
    t = (t > big) ? big : t;
    const T lg = log1p(t);
    RqTerms<T> r;
    r.arg = -a * lg;
    r.iu = pg_rcp_ge1((T)1 + t);
    r.fs = t * r.iu - lg;
    return r;
}

// THE definition of every kind for the VALU bodies: covariance value kv and the factor `base` of dK/dl_k from the scaled squared
// distance sq of direct differences (the Matern-1/2 factor 1/r is only formed from an exact sq, so it is bounded by |D_k| after the
// multiplication by l_k D_k^2; 0 at sq = 0, the derivative's limit there).  The rational quadratic also takes its squared shape a and
// 1 / a, and gives fs, its shape derivative over 2 alpha: dK/dalpha = 2 alpha fs.  The kind is a template parameter: callers dispatch on it
// OUTSIDE their element loops.  The matrix-pipe bodies have forms of their own (KmVal in kmfma.hip: other primitives, other bits).
template <typename T, int KIND> __device__ __forceinline__ void kind_eval(T sig2, T sq, T& kv, T& base, T a, T ia, T& fs) {
    fs = (T)0;
    if constexpr (KIND == PG_KIND_RBF) {
        kv = base = sig2 * pg_exp(-sq);
    } else if constexpr (KIND == PG_KIND_RQ) {
        const RqTerms<T> q = rq_terms<T>(sq, a, ia);
        kv = sig2 * pg_exp(q.arg);
        base = kv * q.iu;
        fs = kv * q.fs;
    } else if constexpr (KIND == PG_KIND_SQDIST) {       // Squared_exponential.distance (covar.py:102-127): the scaled squared distance itself
        kv = sq;
        base = (T)0;
    } else if constexpr (KIND == PG_KIND_MATERN12) {
        const T rr = sqrt(sq);
        const T ex = sig2 * pg_exp(-rr);
        kv = ex;
        base = sq == (T)0 ? (T)0 : ex / rr;
    } else if constexpr (KIND == PG_KIND_MATERN32) {
        const T s3 = (T)1.73205080756887729353;
        const T rr = sqrt(sq);
        const T ex = pg_exp(-s3 * rr);
        kv = sig2 * ((T)1 + s3 * rr) * ex;
        base = sig2 * ex;
    } else {
        static_assert(KIND == PG_KIND_MATERN52, "unknown kernel kind");
        const T s5 = (T)2.23606797749978969641;
        const T rr = sqrt(sq);
        const T ex = pg_exp(-s5 * rr);
        kv = sig2 * ((T)1 + s5 * rr + (T)(5.0 / 3.0) * sq) * ex;
        base = sig2 * ((T)1 + s5 * rr) * ex;
    }
}
template <typename T, int KIND> __device__ __forceinline__ void kind_eval(T sig2, T sq, T& kv, T& base) {
    static_assert(KIND != PG_KIND_RQ, "the rational quadratic needs its shape");
    T fs;
    kind_eval<T, KIND>(sig2, sq, kv, base, (T)0, (T)0, fs);
}
// the value alone (the covariance build): `base` is dead code there
template <typename T, int KIND> __device__ __forceinline__ T kind_value(T sig2, T sq, T a = (T)0, T ia = (T)0) {
    T kv, base, fs;
    kind_eval<T, KIND>(sig2, sq, kv, base, a, ia, fs);
    return kv;
}
// kv and base (and the rational quadratic's fs; 0 otherwise) of a kind other than the squared exponential, chosen at run time (the
// direct-difference gradient kernels)
template <typename T> __device__ __forceinline__ void matern_val(int kind, T sig2, T sq, T& kv, T& base, T a, T ia, T& fs) {
    fs = (T)0;
    if (kind == PG_KIND_RQ) kind_eval<T, PG_KIND_RQ>(sig2, sq, kv, base, a, ia, fs);
    else if (kind == PG_KIND_MATERN12) kind_eval<T, PG_KIND_MATERN12>(sig2, sq, kv, base);
    else if (kind == PG_KIND_MATERN32) kind_eval<T, PG_KIND_MATERN32>(sig2, sq, kv, base);
    else kind_eval<T, PG_KIND_MATERN52>(sig2, sq, kv, base);
}

// Strip (tile row tr, first tile tcs, ntile tiles) of workgroup `b` of a 1-D grid: a workgroup walks up to S consecutive tiles of
// one tile row.  Symmetric builds launch ONLY tiles on or below the diagonal (round 2 launched the full square and let the upper
// half exit at once): column window [c0, c1) in tiles --
//   tile rows c0 .. c1-1 hold r' + 1 tiles (r' = tr - c0: the triangle) = ceil((r' + 1) / S) strips,
//   tile rows c1 .. T-1 hold W = c1 - c0 tiles (the rectangle below it) = ceil(W / S) strips.
__host__ __device__ __forceinline__ long kb_strips_before(int rp, int S) {      // strips in triangle rows 0 .. rp-1
    const long q = rp / S, rem = rp % S;
    return (long)S * q * (q + 1) / 2 + rem * (q + 1);
}
__device__ __forceinline__ void kb_strip_of(int b, int symmetric, int c0, int c1, int S, int& tr, int& tcs, int& ntile) {
    const int W = c1 - c0, SW = (W + S - 1) / S;
    if (!symmetric) {
        tr = b / SW;
        tcs = c0 + (b % SW) * S;
        ntile = min(S, c1 - tcs);
        return;
    }
    const int ntri = (int)kb_strips_before(W, S);
    if (b < ntri) {
        int q = (int)((sqrtf(1.0f + 8.0f * (float)b / (float)S) - 1.0f) * 0.5f);
        while (q > 0 && (long)S * q * (q + 1) / 2 > b) --q;
        while ((long)S * (q + 1) * (q + 2) / 2 <= b) ++q;
        const int within = b - S * q * (q + 1) / 2;         // strips into the block of S rows that hold q + 1 strips each
        const int rem = within / (q + 1), sidx = within % (q + 1);
        const int rp = S * q + rem;
        tr = c0 + rp;
        tcs = c0 + sidx * S;
        ntile = min(S, rp + 1 - sidx * S);
    } else {
        const int j = b - ntri;
        tr = c1 + j / SW;
        tcs = c0 + (j % SW) * S;
        ntile = min(S, c1 - tcs);
    }
}

