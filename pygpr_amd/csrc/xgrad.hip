// Derivatives of a prediction with respect to the test points: the weighted contraction of the kernel's first-argument derivative
//
//   out[p][k] = sum_i W_pi dk(x*_p, z_i) / dx*_pk,   dk/dx*_pk = 2 kind_hcoef(kind) base(r) l_k^2 D_k,   D_k = x*_pk - z_ik
//
// summed over the stationary children of the Compose (white noise has no cross term).  W is a vector u (W_pi = u_i) and / or a dense
// matrix B (W_pi = B_pi, row-major or stored transposed); both outputs come out of ONE pass over the pairs.  The reference's predict
// (gpr.py:76-120) has no derivative in x*; the three Python callers (gpr.py here: predict_grad and the autograd backward) reduce the
// mean, the diagonal variance and the full covariance to this form.
//
// Layout: a workgroup owns 64 test points (one per lane, its point held in registers up to d = 16) and a CHUNK of the training points:
// few test points against many training points is the common call (Bayesian optimisation: m = 1-1000, n ~ 1e4), and row tiles alone
// would leave the chip idle there.  The chunks' partial sums go to a workspace; pg_xgrad_reduce_kernel adds them up (the `part` +
// pg_grad_reduce_kernel pattern of the NLML gradient).  The 64 training points of a tile, their u and the 64 x 64 tile of B are staged
// in LDS; the four waves take sixteen training points each, and their accumulators meet in LDS at the end.
//   * differences are DIRECT and appear to the first power: an expansion x*_pk sum W base - sum W base z_ik cancels on data away from
//     the origin;
//   * the squared distance is formed in the model's dtype as the covariance build forms it; everything downstream is fp64;
//   * Matern-1/2 has a cusp at r = 0: matern_val's base is 0 there (the derivative's limit along any direction is bounded, its sign is
//     not), so a test point on a training point contributes nothing for that pair;
//   * a NaN coordinate of a test point reaches that point's row only (pg_exp keeps a NaN, matern_val's selects are NaN-transparent);
//   * the periodic kind has dk/dx*_pk = -K l_k^2 sin(2 pi D_k / p_k) pi / p_k: the same contraction with sin(2 pi t_k) pi / (2 p_k) in
//     the place of D_k and K as `base`, the phase taken from the difference (per_terms, kfun.h); 1 / p_k is staged beside l^2.
//   * a product spec (PG_SPEC_PRODUCT, stripped by the host; the PROD instantiation): dk/dx* = sum_c (prod_{c' != c} k_c') dk_c/dx*, so
//     each component's factor f of a pair is multiplied by the other components' values at that pair (`others`), for u and B alike;
//     the product is formed explicitly, never as K / k_c: a factor that underflows gives 0.
#include "kbuild.h"
#include "kfun.h"
#include "kpair.h"
#include <type_traits>

#define XT 64        // test points of a workgroup = training points of a staged tile
#define BLD 65       // odd leading dimension of the staged B tile: a lane reads its own row

struct XgradBatch {  // strides between batched experts (elements); 0 shares an operand
    long eq, ez, ehp, eu, eb;
};

// HOLD (d <= 16): the test point and the sixteen differences of a pair live in registers; otherwise the test points are read from
// LDS and the accumulators cover KC = 16 coordinates per pass (passes over the coordinates repeat the distances: d > 16 is rare).
// LDS of pg_xgrad_kernel in bytes: red, the training tile, (!HOLD) the test points, l2s, us, bs, ips -- the carve-up below
template <typename T, int DMAX> static constexpr size_t xgrad_lds_bytes() {
    constexpr int KC = DMAX <= 16 ? DMAX : 16;
    return (size_t)4 * KC * XT * sizeof(double) +
           (size_t)(XT * DMAX + (DMAX <= 16 ? 0 : XT * (DMAX + 1)) + 2 * PG_MAX_COMP * DMAX + XT + XT * BLD) * sizeof(T);
}
template <typename T, int DMAX, bool HU, bool HB, bool PROD = false>
__global__ __launch_bounds__(256) void pg_xgrad_kernel(pg_covspec spec, const double* __restrict__ hp, const T* __restrict__ Xq, long ldq,
                                                       int m, const T* __restrict__ Z, long ldz, int n, int d, const T* __restrict__ u,
                                                       const T* __restrict__ B, long ldb, int trans_b, double* __restrict__ part, int ct,
                                                       long mrows, XgradBatch xb) {
    constexpr bool HOLD = DMAX <= 16;
    constexpr int KC = HOLD ? DMAX : 16;
    const int e = blockIdx.z;
    Xq += e * xb.eq; Z += e * xb.ez; hp += e * xb.ehp;
    if (HU) u += e * xb.eu;
    if (HB) B += e * xb.eb;
    const int nsplit = gridDim.x, sp = blockIdx.x, row0 = blockIdx.y * XT;
    const long psz = (long)nsplit * d * mrows;               // one output's partial sums of one expert
    part += (long)e * 2 * psz;
    const int tiles = (n + XT - 1) / XT;
    const int t0 = sp * ct, t1 = min(t0 + ct, tiles);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* red = reinterpret_cast<double*>(smem_raw);       // [4 waves][KC][64]
    T* xc = reinterpret_cast<T*>(red + 4 * KC * XT);         // [64][DMAX] training points, zero beyond d / n
    T* xrs = xc + XT * DMAX;                                  // !HOLD: [64][DMAX + 1] test points
    T* l2s = xrs + (HOLD ? 0 : XT * (DMAX + 1));              // [ncomp][DMAX] squared inverse length scales, zero beyond d
    T* us = l2s + PG_MAX_COMP * DMAX;                         // [64]
    T* bs = us + XT;                                          // [64][BLD]: bs[p][i] = W of test point p, training point i
    T* ips = bs + XT * BLD;                                   // [ncomp][DMAX] reciprocal periods of the periodic children, zero otherwise

    const int p = row0 + lane;
    T xr[HOLD ? DMAX : 1];
    if constexpr (HOLD) {
#pragma unroll
        for (int k = 0; k < DMAX; ++k) xr[k] = (p < m && k < d) ? Xq[(long)p * ldq + k] : (T)0;
    } else {
        for (int idx = tid; idx < XT * DMAX; idx += 256) {
            const int r = idx / DMAX, k = idx % DMAX, g = row0 + r;
            xrs[r * (DMAX + 1) + k] = (g < m && k < d) ? Xq[(long)g * ldq + k] : (T)0;
        }
    }
    pair_stage_hp<T, true>(spec, hp, d, DMAX, DMAX, l2s, ips, tid, 256);      // (1 / p_k is always staged: no instantiation of its own)

    // PROD: the product of the values of every component but cp at (this lane's test point, the staged training point zc)
    auto others = [&](int cp, const T* zc) -> double {
        double oth = 1.0;
        auto xa = [&](int k) { return HOLD ? xr[HOLD ? k : 0] : xrs[lane * (DMAX + 1) + k]; };
        auto xz = [&](int k) { return zc[k]; };
        for (int c2 = 0; c2 < spec.ncomp; ++c2)
            if (c2 != cp) oth *= (double)pair_value<T, DMAX>(spec, hp, c2, d, l2s + c2 * DMAX, ips + c2 * DMAX, xa, xz);
        return oth;
    };

    for (int k0 = 0; k0 < (HOLD ? 1 : d); k0 += KC) {
        double au[KC], ab[KC];
#pragma unroll
        for (int kk = 0; kk < KC; ++kk) au[kk] = ab[kk] = 0.0;
        for (int cp = 0; cp < spec.ncomp; ++cp) {
            const int kind = spec.kind[cp];
            const double sg = hp[spec.off[cp]];
            const T sig2 = (T)(sg * sg);
            const double f2 = 2.0 * kind_hcoef(kind);
            const double sh = kind_shape2(spec, hp, cp, d);
            const T sha = (T)sh, ish = (T)(1.0 / sh);      // rational quadratic: alpha^2, 1 / alpha^2
            const T* lc = l2s + cp * DMAX;
            for (int tc = t0; tc < t1; ++tc) {
                __syncthreads();          // the previous tile's readers are done (and, first time round, l2s / xrs are published below)
                for (int idx = tid; idx < XT * DMAX; idx += 256) {
                    const int c = idx / DMAX, k = idx % DMAX, g = tc * XT + c;
                    xc[idx] = (g < n && k < d) ? Z[(long)g * ldz + k] : (T)0;
                }
                if (HU && tid < XT) {
                    const int g = tc * XT + tid;
                    us[tid] = g < n ? u[g] : (T)0;
                }
                if (HB) {
                    // padding rows / columns of B are never read: they weigh 0
                    for (int idx = tid; idx < XT * XT; idx += 256) {
                        const int a = idx >> 6, b = idx & 63;
                        if (!trans_b) {           // B[p][i]: a = test point, b = training point (64 lanes read one 64-element row run)
                            const int gp = row0 + a, gi = tc * XT + b;
                            bs[a * BLD + b] = (gp < m && gi < n) ? B[(long)gp * ldb + gi] : (T)0;
                        } else {                  // B stored transposed, Bt[i][p]: a = training point, b = test point
                            const int gi = tc * XT + a, gp = row0 + b;
                            bs[b * BLD + a] = (gp < m && gi < n) ? B[(long)gi * ldb + gp] : (T)0;
                        }
                    }
                }
                __syncthreads();
                if (kind == PG_KIND_PERIODIC) {
                    const T* ipc = ips + cp * DMAX;
                    for (int j = 0; j < 16; ++j) {
                        const int c = wave * 16 + j;
                        const T* zc = xc + c * DMAX;
                        T sq = (T)0;
#pragma unroll
                        for (int k = 0; k < DMAX; ++k)
                            sq += lc[k] * per_sin2<T>(((HOLD ? xr[k] : xrs[lane * (DMAX + 1) + k]) - zc[k]) * ipc[k]);
                        double f = f2 * (double)(sig2 * pg_exp(-sq));
                        if constexpr (PROD) f *= others(cp, zc);
                        const double wu = HU ? f * (double)us[c] : 0.0;
                        const double wb = HB ? f * (double)bs[lane * BLD + c] : 0.0;
#pragma unroll
                        for (int kk = 0; kk < KC; ++kk) {
                            const int k = k0 + kk;
                            T s2, s2w;
                            per_terms<T>(((HOLD ? xr[HOLD ? kk : 0] : xrs[lane * (DMAX + 1) + k]) - zc[k]) * ipc[k], s2, s2w);
                            const double t = (double)lc[k] * (double)s2w * (0.5 * PG_PI) * (double)ipc[k];
                            if (HU) au[kk] += wu * t;
                            if (HB) ab[kk] += wb * t;
                        }
                    }
                    continue;
                }
#pragma unroll 2
                for (int j = 0; j < 16; ++j) {
                    const int c = wave * 16 + j;
                    const T* zc = xc + c * DMAX;
                    T df[HOLD ? DMAX : 1];
                    T sq = (T)0;
#pragma unroll
                    for (int k = 0; k < DMAX; ++k) {
                        const T dd = (HOLD ? xr[k] : xrs[lane * (DMAX + 1) + k]) - zc[k];
                        if constexpr (HOLD) df[k] = dd;
                        sq += lc[k] * dd * dd;
                    }
                    T kv, bt, ft;
                    if (kind == PG_KIND_RBF) bt = sig2 * pg_exp(-sq);
                    else matern_val<T>(kind, sig2, sq, kv, bt, sha, ish, ft);
                    double f = f2 * (double)bt;
                    if constexpr (PROD) f *= others(cp, zc);
                    const double wu = HU ? f * (double)us[c] : 0.0;
                    const double wb = HB ? f * (double)bs[lane * BLD + c] : 0.0;
#pragma unroll
                    for (int kk = 0; kk < KC; ++kk) {
                        const int k = k0 + kk;
                        T dd;
                        if constexpr (HOLD) dd = df[kk];
                        else dd = xrs[lane * (DMAX + 1) + k] - zc[k];
                        const double t = (double)lc[k] * (double)dd;
                        if (HU) au[kk] += wu * t;
                        if (HB) ab[kk] += wb * t;
                    }
                }
            }
        }
        // the four waves' sums of this coordinate block -> the chunk's partial row (k-major: 64 lanes write 64 consecutive doubles)
        auto flush = [&](const double* acc, int o) {
#pragma unroll
            for (int kk = 0; kk < KC; ++kk) red[(wave * KC + kk) * XT + lane] = acc[kk];
            __syncthreads();
            for (int idx = tid; idx < KC * XT; idx += 256) {
                const int kk = idx / XT, l = idx % XT, k = k0 + kk;
                if (k < d)
                    part[o * psz + ((long)sp * d + k) * mrows + row0 + l] =
                        red[kk * XT + l] + red[(KC + kk) * XT + l] + red[(2 * KC + kk) * XT + l] + red[(3 * KC + kk) * XT + l];
            }
            __syncthreads();
        };
        if (HU) flush(au, 0);
        if (HB) flush(ab, 1);
    }
}

// out[e][p][k] (+)= sum over the chunks of the partial sums, in the output's dtype; one thread per (p, k), y = output
template <typename T>
__global__ __launch_bounds__(256) void pg_xgrad_reduce_kernel(const double* __restrict__ part, int nsplit, int m, int d, long mrows,
                                                              T* out_u, long ldou, long eou, T* out_b, long ldob, long eob, int accumulate) {
    const int e = blockIdx.z, o = blockIdx.y;
    T* out = o == 0 ? out_u : out_b;
    if (!out) return;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)m * d) return;
    const int p = (int)(idx / d), k = (int)(idx % d);
    const long psz = (long)nsplit * d * mrows;
    const double* src = part + (long)e * 2 * psz + o * psz + (long)k * mrows + p;
    double s = 0.0;
    for (int q = 0; q < nsplit; ++q) s += src[(long)q * d * mrows];
    T* dst = out + e * (o == 0 ? eou : eob) + (long)p * (o == 0 ? ldou : ldob) + k;
    *dst = accumulate ? (T)((double)*dst + s) : (T)s;
}

// Chunks of the training points: enough workgroups for four per compute unit, at least two tiles (128 points) per chunk.
static void xgrad_split(int ncu, int m, int n, int nexp, int& nsplit, int& ct) {
    const long tr = (m + XT - 1) / XT, tiles = std::max(1, (n + XT - 1) / XT);
    const long target = 4L * std::max(ncu, 1);
    long want = (target + tr * nexp - 1) / (tr * nexp);
    want = std::max(1L, std::min(want, std::max(1L, tiles / 2)));
    ct = (int)((tiles + want - 1) / want);
    nsplit = (int)((tiles + ct - 1) / ct);
}

long pg_xgrad_worksize_impl(int ncu, int m, int n, int d, int nexp) {
    if (m <= 0 || n <= 0 || d <= 0 || nexp <= 0) return 0;
    int nsplit, ct;
    xgrad_split(ncu, m, n, nexp, nsplit, ct);
    const long mrows = (long)((m + XT - 1) / XT) * XT;
    return 2L * nexp * nsplit * d * mrows;
}

template <typename T, int DMAX, bool HU, bool HB, bool PROD>
static int launch_xgrad(hipStream_t st, const pg_covspec& spec, const double* hp, const T* Xq, long ldq, int m, const T* Z, long ldz,
                        int n, int d, const T* u, const T* B, long ldb, int trans_b, double* part, int nsplit, int ct, long mrows,
                        const XgradBatch& xb, int nexp) {
    constexpr size_t lds = xgrad_lds_bytes<T, DMAX>();
    if (int rc = pg_lds_opt_in<pg_xgrad_kernel<T, DMAX, HU, HB, PROD>>(lds)) return rc;   // d > 16 in fp64 passes the 64 KB a kernel gets without opting in
    hipLaunchKernelGGL((pg_xgrad_kernel<T, DMAX, HU, HB, PROD>), dim3(nsplit, (m + XT - 1) / XT, nexp), dim3(256), lds, st, spec, hp, Xq, ldq, m, Z,
                       ldz, n, d, u, B, ldb, trans_b, part, ct, mrows, xb);
    PG_CHECK(hipGetLastError());
    return 0;
}

template <typename T, int DMAX, bool PROD>
static int launch_xgrad_w(hipStream_t st, const pg_covspec& spec, const double* hp, const T* Xq, long ldq, int m, const T* Z, long ldz,
                          int n, int d, const T* u, const T* B, long ldb, int trans_b, double* part, int nsplit, int ct, long mrows,
                          const XgradBatch& xb, int nexp) {
    if (u && B) return launch_xgrad<T, DMAX, true, true, PROD>(st, spec, hp, Xq, ldq, m, Z, ldz, n, d, u, B, ldb, trans_b, part, nsplit, ct, mrows, xb, nexp);
    if (u) return launch_xgrad<T, DMAX, true, false, PROD>(st, spec, hp, Xq, ldq, m, Z, ldz, n, d, u, B, ldb, trans_b, part, nsplit, ct, mrows, xb, nexp);
    return launch_xgrad<T, DMAX, false, true, PROD>(st, spec, hp, Xq, ldq, m, Z, ldz, n, d, u, B, ldb, trans_b, part, nsplit, ct, mrows, xb, nexp);
}

template <typename T>
int pg_xgrad_t(hipStream_t st, int ncu, const pg_covspec& spec_in, const double* hp, long hp_stride, const T* Xq, long ldq, long xq_stride, int m,
               const T* Z, long ldz, long z_stride, int n, int d, const T* u, long u_stride, T* out_u, long ldou, long ou_stride, const T* B,
               long ldb, long b_stride, int trans_b, T* out_b, long ldob, long ob_stride, int accumulate, double* work, long lwork, int nexp) {
    pg_covspec spec;
    const bool prod = pg_spec_strip(spec_in, spec);      // a product spec: the kernel's PROD instantiation
    if (m <= 0) return 0;
    if (n <= 0 || spec.ncomp == 0) {      // no training points / no stationary child: the derivative is 0
        if (accumulate) return 0;
        for (int e = 0; e < nexp; ++e)
            for (int o = 0; o < 2; ++o) {
                T* out = o == 0 ? out_u : out_b;
                if (!out) continue;
                const long ld = o == 0 ? ldou : ldob, es = o == 0 ? ou_stride : ob_stride;
                PG_CHECK(hipMemset2DAsync(out + e * es, ld * sizeof(T), 0, d * sizeof(T), m, st));
            }
        return 0;
    }
    int nsplit, ct;
    xgrad_split(ncu, m, n, nexp, nsplit, ct);
    const long need = pg_xgrad_worksize_impl(ncu, m, n, d, nexp);
    if (lwork < need) { pg_set_error("pg_kernel_xgrad: workspace %ld < %ld doubles", lwork, need); return -3; }
    const long mrows = (long)((m + XT - 1) / XT) * XT;
    const XgradBatch xb = {xq_stride, z_stride, hp_stride, u_stride, b_stride};
    auto go = [&](auto prod_c) {
        return pg_with_dmax(d, [&](auto dmax_c) {
            return launch_xgrad_w<T, decltype(dmax_c)::value, decltype(prod_c)::value>(st, spec, hp, Xq, ldq, m, Z, ldz, n, d, u, B, ldb, trans_b, work,
                                                                                     nsplit, ct, mrows, xb, nexp);
        });
    };
    const int rc = prod ? go(std::true_type{}) : go(std::false_type{});
    if (rc) return rc;
    hipLaunchKernelGGL(pg_xgrad_reduce_kernel<T>, dim3((unsigned)(((long)m * d + 255) / 256), 2, nexp), dim3(256), 0, st, work, nsplit, m, d,
                       mrows, out_u, ldou, ou_stride, out_b, ldob, ob_stride, accumulate);
    PG_CHECK(hipGetLastError());
    return 0;
}
template int pg_xgrad_t<double>(hipStream_t, int, const pg_covspec&, const double*, long, const double*, long, long, int, const double*, long,
                                long, int, int, const double*, long, double*, long, long, const double*, long, long, int, double*, long, long,
                                int, double*, long, int);
template int pg_xgrad_t<float>(hipStream_t, int, const pg_covspec&, const double*, long, const float*, long, long, int, const float*, long,
                               long, int, int, const float*, long, float*, long, long, const float*, long, long, int, float*, long, long,
                               int, double*, long, int);
