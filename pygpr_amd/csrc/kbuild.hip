// Covariance assembly (HBM-bound, O(n^2 d)) and the fused NLML-gradient contraction: entry points, routing and the VALU bodies.
//
// pg_kbuild: K[i][j] = sum_c k_c(r_i, c_j) (+ (sum sigma_n^2 + jitter) on the diagonal of a symmetric build); k_c is the ARD squared
// exponential of PyGPR/covar.py:129-167 (hp = [sigma, l_1..l_d], l are INVERSE length scales, no 1/2 in the exponent) or Matern-5/2,
// -3/2, -1/2 with the same hp layout, or the rational quadratic with its shape alpha behind that block (kind_nparam, kfun.h).  Rows/columns >= the real point count are padding: identity for a symmetric build (keeps the
// padded Cholesky trivial), zero for a cross build.  Which body serves which input:
//   * one child of kind SE / Matern-5/2 / Matern-3/2 / rational quadratic, d <= 16, no accumulate pass: the matrix-pipe kernel of kmfma.hip -- except the
//     fp64 squared exponential at d <= 8, which the FAST body here serves at 0.63-0.66 of the HBM peak;
//   * one fp64 SE child, no accumulate pass, d <= 8 or d > 16: kb_body<FAST>, the expansion |x|^2 + |x'|^2 - 2 x.x' on the VALU;
//   * any other single child (Matern-1/2, d > 16, an accumulate pass): kb_body<PRESC>, direct differences of coordinates
//     pre-multiplied by the inverse length scales;  several children: the general kb_body, l^2 applied per coordinate.
//   * a periodic child (hp = [sigma, l_1..l_d, p_1..p_d]: K = sigma^2 exp(-sum_k l_k^2 sin^2(pi D_k / p_k))), alone or among others: the
//     general kb_body in its PER instantiation -- the phase from the direct difference, 1 / p_k staged beside l^2; never PRESC, FAST or
//     the matrix pipe.
//   * a product spec (PG_SPEC_PRODUCT in ncomp, stripped here on the host: K = prod_c k_c, the locally periodic kernel SE x Periodic): the
//     general kb_body in its PROD instantiation, which always carries the periodic case; never PRESC, FAST or the matrix pipe.
// Direct differences are exactly symmetric and never negative (the reference expands into a GEMM, covar.py:102-127).  One 64x64
// output tile per 256-thread workgroup at a time; both point tiles are staged in LDS k-major ([d][64]); each thread owns a 4x4
// micro-tile whose columns are two 16-byte vectors, so every store instruction writes 256 contiguous bytes per row.
//
// pg_nlml_grad: g_k = 1/2 sum_ij (K^-1 - a a^T)_ij dK_ij/dtheta_k over the lower triangle, with dK recomputed from the point tiles
// on the fly: dK/dsigma = 2K/sigma, dK/dl_k = -2 l_k D_k^2 K (covar.py:169-206), dK/dsigma_n = 2 sigma_n I (covar.py:247-269); the
// Matern kinds as dK/dl_k = coef base l_k D_k^2 (kind_hcoef: coef / 2).  The reference materialises dK[nhp,n,n] and solves against
// it (loss.py:116-121); this is the same number by the K^-1 route.  The rational quadratic adds dK/dalpha = 2 alpha fs (rq_terms).  One
// child of kind SE / Matern-5/2 / Matern-3/2 / rational quadratic at d <= 16 takes
// the matrix-pipe contraction of kmfma.hip; everything else (Matern-1/2, the periodic kind, d > 16, several children, PG_GRAD_MFMA=0)
// takes pg_grad_kernel here: direct differences on the VALU.  The periodic kind: dK/dl_k = -2 K l_k s_k^2, dK/dp_k = K l_k^2
// sin(2 pi t_k) pi t_k / p_k with t_k = D_k / p_k, s_k = sin(pi t_k) (per_terms, kfun.h).
// A product spec: dK/dtheta_{c,j} = (prod_{c' != c} k_c') dk_c/dtheta_{c,j} -- pg_grad_kernel's PROD instantiation multiplies the
// element's weight by the other components' values, and every entry of c follows from the code of the sum.
#include "kbuild.h"
#include "kfun.h"
#include "kpair.h"
#include "kmfma.h"
#include <cstdlib>
#include <type_traits>

#define KT 64
#define TLD 65     // odd leading dimension of the LDS transpose tile: column writes are at worst 2-way conflicted

template <typename T> struct VecOf;
template <> struct VecOf<double> { typedef double type __attribute__((ext_vector_type(2))); static constexpr int N = 2; };
template <> struct VecOf<float> { typedef float type __attribute__((ext_vector_type(4))); static constexpr int N = 4; };

template <typename T>
__device__ __forceinline__ void stage_points(T* dst, const T* __restrict__ X, long ldx, int npts, int p0, int d, int tid,
                                             const double* __restrict__ scale = nullptr, double mul = 1.0) {
    // dst[k][64] <- X[p0 + p][k] (* scale[k]: coordinates pre-multiplied by the inverse length scales); points beyond npts read as zero
    for (int idx = tid; idx < KT * d; idx += 256) {
        const int p = idx / d, k = idx % d;
        const int gp = p0 + p;
        T v = (gp < npts) ? X[(long)gp * ldx + k] : (T)0;
        if (scale) v = (T)((double)v * scale[k] * mul);      // (mul = 2: exact)
        dst[k * KT + p] = v;
    }
}

// The 4 x 4 micro-tile of one thread: rows ty*4 + r, columns two (fp64) or one (fp32) 16-byte vectors at v*(16*VE) + tx*VE.
//   PRESC  : one stationary component whose inverse length scales were folded into the staged coordinates (sq += df * df)
//   CHECKED: the tile touches the diagonal, the padding or an accumulate pass -- per-element fix-ups; interior tiles skip them
// The kernel is bound by fp64 VALU issue, not by HBM, at d = 8 (about 250 VALU cycles per 64 elements against the 120 their
// stores take at 5.3 TB/s): both switches only remove instructions.
//   FAST   : (fp64, PRESC, the component is the squared exponential) the reference's own form of the squared distance,
//            |x|^2 + |x'|^2 - 2 x.x' (covar.py:102-127, there a matmul): one FMA per coordinate instead of a subtraction and an
//            FMA.  The rows are staged times two, -|x|^2 per point waits in LDS (nrm_r, nrm_c), so the accumulator STARTS at
//            -|x|^2 - |x'|^2 and ends as the exponential's argument; pg_exp_tab with sigma^2 folded into its table.
//   PER    : the spec holds a periodic component (never PRESC or FAST: l cannot be folded into the coordinates, the distance is
//            sum_k l_k^2 sin^2(pi D_k / p_k)).  Its coordinate loop takes the phase from the difference, t = D_k / p_k with 1 / p_k
//            staged beside l^2 (ipl); the radial function is the squared exponential's.  An instantiation of its own: the bodies
//            of the other kinds compile exactly as they did without it.
//   PROD   : a product spec (PG_SPEC_PRODUCT): the components' values are MULTIPLIED into the element instead of added (an accumulate
//            pass then adds the product to what is there).  Always with PER -- one instantiation carries every kind --, so never
//            PRESC, FAST or the matrix pipe.  A factor that underflows to 0 gives 0; a NaN factor stays NaN.
template <typename T, bool PRESC, bool CHECKED, bool MIRROR, bool FAST = false, bool PER = false, bool PROD = false>
__device__ __forceinline__ void kb_body(const pg_covspec& spec, const T* xr, const T* xc, const T* l2, const T* sg2, T* tt, int d,
                                        int tr, int tc, int nr, int nc, int symmetric, int accumulate, T* __restrict__ K, long ldk,
                                        int tid, const T* nrm_r = nullptr, const T* nrm_c = nullptr, const double* tab = nullptr,
                                        const T* ipl = nullptr) {
    static_assert(!PER || (!PRESC && !FAST), "the periodic kind takes the general direct-difference body only");
    static_assert(!PROD || PER, "a product takes the body that carries every kind");
    constexpr int VE = VecOf<T>::N, NVC = 4 / VE;   // vectors per row of the micro-tile
    typedef typename VecOf<T>::type vec_t;
    const int tx = tid & 15, ty = tid >> 4;
    T out[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) out[r][c] = (T)0;
    for (int cp = 0; cp < (FAST ? 1 : spec.ncomp); ++cp) {
        const T* lc = l2 + cp * d;
        T sq[4][4];      // the scaled squared distance; FAST: MINUS it, started at -|x|^2 - |x'|^2
        {
            T na[4], nb[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) na[r] = FAST ? nrm_r[ty * 4 + r] : (T)0;
#pragma unroll
            for (int v = 0; v < NVC; ++v)
#pragma unroll
                for (int e = 0; e < VE; ++e) nb[v * VE + e] = FAST ? nrm_c[v * (16 * VE) + tx * VE + e] : (T)0;
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) sq[r][c] = na[r] + nb[c];
        }
        bool periodic = false;
        if constexpr (PER) periodic = spec.kind[cp] == PG_KIND_PERIODIC;
        if constexpr (PER) {
            if (periodic) {
                const T* ipc = ipl + cp * d;
                for (int k = 0; k < d; ++k) {
                    T a[4], b[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) a[r] = xr[k * KT + ty * 4 + r];
#pragma unroll
                    for (int v = 0; v < NVC; ++v) {
                        const vec_t bv = *reinterpret_cast<const vec_t*>(xc + k * KT + v * (16 * VE) + tx * VE);
#pragma unroll
                        for (int e = 0; e < VE; ++e) b[v * VE + e] = bv[e];
                    }
                    const T w = lc[k], ip = ipc[k];
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int c = 0; c < 4; ++c) sq[r][c] += w * per_sin2<T>((a[r] - b[c]) * ip);
                }
            }
        }
#pragma unroll 2
        for (int k = 0; k < (periodic ? 0 : d); ++k) {      // (two coordinates' LDS reads in flight per trip; a periodic component is done)
            T a[4], b[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) a[r] = xr[k * KT + ty * 4 + r];
#pragma unroll
            for (int v = 0; v < NVC; ++v) {
                const vec_t bv = *reinterpret_cast<const vec_t*>(xc + k * KT + v * (16 * VE) + tx * VE);
#pragma unroll
                for (int e = 0; e < VE; ++e) b[v * VE + e] = bv[e];
            }
            const T w = (FAST || PRESC) ? (T)1 : lc[k];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (FAST) sq[r][c] += a[r] * b[c];
                    else if (PRESC) { const T df = a[r] - b[c]; sq[r][c] += df * df; }
                    else { const T df = a[r] - b[c]; sq[r][c] += w * df * df; }
                }
        }
        if (FAST) {
            // The expansion's absolute error is eps |x l|^2, not relative to the distance: near-duplicate points can come out with a slightly
            // POSITIVE argument (K_ij > sigma^2) and, in a symmetric build, the diagonal off sigma^2 by that error.  One v_min per element
            // keeps K_ij <= sigma^2; tiles on the diagonal take the exact 0 where a point meets itself (a NaN argument stays NaN).
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    T a = sq[r][c] > (T)0 ? (T)0 : sq[r][c];
                    if (CHECKED) {
                        if (symmetric && tr == tc && ty * 4 + r == (c / VE) * (16 * VE) + tx * VE + (c % VE) && a == a) a = (T)0;
                    }
                    out[r][c] = (T)pg_exp_tab((double)a, tab);
                }
        } else {
            // the kind is decided ONCE for the sixteen elements: with the dispatch inside the element loop every covariance value sat
            // behind its own branch and the sixteen exponentials ran one after the other, each a chain of dependent operations
            const int kind = spec.kind[cp];
            const T s2 = sg2[cp];
            const T sh = sg2[PG_MAX_COMP + 2 + cp], ish = sg2[2 * PG_MAX_COMP + 2 + cp];      // rational quadratic: alpha^2, 1 / alpha^2
            auto add = [&](auto kind_c) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const T kv = kind_value<T, decltype(kind_c)::value>(s2, sq[r][c], sh, ish);
                        if constexpr (PROD) out[r][c] = cp == 0 ? kv : out[r][c] * kv;
                        else out[r][c] += kv;
                    }
            };
            if (kind == PG_KIND_RQ) add(std::integral_constant<int, PG_KIND_RQ>{});
            else if (kind == PG_KIND_RBF || (PER && kind == PG_KIND_PERIODIC)) add(std::integral_constant<int, PG_KIND_RBF>{});
            else if (kind == PG_KIND_SQDIST) add(std::integral_constant<int, PG_KIND_SQDIST>{});
            else if (kind == PG_KIND_MATERN52) add(std::integral_constant<int, PG_KIND_MATERN52>{});
            else if (kind == PG_KIND_MATERN32) add(std::integral_constant<int, PG_KIND_MATERN32>{});
            else add(std::integral_constant<int, PG_KIND_MATERN12>{});
        }
    }
    const T dg = sg2[PG_MAX_COMP];
    const bool mirror = MIRROR && tc < tr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int gi = tr * KT + ty * 4 + r;
#pragma unroll
        for (int v = 0; v < NVC; ++v) {
            vec_t vec;
#pragma unroll
            for (int e = 0; e < VE; ++e) {
                T val = out[r][v * VE + e];
                if (CHECKED) {
                    const int gj = tc * KT + v * (16 * VE) + tx * VE + e;
                    if (gi >= nr || gj >= nc) val = (symmetric && gi == gj && !accumulate) ? (T)1 : (T)0;
                    else if (symmetric && gi == gj) val += dg;
                }
                vec[e] = val;
                if (MIRROR) { if (mirror) tt[(v * (16 * VE) + tx * VE + e) * TLD + ty * 4 + r] = val; }
            }
            vec_t* dst = reinterpret_cast<vec_t*>(K + (long)gi * ldk + tc * KT + v * (16 * VE) + tx * VE);
            if (CHECKED) { if (accumulate) vec += *dst; }   // a further pass of a Compose with more than PG_MAX_COMP children
            *dst = vec;
        }
    }
    if (MIRROR && mirror) {   // K[tc-tile rows][tr-tile cols] = transpose, read back row-wise so the stores stay 256-byte runs
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int li = ty * 4 + r;
#pragma unroll
            for (int v = 0; v < NVC; ++v) {
                vec_t vec;
#pragma unroll
                for (int e = 0; e < VE; ++e) vec[e] = tt[li * TLD + v * (16 * VE) + tx * VE + e];
                vec_t* dst = reinterpret_cast<vec_t*>(K + (long)(tc * KT + li) * ldk + tr * KT + v * (16 * VE) + tx * VE);
                if (CHECKED) { if (accumulate) vec += *dst; }
                *dst = vec;
            }
        }
    }
}

// MIRROR: a symmetric build that also writes the transposed tiles above the diagonal.  NPF: point coordinates a thread stages per
// tile (64 d / 256, rounded up to 2, 4 or 16).
// A workgroup walks a STRIP of up to S tiles of one tile row (round 2: one tile per workgroup): the row's points, the hyper-parameters
// and the launch are paid once per strip, and the next tile's column points are fetched (global -> registers -> the other LDS
// buffer) while the current tile is computed.  A tile's time was 7 us of staging latency, synchronisation and drain around 1 us of
// arithmetic with four workgroups per CU to hide it (rocprof: 2.55 TB/s on the lower-only build); the strip hides it behind work.
// PER: the spec holds a periodic component (kb_body): 1 / p_k staged behind everything else, the general body only.
// PROD: a product spec (the host strips PG_SPEC_PRODUCT from ncomp first): kb_body multiplies the components; always with PER.
template <typename T, bool MIRROR, int NPF, bool FASTK = false, bool PER = false, bool PROD = false>
__global__ __launch_bounds__(256) void pg_kbuild_kernel(pg_covspec spec, const double* __restrict__ hp,
                                                        const T* __restrict__ Xr, long ldr, int nr,
                                                        const T* __restrict__ Xc, long ldc, int nc, int d,
                                                        int symmetric, int accumulate, double jitter,
                                                        T* __restrict__ K, long ldk, int ctile0, int ctile1, int presc, int S,
                                                        long eX, long ehp, long eK, long eXr) {
    // batched experts: blockIdx.y = expert, each with its own points, hyper-parameters and matrix (cross builds: the row points --
    // the test points of a prediction -- have their own stride, 0 when every expert predicts at the same points)
    Xr += blockIdx.y * eXr; Xc += blockIdx.y * eX; hp += blockIdx.y * ehp; K += blockIdx.y * eK;
    int tr, tcs, ntile;
    kb_strip_of(blockIdx.x, symmetric, ctile0, ctile1, S, tr, tcs, ntile);
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    T* xr = reinterpret_cast<T*>(smem_raw);
    T* xc = xr + KT * d;            // two buffers [d][64]
    T* l2 = xc + 2 * KT * d;        // [ncomp][d] squared inverse length scales
    T* sg2 = l2 + PG_MAX_COMP * d;  // [PG_MAX_COMP] sigma^2, the diagonal term (+ 1 spare), [PG_MAX_COMP] shapes alpha^2 and their reciprocals
    T* tt = sg2 + 3 * PG_MAX_COMP + 2;  // MIRROR: [64][TLD] transposed tile
    T* nrm = tt + (MIRROR ? KT * TLD : 0);                      // fast path: -|x|^2 of the row points [64], of the column points [2][64]
    double* tab = reinterpret_cast<double*>(nrm + 3 * KT);      // fast path: sigma^2 2^(j/32) [32] (fp64 builds only)
    T* ipl = reinterpret_cast<T*>(tab + 32);                    // PER: [ncomp][d] reciprocal periods (0 for the other kinds)
    constexpr bool fast = FASTK;                                // host: one squared-exponential component, fp64, no accumulate pass (presc = 2)
    const int tid = threadIdx.x;
    const double* scale = presc ? hp + spec.off[0] + 1 : nullptr;
    // this thread's share of a point tile: elements idx = tid + 256 u < 64 d  ->  point idx / d, coordinate idx % d
    int pp[NPF], kk[NPF];
    double sc[NPF];
#pragma unroll
    for (int u = 0; u < NPF; ++u) {
        const int idx = tid + 256 * u;
        pp[u] = idx < KT * d ? idx / d : -1;
        kk[u] = idx < KT * d ? idx % d : 0;
        sc[u] = (scale && pp[u] >= 0) ? scale[kk[u]] : 1.0;
    }
    // The prefetch must stay a prefetch: the loads are UNCONDITIONAL (clamped address) and nothing touches their result before
    // store_cols.  Written as `valid ? X[..] * scale : 0` each load sat in its own exec-masked block with `s_waitcnt vmcnt(0)` right
    // behind it -- two serial load latencies per tile, each also waiting for the previous tile's stores to drain.
    T pf[NPF];
    bool pok[NPF];
    auto load_cols = [&](int tc) {
#pragma unroll
        for (int u = 0; u < NPF; ++u) {
            const int gp = tc * KT + pp[u];
            pok[u] = pp[u] >= 0 && gp < nc;
            pf[u] = Xc[(long)min(max(gp, 0), nc - 1) * ldc + kk[u]];
        }
    };
    auto store_cols = [&](T* dst) {
#pragma unroll
        for (int u = 0; u < NPF; ++u)
            if (pp[u] >= 0) dst[kk[u] * KT + pp[u]] = pok[u] ? (T)((double)pf[u] * sc[u]) : (T)0;
    };
    load_cols(tcs);
    stage_points(xr, Xr, ldr, nr, tr * KT, d, tid, scale, fast ? 2.0 : 1.0);
    pair_stage_hp<T, PER>(spec, hp, d, d, d, l2, ipl, tid, 256);
    if (tid < spec.ncomp) {
        const double sg = hp[spec.off[tid]];
        sg2[tid] = (T)(sg * sg);
    }
    if (tid >= 128 && tid < 128 + spec.ncomp) {
        const double a = kind_shape2(spec, hp, tid - 128, d);
        sg2[PG_MAX_COMP + 2 + tid - 128] = (T)a;
        sg2[2 * PG_MAX_COMP + 2 + tid - 128] = (T)(1.0 / a);      // (unused unless the kind has a shape)
    }
    if (tid == 64) {
        double dg = jitter;
        for (int i = 0; i < spec.nnoise; ++i) { const double s = hp[spec.noise_off[i]]; dg += s * s; }
        sg2[PG_MAX_COMP] = (T)dg;
    }
    store_cols(xc);
    if (fast && tid < 32) {
        const double sg = hp[spec.off[0]];
        tab[tid] = sg * sg * pg_exp2_32[tid];
    }
    __syncthreads();
    // dst[p] = mul |x_p|^2 per staged point, thread t0 + p for point p (columns: mul = -1; rows: staged times two, hence -1/4)
    auto norms = [&](const T* pts, T* dst, int t0, T mul) {
        if (tid >= t0 && tid < t0 + KT) {
            T sacc = (T)0;
            for (int k = 0; k < d; ++k) { const T v = pts[k * KT + tid - t0]; sacc += v * v; }
            dst[tid - t0] = mul * sacc;
        }
    };
    if (fast) {
        norms(xr, nrm, KT, (T)-0.25);
        norms(xc, nrm + KT, 0, (T)-1);
        __syncthreads();
    }
    // workgroup-uniform: every tile of the strip lies strictly below the diagonal (or the build is a cross build) and inside the
    // real points -- the strip then runs the body without per-element fix-ups.  ONE body per workgroup: with both bodies inlined
    // in the tile loop the kernel needed 160 VGPRs (three workgroups per CU instead of four).
    const int tcl = tcs + ntile - 1;
    const bool interior = !accumulate && (!symmetric || tcl < tr) && (tr + 1) * KT <= nr && (tcl + 1) * KT <= nc;
    auto walk = [&](auto presc_c, auto checked_c) {      // the strip through kb_body<T, PRESC, CHECKED, MIRROR, FASTK>
        for (int t = 0; t < ntile; ++t) {
            const int tc = tcs + t, cur = t & 1, nxt = cur ^ 1;
            if (t + 1 < ntile) load_cols(tc + 1);           // in flight while this tile is computed
            kb_body<T, decltype(presc_c)::value, decltype(checked_c)::value, MIRROR, FASTK, PER, PROD>(
                spec, xr, xc + cur * KT * d, l2, sg2, tt, d, tr, tc, nr, nc, symmetric, accumulate, K, ldk, tid, nrm, nrm + KT + cur * KT, tab, ipl);
            if (t + 1 < ntile) {
                store_cols(xc + nxt * KT * d);
                __syncthreads();   // publishes the next tile's points; also orders this tile's reads of `tt` before the next one's writes
                if (fast) {
                    norms(xc + nxt * KT * d, nrm + KT + nxt * KT, 0, (T)-1);
                    __syncthreads();
                }
            }
        }
    };
    if constexpr (PER) { if (interior) walk(std::false_type{}, std::false_type{}); else walk(std::false_type{}, std::true_type{}); }
    else if (FASTK || presc) { if (interior) walk(std::true_type{}, std::false_type{}); else walk(std::true_type{}, std::true_type{}); }
    else if constexpr (!FASTK) { if (interior) walk(std::false_type{}, std::false_type{}); else walk(std::false_type{}, std::true_type{}); }
}

// An empty operand (nr == 0 or nc == 0): the whole output is padding -- identity for a symmetric build (lower tiles only unless
// mirrored), zeros for a cross build.  One KT x KT tile per workgroup; the point sets are never touched (the tile kernels load at
// clamped addresses unconditionally, which on an empty operand is a read outside it).
template <typename T>
__global__ __launch_bounds__(256) void pg_kbuild_pad_kernel(T* __restrict__ K, long ldk, int c0, int W, int symmetric, int mirror, long eK) {
    const int tr = blockIdx.x / W, tc = c0 + blockIdx.x % W;
    if (symmetric && !mirror && tc > tr) return;
    T* tile = K + (long)blockIdx.y * eK + (long)tr * KT * ldk + (long)tc * KT;
    for (int idx = threadIdx.x; idx < KT * KT; idx += 256) {
        const int r = idx / KT, c = idx % KT;
        tile[(long)r * ldk + c] = (symmetric && tr == tc && r == c) ? (T)1 : (T)0;
    }
}

// LDS of pg_kbuild_kernel in bytes at dimension d (the fast body's norms and table are always counted; the reciprocal periods only
// for a spec with a periodic component)
template <typename T> static constexpr size_t kb_lds_bytes(int d, bool mirror, bool per = false) {
    return (size_t)(3 * KT * d + PG_MAX_COMP * d + 3 * PG_MAX_COMP + 2 + (mirror ? KT * TLD : 0) + 3 * KT) * sizeof(T) + 32 * sizeof(double) +
           (per ? (size_t)PG_MAX_COMP * d * sizeof(T) : 0);
}

// One instantiation of pg_kbuild_kernel: its dynamic-LDS limit once, then the launch.
template <typename T, bool MIRROR, int NPF, bool FAST, bool PER, bool PROD, typename... Args>
static int kb_launch(dim3 grid, size_t lds, hipStream_t st, Args... args) {
    // large d passes the 64 KB a kernel gets without opting in (134 KB for the mirrored fp64 build at d = 64)
    if (int rc = pg_lds_opt_in<pg_kbuild_kernel<T, MIRROR, NPF, FAST, PER, PROD>>(kb_lds_bytes<T>(PG_MAX_DIM, true, PER))) return rc;
    hipLaunchKernelGGL((pg_kbuild_kernel<T, MIRROR, NPF, FAST, PER, PROD>), grid, dim3(256), lds, st, args...);
    PG_CHECK(hipGetLastError());
    return 0;
}

template <typename T>
int pg_kbuild(hipStream_t st, const pg_covspec& spec_in, const double* hp, const T* Xr, long ldr, int nr,
              const T* Xc, long ldc, int nc, int d, int symmetric, int lower_only, int accumulate, double jitter, T* K,
              long ldk, int rows_pad, int cols_pad, int col0, int col1, int nexp, long eX, long ehp, long eK, long eXr) {
    pg_covspec spec;
    const bool prod = pg_spec_strip(spec_in, spec);      // a product spec: the PROD instantiation of the general body (below)
    if (eXr < 0 || symmetric) eXr = eX;      // symmetric builds: one point set per expert
    if (rows_pad % KT || cols_pad % KT || d < 1 || d > PG_MAX_DIM) {
        pg_set_error("pg_kbuild: bad shape rows_pad=%d cols_pad=%d d=%d", rows_pad, cols_pad, d);
        return -2;
    }
    const bool mirror = symmetric && !lower_only;
    bool per = false;      // a periodic component: the general direct-difference body in its own instantiation, never PRESC / FAST / the matrix pipe
    for (int c = 0; c < spec.ncomp; ++c) per = per || spec.kind[c] == PG_KIND_PERIODIC;
    per = per || prod;     // the product's body always carries the periodic case
    const size_t lds = kb_lds_bytes<T>(d, mirror, per);
    // columns [col0, col1) only (col1 <= 0: all): a lower-only symmetric build in two column windows lets the factorisation
    // start on the first panel while the rest is still being written (pg_potrf_t, BuildReq)
    if (col1 <= 0) { col0 = 0; col1 = cols_pad; }
    if (col0 % KT || col1 % KT || col0 < 0 || col1 > cols_pad || col0 >= col1) {
        pg_set_error("pg_kbuild: bad column window [%d, %d)", col0, col1);
        return -2;
    }
    if (mirror && (col0 != 0 || col1 != cols_pad)) {
        pg_set_error("pg_kbuild: a mirrored build cannot be windowed");
        return -2;
    }
    const int c0 = col0 / KT, c1 = col1 / KT, W = c1 - c0, TR = rows_pad / KT;
    if (nr <= 0 || nc <= 0) {
        if (accumulate || nexp < 1) return 0;      // a further pass leaves the padding alone
        hipLaunchKernelGGL((pg_kbuild_pad_kernel<T>), dim3((unsigned)(TR * W), (unsigned)nexp), dim3(256), 0, st, K, ldk, c0, W, symmetric,
                           mirror ? 1 : 0, eK);
        PG_CHECK(hipGetLastError());
        return 0;
    }
    // strips of up to S tiles of one tile row per workgroup (PG_KB_STRIP; 1 = one tile per workgroup, round 2's granularity)
    // Re-swept with the fast body and the true prefetch (N = 16384, d = 8, lower-only / mirrored, ms): S = 1: 0.326 / 0.561, 2: 0.265 / 0.477,
    // 3: 0.236 / 0.411, 4: 0.224 / 0.406, 5: 0.214 / 0.394, 6: 0.213 / 0.397, 8: 0.233 / 0.424, 12: 0.224 / 0.425, 16: 0.239 / 0.429,
    // 32: 0.259 / 0.459 -- strips whose rows are NOT a multiple of 4 KB long do best (concurrent workgroups spread over the channels)
    static const int strip_env = getenv("PG_KB_STRIP") ? atoi(getenv("PG_KB_STRIP")) : 6;
    const int S = std::max(1, std::min(strip_env, 64));
    const int SW = (W + S - 1) / S;
    // symmetric: the triangle of the window's own tile rows plus the rectangle below it; cross build: every tile of the window
    const long strips = symmetric ? kb_strips_before(W, S) + (long)(TR - c1) * SW : (long)TR * SW;
    if (strips <= 0) return 0;
    // one stationary component (the common Compose([SE, WN])): its inverse length scales go into the staged coordinates (presc = 1; in
    // fp64 (x l) - (x' l) rounds differently from l^2 (x - x')^2 in the last bit) ... and when that component is the squared
    // exponential, fp64 builds take the fast body (kb_body, FAST): presc = 2.  Several components: presc = 0
    const int presc = (spec.ncomp != 1 || per) ? 0 : ((sizeof(T) == 8 && spec.kind[0] == PG_KIND_RBF && !accumulate) ? 2 : 1);
    // One stationary component, d <= 16, no accumulate pass: the distance on the matrix pipe (kmfma.hip).  PG_KB_MFMA = 0: never;
    // 1 (default): wherever the VALU bodies have no fast form -- d > 8, Matern-5/2 and -3/2, fp32; 2: also for the fp64 squared exponential at
    // d <= 8, which the fast body of round 3 serves at 0.63-0.66 of the HBM peak.
    const int mfma_env = getenv("PG_KB_MFMA") ? atoi(getenv("PG_KB_MFMA")) : 1;      // (read per call: tests compare the bodies in one process)
    // (mirrored, lower-only and cross builds of one (kind, dtype, d) all take the same body: their values agree bit for bit)
    // (Matern-1/2 never: it is 1 - r near 0, so the expansion's error in sq reaches K as its square root -- DESIGN.md)
    if (mfma_env && !prod && spec.ncomp == 1 && !accumulate && d <= 16 &&
        (spec.kind[0] == PG_KIND_RBF || spec.kind[0] == PG_KIND_MATERN52 || spec.kind[0] == PG_KIND_MATERN32 || spec.kind[0] == PG_KIND_RQ) &&
        (mfma_env >= 2 || presc != 2 || d > 8))
        return pg_kbuild_mfma<T>(st, spec, hp, Xr, ldr, nr, Xc, ldc, nc, d, symmetric, mirror ? 1 : 0, jitter, K, ldk, c0, c1, S, strips, nexp, eX,
                                 ehp, eK, eXr);
    const int npf = d <= 8 ? 2 : (d <= 16 ? 4 : 16);
    // (mirror, npf, fast, per, prod) -> kb_launch<T, MIRROR, NPF, FAST, PER, PROD>; the fast body exists in fp64 only
    auto go = [&](auto mirror_c, auto npf_c, auto fast_c, auto per_c, auto prod_c) {
        return kb_launch<T, decltype(mirror_c)::value, decltype(npf_c)::value, decltype(fast_c)::value, decltype(per_c)::value,
                         decltype(prod_c)::value>(
            dim3((unsigned)strips, (unsigned)nexp), lds, st, spec, hp, Xr, ldr, nr, Xc, ldc, nc, d, symmetric, accumulate, jitter, K, ldk, c0, c1,
            presc, S, eX, ehp, eK, eXr);
    };
    auto with_npf = [&](auto mirror_c, auto fast_c, auto per_c, auto prod_c) {
        if (npf == 2) return go(mirror_c, std::integral_constant<int, 2>{}, fast_c, per_c, prod_c);
        if (npf == 4) return go(mirror_c, std::integral_constant<int, 4>{}, fast_c, per_c, prod_c);
        return go(mirror_c, std::integral_constant<int, 16>{}, fast_c, per_c, prod_c);
    };
    auto with_mirror = [&](auto fast_c, auto per_c, auto prod_c) {
        return mirror ? with_npf(std::true_type{}, fast_c, per_c, prod_c) : with_npf(std::false_type{}, fast_c, per_c, prod_c);
    };
    if (prod) return with_mirror(std::false_type{}, std::true_type{}, std::true_type{});
    if (per) return with_mirror(std::false_type{}, std::true_type{}, std::false_type{});
    if constexpr (sizeof(T) == 8) {
        if (presc == 2) return with_mirror(std::true_type{}, std::false_type{}, std::false_type{});
    }
    return with_mirror(std::false_type{}, std::false_type{}, std::false_type{});
}
template int pg_kbuild<double>(hipStream_t, const pg_covspec&, const double*, const double*, long, int,
                               const double*, long, int, int, int, int, int, double, double*, long, int, int, int, int, int, long, long, long, long);
template int pg_kbuild<float>(hipStream_t, const pg_covspec&, const double*, const float*, long, int,
                              const float*, long, int, int, int, int, int, double, float*, long, int, int, int, int, int, long, long, long, long);

// ------------------------------------------------------------------------------------------------
// dK stack of the public Covar.kernel_and_grad (covar.py:64-81,169-206,247-269): dK[p][i][j] for
// every hyper-parameter p.  Only the drop-in surface needs it; the NLML path never materialises it.
// ------------------------------------------------------------------------------------------------
// The value of component c at one pair of points, straight from global memory: the factors of a product spec (pg_kgrad_kernel<PROD>)
template <typename T>
__device__ __forceinline__ T kgrad_value(const pg_covspec& spec, const double* __restrict__ hp, int c, const T* xi, const T* xj, int d) {
    const int o = spec.off[c];
    const double sg = hp[o];
    T sq = (T)0;
    if (spec.kind[c] == PG_KIND_PERIODIC) {
        for (int k = 0; k < d; ++k) {
            const double l = hp[o + 1 + k];
            sq += (T)(l * l) * per_sin2<T>((xi[k] - xj[k]) * (T)(1.0 / hp[o + d + 1 + k]));
        }
        return (T)(sg * sg) * pg_exp(-sq);
    }
    for (int k = 0; k < d; ++k) {
        const double l = hp[o + 1 + k];
        const T df = xi[k] - xj[k];
        sq += (T)(l * l) * df * df;
    }
    T kv, base, fs;
    if (spec.kind[c] == PG_KIND_RBF) kind_eval<T, PG_KIND_RBF>((T)(sg * sg), sq, kv, base);
    else {
        const double a = kind_shape2(spec, hp, c, d);
        matern_val<T>(spec.kind[c], (T)(sg * sg), sq, kv, base, (T)a, (T)(1.0 / a), fs);
    }
    return kv;
}

// PROD: a product spec -- every slab of component cp is the sum spec's slab times the product of the OTHER components' values, formed
// explicitly (never K / k_cp: a factor that underflows gives 0).  An instantiation of its own; the sum kernel computes what it did.
template <typename T, bool PROD = false>
__global__ __launch_bounds__(256) void pg_kgrad_kernel(pg_covspec spec, const double* __restrict__ hp,
                                                       const T* __restrict__ X, long ldx, int n, int d,
                                                       T* __restrict__ dK, long slab) {
    const int j = blockIdx.x * 64 + (threadIdx.x & 63);
    const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (i >= n || j >= n) return;
    const long e = (long)i * n + j;
    const T* xi = X + (long)i * ldx;
    const T* xj = X + (long)j * ldx;
    T oth = (T)1;      // PROD: the product of the components other than cp at this pair
    auto put = [&](long idx, T v) {
        if constexpr (PROD) dK[idx] = v * oth;
        else dK[idx] = v;
    };
    for (int cp = 0; cp < spec.ncomp; ++cp) {
        const int o = spec.off[cp];
        const double sg = hp[o];
        if constexpr (PROD) {
            oth = (T)1;
            for (int c2 = 0; c2 < spec.ncomp; ++c2)
                if (c2 != cp) oth *= kgrad_value<T>(spec, hp, c2, xi, xj, d);
        }
        if (spec.kind[cp] == PG_KIND_PERIODIC) {      // sigma, the length-scale slabs from sin^2, the period slabs o + d + 1 .. o + 2 d
            T sp = (T)0;
            for (int k = 0; k < d; ++k) {
                const double l = hp[o + 1 + k];
                sp += (T)(l * l) * per_sin2<T>((xi[k] - xj[k]) * (T)(1.0 / hp[o + d + 1 + k]));
            }
            const T kp = (T)(sg * sg) * pg_exp(-sp);
            put((long)o * slab + e, kp * (T)(2.0 / sg));
            for (int k = 0; k < d; ++k) {
                const double l = hp[o + 1 + k], ip = 1.0 / hp[o + d + 1 + k];
                const T t = (xi[k] - xj[k]) * (T)ip;
                T s2, s2w;
                per_terms<T>(t, s2, s2w);
                put((long)(o + 1 + k) * slab + e, (T)(-2.0 * l) * s2 * kp);
                put((long)(o + d + 1 + k) * slab + e, kp * (T)(l * l * PG_PI * ip) * s2w * t);
            }
            continue;
        }
        T sq = (T)0;
        for (int k = 0; k < d; ++k) {
            const double l = hp[o + 1 + k];
            const T df = xi[k] - xj[k];
            sq += (T)(l * l) * df * df;
        }
        T kv, base, fs;
        if (spec.kind[cp] == PG_KIND_RBF) kind_eval<T, PG_KIND_RBF>((T)(sg * sg), sq, kv, base);
        else {
            const double a = kind_shape2(spec, hp, cp, d);
            matern_val<T>(spec.kind[cp], (T)(sg * sg), sq, kv, base, (T)a, (T)(1.0 / a), fs);
            if (spec.kind[cp] == PG_KIND_RQ) put((long)(o + d + 1) * slab + e, (T)(2.0 * hp[o + d + 1]) * fs);      // the shape slab
        }
        const T coef = (T)(2.0 * kind_hcoef(spec.kind[cp]));
        put((long)o * slab + e, kv * (T)(2.0 / sg));
        for (int k = 0; k < d; ++k) {
            const T df = xi[k] - xj[k];
            put((long)(o + 1 + k) * slab + e, coef * (T)hp[o + 1 + k] * df * df * base);
        }
    }
    for (int q = 0; q < spec.nnoise; ++q)
        dK[(long)spec.noise_off[q] * slab + e] = (i == j) ? (T)(2.0 * hp[spec.noise_off[q]]) : (T)0;
}

template <typename T>
int pg_kgrad(hipStream_t st, const pg_covspec& spec_in, const double* hp, const T* X, long ldx, int n, int d, T* dK) {
    if (n <= 0 || d < 1 || d > PG_MAX_DIM) { pg_set_error("pg_kernel_grad_build: bad shape n=%d d=%d", n, d); return -2; }
    pg_covspec spec;
    const dim3 grid((n + 63) / 64, (n + 3) / 4);
    if (pg_spec_strip(spec_in, spec))
        hipLaunchKernelGGL((pg_kgrad_kernel<T, true>), grid, dim3(256), 0, st, spec, hp, X, ldx, n, d, dK, (long)n * n);
    else
        hipLaunchKernelGGL((pg_kgrad_kernel<T, false>), grid, dim3(256), 0, st, spec, hp, X, ldx, n, d, dK, (long)n * n);
    PG_CHECK(hipGetLastError());
    return 0;
}
template int pg_kgrad<double>(hipStream_t, const pg_covspec&, const double*, const double*, long, int, int, double*);
template int pg_kgrad<float>(hipStream_t, const pg_covspec&, const double*, const float*, long, int, int, float*);

// ------------------------------------------------------------------------------------------------
// expert partitioning (sampler.py:68-119): squared distances to a small set of centres and the nearest centre.
// One thread per point, centres staged in LDS; direct differences (the reference expands into a GEMM, sampler.py:94-100).
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void pg_centres_kernel(const T* __restrict__ X, long ldx, int n, const T* __restrict__ Cn,
                                                         long ldc, int m, int d, T* __restrict__ D, long ldd,
                                                         int* __restrict__ idx, int chunk) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    T* cs = reinterpret_cast<T*>(smem_raw);          // [chunk][d]
    const int i = blockIdx.x * 256 + threadIdx.x;
    T best = (T)0;
    int arg = 0;
    for (int j0 = 0; j0 < m; j0 += chunk) {
        const int mc = min(chunk, m - j0);
        __syncthreads();
        for (int e = threadIdx.x; e < mc * d; e += 256) cs[e] = Cn[(long)(j0 + e / d) * ldc + e % d];
        __syncthreads();
        if (i < n) {
            for (int j = 0; j < mc; ++j) {
                T s = (T)0;
                for (int k = 0; k < d; ++k) {
                    const T df = X[(long)i * ldx + k] - cs[j * d + k];
                    s += df * df;
                }
                if (D) D[(long)i * ldd + j0 + j] = s;
                if ((j0 + j == 0) || s < best) { best = s; arg = j0 + j; }
            }
        }
    }
    if (idx && i < n) idx[i] = arg;
}

template <typename T>
int pg_centres(hipStream_t st, const T* X, long ldx, int n, const T* Cn, long ldc, int m, int d, T* D, long ldd, int* idx) {
    if (n <= 0 || m <= 0 || d < 1 || d > PG_MAX_DIM) { pg_set_error("pg_sqdist: bad shape n=%d m=%d d=%d", n, m, d); return -2; }
    // centres are staged in chunks that fit the 64 KB of LDS a kernel gets without opting in, whatever d is
    const int chunk = std::max(1, std::min(std::min(m, 1024), (int)(48 * 1024 / (d * sizeof(T)))));
    const size_t lds = (size_t)chunk * d * sizeof(T);
    hipLaunchKernelGGL(pg_centres_kernel<T>, dim3((n + 255) / 256), dim3(256), lds, st, X, ldx, n, Cn, ldc, m, d, D, ldd, idx,
                       chunk);
    PG_CHECK(hipGetLastError());
    return 0;
}
template int pg_centres<double>(hipStream_t, const double*, long, int, const double*, long, int, int, double*, long, int*);
template int pg_centres<float>(hipStream_t, const float*, long, int, const float*, long, int, int, float*, long, int*);

// ------------------------------------------------------------------------------------------------
// fused gradient contraction
// ------------------------------------------------------------------------------------------------
// One workgroup walks up to GCH column tiles of its tile row with the accumulators in registers: the row's point tile, the
// cross-wave reduction and the partial-sum row are paid once per strip instead of once per 64 x 64 tile.  Measured at
// N = 16384, D = 8 (contraction + reduce): one tile per workgroup 873 + 120 us, strips of 4 826 + 33 us, strips of 16
// 1061 + 11 us (imbalance); keeping the column point and squared differences in registers (138 VGPRs) 1179 us.
// PER: the spec holds a periodic component.  Its element takes sin^2(pi D_k / p_k) where the others take D_k^2 (length-scale entries)
// and sums sin(2 pi D_k / p_k) D_k / p_k for its d period entries; the fold's slots of a child follow its block, kind_nparam wide:
// sigma, l_1..l_DMAX, then whatever the kind keeps behind them (the rational quadratic's shape, the periods) from slot DMAX + 1 on.
// An instantiation of its own: the other kinds' kernels compile exactly as they did without it.
// PROD: a product spec (always with PER: one instantiation carries every kind).  The product rule enters as a WEIGHT: for component
// cp the element's weight is multiplied by the product of the other components' values, evaluated from the operands already in LDS
// (elem_value) -- explicitly, never as K / k_cp: a factor that underflows gives 0.  Every entry of cp (sigma, length scales, shape,
// periods) then follows from the code of the sum; the trace of W for the noise entries takes the unmodified weight, and the reduce
// kernel's scales are unchanged.
// The per-pair body, elem_value and the fold below are also the text of pg_cross_grad_kernel (sparse.hip) and pg_lowrank_grad_kernel
// (lowrank.hip), to be changed together: as shared functions they are compiled to other registers.
#define GCH 4
// LDS of pg_grad_kernel in bytes: red, the row tile and two column tiles, l2 (and ipl) -- the carve-up below
template <typename T, int DMAX, bool PER> static constexpr size_t grad_lds_bytes() {
    return 4 * kind_nparam(PER ? PG_KIND_PERIODIC : PG_KIND_RQ, DMAX) * sizeof(double) +
           (size_t)(3 * KT * DMAX + (PER ? 2 : 1) * PG_MAX_COMP * DMAX) * sizeof(T);
}
template <typename T, int DMAX, bool PER = false, bool PROD = false>
__global__ __launch_bounds__(256) void pg_grad_kernel(pg_covspec spec, const double* __restrict__ hp,
                                                      const T* __restrict__ X, long ldx, int n, int d,
                                                      const T* __restrict__ Kinv, long ldk,
                                                      const T* __restrict__ alpha, double* __restrict__ part,
                                                      int nhp, GradBatch gb) {
    // batched experts: blockIdx.z = expert, each with its own points, hyper-parameters, K^-1, weights and partial sums
    X += blockIdx.z * gb.eX; hp += blockIdx.z * gb.ehp; Kinv += blockIdx.z * gb.eK; alpha += blockIdx.z * gb.ea; part += blockIdx.z * gb.epart;
    const int tr = blockIdx.y;
    const int c0 = blockIdx.x * GCH, c1 = min(c0 + GCH, tr + 1);   // column tiles [c0, c1), none above the diagonal
    const int blk = tr * gridDim.x + blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (c0 > tr) {   // strip entirely above the diagonal: its partial row must still be zero
        for (int idx = tid; idx < nhp; idx += 256) part[(long)blk * nhp + idx] = 0.0;
        return;
    }
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int RS = kind_nparam(PER ? PG_KIND_PERIODIC : PG_KIND_RQ, DMAX);      // slots of the widest block this kernel folds
    double* red = reinterpret_cast<double*>(smem_raw);             // [4 waves][RS]: sigma, l_1..l_DMAX, the shape | the periods
    T* xr = reinterpret_cast<T*>(red + 4 * RS);                     // [DMAX][64], zero for k >= d
    T* xc = xr + KT * DMAX;                                         // two buffers [DMAX][64]
    T* l2 = xc + 2 * KT * DMAX;                                     // [ncomp][DMAX], zero for k >= d
    T* ipl = l2 + PG_MAX_COMP * DMAX;                               // PER: [ncomp][DMAX] reciprocal periods, zero for k >= d / other kinds
    for (int idx = tid; idx < KT * DMAX; idx += 256) {
        const int p = idx / DMAX, k = idx % DMAX;
        const int gr = tr * KT + p;
        xr[k * KT + p] = (k < d && gr < n) ? X[(long)gr * ldx + k] : (T)0;
    }
    pair_stage_hp<T, PER>(spec, hp, d, DMAX, DMAX, l2, ipl, tid, 256);
    for (int idx = tid; idx < nhp; idx += 256) part[(long)blk * nhp + idx] = 0.0;
    static_assert(!PROD || PER, "a product takes the instantiation that carries every kind");
    // PROD: component c's value at (row, this lane's column) of the point tile xb.  kpair.h's pair_value written out: taking it moved the
    // d > 16 product instantiations of this kernel to more scratch memory
    auto elem_value = [&](int c, int row, const T* xb) -> T {
        const T* lc = l2 + c * DMAX;
        const int kind = spec.kind[c];
        const double sg = hp[spec.off[c]];
        const T sig2 = (T)(sg * sg);
        T sq = (T)0;
        if (kind == PG_KIND_PERIODIC) {
            const T* ipc = ipl + c * DMAX;
#pragma unroll
            for (int k = 0; k < DMAX; ++k) sq += lc[k] * per_sin2<T>((xr[k * KT + row] - xb[k * KT + lane]) * ipc[k]);
            return kind_value<T, PG_KIND_RBF>(sig2, sq);
        }
#pragma unroll
        for (int k = 0; k < DMAX; ++k) {
            const T df = xr[k * KT + row] - xb[k * KT + lane];
            sq += lc[k] * df * df;
        }
        if (kind == PG_KIND_RBF) return kind_value<T, PG_KIND_RBF>(sig2, sq);
        const double sh = kind_shape2(spec, hp, c, d);
        T kt, bt, ft;
        matern_val<T>(kind, sig2, sq, kt, bt, (T)sh, (T)(1.0 / sh), ft);
        return kt;
    };

    // element e of this thread: row = 4 e + wave (one wave reads one 64-wide row: 512 contiguous bytes),
    // column = lane.  W = weight * (Kinv - a a^T): 2 below the diagonal, 1 on it, 0 above / in padding.
    double tr_w = 0.0;
    int it = 0;   // running tile counter: selects the point-tile buffer
    for (int cp = 0; cp < max(spec.ncomp, 1); ++cp) {
        const bool have = cp < spec.ncomp;      // ncomp == 0 (pure white noise): only the trace of W is needed
        const int o = have ? spec.off[cp] : 0;
        const double sg = have ? hp[o] : 0.0;
        const T sig2 = (T)(sg * sg);
        const T* lc = l2 + cp * DMAX;
        const int kind = have ? spec.kind[cp] : PG_KIND_RBF;
        const double sh = have ? kind_shape2(spec, hp, cp, d) : 0.0;
        const T sha = (T)sh, ish = (T)(1.0 / sh);      // rational quadratic: alpha^2, 1 / alpha^2
        double accf = 0.0;                            // ... and its shape entry, sum W K fs
        double acc[DMAX + 1];
#pragma unroll
        for (int k = 0; k <= DMAX; ++k) acc[k] = 0.0;
        double accp[PER ? DMAX : 1];                  // ... the periodic kind's period entries, sum W K sin(2 pi t_k) t_k
#pragma unroll
        for (int k = 0; k < (PER ? DMAX : 1); ++k) accp[k] = 0.0;
        for (int tc = c0; tc < c1; ++tc, ++it) {
            T* xb = xc + (it & 1) * KT * DMAX;
            for (int idx = tid; idx < KT * DMAX; idx += 256) {
                const int p = idx / DMAX, k = idx % DMAX;
                const int gc = tc * KT + p;
                xb[k * KT + p] = (k < d && gc < n) ? X[(long)gc * ldx + k] : (T)0;
            }
            __syncthreads();   // also orders this buffer's previous readers (two tiles ago) before the writes above
            const int gj = tc * KT + lane;
            const double aj = (gj < n) ? (double)alpha[gj] : 0.0;
#pragma unroll 2
            for (int e = 0; e < 16; ++e) {
                const int row = 4 * e + wave;
                const int gi = tr * KT + row;
                double w = 0.0;
                if (gi < n && gj <= gi) {
                    w = (double)Kinv[(long)gi * ldk + gj] - (double)alpha[gi] * aj;
                    if (gj < gi) w *= 2.0; else if (cp == 0) tr_w += w;
                }
                if (!have) continue;
                if constexpr (PROD) {      // the product rule: the others' values weigh this component's element
                    for (int c2 = 0; c2 < spec.ncomp; ++c2)
                        if (c2 != cp) w *= (double)elem_value(c2, row, xb);
                }
                if constexpr (PER) {
                    if (kind == PG_KIND_PERIODIC) {      // (padding coordinates: l^2 = 1 / p = 0, so t = 0 and both terms vanish)
                        const T* ipc = ipl + cp * DMAX;
                        T sp = (T)0;
#pragma unroll
                        for (int k = 0; k < DMAX; ++k) sp += lc[k] * per_sin2<T>((xr[k * KT + row] - xb[k * KT + lane]) * ipc[k]);
                        const double wk = w * (double)kind_value<T, PG_KIND_RBF>(sig2, sp);
                        acc[0] += wk;
#pragma unroll
                        for (int k = 0; k < DMAX; ++k) {
                            const T t = (xr[k * KT + row] - xb[k * KT + lane]) * ipc[k];
                            T s2, s2w;
                            per_terms<T>(t, s2, s2w);
                            acc[1 + k] += wk * (double)s2;
                            accp[k] += wk * (double)s2w * (double)t;
                        }
                        continue;
                    }
                }
                T sq = (T)0;
#pragma unroll
                for (int k = 0; k < DMAX; ++k) {
                    const T df = xr[k * KT + row] - xb[k * KT + lane];
                    sq += lc[k] * df * df;
                }
                double kv, base;   // dK/dl_k = base * l_k * D_k^2 (sign and constants applied in the reduce)
                if (kind == PG_KIND_RBF) {
                    kv = (double)kind_value<T, PG_KIND_RBF>(sig2, sq);
                    base = kv;
                } else {
                    T kt, bt, ft;
                    matern_val<T>(kind, sig2, sq, kt, bt, sha, ish, ft);
                    kv = (double)kt;
                    base = (double)bt;
                    accf += w * (double)ft;
                }
                acc[0] += w * kv;
                const double wb = w * base;
#pragma unroll
                for (int k = 0; k < DMAX; ++k) {
                    const double df = (double)(xr[k * KT + row] - xb[k * KT + lane]);
                    acc[1 + k] += wb * df * df;
                }
            }
        }
        if (have) {
#pragma unroll
            for (int k = 0; k <= DMAX; ++k) {
                const double s = wave_sum(acc[k]);
                if (lane == 0) red[wave * RS + k] = s;
            }
            if (kind == PG_KIND_RQ) {
                const double s = wave_sum(accf);
                if (lane == 0) red[wave * RS + DMAX + 1] = s;
            }
            if constexpr (PER) {
                if (kind == PG_KIND_PERIODIC) {
#pragma unroll
                    for (int k = 0; k < DMAX; ++k) {
                        const double s = wave_sum(accp[k]);
                        if (lane == 0) red[wave * RS + DMAX + 1 + k] = s;
                    }
                }
            }
            __syncthreads();
            if (tid < kind_nparam(kind, d)) {      // the child's block: sigma, l_1..l_d (slots 0..d), what sits behind them (slots DMAX + 1 ..)
                const int q = tid <= d ? tid : DMAX + 1 + (tid - d - 1);
                part[(long)blk * nhp + o + tid] = red[q] + red[RS + q] + red[2 * RS + q] + red[3 * RS + q];
            }
            __syncthreads();
        }
    }
    {
        const double s = wave_sum(tr_w);
        if (lane == 0) red[wave * RS] = s;
        __syncthreads();
        if (tid < spec.nnoise)
            part[(long)blk * nhp + spec.noise_off[tid]] =
                red[0] + red[RS] + red[2 * RS] + red[3 * RS];
    }
}

// grad[p] = scale_p * sum_blocks part[b][p].  presc: the partial sums came from pg_grad_mfma (kmfma.hip), whose length-scale entries
// hold sums of (l_k D_k)^2 -- the inverse length scales are folded into its staged coordinates; pg_grad_kernel sums D_k^2 (presc = 0).
__global__ __launch_bounds__(256) void pg_grad_reduce_kernel(pg_covspec spec, const double* __restrict__ hp,
                                                             const double* __restrict__ part, int nblk, int nhp,
                                                             int d, double* __restrict__ grad, int presc, GradBatch gb) {
    __shared__ double red[4];
    hp += blockIdx.z * gb.ehp; part += blockIdx.z * gb.epart; grad += blockIdx.z * gb.egrad;
    const int p = blockIdx.x, tid = threadIdx.x;
    double s = 0.0;
    for (int b = tid; b < nblk; b += 256) s += part[(long)b * nhp + p];
    s = wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        s = red[0] + red[1] + red[2] + red[3];
        double scale = 0.0;
        bool mine = false;   // entries of children that are not in this spec belong to another pass of a long Compose
        for (int c = 0; c < spec.ncomp; ++c) {
            bool hit = false;
            const double sc = 0.5 * kind_entry_scale(spec, hp, c, p, d, hit);      // the NLML's 1/2
            if (!hit) continue;
            scale = sc;
            mine = true;
            // the matrix-pipe contraction summed (l_k D_k)^2: -l_k S = -S' / l_k (l_k = 0: S' = 0 and the derivative is 0)
            if (presc && p > spec.off[c] && p <= spec.off[c] + d) scale = hp[p] != 0.0 ? kind_hcoef(spec.kind[c]) / hp[p] : 0.0;
        }
        for (int i = 0; i < spec.nnoise; ++i)
            if (p == spec.noise_off[i]) { scale = 0.5 * 2.0 * hp[p]; mine = true; }   // dK/dsigma_n = 2 sigma_n I
        if (mine) grad[p] = scale * s;
    }
}

template <typename T, int DMAX, bool PER, bool PROD>
static int launch_grad(hipStream_t st, const pg_covspec& spec, const double* hp, const T* X, long ldx, int n,
                       int d, const T* Kinv, long ldk, const T* alpha, double* part, int nhp, int tiles, const GradBatch& gb, int nexp) {
    constexpr size_t lds = grad_lds_bytes<T, DMAX, PER>();
    if (int rc = pg_lds_opt_in<pg_grad_kernel<T, DMAX, PER, PROD>>(lds)) return rc;   // d > 32 needs more than the 64 KB a kernel gets without opting in
    hipLaunchKernelGGL((pg_grad_kernel<T, DMAX, PER, PROD>), dim3((tiles + GCH - 1) / GCH, tiles, nexp), dim3(256), lds, st, spec, hp, X, ldx,
                       n, d, Kinv, ldk, alpha, part, nhp, gb);
    PG_CHECK(hipGetLastError());
    return 0;
}

template <typename T>
int pg_nlml_grad_t(hipStream_t st, const pg_covspec& spec_in, const double* hp, const T* X, long ldx, int n, int d,
                   const T* Kinv, long ldk, const T* alpha, double* grad, int nhp, double* work, long lwork,
                   int nexp, long ehp, long eX, long eK, long ea, long egrad) {
    pg_covspec spec;
    const bool prod = pg_spec_strip(spec_in, spec);      // a product spec: pg_grad_kernel's PROD instantiation, never the matrix pipe
    const int tiles = (n + KT - 1) / KT;
    const long need = (long)tiles * tiles * nhp;
    if (nexp < 1 || nexp > 65535) { pg_set_error("pg_nlml_grad: 1 <= nexp <= 65535"); return -2; }
    if (lwork < need * nexp) { pg_set_error("pg_nlml_grad: workspace %ld < %ld doubles", lwork, need * nexp); return -3; }
    const GradBatch gb = {eX, ehp, eK, ea, need, egrad};
    int rc;
    // One stationary component, d <= 16: the contraction on the matrix pipe (kmfma.hip; PG_GRAD_MFMA=0: pg_grad_kernel for every input,
    // the independent direct-difference yardstick of the tests)
    const int mfma_env = getenv("PG_GRAD_MFMA") ? atoi(getenv("PG_GRAD_MFMA")) : 1;   // (read per call: tests compare the bodies in one process)
    // (not Matern-1/2: its factor e^-r / r is unbounded near r = 0, and the expansion's cancellation error is u |x|^2 sum |G| -- DESIGN.md)
    if (mfma_env && !prod && spec.ncomp == 1 && d <= 16 && n >= 1 &&
        (spec.kind[0] == PG_KIND_RBF || spec.kind[0] == PG_KIND_MATERN52 || spec.kind[0] == PG_KIND_MATERN32 || spec.kind[0] == PG_KIND_RQ)) {
        int nblk = 0;
        if ((rc = pg_grad_mfma<T>(st, spec, hp, X, ldx, n, d, Kinv, ldk, alpha, work, nhp, tiles, gb, nexp, &nblk))) return rc;
        hipLaunchKernelGGL(pg_grad_reduce_kernel, dim3(nhp, 1, nexp), dim3(256), 0, st, spec, hp, work, nblk, nhp, d, grad, 1, gb);
        PG_CHECK(hipGetLastError());
        return 0;
    }
    if (d > PG_MAX_DIM) { pg_set_error("pg_nlml_grad: d=%d > %d", d, PG_MAX_DIM); return -2; }
    // (a periodic component never takes the matrix pipe: the whitelist above)
    rc = pg_with_kinds(spec, prod, [&](auto per_c, auto prod_c) {
        return pg_with_dmax(d, [&](auto dmax_c) {
            return launch_grad<T, decltype(dmax_c)::value, decltype(per_c)::value, decltype(prod_c)::value>(st, spec, hp, X, ldx, n, d, Kinv, ldk,
                                                                                                            alpha, work, nhp, tiles, gb, nexp);
        });
    });
    if (rc) return rc;
    hipLaunchKernelGGL(pg_grad_reduce_kernel, dim3(nhp, 1, nexp), dim3(256), 0, st, spec, hp, work, tiles * ((tiles + GCH - 1) / GCH), nhp,
                       d, grad, 0, gb);
    PG_CHECK(hipGetLastError());
    return 0;
}
long pg_nlml_grad_worksize_impl(int n, int nhp) {
    const long tiles = (n + KT - 1) / KT;
    return tiles * tiles * nhp;
}
template int pg_nlml_grad_t<double>(hipStream_t, const pg_covspec&, const double*, const double*, long, int, int,
                                    const double*, long, const double*, double*, int, double*, long, int, long, long, long, long, long);
template int pg_nlml_grad_t<float>(hipStream_t, const pg_covspec&, const double*, const float*, long, int, int,
                                   const float*, long, const float*, double*, int, double*, long, int, long, long, long, long, long);
