// The direct-difference per-pair forms of the stationary kinds, shared by every VALU kernel that evaluates or differentiates a
// component from a pair of points: how the hyper-parameters are staged, how the scaled squared distance is formed, one component's
// value (the product rule's factor) and the reduce kernels' scale of an entry.  kfun.h keeps the scalar math (kind_eval, per_terms,
// ...).  Everything is a forceinline template: a kernel names its own coordinates through two lambdas xa(k), xb(k) -- an LDS tile
// xr[k * 64 + row], registers xj[k], a point in global memory -- and keeps its own loops, unroll pragmas and barriers.
// What is NOT here, and why, is listed in DESIGN.md 4.24: the hyper-parameter gradient's per-pair body and fold, which three kernels
// still carry (pg_grad_kernel, pg_cross_grad_kernel, pg_lowrank_grad_kernel), and two of the product rule's factors.
#pragma once
#include "kfun.h"

// l2[c * stride + k] = l_ck^2 and (PER) ipl[c * stride + k] = 1 / p_ck for the periodic components, 0 for the others; k < kw, zero
// for k >= d (padding coordinates then add nothing to a distance and t = 0 to a phase).  kw, stride: the tile kernels pass their
// DMAX for both, kernels that loop to the run-time d pass d and their own stride.  Thread tid of nthr; the caller's barrier publishes.
template <typename T, bool PER>
__device__ __forceinline__ void pair_stage_hp(const pg_covspec& spec, const double* __restrict__ hp, int d, int kw, int stride, T* l2, T* ipl,
                                              int tid, int nthr) {
    for (int idx = tid; idx < spec.ncomp * kw; idx += nthr) {
        const int c = idx / kw, k = idx % kw;
        const double l = (k < d) ? hp[spec.off[c] + 1 + k] : 0.0;
        l2[c * stride + k] = (T)(l * l);
        if constexpr (PER) ipl[c * stride + k] = (k < d && spec.kind[c] == PG_KIND_PERIODIC) ? (T)(1.0 / hp[spec.off[c] + d + 1 + k]) : (T)0;
    }
}

// sum_k l_k^2 D_k^2, D_k = xa(k) - xb(k), in the model's dtype
template <typename T, int DMAX, class XA, class XB> __device__ __forceinline__ T pair_sq(const T* lc, XA xa, XB xb) {
    T sq = (T)0;
#pragma unroll
    for (int k = 0; k < DMAX; ++k) {
        const T df = xa(k) - xb(k);
        sq += lc[k] * df * df;
    }
    return sq;
}
// the periodic kind's: sum_k l_k^2 sin^2(pi D_k / p_k)
template <typename T, int DMAX, class XA, class XB> __device__ __forceinline__ T pair_sq_per(const T* lc, const T* ipc, XA xa, XB xb) {
    T sq = (T)0;
#pragma unroll
    for (int k = 0; k < DMAX; ++k) sq += lc[k] * per_sin2<T>((xa(k) - xb(k)) * ipc[k]);
    return sq;
}

// Component c's value at one pair: the factor the product rule multiplies into the other components' weights.  Formed explicitly,
// never as K / k_c (a factor that underflows gives 0).  lc, ipc: the component's rows of the staged l2 / ipl.
template <typename T, int DMAX, class XA, class XB>
__device__ __forceinline__ T pair_value(const pg_covspec& spec, const double* __restrict__ hp, int c, int d, const T* lc, const T* ipc, XA xa,
                                        XB xb) {
    const int kind = spec.kind[c];
    const double sg = hp[spec.off[c]];
    const T sig2 = (T)(sg * sg);
    if (kind == PG_KIND_PERIODIC) return kind_value<T, PG_KIND_RBF>(sig2, pair_sq_per<T, DMAX>(lc, ipc, xa, xb));
    const T sq = pair_sq<T, DMAX>(lc, xa, xb);
    if (kind == PG_KIND_RBF) return kind_value<T, PG_KIND_RBF>(sig2, sq);
    const double sh = kind_shape2(spec, hp, c, d);
    T kt, bt, ft;
    matern_val<T>(kind, sig2, sq, kt, bt, (T)sh, (T)(1.0 / sh), ft);
    return kt;
}

// The factor between a slot sum of the gradient kernels (sum W K, sum W base D_k^2, sum W K fs, sum W K sin(2 pi t_k) t_k) and
// d/dtheta_p sum W K for entry p, if p lies in component c's block (`mine` is then set; otherwise it is left alone and 0 returned).
// The NLML's reduce halves it.
__device__ __forceinline__ double kind_entry_scale(const pg_covspec& spec, const double* __restrict__ hp, int c, int p, int d, bool& mine) {
    const int o = spec.off[c];
    double scale = 0.0;
    if (p == o) { scale = 2.0 / hp[o]; mine = true; }       // dK/dsigma = 2K/sigma
    else if (p > o && p <= o + d) { scale = 2.0 * kind_hcoef(spec.kind[c]) * hp[p]; mine = true; }      // SE: -2 l_k D_k^2 K, Matern: coef base l_k D_k^2
    else if (spec.kind[c] == PG_KIND_RQ && p == o + d + 1) { scale = 2.0 * hp[p]; mine = true; }        // dK/dalpha = 2 alpha K fs
    else if (spec.kind[c] == PG_KIND_PERIODIC && p > o + d && p <= o + 2 * d) {
        const double l = hp[p - d];     // dK/dp_k = K l_k^2 sin(2 pi t_k) pi t_k / p_k
        scale = l * l * PG_PI / hp[p];
        mine = true;
    }
    return scale;
}
