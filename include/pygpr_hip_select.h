/*
 * libpygpr_hip -- greedy inducing-point selection for the inducing-point GP (pygpr_amd/sparse.py): the partial pivoted Cholesky
 * factorisation of k(X, X), pivoting on the largest residual prior variance.  A fifth public header of the same library: the entry
 * points below are new (the reference has no sparse model), pygpr_amd/_lib.py binds them from this file as it binds
 * include/pygpr_hip.h, and the same closed type vocabulary applies.
 *
 * With kdiag the constant prior variance of the spec's stationary part (the sum of sigma_c^2, their product for a product spec) and
 * r_i = kdiag for every i < n, step j = 0, 1, ... takes
 *     p = argmax_i r_i          strict `>` in index order: a tie takes the lowest index, a NaN is never a maximum
 * and stops unless r_p > floor; otherwise
 *     l_i = (k(x_i, x_p) - sum_{t < j} L[i][t] L[p][t]) / sqrt(r_p),   L[i][j] = l_i,   r_i <- r_i - l_i^2  (no clamp),   r_p <- 0,
 *     piv[j] = p,   trace[j] = sum_i r_i.
 * trace[j] is the trace term n kdiag - tr(Kuu^-1 Kuf Kfu) of the collapsed bound for the first j + 1 pivots as inducing points (taken
 * without jitter): the prior variance the selected set leaves unexplained, summed over the training points.
 *
 * Conventions: those of include/pygpr_hip.h --
 *   - every pointer is a DEVICE pointer owned by the caller; the library allocates nothing
 *   - alignment: scalar throughout -- any base pointer, any ldx >= d; gaps are neither read nor written
 *   - calls are asynchronous on `stream`; return 0 = enqueued, <0 = bad argument / HIP error (text via pg_last_error())
 */
#ifndef PYGPR_HIP_SELECT_H
#define PYGPR_HIP_SELECT_H

#include "pygpr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Up to m_max pivots of X [n][d] at ldx under the stationary components of `spec` (1..PG_MAX_COMP of them, a product spec included,
 * never PG_KIND_SQDIST; the noise entries are ignored).  dtype must be PG_F64;  1 <= d <= PG_MAX_DIM;  0 <= m_max <= n.  k is evaluated
 * per pair from direct differences with the forms of pg_kernel_cross_grad, the factors of a product spec formed explicitly.
 *   count[0]          the number of pivots taken (<= m_max; smaller when the largest residual no longer exceeds `floor`)
 *   piv[0 .. count)   the pivots in selection order;  trace[0 .. count)  the residual sums (fp64)
 *   resid[0 .. n)     the final residual diagonal (fp64): the prior variance left unexplained at every point
 * Entries of piv and trace from `count` on are not touched.  With m_max == 0 (n == 0 included) count[0] = 0 and nothing else is written.
 * Every step is two ordinary launches on `stream` -- the column, the residual update and per-workgroup (max, index, sum) partials; one
 * workgroup that folds them in index order -- and all m_max steps are enqueued at once: nothing is read back, the launches behind a
 * stop return at once.  Sums run in a fixed order: a call is bit-reproducible.  A point with a NaN coordinate gets a NaN residual and
 * is never selected; trace is NaN from the first step on then.
 * work: pg_greedy_select_worksize(n, m_max) doubles, scratch of the call (nothing in it needs initialising): the factor, one column per
 * pivot with the points contiguous, the residuals and the partials.  The worksize is -1 for a negative argument or m_max > n. */
long pg_greedy_select_worksize(int n, int m_max);   /* doubles */
int pg_greedy_select(pg_handle h, int dtype, const pg_covspec* spec, const double* hp, const void* X, long ldx, int n, int d, int m_max,
                     double floor, int* piv, int* count, double* trace, double* resid, void* work, void* stream);

#ifdef __cplusplus
}
#endif
#endif
