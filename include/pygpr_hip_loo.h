/*
 * libpygpr_hip -- leave-one-out cross-validation (Rasmussen & Williams, section 5.4.2) on a fitted exact GP.  A second public header
 * of the same library: the entry points below are new (the reference has no LOO), pygpr_amd/_lib.py binds them from this file as it
 * binds include/pygpr_hip.h, and the same closed type vocabulary applies.
 *
 * With c_i = [K^-1]_ii = sum_{k >= i} (L^-1)_ki^2 and alpha = K^-1 y the leave-one-out predictive distribution of y_i is
 *   mu_i = y_i - alpha_i / c_i,   var_i = 1 / c_i,
 * and the negative log predictive density (the LOO loss) is
 *   L_loo = sum_i [ -1/2 log c_i + alpha_i^2 / (2 c_i) ] + n/2 log 2pi.
 * With w_i = 1/(2 c_i) + alpha_i^2 / (2 c_i^2), v_i = alpha_i / c_i, b = K^-1 v, p = (alpha + b)/sqrt2, q = (alpha - b)/sqrt2 and
 * S = K^-1 diag(sqrt(2 w)) its gradient is
 *   dL_loo/dtheta_k = 1/2 sum_ab (S S^T + q q^T - p p^T)_ab dK_ab/dtheta_k,
 * i.e. pg_nlml_grad with Kinv := S S^T + q q^T (lower triangle) and alpha := p.
 *
 * Conventions: those of include/pygpr_hip.h --
 *   - every matrix/vector pointer is a DEVICE pointer owned by the caller; the library allocates nothing
 *   - matrices are row-major with a leading dimension in elements; dtype is PG_F64 or PG_F32; n_pad % 256 == 0
 *   - alignment: pg_loo_terms (Minv) and pg_loo_weights (Kinv) move 16-byte words at base + r * ld + c and REFUSE, before anything
 *     is enqueued, a matrix whose base pointer or leading dimension is not a multiple of 16 bytes; any ld >= width that keeps that
 *     rule is honoured, gaps are neither read nor written.  Their vector operands and all of pg_loo_fold are scalar: any alignment,
 *     any ld >= width
 *   - triangular operands: Minv is read on and below its diagonal 128 x 128 blocks only (what lies above those blocks may hold
 *     anything, NaN included)
 *   - calls are asynchronous on `stream`; return 0 = enqueued, <0 = bad argument / HIP error (text via pg_last_error())
 */
#ifndef PYGPR_HIP_LOO_H
#define PYGPR_HIP_LOO_H

#include "pygpr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Leave-one-out terms of the n real points of a model padded to n_pad, from Minv = L^-1 (lower), alpha = K^-1 y and y:
 *   c[i] = sum_{i <= k < n} Minv[k][i]^2, mu[i] = y[i] - alpha[i] / c[i], var[i] = 1 / c[i]   (i < n, in the model's dtype),
 *   out[0] = L_loo (fp64).
 * Rows and columns from n on (the identity padding) do not contribute and are not read.  c is accumulated in fp64 for both dtypes;
 * mu, var and the loss are formed from that sum before it is rounded to the dtype.  A NaN in y[i] or alpha[i] gives NaN in mu[i] and in
 * out[0] and nowhere else.  Two launches: the column sums of squares of the lower triangle in chunks of 256 rows (one HBM pass over
 * n^2 / 2 elements, no tile right of the diagonal is launched), then the sums over the chunks with mu, var and the loss.
 * work: pg_loo_terms_worksize(n_pad) doubles, scratch of the call (nothing in it needs initialising).  1 <= n <= n_pad. */
long pg_loo_terms_worksize(int n_pad);   /* doubles */
int pg_loo_terms(pg_handle h, int dtype, int n, int n_pad, const void* Minv, long ldm, const void* alpha, const void* y, void* c, void* mu,
                 void* var, double* out, double* work, void* stream);

/* The operands of the LOO gradient from c (pg_loo_terms), alpha and the FULL symmetric Kinv = K^-1 (pg_lauum, then pg_symmetrize),
 * in one pass over the real n x n part of Kinv:
 *   b = Kinv v is taken from the entries as they are read, then Kinv[i][j] <- Kinv[i][j] sqrt(2 w_j) in place (S; w > 0 always),
 *   p[i] = (alpha[i] + b[i]) / sqrt2,  q[i] = (alpha[i] - b[i]) / sqrt2   (i < n; fp64 accumulation for both dtypes).
 * Rows and columns from n on are neither read nor written: an identity padding stays the identity, so S S^T over n_pad has the
 * identity there too.  p and q must not alias c or alpha. */
int pg_loo_weights(pg_handle h, int dtype, int n, const void* c, const void* alpha, void* Kinv, long ldk, void* p, void* q, void* stream);

/* M[i][j] += q[i] q[j] for j <= i < n: the rank-one term folded into the lower triangle of M = S S^T (pg_gemm_raw, variant 0,
 * tri = 1), after which pg_nlml_grad(Kinv := M, alpha := p) is the LOO gradient.  Nothing above the diagonal is touched. */
int pg_loo_fold(pg_handle h, int dtype, int n, void* M, long ldm, const void* q, void* stream);

#ifdef __cplusplus
}
#endif
#endif
