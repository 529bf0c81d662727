/*
 * libpygpr_hip -- the rectangular hyper-parameter contraction of the inducing-point GP (Titsias' collapsed bound, pygpr_amd/sparse.py).
 * A fourth public header of the same library: the entry points below are new (the reference has no sparse model), pygpr_amd/_lib.py
 * binds them from this file as it binds include/pygpr_hip.h, and the same closed type vocabulary applies.
 *
 * The bound's derivative in a hyper-parameter theta_p is  sum G_uu o dKuu/dtheta_p + sum_c sum G_uf,c o dKuf_c/dtheta_p  + explicit terms,
 * with Kuu = k(Z, Z) on the m inducing points and Kuf_c = k(Z, X_c) on a chunk of the n training points.  Neither derivative matrix is
 * ever formed: pg_kernel_cross_grad contracts a weight matrix W [m x n] against dk(z_i, x_j)/dtheta_p rebuilt from the point tiles, the
 * way pg_nlml_grad contracts K^-1 - alpha alpha^T on one point set.  The Kuu part is the same call with X = Z and W = G_uu.
 *
 * Conventions: those of include/pygpr_hip.h --
 *   - every pointer is a DEVICE pointer owned by the caller; the library allocates nothing
 *   - matrices are row-major with a leading dimension in elements; dtype is PG_F64 or PG_F32
 *   - alignment: scalar throughout -- any base pointer, any ld >= width; gaps are neither read nor written
 *   - calls are asynchronous on `stream`; return 0 = enqueued, <0 = bad argument / HIP error (text via pg_last_error())
 */
#ifndef PYGPR_HIP_SPARSE_H
#define PYGPR_HIP_SPARSE_H

#include "pygpr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* grad[p] (+)= sum_{i < m, j < n} W[i][j] dk(z_i, x_j)/dtheta_p  for every parameter p of the spec's stationary components: sigma, the
 * length scales, the rational quadratic's shape, the periodic kind's periods.  A product spec (PG_SPEC_PRODUCT) weighs the element of
 * factor c with the values of the other factors, formed explicitly.  No factor 1/2, no symmetry: every (i, j) counts once, so the Kuu
 * part of a bound takes the full symmetric G_uu.  The derivative forms per pair are pg_nlml_grad's, from direct differences.
 *   Z [m][d] at ldz: the row points (the inducing points);  X [n][d] at ldx: the column points;  1 <= d <= PG_MAX_DIM;  m, n >= 0
 *   W [m][n] at ldw, row-major, rows = Z.  Only [0, m) x [0, n) is read.
 *   hp: the model's hyper-parameters (fp64);  grad: fp64, at least as long as the spec's blocks reach (off[c] + the block's width)
 *   accumulate: 0 overwrites the spec's entries, non-zero adds to them.  Entries at noise_off and entries outside the spec are neither
 *   read nor written in either mode.
 * Pair arithmetic runs in dtype; the partial sums and the output are fp64.  Two launches: one workgroup per strip of up to four 64 x 64
 * tiles of W writes its partial sums into `work`, a reduce kernel folds them in a fixed order -- a call is bit-reproducible.  A NaN in a
 * point, a weight or a hyper-parameter reaches the entries it enters.
 * work: pg_kernel_cross_grad_worksize(m, n, nhp) doubles with nhp >= the reach of the spec's blocks (the model's parameter count), scratch
 * of the call (nothing in it needs initialising).  The worksize is -1 for a negative argument. */
long pg_kernel_cross_grad_worksize(int m, int n, int nhp);   /* doubles */
int pg_kernel_cross_grad(pg_handle h, int dtype, const pg_covspec* spec, const double* hp, const void* Z, long ldz, int m, const void* X,
                         long ldx, int n, int d, const void* W, long ldw, double* grad, int accumulate, void* work, void* stream);

#ifdef __cplusplus
}
#endif
#endif
