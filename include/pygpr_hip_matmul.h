/*
 * libpygpr_hip -- the matrix-free covariance product of the iterative exact GP (pygpr_amd/iterative.py).
 * A sixth public header of the same library: the entry points below are new (the reference has no iterative solver), pygpr_amd/_lib.py
 * binds them from this file as it binds include/pygpr_hip.h, and the same closed type vocabulary applies.
 *
 * Conjugate gradients on A = k(X, X) + shift I need A V and nothing else of A.  pg_kernel_matmul forms the product from the point tiles:
 * a 16 x 16 block of covariance values is evaluated in the accumulator layout of the fp64 matrix instruction and is at once the operand
 * of the product over the column points -- the n x n matrix is never written, in HBM or in LDS.
 *
 * Conventions: those of include/pygpr_hip.h --
 *   - every pointer is a DEVICE pointer owned by the caller; the library allocates nothing
 *   - matrices are row-major with a leading dimension in elements
 *   - alignment: scalar throughout -- any base pointer, any ld >= width; gaps are neither read nor written
 *   - calls are asynchronous on `stream`; return 0 = enqueued, <0 = bad argument / HIP error (text via pg_last_error())
 */
#ifndef PYGPR_HIP_MATMUL_H
#define PYGPR_HIP_MATMUL_H

#include "pygpr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Cross form (Xc != NULL):   OUT[i][c] = sum_{j < nc} k(Xr_i, Xc_j) V[j][c]                       for i < nr, c < nrhs.  No noise term,
 *                            as in pg_kernel_build's cross form.
 * Symmetric form (Xc NULL):  OUT[i][c] = sum_{j < nr} k(Xr_i, Xr_j) V[j][c] + shift V[i][c],   shift = sum sigma_n^2 + jitter -- the
 *                            operator whose matrix the symmetric pg_kernel_build writes.  nc and ldc are ignored.
 *   spec: the stationary components are summed, or multiplied for a product spec (PG_SPEC_PRODUCT) with the factors formed explicitly;
 *         every kind but PG_KIND_SQDIST.  The per-pair forms are pg_kernel_cross_grad's: direct differences, nothing expanded.
 *   Xr [nr][d] at ldr, Xc [nc][d] at ldc, V [nc][nrhs] at ldv, OUT [nr][nrhs] at ldo;  1 <= d <= PG_MAX_DIM;  nr, nc, nrhs >= 0
 *   dtype: PG_F64 only.  jitter is read in the symmetric form only.
 * Only [0, nr) x [0, nrhs) of OUT is written; the inputs stay inputs (OUT must not overlap them).  An empty sum (nc == 0) writes zeros,
 * or shift V in the symmetric form.  A NaN in a point, in V or in hp reaches the entries it enters.
 * The sum over j runs in an order fixed by (nr, nc, nrhs) alone and there are no atomics: a call is bit-reproducible.  With few row
 * tiles the column range is cut into segments whose partial tiles go to `work`; a second launch folds them in segment order.  More
 * than 32 right-hand sides are taken in blocks of 32 columns, the covariance values evaluated again for each block.
 * work: pg_kernel_matmul_worksize(nr, nc, nrhs) doubles (0 when the call needs no segments: work may be NULL then), scratch of the call
 * (nothing in it needs initialising).  The symmetric form's size is that of nc = nr.  The worksize is -1 for a negative argument. */
long pg_kernel_matmul_worksize(int nr, int nc, int nrhs);      /* doubles */
int pg_kernel_matmul(pg_handle h, int dtype, const pg_covspec* spec, const double* hp, const void* Xr, long ldr, int nr, const void* Xc,
                     long ldc, int nc, int d, const void* V, long ldv, int nrhs, double jitter, void* OUT, long ldo, void* work,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif
