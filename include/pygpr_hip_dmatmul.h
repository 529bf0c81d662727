/*
 * libpygpr_hip -- the matrix-free product of the covariance's first-argument derivative (pygpr_amd/iterative.py: predict_grad;
 * pygpr_amd/pathwise.py: FunctionSamples.grad).
 * A ninth public header of the same library: the entry points below are new (the reference has no iterative solver), pygpr_amd/_lib.py
 * binds them from this file as it binds include/pygpr_hip.h, and the same closed type vocabulary applies.
 *
 * The derivative of k(x*, X) V in the test points needs sum_j dk(x*_i, x_j)/dx*_ik V[j][c] and nothing else of dk.  pg_kernel_matmul_dx
 * forms it from the point tiles as pg_kernel_matmul forms K V: a pair's radial factor is evaluated once, and for every coordinate k the
 * 16 x 16 block of derivative values stands in the accumulator layout of the fp64 matrix instruction, at once the operand of the
 * product over the column points -- no nr x nc array is written, in HBM or in LDS.
 *
 * Conventions: those of include/pygpr_hip.h --
 *   - every pointer is a DEVICE pointer owned by the caller; the library allocates nothing
 *   - matrices are row-major with a leading dimension in elements
 *   - alignment: scalar throughout -- any base pointer, any ld >= width; gaps are neither read nor written
 *   - calls are asynchronous on `stream`; return 0 = enqueued, <0 = bad argument / HIP error (text via pg_last_error())
 */
#ifndef PYGPR_HIP_DMATMUL_H
#define PYGPR_HIP_DMATMUL_H

#include "pygpr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* OUT[i * ldo + k * ldk + c] = sum_{j < nc} dk(Xr_i, Xc_j)/dXr_ik V[j][c]        for i < nr, k < d, c < nrhs;  ldk >= nrhs, ldo >= d ldk.
 * Cross form only: Xc == NULL is refused (-1).  Xc may be the same buffer as Xr: the sum then runs over every j, j = i included, and
 * the point is differentiated in its first place only.
 *   spec: the stationary components are summed; a product spec (PG_SPEC_PRODUCT) takes the product rule, the other factors' values
 *         formed explicitly and never as K / k_c.  Every kind but PG_KIND_SQDIST.  The per-pair derivative is pg_kernel_xgrad's: direct
 *         differences, nothing expanded; a Matern-1/2 pair at r = 0 contributes 0; the periodic kind takes its phase from the
 *         coordinate difference.  Noise has no cross term.
 *   Xr [nr][d] at ldr, Xc [nc][d] at ldc, V [nc][nrhs] at ldv;  1 <= d <= PG_MAX_DIM;  nr, nc, nrhs >= 0
 *   dtype: PG_F64 only.
 * Only [0, nr) x [0, d) x [0, nrhs) of OUT is written; the inputs stay inputs (OUT must not overlap them).  An empty sum (nc == 0)
 * writes zeros.  A NaN reaches exactly the entries it enters: one in V[j][c] column c of every row and coordinate, one in a row point
 * that row.
 * The sum over j runs in an order fixed by (nr, nc, d, nrhs) alone and there are no atomics: a call is bit-reproducible.  With few row
 * tiles the column range is cut into segments whose partial tiles go to `work`; a second launch folds them in segment order.  More
 * than 32 right-hand sides are taken in blocks of 32 columns and more than 8 coordinates in chunks of 8, the pairs' radial factors
 * evaluated again for each.
 * work: pg_kernel_matmul_dx_worksize(nr, nc, d, nrhs) doubles (0 when the call needs no segments: work may be NULL then), scratch of
 * the call (nothing in it needs initialising).  The worksize is -1 for a negative argument. */
long pg_kernel_matmul_dx_worksize(int nr, int nc, int d, int nrhs);      /* doubles */
int pg_kernel_matmul_dx(pg_handle h, int dtype, const pg_covspec* spec, const double* hp, const void* Xr, long ldr, int nr, const void* Xc,
                        long ldc, int nc, int d, const void* V, long ldv, int nrhs, void* OUT, long ldo, long ldk, void* work,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif
