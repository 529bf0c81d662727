/*
 * libpygpr_hip -- the squared row norms of a cross-covariance, for the certified variance bounds of pygpr_amd/varcache.py.
 * A tenth public header of the same library: the entry points below are new (the reference has nothing like them), pygpr_amd/_lib.py
 * binds them from this file as it binds include/pygpr_hip.h, and the same closed type vocabulary applies.
 *
 * The Galerkin residual of a cached variance, r* = k* - A Q c*, has |r*|^2 = |k*|^2 - 2 c*^T (A Q)^T k* + ...; the first term,
 * |k*|^2 = sum_j k(x*, x_j)^2, is not linear in k, so no product against a fixed matrix forms it for a sum of kinds.
 * pg_kernel_rowsq forms it from the point tiles as pg_kernel_matmul (include/pygpr_hip_matmul.h) forms K V: the covariance values are
 * evaluated in registers and squared there -- the nr x nc matrix is never written, in HBM or in LDS.
 *
 * Conventions: those of include/pygpr_hip.h --
 *   - every pointer is a DEVICE pointer owned by the caller; the library allocates nothing
 *   - matrices are row-major with a leading dimension in elements
 *   - alignment: scalar throughout -- any base pointer, any ld >= width; gaps are neither read nor written
 *   - calls are asynchronous on `stream`; return 0 = enqueued, <0 = bad argument / HIP error (text via pg_last_error())
 */
#ifndef PYGPR_HIP_ROWSQ_H
#define PYGPR_HIP_ROWSQ_H

#include "pygpr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* OUT[i] = sum_{j < nc} k(Xr_i, Xc_j)^2      for i < nr.  Cross form only (Xc may be Xr), no noise term, as in pg_kernel_build's
 * cross form.
 *   spec: the stationary components are summed, or multiplied for a product spec (PG_SPEC_PRODUCT) with the factors formed explicitly,
 *         and the sum or product is squared; every kind but PG_KIND_SQDIST.  The per-pair forms are pg_kernel_matmul's: direct
 *         differences, nothing expanded.  The noise entries of the spec are not read.
 *   Xr [nr][d] at ldr, Xc [nc][d] at ldc, OUT [nr][1] at ldo (ldo >= 1: entry i is OUT[i * ldo]);  1 <= d <= PG_MAX_DIM;  nr, nc >= 0
 *   dtype: PG_F64 only.
 * Only the nr entries of OUT are written; the inputs stay inputs (OUT must not overlap them).  An empty sum (nc == 0) writes zeros.
 * A NaN in a row point reaches that row's entry, a NaN in a column point or in hp every entry.
 * The sum over j runs in an order fixed by (nr, nc) alone and there are no atomics: a call is bit-reproducible.  With few row tiles
 * the column range is cut into segments (pg_kernel_matmul's, at one right-hand side) whose partial sums go to `work`; a second launch
 * folds them in segment order.
 * work: pg_kernel_rowsq_worksize(nr, nc) doubles (0 when the call needs no segments: work may be NULL then), scratch of the call
 * (nothing in it needs initialising).  The worksize is -1 for a negative argument. */
long pg_kernel_rowsq_worksize(int nr, int nc);      /* doubles */
int pg_kernel_rowsq(pg_handle h, int dtype, const pg_covspec* spec, const double* hp, const void* Xr, long ldr, int nr, const void* Xc,
                    long ldc, int nc, int d, void* OUT, long ldo, void* work, void* stream);

#ifdef __cplusplus
}
#endif
#endif
