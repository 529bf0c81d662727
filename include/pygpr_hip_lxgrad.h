/*
 * libpygpr_hip -- the training-input contraction against a low-rank weight: the gradient of the iterative exact GP's stochastic
 * marginal likelihood in the training inputs (pygpr_amd/stochastic.py: Stochastic_MLE.grad_x).
 * An eleventh public header of the same library: the entry points below are new (the reference has no iterative solver), pygpr_amd/_lib.py
 * binds them from this file as it binds include/pygpr_hip.h, and the same closed type vocabulary applies.
 *
 * With probe vectors the derivative of the log marginal likelihood in the covariance matrix is a weight of rank t + 1, W = U V^T (see
 * include/pygpr_hip_lowrank.h).  Both arguments of k carry a training input, so its gradient in x_i is
 * sum_j (W_ij + W_ji) dk(x_i, x_j)/dx_ik.  pg_kernel_lowrank_xgrad forms each 16 x 16 block of the weight on the fp64 matrix pipe from
 * the factor panels, transposed so that it arrives in the layout in which pg_kernel_matmul_dx (include/pygpr_hip_dmatmul.h) evaluates the
 * pair derivatives, and contracts the two in registers -- neither the n x n weight nor dk is written, in HBM or in LDS.
 *
 * Conventions: those of include/pygpr_hip.h --
 *   - every pointer is a DEVICE pointer owned by the caller; the library allocates nothing
 *   - matrices are row-major with a leading dimension in elements
 *   - alignment: scalar throughout -- any base pointer, any ld >= width; gaps are neither read nor written
 *   - calls are asynchronous on `stream`; return 0 = enqueued, <0 = bad argument / HIP error (text via pg_last_error())
 */
#ifndef PYGPR_HIP_LXGRAD_H
#define PYGPR_HIP_LXGRAD_H

#include "pygpr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Cross form (Xc != NULL):   OUT[i][k] (+)= sum_{j < nc} (sum_{t < r} U[i][t] V[j][t]) dk(Xr_i, Xc_j)/dXr_ik      for i < nr, k < d.
 *                            Xc may be the same buffer as Xr: the point is differentiated in its first place only.
 * Symmetric form (Xc NULL):  OUT[i][k] (+)= sum_{j < nr} (sum_t U[i][t] V[j][t] + V[i][t] U[j][t]) dk(Xr_i, Xr_j)/dXr_ik -- the gradient
 *                            in Xr of sum_ij (U V^T)_ij k(Xr_i, Xr_j), both places of k differentiated.  V is [nr][r] and must not be
 *                            NULL; nc and ldc are ignored.
 *   spec: the stationary components are summed; a product spec (PG_SPEC_PRODUCT) takes the product rule, the other factors' values
 *         formed explicitly and never as K / k_c.  Every kind but PG_KIND_SQDIST.  The per-pair derivative is pg_kernel_xgrad's and
 *         pg_kernel_matmul_dx's: direct differences, nothing expanded; a pair at r = 0 (the diagonal of the symmetric form included)
 *         contributes 0 for every kind, Matern-1/2 by convention; the periodic kind takes its phase from the coordinate difference.
 *         Noise and jitter have no derivative in a point; the noise entries of the spec are not read.
 *   Xr [nr][d] at ldr, Xc [nc][d] at ldc, U [nr][r] at ldu, V [nc][r] at ldv, OUT [nr][d] at ldo;  1 <= d <= PG_MAX_DIM;  nr, nc >= 0;
 *   0 <= r <= 64 (a larger rank is refused: split the columns and accumulate);  ldr, ldc, ldo >= d;  ldu, ldv >= r
 *   accumulate: 0 overwrites [0, nr) x [0, d) of OUT, non-zero adds to it.  Nothing else of OUT is read or written.
 *   dtype: PG_F64 only.
 * r == 0 or nc == 0 is the empty sum: zeros, or OUT as it is when accumulating.  nr == 0 does nothing.  The inputs stay inputs (OUT must
 * not overlap them).
 * A NaN reaches exactly the entries it enters.  Cross form: one in a row point or in U[i] reaches row i of OUT and no other; one in V[j]
 * or in a column point reaches every row (0 NaN is NaN: a zero weight does not shield a row).  Symmetric form: every point is a row and
 * a column point and both factors stand on both sides, so a NaN in any of them reaches every row.  One in hp reaches every entry.
 * The sum over j runs in an order fixed by (nr, nc, d, r) alone and there are no atomics: a call is bit-reproducible.  With few row tiles
 * the column range is cut into segments (pg_kernel_matmul's, at one right-hand side), and more than 32 factor columns are taken in two
 * passes over the pairs; the partial sums of segments and passes go to `work` and a second launch folds them in their order.  More than
 * 8 coordinates are taken in chunks of 8, the pairs' radial factors and weights evaluated again for each.
 * work: pg_kernel_lowrank_xgrad_worksize(nr, nc, d, r) doubles (0 when the call has one segment and one pass: work may be NULL then),
 * scratch of the call (nothing in it needs initialising).  The symmetric form's size is that of nc = nr.  The worksize is -1 for a
 * negative argument. */
long pg_kernel_lowrank_xgrad_worksize(int nr, int nc, int d, int r);      /* doubles */
int pg_kernel_lowrank_xgrad(pg_handle h, int dtype, const pg_covspec* spec, const double* hp, const void* Xr, long ldr, int nr, const void* Xc,
                            long ldc, int nc, int d, const void* U, long ldu, const void* V, long ldv, int r, void* OUT, long ldo,
                            int accumulate, void* work, void* stream);

#ifdef __cplusplus
}
#endif
#endif
