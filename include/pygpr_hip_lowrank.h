/*
 * libpygpr_hip -- the hyper-parameter contraction against a low-rank weight: the gradient kernel of the iterative exact GP's stochastic
 * marginal likelihood (pygpr_amd/stochastic.py).
 * A seventh public header of the same library: the entry points below are new (the reference has no iterative solver), pygpr_amd/_lib.py
 * binds them from this file as it binds include/pygpr_hip.h, and the same closed type vocabulary applies.
 *
 * With probe vectors the gradient of the log marginal likelihood is  sum_ij W_ij dK_ij/dtheta_p  with a weight of rank t + 1,
 * W = 1/2 [ (1/t) sum_i (A^-1 z_i)(P^-1 z_i)^T - alpha alpha^T ] = U V^T.  pg_kernel_lowrank_grad is pg_kernel_cross_grad
 * (include/pygpr_hip_sparse.h) for such a weight: each 16 x 16 block of W is formed from the factor panels on the fp64 matrix pipe and
 * meets the pair derivatives in registers -- the n x n weight is never written, in HBM or in LDS.
 *
 * Conventions: those of include/pygpr_hip.h --
 *   - every pointer is a DEVICE pointer owned by the caller; the library allocates nothing
 *   - matrices are row-major with a leading dimension in elements
 *   - alignment: scalar throughout -- any base pointer, any ld >= width; gaps are neither read nor written
 *   - calls are asynchronous on `stream`; return 0 = enqueued, <0 = bad argument / HIP error (text via pg_last_error())
 */
#ifndef PYGPR_HIP_LOWRANK_H
#define PYGPR_HIP_LOWRANK_H

#include "pygpr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Cross form (Xc != NULL):   grad[p] (+)= sum_{i < nr, j < nc} (sum_{t < r} U[i][t] V[j][t]) dk(Xr_i, Xc_j)/dtheta_p  for every parameter
 *                            p of the spec's stationary components -- pg_kernel_cross_grad's contract with W = U V^T: the same per-pair
 *                            forms from direct differences, the same product rule (PG_SPEC_PRODUCT) with the other factors formed
 *                            explicitly, no factor 1/2, every (i, j) counted once.
 * Symmetric form (Xc NULL):  the same sum over all ordered pairs of the one point set Xr, the diagonal counted once; V is [nr][r], nc and
 *                            ldc are ignored.  dk is symmetric there, so only tiles on and below the diagonal are walked, with the
 *                            weight W_ij + W_ji off the diagonal.
 *   Xr [nr][d] at ldr, Xc [nc][d] at ldc, U [nr][r] at ldu, V [nc][r] at ldv;  1 <= d <= PG_MAX_DIM;  nr, nc >= 0;  0 <= r <= 64 (a larger
 *   rank: split the columns and accumulate)
 *   hp: the model's hyper-parameters (fp64);  grad: fp64, at least as long as the spec's blocks reach (off[c] + the block's width)
 *   accumulate: 0 overwrites the spec's entries, non-zero adds to them.  Entries at noise_off and entries outside the spec are neither
 *   read nor written in either mode.
 *   dtype: PG_F64 only; every kind but PG_KIND_SQDIST.
 * r == 0 or an empty point set is the empty sum: zeros, or grad as it is when accumulating.  The inputs stay inputs.  A NaN in a point,
 * in U, in V or in hp reaches the entries it enters.
 * The order of the sum is fixed by (nr, nc, r) alone and there are no atomics: one workgroup per column tile and segment of the row
 * tiles writes its partial sums into `work`, pg_kernel_cross_grad's reduce folds them in a fixed order -- a call is bit-reproducible.
 * More than 32 factor columns are taken in two passes over the pairs.
 * work: pg_kernel_lowrank_grad_worksize(nr, nc, r, nhp) doubles with nhp >= the reach of the spec's blocks (the model's parameter
 * count), scratch of the call (nothing in it needs initialising); 0 for an empty sum (work may be NULL then).  The symmetric form's
 * size is that of nc = nr.  The worksize is -1 for a negative argument. */
long pg_kernel_lowrank_grad_worksize(int nr, int nc, int r, int nhp);   /* doubles */
int pg_kernel_lowrank_grad(pg_handle h, int dtype, const pg_covspec* spec, const double* hp, const void* Xr, long ldr, int nr, const void* Xc,
                           long ldc, int nc, int d, const void* U, long ldu, const void* V, long ldv, int r, double* grad, int accumulate,
                           void* work, void* stream);

#ifdef __cplusplus
}
#endif
#endif
