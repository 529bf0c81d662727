/*
 * libpygpr_hip -- the matrix-free random-feature product of pathwise function samples (pygpr_amd/pathwise.py).
 * An eighth public header of the same library: the entry points below are new (the reference draws no function samples),
 * pygpr_amd/_lib.py binds them from this file as it binds include/pygpr_hip.h, and the same closed type vocabulary applies.
 *
 * A prior function drawn from random Fourier features is Phi(.) w with Phi[i][f] = cos(2 pi (x_i . nu_f + u_f)).  Phi is nr x nf and
 * is never written: pg_feature_matmul evaluates a 16 x 16 block of Phi^T in the accumulator layout of the fp64 matrix instruction,
 * where it is at once the operand of the product over the features -- pg_kernel_matmul (include/pygpr_hip_matmul.h) with another
 * pair function, the feature in the place of the column point.
 *
 * Conventions: those of include/pygpr_hip.h --
 *   - every pointer is a DEVICE pointer owned by the caller; the library allocates nothing
 *   - matrices are row-major with a leading dimension in elements
 *   - alignment: scalar throughout -- any base pointer, any ld >= width; gaps are neither read nor written
 *   - calls are asynchronous on `stream`; return 0 = enqueued, <0 = bad argument / HIP error (text via pg_last_error())
 */
#ifndef PYGPR_HIP_FEATURE_H
#define PYGPR_HIP_FEATURE_H

#include "pygpr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* OUT[i][c] = sum_{f < nf} cos(2 pi (sum_{k < d} X[i][k] NU[f][k] + U[f])) W[f][c]                       for i < nr, c < nrhs.
 *   X [nr][d] at ldx, NU [nf][d] at ldn: frequencies in cycles per unit; U [nf]: phases in cycles (0: the cosine, -0.25: the sine);
 *   W [nf][nrhs] at ldw, OUT [nr][nrhs] at ldo;  1 <= d <= PG_MAX_DIM;  nr, nf, nrhs >= 0.
 *   The argument t = x . nu + u is reduced as r = t - rint(t) and the cosine taken as 1 - 2 sin^2(pi r) on [-1/2, 1/2]: no product
 *   with pi is rounded, and an argument of any size costs the same.  There is no amplitude and no covariance spec: amplitudes belong in W.
 *   dtype: PG_F64 only.
 * Only [0, nr) x [0, nrhs) of OUT is written; the inputs stay inputs (OUT must not overlap them).  An empty sum (nf == 0) writes zeros.
 * A NaN reaches exactly the entries it enters: a row of X its row of OUT, an entry of W its column, a frequency or a phase everything.
 * The sum over f runs in an order fixed by (nr, nf, nrhs) alone and there are no atomics: a call is bit-reproducible.  With few row
 * tiles the feature range is cut into segments whose partial tiles go to `work`; a second launch folds them in segment order.  More
 * than 32 right-hand sides are taken in blocks of 32 columns, the features evaluated again for each block.
 * work: pg_feature_matmul_worksize(nr, nf, nrhs) doubles (0 when the call needs no segments: work may be NULL then), scratch of the
 * call (nothing in it needs initialising).  The worksize is -1 for a negative argument. */
long pg_feature_matmul_worksize(int nr, int nf, int nrhs);      /* doubles */
int pg_feature_matmul(pg_handle h, int dtype, const void* X, long ldx, int nr, const void* NU, long ldn, int nf, int d, const void* U,
                      const void* W, long ldw, int nrhs, void* OUT, long ldo, void* work, void* stream);

#ifdef __cplusplus
}
#endif
#endif
