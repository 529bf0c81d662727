/*
 * libpygpr_hip -- the nearest-neighbour (Vecchia) GP of pygpr_amd/vecchia.py: a brute-force neighbour search and the per-target
 * conditional blocks p(y_i | y_N(i)) with their loss, gradient and predictions.
 * A twelfth public header of the same library: the entry points below are new (the reference has nothing like them), pygpr_amd/_lib.py
 * binds them from this file as it binds include/pygpr_hip.h, and the same closed type vocabulary applies (with `const int*` for a
 * neighbour table that is read).
 *
 * Every target i is conditioned on at most m <= 63 points N(i).  Its block is B = (N(i), i) with the target LAST, b = |B| <= 64, and
 *   A_B   the spec's stationary part on the block's points (summed, or multiplied for a product spec), plus sum sigma_n^2 + jitter
 *         on the diagonal: pg_kernel_build's symmetric matrix restricted to the block
 *   c     = A_B^-1 e_last / (A_B^-1)_last,last  (c_last = 1),   v = 1 / (A_B^-1)_last,last,   r = c^T y_B
 *   loss  = sum_i 1/2 [log v_i + r_i^2 / v_i + log 2 pi]
 *   grad  = 1/2 sum_i sum_{p,q in B_i} W_pq dA_pq/dtheta,   W = (1/v - (r/v)^2) c c^T - (r/v)(a c^T + c a^T),   a = [A_NN^-1 y_N ; 0]
 * Nothing n x n, or n x m x m, is ever written: one wavefront builds its block in LDS from direct differences, factors it there
 * (Cholesky, in place, a packed lower triangle), solves twice and contracts the rank-two weight against the per-pair derivative forms.
 *
 * Conventions: those of include/pygpr_hip.h --
 *   - every pointer is a DEVICE pointer owned by the caller; the library allocates nothing
 *   - matrices are row-major with a leading dimension in elements
 *   - alignment: scalar throughout -- any base pointer, any ld >= width; gaps are neither read nor written
 *   - calls are asynchronous on `stream`; return 0 = enqueued, <0 = bad argument / HIP error (text via pg_last_error())
 */
#ifndef PYGPR_HIP_VECCHIA_H
#define PYGPR_HIP_VECCHIA_H

#include "pygpr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* nbr[i][0 .. m-1] = the up to m candidates j of Xc with the smallest  sum_k (s_k (Xq_ik - Xc_jk))^2  for every query i < q, ordered by
 * (distance, index), nearest first, a tie to the lower index; unfilled slots hold -1.  The terms are added in ascending k in fp64.
 * A candidate whose distance is NaN is never selected.
 *   causal != 0: the candidates of query i are j < min(i, n) (Xq is then Xc and q <= n);  causal == 0: every j < n.
 *   Xq [q][d] at ldq, Xc [n][d] at ldc, s [d] or NULL (all ones), nbr [q][m] int32 at ldn;  1 <= d <= PG_MAX_DIM, 1 <= m <= 63, q, n >= 0
 *   dtype: PG_F64 only.
 * Brute force, q n d operations: one wavefront per query walks the candidates 64 at a time.  No atomics: the result is a function of
 * the inputs alone.  The inputs stay inputs; only the q x m entries of nbr are written. */
int pg_knn(pg_handle h, int dtype, const void* Xq, long ldq, int q, const void* Xc, long ldc, int n, int d, const double* s, int m, int causal,
           int* nbr, long ldn, void* stream);

/* The conditional terms of targets first .. first + count - 1 and their sums.  Target t's block is the valid entries (0 <= j < n) of
 * row t of nbr, in their order, followed by point first + t.
 *   cmean[t] = y_i - r_i,  cvar[t] = v_i  (i = first + t);   out[0] = the loss summed over these targets;
 *   grad[0 .. nhp-1] = its derivative in every entry of hp (want_grad != 0; grad may be NULL otherwise; entries of hp that belong to no
 *   component and no noise term get 0);
 *   info[0] = 0, or 1 + the lowest point index first + t whose block met a pivot that is not positive (NaN included).  That target's
 *   cmean and cvar are NaN, and so are out[0] and the gradient; every other target's terms are what they are without it.
 *   spec: every kind but PG_KIND_SQDIST, summed or PG_SPEC_PRODUCT; the noise entries are squared and added to every block's diagonal
 *         with `jitter`.  hp has nhp entries.
 *   X [n][d] at ldx, Y [n], nbr [count][m] at ldn;  1 <= d <= PG_MAX_DIM, 1 <= m <= 63, 0 <= first, count >= 0, first + count <= n
 *   dtype: PG_F64 only.
 * Sums over the targets go through per-workgroup partial sums in `work`, which a second launch folds in workgroup order: no atomics,
 * a call is bit-reproducible.  An evaluation cut into chunks of targets is DEFINED as the sum of the chunks' out and grad in chunk order.
 * work: pg_vecchia_nlml_grad_worksize(count, d, nhp) doubles, scratch of the call (nothing in it needs initialising); -1 for a bad
 * argument.  The inputs stay inputs. */
long pg_vecchia_nlml_grad_worksize(int count, int d, int nhp);      /* doubles */
int pg_vecchia_nlml_grad(pg_handle h, int dtype, const pg_covspec* spec, const double* hp, int nhp, const void* X, long ldx, int n, int d,
                         const void* Y, const int* nbr, long ldn, int m, int first, int count, double jitter, int want_grad, void* cmean,
                         void* cvar, double* out, double* grad, int* info, void* work, void* stream);

/* Predictions at q points: query t's block is the valid entries of row t of nbr (indices into X) followed by Xq_t.  The block's last
 * diagonal entry is the prior variance plus sum sigma_n^2 WITHOUT jitter, the training points' diagonal carries `jitter` as above.
 *   mean[t] = -sum_{p < last} c_p y_p,   var[t] = v  (var may be NULL: the mean only);  info as above with the query's index.
 *   Xq [q][d] at ldq, nbr [q][m] at ldn; the other arguments as above.
 * work: pg_vecchia_predict_worksize(q, d) doubles. */
long pg_vecchia_predict_worksize(int q, int d);      /* doubles */
int pg_vecchia_predict(pg_handle h, int dtype, const pg_covspec* spec, const double* hp, const void* X, long ldx, int n, int d, const void* Y,
                       const void* Xq, long ldq, int q, const int* nbr, long ldn, int m, double jitter, void* mean, void* var, int* info,
                       void* work, void* stream);

#ifdef __cplusplus
}
#endif
#endif
