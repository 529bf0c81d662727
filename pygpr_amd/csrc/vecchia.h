#pragma once
#include "common.h"
#include "pygpr_hip_vecchia.h"

// vecchia.hip: the nearest-neighbour (Vecchia) GP -- brute-force neighbour search and the per-target conditional blocks; see
// include/pygpr_hip_vecchia.h
int pg_knn_impl(hipStream_t st, const double* Xq, long ldq, int q, const double* Xc, long ldc, int n, int d, const double* s, int m, int causal,
                int* nbr, long ldn);
long pg_vecchia_worksize_impl(int count, int d, int nhp);      // doubles; nhp = 0: the prediction's
int pg_vecchia_nlml_grad_impl(hipStream_t st, const pg_covspec& spec, const double* hp, int nhp, const double* X, long ldx, int n, int d,
                              const double* Y, const int* nbr, long ldn, int m, int first, int count, double jitter, int want_grad,
                              double* cmean, double* cvar, double* out, double* grad, int* info, double* work);
int pg_vecchia_predict_impl(hipStream_t st, const pg_covspec& spec, const double* hp, const double* X, long ldx, int n, int d, const double* Y,
                            const double* Xq, long ldq, int q, const int* nbr, long ldn, int m, double jitter, double* mean, double* var,
                            int* info, double* work);
