#pragma once
#include "common.h"
#include "pygpr_hip_lowrank.h"

// lowrank.hip: grad[p] (+)= sum_ij (U V^T)_ij dk(xr_i, xc_j)/dtheta_p without the weight matrix; see pg_kernel_lowrank_grad
long pg_lowrank_grad_worksize_impl(int nr, int nc, int r, int nhp);
int pg_lowrank_grad_impl(hipStream_t st, const pg_covspec& spec, const double* hp, const double* Xr, long ldr, int nr, const double* Xc, long ldc,
                         int nc, int d, int sym, const double* U, long ldu, const double* V, long ldv, int r, double* grad, int accumulate,
                         double* work);
