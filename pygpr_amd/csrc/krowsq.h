#pragma once
#include "common.h"
#include "pygpr_hip_rowsq.h"

// krowsq.hip: OUT[i] = sum_j k(Xr_i, Xc_j)^2 without writing k; see pg_kernel_rowsq
long pg_krowsq_worksize_impl(int nr, int nc);
int pg_krowsq_impl(hipStream_t st, const pg_covspec& spec, const double* hp, const double* Xr, long ldr, int nr, const double* Xc, long ldc,
                   int nc, int d, double* OUT, long ldo, double* work);
