#pragma once
#include "common.h"
#include "pygpr_hip_matmul.h"

// kmatmul.hip: OUT = k(Xr, Xc) V (+ shift V in the symmetric form) without writing K; see pg_kernel_matmul
long pg_kmatmul_worksize_impl(int nr, int nc, int nrhs);
int pg_kmatmul_impl(hipStream_t st, const pg_covspec& spec, const double* hp, const double* Xr, long ldr, int nr, const double* Xc, long ldc,
                    int nc, int d, int sym, const double* V, long ldv, int nrhs, double jitter, double* OUT, long ldo, double* work);
