#pragma once
#include "common.h"
#include "pygpr_hip_lxgrad.h"

// lxgrad.hip: OUT[i][k] (+)= sum_j (U V^T [+ V U^T])_ij dk(Xr_i, Xc_j)/dXr_ik without writing the weight or dk; see pg_kernel_lowrank_xgrad
#define LXG_RC 32      // factor columns of one pass over the pairs

static inline int lxg_npass(int r) { return (r + LXG_RC - 1) / LXG_RC; }

long pg_lxgrad_worksize_impl(int nr, int nc, int d, int r);
int pg_lxgrad_impl(hipStream_t st, const pg_covspec& spec, const double* hp, const double* Xr, long ldr, int nr, const double* Xc, long ldc,
                   int nc, int d, int sym, const double* U, long ldu, const double* V, long ldv, int r, double* OUT, long ldo, int accumulate,
                   double* work);
