#pragma once
#include "common.h"
#include "pygpr_hip_dmatmul.h"

// dmatmul.hip: OUT[i][k][c] = sum_j dk(Xr_i, Xc_j)/dXr_ik V[j][c] without writing dk; see pg_kernel_matmul_dx
#define DMM_KC 8      // coordinates of the output one workgroup accumulates (a chunk); dimensions <= 4 take one chunk of 4

// the chunk of dimension d and how many of them cover it
static inline int dmm_chunk(int d) { return d <= 4 ? 4 : DMM_KC; }
static inline int dmm_nchunk(int d) { return (d + dmm_chunk(d) - 1) / dmm_chunk(d); }

long pg_dmatmul_worksize_impl(int nr, int nc, int d, int nrhs);
int pg_dmatmul_impl(hipStream_t st, const pg_covspec& spec, const double* hp, const double* Xr, long ldr, int nr, const double* Xc, long ldc,
                    int nc, int d, const double* V, long ldv, int nrhs, double* OUT, long ldo, long ldk, double* work);
