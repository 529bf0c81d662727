#pragma once
#include "common.h"
#include "pygpr_hip_feature.h"

// fmatmul.hip: OUT = Phi(X) W for random Fourier features without writing Phi; see pg_feature_matmul
long pg_fmatmul_worksize_impl(int nr, int nf, int nrhs);
int pg_fmatmul_impl(hipStream_t st, const double* X, long ldx, int nr, const double* NU, long ldn, int nf, int d, const double* U,
                    const double* W, long ldw, int nrhs, double* OUT, long ldo, double* work);
