#pragma once
#include "common.h"
#include "pygpr_hip_sparse.h"

// sparse.hip: grad[p] (+)= sum_{i < m, j < n} W_ij dk(z_i, x_j)/dtheta_p over the stationary components of the spec; see pg_kernel_cross_grad
long pg_cross_grad_worksize_impl(int m, int n, int nhp);
int pg_cross_grad_extent(const pg_covspec& spec, int d);      // entries of hp / grad the spec's stationary blocks reach (1 + the last index)
template <typename T>
int pg_cross_grad_t(hipStream_t st, const pg_covspec& spec, const double* hp, const T* Z, long ldz, int m, const T* X, long ldx, int n, int d,
                    const T* W, long ldw, double* grad, int accumulate, double* work);
// the fold of the slot rows part[nblk][pw] into grad with the scales of each entry (pg_cross_grad_reduce_kernel); `spec` stripped of its
// product flag.  lowrank.hip writes the same slot layout and folds with this.
int pg_cross_grad_reduce(hipStream_t st, const pg_covspec& spec, const double* hp, const double* part, long nblk, int pw, int d, double* grad,
                         int accumulate);
