#pragma once
#include "common.h"
#include "pygpr_hip_select.h"

// select.hip: greedy conditional-variance selection (partial pivoted Cholesky of k(X, X)); see pg_greedy_select
long pg_greedy_select_worksize_impl(int n, int m_max);
int pg_greedy_select_impl(hipStream_t st, const pg_covspec& spec, const double* hp, const double* X, long ldx, int n, int d, int m_max,
                          double floor, int* piv, int* count, double* trace, double* resid, double* work);
