#pragma once
#include "common.h"
#include "pygpr_hip.h"

struct GradBatch {          // strides between batched experts of the gradient contraction (elements); all zero for one expert
    long eX, ehp, eK, ea, epart, egrad;
};
// A product spec (PG_SPEC_PRODUCT in ncomp): every host routine below takes the spec as the caller gave it and strips the flag with
// this before anything loops over ncomp -- the kernels get the clean copy and the choice of their PROD instantiation.
static inline bool pg_spec_strip(const pg_covspec& in, pg_covspec& out) {
    out = in;
    out.ncomp = in.ncomp & ~PG_SPEC_PRODUCT;
    return (in.ncomp & PG_SPEC_PRODUCT) != 0;
}
// f(PER, PROD) as std::bool_constant for a stripped spec: a periodic component takes an instantiation of its own (the other kinds'
// kernels compile exactly as they did without it), a product the one that carries every kind.
template <class F> static inline int pg_with_kinds(const pg_covspec& spec, bool prod, F f) {
    bool per = false;
    for (int c = 0; c < spec.ncomp; ++c) per = per || spec.kind[c] == PG_KIND_PERIODIC;
    return prod ? f(std::true_type{}, std::true_type{}) : (per ? f(std::true_type{}, std::false_type{}) : f(std::false_type{}, std::false_type{}));
}
template <typename T>
int pg_kbuild(hipStream_t st, const pg_covspec& spec, const double* hp, const T* Xr, long ldr, int nr,
              const T* Xc, long ldc, int nc, int d, int symmetric, int lower_only, int accumulate, double jitter, T* K,
              long ldk, int rows_pad, int cols_pad, int col0 = 0, int col1 = 0,    // [col0, col1): column window (0, 0 = all)
              int nexp = 1, long eX = 0, long ehp = 0, long eK = 0,                // batched experts: strides of X (= Xc), hp and K
              long eXr = -1);                                                      // ... and of the row points of a cross build (-1: eX)
template <typename T>
int pg_nlml_grad_t(hipStream_t st, const pg_covspec& spec, const double* hp, const T* X, long ldx, int n, int d,
                   const T* Kinv, long ldk, const T* alpha, double* grad, int nhp, double* work, long lwork,
                   int nexp = 1, long ehp = 0, long eX = 0, long eK = 0, long ea = 0, long egrad = 0);   // batched experts: strides
long pg_nlml_grad_worksize_impl(int n, int nhp);
template <typename T>
int pg_centres(hipStream_t st, const T* X, long ldx, int n, const T* Cn, long ldc, int m, int d, T* D, long ldd, int* idx);
template <typename T>
int pg_kgrad(hipStream_t st, const pg_covspec& spec, const double* hp, const T* X, long ldx, int n, int d, T* dK);
// xgrad.hip: out[p][k] (+)= sum_i W_pi dk(Xq_p, Z_i)/dXq_pk for W = u (vector) and / or B (matrix); see pg_kernel_xgrad
long pg_xgrad_worksize_impl(int ncu, int m, int n, int d, int nexp);
template <typename T>
int pg_xgrad_t(hipStream_t st, int ncu, const pg_covspec& spec, const double* hp, long hp_stride, const T* Xq, long ldq, long xq_stride, int m,
               const T* Z, long ldz, long z_stride, int n, int d, const T* u, long u_stride, T* out_u, long ldou, long ou_stride, const T* B,
               long ldb, long b_stride, int trans_b, T* out_b, long ldob, long ob_stride, int accumulate, double* work, long lwork, int nexp);
