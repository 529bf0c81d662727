// Leave-one-out cross-validation (include/pygpr_hip_loo.h; Rasmussen & Williams 5.4.2) from what a fitted model already holds:
// with c_i = [K^-1]_ii = sum_{k >= i} (L^-1)_ki^2 and alpha = K^-1 y
//   mu_i = y_i - alpha_i / c_i,  var_i = 1 / c_i,  L_loo = sum_i [ -1/2 log c_i + alpha_i^2 / (2 c_i) ] + n/2 log 2pi.
// pg_loo_terms is one HBM-bound pass over the lower triangle of L^-1 (column sums of squares, fp64 accumulation for both dtypes);
// pg_loo_weights and pg_loo_fold are the two n^2 passes that turn K^-1 into the operands of the gradient
//   grad_k = 1/2 sum (S S^T + q q^T - p p^T) o dK/dtheta_k,  S = K^-1 diag(sqrt(2 w)),
// whose n^3 product runs on the GEMM core and whose contraction is pg_nlml_grad, unchanged.
#include "linalg.h"

#define LOO_CH 256      // rows of L^-1 per chunk: one row of partial sums in the workspace per chunk
#define LOO_CW 128      // columns per strip = the diagonal block above which L^-1 is never read
#define LAUNCH_CHECK() PG_CHECK(hipGetLastError())

typedef double pg_d2 __attribute__((ext_vector_type(2)));
template <typename T> struct LooVec;
template <> struct LooVec<double> { typedef pg_d2 type; };
template <> struct LooVec<float> { typedef pg_f4 type; };

// Chunk ri (rows [256 ri, 256 ri + 256)) meets the strips cj <= 2 ri + 1 of the lower triangle: ri (ri + 1) blocks precede it in
// the launch, so block t belongs to the chunk ri with ri (ri + 1) <= t < (ri + 1)(ri + 2).  Strips to the right of a chunk are
// never launched; the last chunk's strips of pure padding (columns >= n) are cut off the end of the grid.
__device__ __forceinline__ void loo_block(int t, int& ri, int& cj) {
    ri = (int)((sqrtf(4.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
    while ((ri + 1) * (ri + 2) <= t) ++ri;
    while (ri * (ri + 1) > t) --ri;
    cj = t - ri * (ri + 1);
}

// part[ri][c] = sum over the rows k of chunk ri, c <= k < n, of M[k][c]^2.  A row lane reads 16-byte words along the row; the
// rows of a strip that lie above its diagonal 128-block are not touched (they may hold anything), the entries above the diagonal
// inside that block are read and dropped.
template <typename T>
__global__ __launch_bounds__(256) void loo_colsq_kernel(const T* __restrict__ M, long ldm, int n, double* __restrict__ part, long ldw,
                                                        unsigned* __restrict__ ticket) {
    typedef typename LooVec<T>::type vec_t;
    constexpr int V = 16 / (int)sizeof(T);
    constexpr int CT = LOO_CW / V;      // threads along a row: 64 (fp64: one wavefront per row) / 32 (fp32)
    constexpr int RL = 256 / CT;        // rows in flight per step
    __shared__ double red[RL][LOO_CW];
    const int tid = threadIdx.x;
    int ri, cj;
    loo_block(blockIdx.x, ri, cj);
    if (blockIdx.x == 0 && tid == 0) *ticket = 0u;      // the finishing launch counts its workgroups through this word
    const int ct = tid % CT, rl = tid / CT;
    const int c0 = cj * LOO_CW + ct * V;
    const int r_lo = max(ri * LOO_CH, cj * LOO_CW);
    const int r_hi = min(ri * LOO_CH + LOO_CH, n);
    double acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0.0;
#pragma unroll 4
    for (int r = r_lo + rl; r < r_hi; r += RL) {
        const vec_t x = *reinterpret_cast<const vec_t*>(M + (long)r * ldm + c0);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const double e = (r >= c0 + v) ? (double)x[v] : 0.0;
            acc[v] += e * e;
        }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) red[rl][ct * V + v] = acc[v];
    __syncthreads();
    if (tid < LOO_CW) {
        double s = 0.0;
#pragma unroll
        for (int l = 0; l < RL; ++l) s += red[l][tid];
        part[(long)ri * ldw + cj * LOO_CW + tid] = s;
    }
}

// c_i = the sum of column i's partial sums (chunks i / 256 .. nch - 1), then mu, var and the point's term of the loss; the
// workgroups' sums of terms meet in lossp, and the workgroup that draws the last ticket adds them up in a fixed order.
template <typename T>
__global__ __launch_bounds__(256) void loo_finish_kernel(const double* __restrict__ part, long ldw, int nch, const T* __restrict__ alpha,
                                                         const T* __restrict__ y, int n, T* __restrict__ c, T* __restrict__ mu,
                                                         T* __restrict__ var, double* lossp, unsigned* ticket, double* __restrict__ out) {
    __shared__ double red[4];
    __shared__ int last;
    const int tid = threadIdx.x, i = blockIdx.x * 256 + tid;
    double term = 0.0;
    if (i < n) {
        double s = 0.0;
        for (int ri = i / LOO_CH; ri < nch; ++ri) s += part[(long)ri * ldw + i];
        const double a = (double)alpha[i];
        c[i] = (T)s;
        var[i] = (T)(1.0 / s);
        const double yi = (double)y[i];
        mu[i] = (T)(yi - a / s);
        term = -0.5 * log(s) + 0.5 * a * a / s;      // = 1/2 log var_i + (y_i - mu_i)^2 / (2 var_i) without the cancellation ...
        if (yi != yi) term = yi;                     // ... so a NaN target, which that form would carry into the loss, is passed on by hand
    }
    term = wave_sum(term);
    if ((tid & 63) == 0) red[tid >> 6] = term;
    __syncthreads();
    if (tid == 0) {
        __hip_atomic_store(lossp + blockIdx.x, red[0] + red[1] + red[2] + red[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    double s = 0.0;
    for (int b = tid; b < (int)gridDim.x; b += 256) s += __hip_atomic_load(lossp + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s = wave_sum(s);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) out[0] = red[0] + red[1] + red[2] + red[3] + 0.5 * (double)n * 1.83787706640934548356;
}

// One pass over the real n x n part of the full symmetric K^-1, a wavefront per LOO_WR rows: b_i = sum_j Kinv_ij v_j from the
// entries as read, then Kinv_ij *= sqrt(2 w_j) written back -- v_j = alpha_j / c_j and sqrt(2 w_j) = sqrt(c_j + alpha_j^2) / c_j
// are formed once per column word and serve all rows of the wavefront.  p = (alpha + b) / sqrt2, q = (alpha - b) / sqrt2.
#define LOO_WR 8
template <typename T>
__global__ __launch_bounds__(256) void loo_weights_kernel(const T* __restrict__ c, const T* __restrict__ alpha, T* __restrict__ Kinv, long ldk,
                                                          int n, T* __restrict__ p, T* __restrict__ q) {
    typedef typename LooVec<T>::type vec_t;
    constexpr int V = 16 / (int)sizeof(T);
    const int lane = threadIdx.x & 63;
    const int r0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * LOO_WR;
    if (r0 >= n) return;
    double dot[LOO_WR];
#pragma unroll
    for (int k = 0; k < LOO_WR; ++k) dot[k] = 0.0;
    for (int j0 = lane * V; j0 < n; j0 += 64 * V) {
        double sc[V], vv[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int j = j0 + v;
            const double cj = j < n ? (double)c[j] : 1.0, aj = j < n ? (double)alpha[j] : 0.0;
            const double ic = 1.0 / cj;
            sc[v] = sqrt(cj + aj * aj) * ic;
            vv[v] = aj * ic;
        }
#pragma unroll
        for (int k = 0; k < LOO_WR; ++k) {
            const int r = r0 + k;
            if (r < n) {
                vec_t* w = reinterpret_cast<vec_t*>(Kinv + (long)r * ldk + j0);
                vec_t x = *w;
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    if (j0 + v < n) {      // the columns of the padding keep their bits
                        dot[k] += (double)x[v] * vv[v];
                        x[v] = (T)((double)x[v] * sc[v]);
                    }
                }
                *w = x;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < LOO_WR; ++k) {
        const double b = wave_sum(dot[k]);
        const int r = r0 + k;
        if (lane == 0 && r < n) {
            const double a = (double)alpha[r];
            p[r] = (T)((a + b) * 0.70710678118654752440);
            q[r] = (T)((a - b) * 0.70710678118654752440);
        }
    }
}

// M[r][c] += q_r q_c on the lower triangle of the real n x n part, 64 x 64 tiles on and below the diagonal only (tile t of the
// launch is (tr, tc) with tr (tr + 1) / 2 tiles before its row)
template <typename T> __global__ __launch_bounds__(256) void loo_fold_kernel(T* __restrict__ M, long ldm, int n, const T* __restrict__ q) {
    const int t = blockIdx.x;
    int tr = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
    while ((tr + 1) * (tr + 2) / 2 <= t) ++tr;
    while (tr * (tr + 1) / 2 > t) --tr;
    const int tc = t - tr * (tr + 1) / 2;
    for (int idx = threadIdx.x; idx < 64 * 64; idx += 256) {
        const int i = tr * 64 + (idx >> 6), j = tc * 64 + (idx & 63);
        if (i < n && j <= i) {
            T* e = M + (long)i * ldm + j;
            *e = (T)((double)*e + (double)q[i] * (double)q[j]);
        }
    }
}

long pg_loo_terms_worksize_impl(int n_pad) {
    const long nch = n_pad / LOO_CH;
    return nch * n_pad + nch + 2;       // the chunks' partial sums, the finishing workgroups' loss terms, the ticket word
}

template <typename T>
int pg_loo_terms_t(hipStream_t st, int n, int n_pad, const T* Minv, long ldm, const T* alpha, const T* y, T* c, T* mu, T* var, double* out,
                   double* work) {
    const int nch = (n + LOO_CH - 1) / LOO_CH, nstrip = (n + LOO_CW - 1) / LOO_CW;
    const int blocks = nch * (nch + 1) - (2 * nch - nstrip);
    double* lossp = work + (long)(n_pad / LOO_CH) * n_pad;
    unsigned* ticket = reinterpret_cast<unsigned*>(lossp + n_pad / LOO_CH);
    hipLaunchKernelGGL(loo_colsq_kernel<T>, dim3(blocks), dim3(256), 0, st, Minv, ldm, n, work, (long)n_pad, ticket);
    hipLaunchKernelGGL(loo_finish_kernel<T>, dim3(nch), dim3(256), 0, st, (const double*)work, (long)n_pad, nch, alpha, y, n, c, mu, var, lossp,
                       ticket, out);
    LAUNCH_CHECK();
    return 0;
}

template <typename T> int pg_loo_weights_t(hipStream_t st, int n, const T* c, const T* alpha, T* Kinv, long ldk, T* p, T* q) {
    hipLaunchKernelGGL(loo_weights_kernel<T>, dim3((n + 4 * LOO_WR - 1) / (4 * LOO_WR)), dim3(256), 0, st, c, alpha, Kinv, ldk, n, p, q);
    LAUNCH_CHECK();
    return 0;
}

template <typename T> int pg_loo_fold_t(hipStream_t st, int n, T* M, long ldm, const T* q) {
    const int t = (n + 63) / 64;
    hipLaunchKernelGGL(loo_fold_kernel<T>, dim3(t * (t + 1) / 2), dim3(256), 0, st, M, ldm, n, q);
    LAUNCH_CHECK();
    return 0;
}

#define INST(T)                                                                                                              \
    template int pg_loo_terms_t<T>(hipStream_t, int, int, const T*, long, const T*, const T*, T*, T*, T*, double*, double*); \
    template int pg_loo_weights_t<T>(hipStream_t, int, const T*, const T*, T*, long, T*, T*);                                \
    template int pg_loo_fold_t<T>(hipStream_t, int, T*, long, const T*);
INST(double)
INST(float)
