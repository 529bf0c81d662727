// Conditioning a fitted exact GP on k new points: a block extension of the factor L, its inverse Minv = L^-1, the 128-blocks of
// inv_diag, u = L^-1 y and alpha, with the hyper-parameters unchanged (the reference has no such entry point).  With Kt = k(Xn, X)
// [k x n] and Knn = k(Xn, Xn) + noise + jitter I:
//
//   Vt = Kt Minv^T,  S = Knn - Vt Vt^T = Ls Ls^T,  Lsi = Ls^-1
//   L   <- [[L, 0], [Vt, Ls]]
//   Minv <- [[Minv, 0], [-Lsi (Vt Minv), Lsi]]
//   u   <- [u; Lsi (yn - Vt u)],  alpha = Minv^T u
//
// Launches, in stream order:
//   1. vt     : Vt[i][j] = sum_{l <= j} Kt[i][l] Minv[j][l].  A workgroup owns a strip of 32 rows j of Minv and walks their columns in
//               chunks of 32, the chunk of all k rows of Kt staged beside it in LDS: every element of Minv's lower triangle is read
//               once.  The same workgroup emits its strip's partial sums of Vt Vt^T and Vt u.
//   2. sum x2 : the strips' partial sums added up in two levels (32 segments, then one), in a fixed order.
//   3. schur  : one workgroup.  S in LDS (k <= 128: 132 KiB in fp64), its Cholesky factor Ls in place; a pivot that is not > 0 (NaN
//               included) sets *info = n + c + 1 and ends the call's device work.  Then Lsi by substitution (one column per thread,
//               stored transposed in the upper triangle) and the tail of u.  Everything goes to the workspace.
//   4. rows   : P[i][l] = sum_{j >= l} Vt[i][j] Minv[j][l]: a workgroup owns 32 columns of Minv and a chunk of 2048 rows; partial sums
//               per row chunk.  Minv's lower triangle is read once more.
//   5. epi    : adds the row chunks' partials and forms the new rows of L^-1, W = -Lsi P.
//   6. commit : the only launch that writes the model's buffers, and only if *info == 0: rows n .. n+k-1 of L (Vt, Ls, zeros) and of
//               Minv (W, Lsi, zeros), the same rows of the 128-blocks of inv_diag they cross, and u's tail.
//   7. alpha  : Minv^T u over the new Minv (its third read): pg_trmv's transposed pass, but with explicit bounds and gated on *info.
// Launches 1 and 4 read rows < n of Minv only; launch 6 writes rows >= n only.  Every read of Minv is of its lower triangle with
// explicit l <= j bounds: its strictly upper part is scratch.  All sums accumulate in fp64, for both storage types.
#include "linalg.h"
#include <cmath>

#define AP_RS 32        // strip of Minv rows (vt) / columns (rows) owned by a workgroup
#define AP_CC 32        // inner chunk staged in LDS
#define AP_LD 33        // odd LDS leading dimension of a staged chunk
#define AP_RC 2048      // rows of Minv per workgroup in the row pass
#define AP_SEG 32       // segments of the first level of the partial-sum reduction

// the thread tile of launches 1 and 4: a thread accumulates 4 strip entries x 4 of the k vectors over a share of the inner chunk;
// kg = next power of two >= ceil(k / 4), so 8 kg tiles and P = 256 / (8 kg) threads (adjacent lanes) per tile
static inline int ap_kg(int k) {
    int kg = 1;
    while (4 * kg < k) kg *= 2;
    return kg;
}

struct ApTile {
    int part, P, rg, ig;
};

__device__ __forceinline__ ApTile ap_tile(int kg) {
    ApTile t;
    t.P = 256 / (8 * kg);
    t.part = threadIdx.x % t.P;
    const int tile = threadIdx.x / t.P;
    t.rg = tile % 8;
    t.ig = tile / 8;
    return t;
}

// acc[r][q] += sum over this thread's share of the chunk of A[rg*4 + r][c] B[ig*4 + q][c]
__device__ __forceinline__ void ap_fma(const double* A, const double* B, const ApTile& t, double acc[4][4]) {
    for (int c = t.part; c < AP_CC; c += t.P) {
        double a[4], b[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) a[r] = A[(t.rg * 4 + r) * AP_LD + c];
#pragma unroll
        for (int q = 0; q < 4; ++q) b[q] = B[(t.ig * 4 + q) * AP_LD + c];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[r][q] += a[r] * b[q];
    }
}

// the P lanes of a tile are adjacent and P divides 64: butterfly inside the group, fixed order
__device__ __forceinline__ void ap_reduce(double acc[4][4], int P) {
    for (int o = P / 2; o > 0; o >>= 1)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[r][q] += __shfl_xor(acc[r][q], o, 64);
}

// 1. Vt and the strip's partial sums of Vt Vt^T (k x k) and Vt u (k): part + s * E, E = k k + k
template <typename T>
__global__ __launch_bounds__(256) void append_vt_kernel(const T* __restrict__ Minv, long ldm, int n, const T* __restrict__ Kt, long ldkt,
                                                        int k, int kg, const T* __restrict__ u, double* __restrict__ vt, long ldv,
                                                        double* __restrict__ part, long E) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int kq = 4 * kg, tid = threadIdx.x;
    double* ms = reinterpret_cast<double*>(smem_raw);    // [AP_RS][AP_LD]: Minv[j0 + r][c0 + c]
    double* ks = ms + AP_RS * AP_LD;                     // [kq][AP_LD]:    Kt[i][c0 + c], rows >= k zero
    const int s = gridDim.x - 1 - blockIdx.x;            // the long strips (bottom of the matrix) first
    const int j0 = s * AP_RS, jend = min(j0 + AP_RS, n);
    const ApTile t = ap_tile(kg);
    for (int idx = tid; idx < (kq - k) * AP_LD; idx += 256) ks[k * AP_LD + idx] = 0.0;
    double acc[4][4] = {};
    for (int c0 = 0; c0 < jend; c0 += AP_CC) {
        __syncthreads();
        for (int idx = tid; idx < AP_RS * AP_CC; idx += 256) {
            const int r = idx / AP_CC, c = idx % AP_CC, j = j0 + r, l = c0 + c;
            ms[r * AP_LD + c] = (j < jend && l <= j) ? (double)Minv[(long)j * ldm + l] : 0.0;
        }
        for (int idx = tid; idx < k * AP_CC; idx += 256) {
            const int i = idx / AP_CC, c = idx % AP_CC, l = c0 + c;
            ks[i * AP_LD + c] = l < jend ? (double)Kt[(long)i * ldkt + l] : 0.0;
        }
        __syncthreads();
        ap_fma(ms, ks, t, acc);
    }
    ap_reduce(acc, t.P);
    __syncthreads();
    double* vs = ks;                                     // [AP_RS][kq]: Vt[i][j0 + r] (fits: kq AP_RS <= kq AP_LD)
    if (t.part == 0)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) vs[(t.rg * 4 + r) * kq + t.ig * 4 + q] = acc[r][q];
    __syncthreads();
    for (int idx = tid; idx < k * AP_RS; idx += 256) {
        const int i = idx / AP_RS, r = idx % AP_RS;
        if (j0 + r < jend) vt[(long)i * ldv + j0 + r] = vs[r * kq + i];
    }
    double* pp = part + (long)s * E;
    for (int idx = tid; idx < k * k + k; idx += 256) {
        double g = 0.0;
        if (idx < k * k) {
            const int i = idx / k, i2 = idx % k;
            for (int r = 0; r < AP_RS; ++r) g += vs[r * kq + i] * vs[r * kq + i2];
        } else {
            const int i = idx - k * k;
            for (int r = 0; r < jend - j0; ++r) g += vs[r * kq + i] * (double)u[j0 + r];
        }
        pp[idx] = g;
    }
}

// 2. out[g][idx] = sum of rows [g per, min((g + 1) per, nrow)) of part[row][idx], idx < E
__global__ __launch_bounds__(256) void append_sum_kernel(const double* __restrict__ part, long E, int nrow, int per, double* __restrict__ out) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= E) return;
    const int g = blockIdx.y, r1 = min((g + 1) * per, nrow);
    double s = 0.0;
    for (int r = g * per; r < r1; ++r) s += part[(long)r * E + idx];
    out[(long)g * E + idx] = s;
}

// 3. S = Knn - Vt Vt^T, Ls, Lsi, ut = Lsi (yn - Vt u) -> ls, lsi [k][k] (zeros above the diagonal), ut [k]
template <typename T>
__global__ __launch_bounds__(256) void append_schur_kernel(const double* __restrict__ red, int k, int n, const T* __restrict__ Knn, long ldknn,
                                                           const T* __restrict__ yn, double* __restrict__ ls, double* __restrict__ lsi,
                                                           double* __restrict__ ut, int* __restrict__ info) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x, ld = k + 1;
    double* S = reinterpret_cast<double*>(smem_raw);     // [k][k + 1]: Ls in the lower triangle, Lsi^T strictly above
    double* dg = S + k * ld;                             // [k] 1 / Ls[i][i] = Lsi[i][i]
    double* rr = dg + k;                                 // [k] yn - Vt u
    const double* G = red;
    const double* h = red + (long)k * k;
    for (int idx = tid; idx < k * k; idx += 256) {
        const int i = idx / k, j = idx % k;
        if (j <= i) S[i * ld + j] = (double)Knn[(long)i * ldknn + j] - G[idx];
    }
    if (tid < k) rr[tid] = (double)yn[tid] - h[tid];
    __syncthreads();
    for (int c = 0; c < k; ++c) {
        const double piv = S[c * ld + c];
        if (!(piv > 0.0)) {                              // uniform: every thread read the same pivot
            if (tid == 0) *info = n + c + 1;
            return;
        }
        const double dd = sqrt(piv);
        for (int i = c + 1 + tid; i < k; i += 256) S[i * ld + c] /= dd;
        __syncthreads();
        if (tid == 0) S[c * ld + c] = dd;                // nobody reads it before the next pivot
        const int m = k - c - 1;
        for (int idx = tid; idx < m * m; idx += 256) {
            const int ii = idx / m, jj = idx % m;
            if (jj <= ii) {
                const int i = c + 1 + ii, j = c + 1 + jj;
                S[i * ld + j] -= S[i * ld + c] * S[j * ld + c];
            }
        }
        __syncthreads();
    }
    if (tid < k) dg[tid] = 1.0 / S[tid * ld + tid];
    __syncthreads();
    // column c of Lsi by forward substitution; X[i][c] (i > c) is kept at S[c][i]: only thread c touches row c's upper part
    if (tid < k) {
        const int c = tid;
        for (int i = c + 1; i < k; ++i) {
            double s0 = S[i * ld + c] * dg[c], s1 = 0.0;
            int m = c + 1;
            for (; m + 1 < i; m += 2) {
                s0 += S[i * ld + m] * S[c * ld + m];
                s1 += S[i * ld + m + 1] * S[c * ld + m + 1];
            }
            if (m < i) s0 += S[i * ld + m] * S[c * ld + m];
            S[c * ld + i] = -(s0 + s1) * dg[i];
        }
    }
    __syncthreads();
    if (tid < k) {
        const int i = tid;
        double s = dg[i] * rr[i];
        for (int m = 0; m < i; ++m) s += S[m * ld + i] * rr[m];
        ut[i] = s;
    }
    for (int idx = tid; idx < k * k; idx += 256) {
        const int i = idx / k, j = idx % k;
        ls[idx] = j <= i ? S[i * ld + j] : 0.0;
        lsi[idx] = j < i ? S[j * ld + i] : (j == i ? dg[i] : 0.0);
    }
    if (tid == 0) *info = 0;
}

// 4. part[(rc k + i) ldp + l] = sum_{j in row chunk rc, j >= l, j < n} Vt[i][j] Minv[j][l] for the 32 columns l of this workgroup
template <typename T>
__global__ __launch_bounds__(256) void append_rows_kernel(const T* __restrict__ Minv, long ldm, int n, const double* __restrict__ vt, long ldv,
                                                          int k, int kg, double* __restrict__ part, long ldp, const int* __restrict__ info) {
    if (*info) return;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int kq = 4 * kg, tid = threadIdx.x;
    double* ms = reinterpret_cast<double*>(smem_raw);    // [AP_RS][AP_LD]: Minv[j00 + c][l0 + r] (transposed: columns own the strip)
    double* vs = ms + AP_RS * AP_LD;                     // [kq][AP_LD]:    Vt[i][j00 + c], rows >= k zero
    const int cs = blockIdx.x, rc = blockIdx.y;                      // the long column strips (left of the matrix) first
    const int l0 = cs * AP_RS;
    const int jlo = max(rc * AP_RC, l0), jhi = min((rc + 1) * AP_RC, n);
    if (jlo >= jhi) return;
    const ApTile t = ap_tile(kg);
    for (int idx = tid; idx < (kq - k) * AP_LD; idx += 256) vs[k * AP_LD + idx] = 0.0;
    double acc[4][4] = {};
    for (int j00 = jlo; j00 < jhi; j00 += AP_CC) {
        __syncthreads();
        for (int idx = tid; idx < AP_CC * AP_RS; idx += 256) {
            const int c = idx / AP_RS, r = idx % AP_RS, j = j00 + c, l = l0 + r;
            ms[r * AP_LD + c] = (j < jhi && l <= j) ? (double)Minv[(long)j * ldm + l] : 0.0;
        }
        for (int idx = tid; idx < k * AP_CC; idx += 256) {
            const int i = idx / AP_CC, c = idx % AP_CC, j = j00 + c;
            vs[i * AP_LD + c] = j < jhi ? vt[(long)i * ldv + j] : 0.0;
        }
        __syncthreads();
        ap_fma(ms, vs, t, acc);
    }
    ap_reduce(acc, t.P);
    if (t.part == 0)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int l = l0 + t.rg * 4 + r;
            if (l >= n) continue;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = t.ig * 4 + q;
                if (i < k) part[((long)rc * k + i) * ldp + l] = acc[r][q];
            }
        }
}

// 5. W[i][l] = -sum_{i2 <= i} Lsi[i][i2] P[i2][l], P = the sum of the row chunks' partials (chunks from l's own on)
__global__ __launch_bounds__(256) void append_rows_epi_kernel(const double* __restrict__ part, long ldp, int nrc, int n, int k,
                                                              const double* __restrict__ lsi, double* __restrict__ w, long ldw,
                                                              const int* __restrict__ info) {
    if (*info) return;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* ps = reinterpret_cast<double*>(smem_raw);    // [k][AP_LD]
    const int tid = threadIdx.x, l0 = blockIdx.x * AP_RS, rc0 = l0 / AP_RC;
    for (int idx = tid; idx < k * AP_RS; idx += 256) {
        const int i = idx / AP_RS, c = idx % AP_RS, l = l0 + c;
        double s = 0.0;
        if (l < n)
            for (int rc = rc0; rc < nrc; ++rc) s += part[((long)rc * k + i) * ldp + l];
        ps[i * AP_LD + c] = s;
    }
    __syncthreads();
    for (int idx = tid; idx < k * AP_RS; idx += 256) {
        const int i = idx / AP_RS, c = idx % AP_RS, l = l0 + c;
        if (l >= n) continue;
        double s = 0.0;
        for (int i2 = 0; i2 <= i; ++i2) s += lsi[i * k + i2] * ps[i2 * AP_LD + c];
        w[(long)i * ldw + l] = -s;
    }
}

// 6. rows n + r of L, Minv and inv_diag's block, u[n + r]; grid (n_pad / 256, k)
template <typename T>
__global__ __launch_bounds__(256) void append_commit_kernel(int n, int k, const double* __restrict__ vt, const double* __restrict__ w, long ldv,
                                                            const double* __restrict__ ls, const double* __restrict__ lsi,
                                                            const double* __restrict__ ut, T* __restrict__ L, long ldl, T* __restrict__ Minv,
                                                            long ldm, T* __restrict__ invd, T* __restrict__ u, const int* __restrict__ info) {
    if (*info) return;
    const int r = blockIdx.y, g = n + r, c = blockIdx.x * 256 + threadIdx.x;
    double lv = 0.0, mv = 0.0;
    if (c < n) {
        lv = vt[(long)r * ldv + c];
        mv = w[(long)r * ldv + c];
    } else if (c <= g) {
        lv = ls[r * k + (c - n)];
        mv = lsi[r * k + (c - n)];
    }
    L[(long)g * ldl + c] = (T)lv;
    Minv[(long)g * ldm + c] = (T)mv;
    const int b = g / 128;
    if (c >= b * 128 && c < b * 128 + 128) invd[(long)b * 128 * 128 + (long)(g % 128) * 128 + (c - b * 128)] = (T)mv;
    if (c == 0) u[g] = (T)ut[r];
}

// 7. part[rc][j] = sum_{i in row chunk rc, j <= i < nt} Minv[i][j] u[i]: gemv_t_partial_kernel's pass with explicit bounds (the strictly
// upper part of Minv's diagonal 128-blocks is not read either), then alpha[j] = sum_{rc >= j / 256} part[rc][j] if *info == 0
template <typename T>
__global__ __launch_bounds__(256) void append_alpha_partial_kernel(const T* __restrict__ Minv, long ldm, int nt, const T* __restrict__ u,
                                                                   double* __restrict__ part, long ldp, const int* __restrict__ info) {
    if (*info) return;
    const int cc = blockIdx.x, rc = blockIdx.y, tid = threadIdx.x;
    if (rc < cc) return;
    __shared__ double xs[256];
    const int i0 = rc * 256, j = cc * 256 + tid;
    xs[tid] = i0 + tid < nt ? (double)u[i0 + tid] : 0.0;
    __syncthreads();
    const int ilo = max(i0, j) - i0, ihi = min(i0 + 256, nt) - i0;
    const T* a = Minv + (long)i0 * ldm + j;
    double s = 0.0;
    for (int i = ilo; i < ihi; ++i) s += (double)a[(long)i * ldm] * xs[i];
    part[(long)rc * ldp + j] = s;
}

template <typename T>
__global__ __launch_bounds__(256) void append_alpha_reduce_kernel(const double* __restrict__ part, long ldp, int nrc, T* __restrict__ alpha,
                                                                  const int* __restrict__ info) {
    if (*info) return;
    const int j = blockIdx.x * 256 + threadIdx.x;
    double s = 0.0;
    for (int rc = j / 256; rc < nrc; ++rc) s += part[(long)rc * ldp + j];
    alpha[j] = (T)s;
}

// workspace layout, in bytes, every region 256-byte aligned
struct ApWork {
    long vt, w, red, part2, ls, lsi, ut, scratch, total;
};

static long ap_al(long b) { return (b + 255) / 256 * 256; }

static ApWork ap_layout(int n_pad, int k) {
    const long E = (long)k * k + k;
    const long nstrip = (n_pad + AP_RS - 1) / AP_RS, nrc = (n_pad + AP_RC - 1) / AP_RC;
    long scratch = std::max(nstrip * E * 8, nrc * k * (long)n_pad * 8);
    scratch = std::max(scratch, (long)(n_pad / 256) * n_pad * 8);          // launch 7's partials (after the row pass is done with it)
    ApWork a;
    long o = 0;
    a.vt = o; o += ap_al((long)k * n_pad * 8);
    a.w = o; o += ap_al((long)k * n_pad * 8);
    a.red = o; o += ap_al(E * 8);
    a.part2 = o; o += ap_al(AP_SEG * E * 8);
    a.ls = o; o += ap_al((long)k * k * 8);
    a.lsi = o; o += ap_al((long)k * k * 8);
    a.ut = o; o += ap_al((long)k * 8);
    a.scratch = o; o += ap_al(scratch);
    a.total = o;
    return a;
}

long pg_chol_append_worksize_impl(int tsize, int n_pad, int k) {
    if (n_pad <= 0 || k < 1 || k > PG_APPEND_KMAX) return -1;
    return (ap_layout(n_pad, k).total + tsize - 1) / tsize;
}

template <typename T>
int pg_chol_append_t(pg_ctx*, hipStream_t st, int n, int k, int n_pad, T* L, long ldl, T* invd, T* Minv, long ldm, const T* Kt, long ldkt,
                     const T* Knn, long ldknn, const T* yn, T* u, T* alpha, void* work, int* info) {
    const ApWork a = ap_layout(n_pad, k);
    char* wb = static_cast<char*>(work);
    double* vt = reinterpret_cast<double*>(wb + a.vt);
    double* w = reinterpret_cast<double*>(wb + a.w);
    double* red = reinterpret_cast<double*>(wb + a.red);
    double* part2 = reinterpret_cast<double*>(wb + a.part2);
    double* ls = reinterpret_cast<double*>(wb + a.ls);
    double* lsi = reinterpret_cast<double*>(wb + a.lsi);
    double* ut = reinterpret_cast<double*>(wb + a.ut);
    double* scratch = reinterpret_cast<double*>(wb + a.scratch);
    const long E = (long)k * k + k;
    const int kg = ap_kg(k), kq = 4 * kg;
    const int nstrip = (n + AP_RS - 1) / AP_RS, nrc = (n + AP_RC - 1) / AP_RC;
    const size_t lds_tile = (size_t)(AP_RS + kq) * AP_LD * sizeof(double);
    hipLaunchKernelGGL(append_vt_kernel<T>, dim3(nstrip), dim3(256), lds_tile, st, Minv, ldm, n, Kt, ldkt, k, kg, u, vt, (long)n_pad,
                       scratch, E);
    PG_CHECK(hipGetLastError());
    const int seg = std::min(AP_SEG, nstrip), per = (nstrip + seg - 1) / seg;
    const unsigned eb = (unsigned)((E + 255) / 256);
    hipLaunchKernelGGL(append_sum_kernel, dim3(eb, seg), dim3(256), 0, st, scratch, E, nstrip, per, part2);
    hipLaunchKernelGGL(append_sum_kernel, dim3(eb, 1), dim3(256), 0, st, part2, E, seg, seg, red);
    PG_CHECK(hipGetLastError());
    const size_t lds_schur = ((size_t)k * (k + 1) + 2 * k) * sizeof(double);
    static bool attr_set[2] = {false, false};
    if (!attr_set[sizeof(T) == 8]) {
        PG_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(append_schur_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)(((size_t)PG_APPEND_KMAX * (PG_APPEND_KMAX + 1) + 2 * PG_APPEND_KMAX) * sizeof(double))));
        attr_set[sizeof(T) == 8] = true;
    }
    hipLaunchKernelGGL(append_schur_kernel<T>, dim3(1), dim3(256), lds_schur, st, red, k, n, Knn, ldknn, yn, ls, lsi, ut, info);
    PG_CHECK(hipGetLastError());
    hipLaunchKernelGGL(append_rows_kernel<T>, dim3(nstrip, nrc), dim3(256), lds_tile, st, Minv, ldm, n, vt, (long)n_pad, k, kg, scratch,
                       (long)n_pad, info);
    hipLaunchKernelGGL(append_rows_epi_kernel, dim3(nstrip), dim3(256), (size_t)k * AP_LD * sizeof(double), st, scratch, (long)n_pad, nrc,
                       n, k, lsi, w, (long)n_pad, info);
    hipLaunchKernelGGL(append_commit_kernel<T>, dim3(n_pad / 256, k), dim3(256), 0, st, n, k, vt, w, (long)n_pad, ls, lsi, ut, L, ldl, Minv,
                       ldm, invd, u, info);
    PG_CHECK(hipGetLastError());
    hipLaunchKernelGGL(append_alpha_partial_kernel<T>, dim3(n_pad / 256, n_pad / 256), dim3(256), 0, st, Minv, ldm, n + k, u, scratch,
                       (long)n_pad, info);
    hipLaunchKernelGGL(append_alpha_reduce_kernel<T>, dim3(n_pad / 256), dim3(256), 0, st, scratch, (long)n_pad, n_pad / 256, alpha, info);
    PG_CHECK(hipGetLastError());
    return 0;
}

template int pg_chol_append_t<double>(pg_ctx*, hipStream_t, int, int, int, double*, long, double*, double*, long, const double*, long,
                                      const double*, long, const double*, double*, double*, void*, int*);
template int pg_chol_append_t<float>(pg_ctx*, hipStream_t, int, int, int, float*, long, float*, float*, long, const float*, long,
                                     const float*, long, const float*, float*, float*, void*, int*);
