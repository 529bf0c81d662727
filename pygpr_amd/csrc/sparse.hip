// The rectangular hyper-parameter contraction of the inducing-point GP (include/pygpr_hip_sparse.h):
//   grad[p] (+)= sum_{i < m, j < n} W_ij dk(z_i, x_j)/dtheta_p
// for every parameter of the spec's stationary components.  pg_grad_kernel (kbuild.hip) on two point sets: the weight is a matrix the
// caller hands over instead of K^-1 - alpha alpha^T on the lower triangle, so there is no diagonal, no doubling and no noise trace, and
// the grid is the full rectangle of 64 x 64 tiles.  The per-pair forms are kfun.h's, from direct differences; staging and the reduce's
// scales are kpair.h's (without the 1/2 of the NLML).  The per-pair body and the fold into a child's slots are written out here as in
// pg_grad_kernel (kbuild.hip) and pg_lowrank_grad_kernel (lowrank.hip): the same text three times, to be changed together -- as one
// shared function it is compiled to other registers.
// HBM-bound on W: one 8-byte weight per pair is read once, one wave reads one 64-wide row of a tile per step (512 contiguous bytes in
// fp64, 256 in fp32), both point tiles sit in LDS k-major ([k][64]: the 64 lanes of a wave read 64 consecutive words, every wave reads
// the row point as a broadcast).  No matrix-pipe body.
#include "kfun.h"
#include "kpair.h"
#include "kbuild.h"
#include "sparse.h"
#include <type_traits>

#define ST_T 64      // tile edge
#define ST_CH 4      // column tiles one workgroup walks with its accumulators in registers (pg_grad_kernel's strip)

// LDS of pg_cross_grad_kernel in bytes: red, the row tile and two column tiles, l2 (and ipl) -- the carve-up below
template <typename T, int DMAX, bool PER> static constexpr size_t cross_grad_lds_bytes() {
    return 4 * kind_nparam(PER ? PG_KIND_PERIODIC : PG_KIND_RQ, DMAX) * sizeof(double) + (size_t)(3 * ST_T * DMAX + (PER ? 2 : 1) * PG_MAX_COMP * DMAX) * sizeof(T);
}
template <typename T, int DMAX, bool PER, bool PROD>
__global__ __launch_bounds__(256) void pg_cross_grad_kernel(pg_covspec spec, const double* __restrict__ hp, const T* __restrict__ Z, long ldz,
                                                            int m, const T* __restrict__ X, long ldx, int n, int d,
                                                            const T* __restrict__ W, long ldw, double* __restrict__ part, int pw, int tiles_n) {
    static_assert(!PROD || PER, "a product takes the instantiation that carries every kind");
    const int tr = blockIdx.y;
    const int c0 = blockIdx.x * ST_CH, c1 = min(c0 + ST_CH, tiles_n);      // column tiles [c0, c1): never empty (the grid is ceil(tiles_n / ST_CH) wide)
    const long blk = (long)tr * gridDim.x + blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int RS = kind_nparam(PER ? PG_KIND_PERIODIC : PG_KIND_RQ, DMAX);      // slots of the widest block this kernel folds
    double* red = reinterpret_cast<double*>(smem_raw);             // [4 waves][RS]: sigma, l_1..l_DMAX, the shape | the periods
    T* xr = reinterpret_cast<T*>(red + 4 * RS);                     // the row points' tile [DMAX][64], zero for k >= d and rows >= m
    T* xc = xr + ST_T * DMAX;                                       // two buffers [DMAX][64] of column points
    T* l2 = xc + 2 * ST_T * DMAX;                                   // [ncomp][DMAX] squared inverse length scales, zero for k >= d
    T* ipl = l2 + PG_MAX_COMP * DMAX;                               // PER: [ncomp][DMAX] reciprocal periods, zero for k >= d / other kinds
    for (int idx = tid; idx < ST_T * DMAX; idx += 256) {
        const int p = idx / DMAX, k = idx % DMAX;
        const int gr = tr * ST_T + p;
        xr[k * ST_T + p] = (k < d && gr < m) ? Z[(long)gr * ldz + k] : (T)0;
    }
    pair_stage_hp<T, PER>(spec, hp, d, DMAX, DMAX, l2, ipl, tid, 256);
    // PROD: component c's value at (row, this lane's column) of the point tile xb.  kpair.h's pair_value written out: taking it moved the
    // d > 16 product instantiations of this kernel to more scratch memory
    auto elem_value = [&](int c, int row, const T* xb) -> T {
        const T* lc = l2 + c * DMAX;
        const int kind = spec.kind[c];
        const double sg = hp[spec.off[c]];
        const T sig2 = (T)(sg * sg);
        T sq = (T)0;
        if (kind == PG_KIND_PERIODIC) {
            const T* ipc = ipl + c * DMAX;
#pragma unroll
            for (int k = 0; k < DMAX; ++k) sq += lc[k] * per_sin2<T>((xr[k * ST_T + row] - xb[k * ST_T + lane]) * ipc[k]);
            return kind_value<T, PG_KIND_RBF>(sig2, sq);
        }
#pragma unroll
        for (int k = 0; k < DMAX; ++k) {
            const T df = xr[k * ST_T + row] - xb[k * ST_T + lane];
            sq += lc[k] * df * df;
        }
        if (kind == PG_KIND_RBF) return kind_value<T, PG_KIND_RBF>(sig2, sq);
        const double sh = kind_shape2(spec, hp, c, d);
        T kt, bt, ft;
        matern_val<T>(kind, sig2, sq, kt, bt, (T)sh, (T)(1.0 / sh), ft);
        return kt;
    };

    // element e of this thread: row = 4 e + wave (one wave reads one 64-wide row of W), column = lane; 0 in the padding
    int it = 0;   // running tile counter: selects the point-tile buffer
    for (int cp = 0; cp < spec.ncomp; ++cp) {
        const int o = spec.off[cp];
        const double sg = hp[o];
        const T sig2 = (T)(sg * sg);
        const T* lc = l2 + cp * DMAX;
        const int kind = spec.kind[cp];
        const double sh = kind_shape2(spec, hp, cp, d);
        const T sha = (T)sh, ish = (T)(1.0 / sh);      // rational quadratic: alpha^2, 1 / alpha^2
        double accf = 0.0;                            // ... and its shape entry, sum W K fs
        double acc[DMAX + 1];                         // sigma: sum W K;  l_k: sum W base D_k^2 (the periodic kind: sum W K sin^2)
#pragma unroll
        for (int k = 0; k <= DMAX; ++k) acc[k] = 0.0;
        double accp[PER ? DMAX : 1];                  // the periodic kind's period entries, sum W K sin(2 pi t_k) t_k
#pragma unroll
        for (int k = 0; k < (PER ? DMAX : 1); ++k) accp[k] = 0.0;
        for (int tc = c0; tc < c1; ++tc, ++it) {
            T* xb = xc + (it & 1) * ST_T * DMAX;
            for (int idx = tid; idx < ST_T * DMAX; idx += 256) {
                const int p = idx / DMAX, k = idx % DMAX;
                const int gc = tc * ST_T + p;
                xb[k * ST_T + p] = (k < d && gc < n) ? X[(long)gc * ldx + k] : (T)0;
            }
            __syncthreads();   // also orders this buffer's previous readers (two tiles ago) before the writes above
            const int gj = tc * ST_T + lane;
#pragma unroll 2
            for (int e = 0; e < 16; ++e) {
                const int row = 4 * e + wave;
                const int gi = tr * ST_T + row;
                double w = (gi < m && gj < n) ? (double)W[(long)gi * ldw + gj] : 0.0;
                if constexpr (PROD) {      // the product rule: the others' values weigh this component's element
                    for (int c2 = 0; c2 < spec.ncomp; ++c2)
                        if (c2 != cp) w *= (double)elem_value(c2, row, xb);
                }
                if constexpr (PER) {
                    if (kind == PG_KIND_PERIODIC) {      // (padding coordinates: l^2 = 1 / p = 0, so t = 0 and both terms vanish)
                        const T* ipc = ipl + cp * DMAX;
                        T sp = (T)0;
#pragma unroll
                        for (int k = 0; k < DMAX; ++k) sp += lc[k] * per_sin2<T>((xr[k * ST_T + row] - xb[k * ST_T + lane]) * ipc[k]);
                        const double wk = w * (double)kind_value<T, PG_KIND_RBF>(sig2, sp);
                        acc[0] += wk;
#pragma unroll
                        for (int k = 0; k < DMAX; ++k) {
                            const T t = (xr[k * ST_T + row] - xb[k * ST_T + lane]) * ipc[k];
                            T s2, s2w;
                            per_terms<T>(t, s2, s2w);
                            acc[1 + k] += wk * (double)s2;
                            accp[k] += wk * (double)s2w * (double)t;
                        }
                        continue;
                    }
                }
                T sq = (T)0;
#pragma unroll
                for (int k = 0; k < DMAX; ++k) {
                    const T df = xr[k * ST_T + row] - xb[k * ST_T + lane];
                    sq += lc[k] * df * df;
                }
                double kv, base;   // dK/dl_k = base * l_k * D_k^2 (sign and constants applied in the reduce)
                if (kind == PG_KIND_RBF) {
                    kv = (double)kind_value<T, PG_KIND_RBF>(sig2, sq);
                    base = kv;
                } else {
                    T kt, bt, ft;
                    matern_val<T>(kind, sig2, sq, kt, bt, sha, ish, ft);
                    kv = (double)kt;
                    base = (double)bt;
                    accf += w * (double)ft;
                }
                acc[0] += w * kv;
                const double wb = w * base;
#pragma unroll
                for (int k = 0; k < DMAX; ++k) {
                    const double df = (double)(xr[k * ST_T + row] - xb[k * ST_T + lane]);
                    acc[1 + k] += wb * df * df;
                }
            }
        }
#pragma unroll
        for (int k = 0; k <= DMAX; ++k) {
            const double s = wave_sum(acc[k]);
            if (lane == 0) red[wave * RS + k] = s;
        }
        if (kind == PG_KIND_RQ) {
            const double s = wave_sum(accf);
            if (lane == 0) red[wave * RS + DMAX + 1] = s;
        }
        if constexpr (PER) {
            if (kind == PG_KIND_PERIODIC) {
#pragma unroll
                for (int k = 0; k < DMAX; ++k) {
                    const double s = wave_sum(accp[k]);
                    if (lane == 0) red[wave * RS + DMAX + 1 + k] = s;
                }
            }
        }
        __syncthreads();
        if (tid < kind_nparam(kind, d)) {      // the child's block: sigma, l_1..l_d (slots 0..d), what sits behind them (slots DMAX + 1 ..)
            const int q = tid <= d ? tid : DMAX + 1 + (tid - d - 1);
            part[blk * pw + o + tid] = red[q] + red[RS + q] + red[2 * RS + q] + red[3 * RS + q];      // (o + the block's width <= pw: the host's extent)
        }
        __syncthreads();
    }
}

// grad[p] = (accumulate ? grad[p] : 0) + scale_p * sum_blocks part[b][p] for the entries of the spec's stationary blocks; every other p
// (noise entries, children of another pass) leaves before anything is read: their columns of `part` were never written.
__global__ __launch_bounds__(256) void pg_cross_grad_reduce_kernel(pg_covspec spec, const double* __restrict__ hp, const double* __restrict__ part,
                                                                   long nblk, int pw, int d, double* __restrict__ grad, int accumulate) {
    __shared__ double red[4];
    const int p = blockIdx.x, tid = threadIdx.x;
    double scale = 0.0;
    bool mine = false;
    for (int c = 0; c < spec.ncomp; ++c) {
        bool hit = false;
        const double sc = kind_entry_scale(spec, hp, c, p, d, hit);
        if (hit) { scale = sc; mine = true; }
    }
    if (!mine) return;
    double s = 0.0;
    for (long b = tid; b < nblk; b += 256) s += part[b * pw + p];
    s = wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        s = red[0] + red[1] + red[2] + red[3];
        grad[p] = (accumulate ? grad[p] : 0.0) + scale * s;
    }
}

int pg_cross_grad_reduce(hipStream_t st, const pg_covspec& spec, const double* hp, const double* part, long nblk, int pw, int d, double* grad,
                         int accumulate) {
    hipLaunchKernelGGL(pg_cross_grad_reduce_kernel, dim3(pw), dim3(256), 0, st, spec, hp, part, nblk, pw, d, grad, accumulate);
    PG_CHECK(hipGetLastError());
    return 0;
}

static inline long cg_strips(int n) { return ((long)(n + ST_T - 1) / ST_T + ST_CH - 1) / ST_CH; }

long pg_cross_grad_worksize_impl(int m, int n, int nhp) {
    return (long)((m + ST_T - 1) / ST_T) * cg_strips(n) * nhp;
}

int pg_cross_grad_extent(const pg_covspec& spec_in, int d) {
    pg_covspec spec;
    pg_spec_strip(spec_in, spec);
    int ext = 0;
    for (int c = 0; c < spec.ncomp; ++c) ext = std::max(ext, spec.off[c] + kind_nparam(spec.kind[c], d));
    return ext;
}

template <typename T, int DMAX, bool PER, bool PROD>
static int launch_cross_grad(hipStream_t st, const pg_covspec& spec, const double* hp, const T* Z, long ldz, int m, const T* X, long ldx, int n,
                             int d, const T* W, long ldw, double* part, int pw, int tiles_m, int tiles_n) {
    constexpr size_t lds = cross_grad_lds_bytes<T, DMAX, PER>();
    if (int rc = pg_lds_opt_in<pg_cross_grad_kernel<T, DMAX, PER, PROD>>(lds)) return rc;   // d > 32 needs more than the 64 KB a kernel gets without opting in
    hipLaunchKernelGGL((pg_cross_grad_kernel<T, DMAX, PER, PROD>), dim3((tiles_n + ST_CH - 1) / ST_CH, tiles_m), dim3(256), lds, st, spec, hp, Z,
                       ldz, m, X, ldx, n, d, W, ldw, part, pw, tiles_n);
    PG_CHECK(hipGetLastError());
    return 0;
}

template <typename T>
int pg_cross_grad_t(hipStream_t st, const pg_covspec& spec_in, const double* hp, const T* Z, long ldz, int m, const T* X, long ldx, int n, int d,
                    const T* W, long ldw, double* grad, int accumulate, double* work) {
    pg_covspec spec;
    const bool prod = pg_spec_strip(spec_in, spec);
    const int pw = pg_cross_grad_extent(spec, d);
    if (pw == 0) return 0;                            // no stationary component: no entry is this call's
    const int tiles_m = (m + ST_T - 1) / ST_T, tiles_n = (n + ST_T - 1) / ST_T;
    const long nblk = (long)tiles_m * cg_strips(n);
    if (nblk > 0) {
        const int rc = pg_with_kinds(spec, prod, [&](auto per_c, auto prod_c) {
            return pg_with_dmax(d, [&](auto dmax_c) {
                return launch_cross_grad<T, decltype(dmax_c)::value, decltype(per_c)::value, decltype(prod_c)::value>(
                    st, spec, hp, Z, ldz, m, X, ldx, n, d, W, ldw, work, pw, tiles_m, tiles_n);
            });
        });
        if (rc) return rc;
    }
    // (m == 0 or n == 0: an empty sum -- the reduce alone zeroes the spec's entries, or leaves them when accumulating)
    return pg_cross_grad_reduce(st, spec, hp, work, nblk, pw, d, grad, accumulate);
}

template int pg_cross_grad_t<double>(hipStream_t, const pg_covspec&, const double*, const double*, long, int, const double*, long, int, int,
                                     const double*, long, double*, int, double*);
template int pg_cross_grad_t<float>(hipStream_t, const pg_covspec&, const double*, const float*, long, int, const float*, long, int, int,
                                    const float*, long, double*, int, double*);
