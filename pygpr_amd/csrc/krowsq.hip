// The squared row norms of a cross-covariance (include/pygpr_hip_rowsq.h):
//   OUT[i] = sum_j k(xr_i, xc_j)^2
// without K ever being written.  kmatmul.hip's walk with the matrix instructions taken out: where that kernel hands the four values
// kv[r] = k(xr[i0 + c16], xc[j0 + g + 4 r]) of a lane (g = lane >> 4, c16 = lane & 15) to v_mfma_f64_16x16x4_f64 against a panel of V,
// this one adds kv[r]^2 to the lane's own accumulator.  The sixteen lanes of one g share their column points, the four g of one c16 their
// row point: at the end of the walk the four partial sums of a row are added in the order g = 0, 1, 2, 3.
//   workgroup   256 threads own 64 rows of OUT and one segment of the column range; wave w owns rows 16 w .. 16 w + 15
//   row point   a lane evaluates every one of its pairs against the SAME row point i0 + c16: its coordinates live in registers
//   column tile 64 points k-major in LDS ([k][64]: the 16 lanes of one g read one word as a broadcast), double-buffered; the next tile
//               travels global -> registers while this one is computed
//   pair        kfun.h's forms from direct differences, four pairs interleaved exactly as kmatmul.hip interleaves them (that loop is
//               repeated here, not shared: kmatmul.hip is left as it is)
// Bound by fp64 VALU issue on the pair evaluation, like its parent: one multiply-add per pair replaces the
// product's share of a matrix instruction, against some fifty fp64 operations of the evaluation.
#include "kfun.h"
#include "kpair.h"
#include "kbuild.h"
#include "kmatmul.h"
#include "krowsq.h"
#include <type_traits>

// LDS of pg_krowsq_kernel in bytes: two point tiles, l2 (and ipl), cpar -- the carve-up below
template <int DMAX, bool PER> static constexpr size_t krowsq_lds_bytes() {
    return (size_t)(2 * MM_T * DMAX + (PER ? 2 : 1) * PG_MAX_COMP * DMAX + 4 * PG_MAX_COMP) * sizeof(double);
}
// partial sums: part[seg][tiles_r * 64]
template <int DMAX, bool PER, bool PROD>
__global__ __launch_bounds__(256) void pg_krowsq_kernel(pg_covspec spec, const double* __restrict__ hp, const double* __restrict__ Xr, long ldr,
                                                        int nr, const double* __restrict__ Xc, long ldc, int nc, int d,
                                                        double* __restrict__ OUT, long ldo, double* __restrict__ part, int tps, int tiles_c) {
    static_assert(!PROD || PER, "a product takes the instantiation that carries every kind");
    static_assert((MM_T * DMAX) % 256 == 0, "every thread stages the same number of coordinates");
    constexpr int NXP = (MM_T * DMAX) / 256;             // coordinates a thread stages per tile
    const int tr = blockIdx.x, seg = blockIdx.y;
    const int t0 = seg * tps, t1 = min(t0 + tps, tiles_c);
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c16 = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* xc = reinterpret_cast<double*>(smem_raw);          // two buffers [DMAX][64] of column points, zero for k >= d and points >= nc
    double* l2 = xc + 2 * MM_T * DMAX;                          // [ncomp][DMAX] squared inverse length scales, zero for k >= d
    double* ipl = l2 + PG_MAX_COMP * DMAX;                      // PER: [ncomp][DMAX] reciprocal periods, zero for k >= d / other kinds
    double* cpar = ipl + (PER ? PG_MAX_COMP * DMAX : 0);        // [ncomp][4]: sigma^2, the squared shape, its reciprocal
    pair_stage_hp<double, PER>(spec, hp, d, DMAX, DMAX, l2, ipl, tid, 256);
    if (tid < spec.ncomp) {
        const double sg = hp[spec.off[tid]], sh = kind_shape2(spec, hp, tid, d);
        cpar[4 * tid] = sg * sg;
        cpar[4 * tid + 1] = sh;
        cpar[4 * tid + 2] = 1.0 / sh;
    }
    // this lane's row point, in registers for the whole walk (zero for k >= d and rows >= nr)
    const int i0 = 16 * wave;
    const int gi_pt = tr * MM_T + i0 + c16;
    double xi[DMAX];
#pragma unroll
    for (int k = 0; k < DMAX; ++k) xi[k] = (k < d && gi_pt < nr) ? Xr[(long)gi_pt * ldr + k] : 0.0;

    // global -> registers at clamped addresses (every address is an element of the operand: gaps are not read), registers -> LDS
    double xpf[NXP];
    auto fetch = [&](int tc) {
#pragma unroll
        for (int u = 0; u < NXP; ++u) {
            const int idx = tid + 256 * u, p = idx / DMAX, k = idx % DMAX;
            const int gc = tc * MM_T + p;
            const double v = Xc[(long)min(gc, nc - 1) * ldc + min(k, d - 1)];
            xpf[u] = (k < d && gc < nc) ? v : 0.0;
        }
    };
    auto stash = [&](int buf) {
        double* xb = xc + buf * MM_T * DMAX;
#pragma unroll
        for (int u = 0; u < NXP; ++u) {
            const int idx = tid + 256 * u, p = idx / DMAX, k = idx % DMAX;
            xb[k * MM_T + p] = xpf[u];
        }
    };

    double acc = 0.0;
    fetch(t0);      // (a launch has t0 < t1 <= tiles_c and nc >= 1: the plan gives no segment to an empty column range)
    for (int tc = t0, it = 0; tc < t1; ++tc, ++it) {
        const int buf = it & 1;
        stash(buf);
        __syncthreads();   // also orders this buffer's previous readers (two tiles ago) before the writes above, and the parameters' first readers
        if (tc + 1 < t1) fetch(tc + 1);
        const double* xb = xc + buf * MM_T * DMAX;
        const int jlim = nc - tc * MM_T;      // column points of this tile that exist
#pragma unroll 1
        for (int jb = 0; jb < 4; ++jb) {
            const int j0 = 16 * jb + g;       // this lane's column points: j0 + 4 r
            double kv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) kv[r] = PROD ? 1.0 : 0.0;
            for (int c = 0; c < spec.ncomp; ++c) {
                const double* lc = l2 + c * DMAX;
                const int kind = spec.kind[c];
                const double sig2 = cpar[4 * c];
                double sq[4] = {0.0, 0.0, 0.0, 0.0};
                double val[4];
                bool done = false;
                if constexpr (PER) {
                    if (kind == PG_KIND_PERIODIC) {      // (padding coordinates: l^2 = 1 / p = 0, so the term vanishes)
                        const double* ipc = ipl + c * DMAX;
#pragma unroll
                        for (int k = 0; k < DMAX; ++k)
#pragma unroll
                            for (int r = 0; r < 4; ++r) sq[r] += lc[k] * per_sin2<double>((xi[k] - xb[k * MM_T + j0 + 4 * r]) * ipc[k]);
#pragma unroll
                        for (int r = 0; r < 4; ++r) val[r] = kind_value<double, PG_KIND_RBF>(sig2, sq[r]);
                        done = true;
                    }
                }
                if (!done) {
#pragma unroll
                    for (int k = 0; k < DMAX; ++k)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const double df = xi[k] - xb[k * MM_T + j0 + 4 * r];
                            sq[r] += lc[k] * df * df;
                        }
                    if (kind == PG_KIND_RBF) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) val[r] = kind_value<double, PG_KIND_RBF>(sig2, sq[r]);
                    } else {
                        const double sha = cpar[4 * c + 1], ish = cpar[4 * c + 2];
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            double bt, ft;
                            matern_val<double>(kind, sig2, sq[r], val[r], bt, sha, ish, ft);
                        }
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) kv[r] = PROD ? kv[r] * val[r] : kv[r] + val[r];
            }
            // (a column point past the end was staged as the origin: its value is finite or not as the row point decides -- the select
            // keeps it out of the sum, so that a row's entry is non-finite only through pairs that exist)
#pragma unroll
            for (int r = 0; r < 4; ++r) kv[r] = (j0 + 4 * r < jlim) ? kv[r] : 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) acc = fma(kv[r], kv[r], acc);
        }
    }

    // the four g of a row, in their order: lane c16 + 16 g' of this wave holds the partial sum of g'
    double s = __shfl(acc, c16, 64);
#pragma unroll
    for (int gg = 1; gg < 4; ++gg) s += __shfl(acc, c16 + 16 * gg, 64);
    if (g != 0) return;
    const int gi = tr * MM_T + i0 + c16;
    if (part) {
        part[(long)seg * gridDim.x * MM_T + gi] = s;      // (rows behind nr included: the buffer holds tiles_r * 64 of them a segment)
        return;
    }
    if (gi < nr) OUT[(long)gi * ldo] = s;
}

// OUT[i] = sum_{seg < nseg} part[seg][i], the segments in their order; nseg = 0: the empty sum
__global__ __launch_bounds__(256) void pg_krowsq_fold_kernel(const double* __restrict__ part, int nseg, long rows_pad, int nr,
                                                             double* __restrict__ OUT, long ldo) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nr) return;
    double s = 0.0;
    for (int sg = 0; sg < nseg; ++sg) s += part[(long)sg * rows_pad + i];
    OUT[i * ldo] = s;
}

long pg_krowsq_worksize_impl(int nr, int nc) {
    const MmPlan p = mm_plan(nr, nc, 1);
    return p.nseg > 1 ? (long)p.nseg * p.tiles_r * MM_T : 0;
}

template <int DMAX, bool PER, bool PROD>
static int launch_krowsq(hipStream_t st, const MmPlan& p, const pg_covspec& spec, const double* hp, const double* Xr, long ldr, int nr,
                         const double* Xc, long ldc, int nc, int d, double* OUT, long ldo, double* part) {
    constexpr size_t lds = krowsq_lds_bytes<DMAX, PER>();
    if (int rc = pg_lds_opt_in<pg_krowsq_kernel<DMAX, PER, PROD>>(lds)) return rc;   // d > 32 needs more than the 64 KB a kernel gets without opting in
    hipLaunchKernelGGL((pg_krowsq_kernel<DMAX, PER, PROD>), dim3(p.tiles_r, p.nseg, 1), dim3(256), lds, st, spec, hp, Xr, ldr, nr, Xc, ldc, nc,
                       d, OUT, ldo, part, p.tps, p.tiles_c);
    PG_CHECK(hipGetLastError());
    return 0;
}

int pg_krowsq_impl(hipStream_t st, const pg_covspec& spec_in, const double* hp, const double* Xr, long ldr, int nr, const double* Xc, long ldc,
                   int nc, int d, double* OUT, long ldo, double* work) {
    if (nr == 0) return 0;
    pg_covspec spec;
    const bool prod = pg_spec_strip(spec_in, spec);
    const MmPlan p = mm_plan(nr, nc, 1);
    double* part = p.nseg > 1 ? work : nullptr;
    if (p.nseg > 0) {
        const int rc = pg_with_kinds(spec, prod, [&](auto per_c, auto prod_c) {
            return pg_with_dmax(d, [&](auto dmax_c) {
                return launch_krowsq<decltype(dmax_c)::value, decltype(per_c)::value, decltype(prod_c)::value>(st, p, spec, hp, Xr, ldr, nr, Xc,
                                                                                                                 ldc, nc, d, OUT, ldo, part);
            });
        });
        if (rc) return rc;
    }
    if (p.nseg != 1) {      // the segments in their order, or the empty sum
        hipLaunchKernelGGL(pg_krowsq_fold_kernel, dim3((unsigned)((nr + 255) / 256)), dim3(256), 0, st, part, p.nseg, (long)p.tiles_r * MM_T, nr,
                           OUT, ldo);
        PG_CHECK(hipGetLastError());
    }
    return 0;
}
