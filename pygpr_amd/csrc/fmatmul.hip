// The matrix-free random-feature product (include/pygpr_hip_feature.h):
//   OUT[i][c] = sum_f cos(2 pi (x_i . nu_f + u_f)) W[f][c]
// without Phi ever being written.  kmatmul.hip's kernel with another pair function, the feature in the place of the column point: a
// 16 x 16 block of Phi^T -- block row = feature, block column = row point -- is evaluated in the accumulator layout of
// v_mfma_f64_16x16x4_f64, so register r of a lane (g = lane >> 4, c16 = lane & 15) holds Phi[i0 + c16][f0 + g + 4 r], which read as an
// A operand is A[i = c16][k = g]: the four features f0 + 4 r .. f0 + 4 r + 3 of one k-step.  The B operand of that step is
// W[f0 + g + 4 r][c16] from LDS, the result OUT[i0 + g + 4 r][c16].
//   workgroup    256 threads own 64 rows of OUT, one block of up to 32 right-hand sides and one segment of the feature range; wave w
//                owns rows 16 w .. 16 w + 15, its accumulators (4 or 8 doubles a lane) stay in registers for the whole walk
//   row point    a lane evaluates every one of its pairs against the SAME row point i0 + c16: its coordinates live in registers
//   feature tile 64 features k-major in LDS ([DMAX + 1][64]: d frequencies and, as the last row, the phase; the 16 lanes of one g read
//                one word as a broadcast) and the 64 x 16 panels of W beside them, double-buffered with one barrier per tile; the
//                next tile travels global -> registers while this one is computed
//   pair         t = u + sum_k x_k nu_k in cycles, then kfun.h's pg_sincospi, which reduces r = t - rint(t) and gives sin(pi r) on
//                [-1/2, 1/2]; cos(2 pi t) = 1 - 2 sin^2(pi r).  No product with pi is rounded, an argument of any size costs the same
// The plan (segments, blocks of 32 columns) and the fold of the segments are kmatmul.hip's (kmatmul.h).
#include "kfun.h"
#include "kmatmul.h"
#include "fmatmul.h"
#include <type_traits>

// LDS of pg_fmatmul_kernel in bytes: two feature tiles with their phase row, two panels of W -- the carve-up below
template <int DMAX, int NB> static constexpr size_t fmatmul_lds_bytes() {
    return (size_t)(2 * MM_T * (DMAX + 1) + 2 * NB * MM_T * MM_PANEL) * sizeof(double);
}
// partial tiles: part[seg][blk][tiles_r * 64][MM_BLOCK]
template <int DMAX, int NB>
__global__ __launch_bounds__(256) void pg_fmatmul_kernel(const double* __restrict__ X, long ldx, int nr, const double* __restrict__ NU, long ldn,
                                                         int nf, int d, const double* __restrict__ U, const double* __restrict__ W, long ldw,
                                                         int nrhs, double* __restrict__ OUT, long ldo, double* __restrict__ part, int tps,
                                                         int tiles_f) {
    constexpr int NXP = (MM_T * DMAX) / 256;             // frequencies a thread stages per tile
    constexpr int NVP = (MM_T * MM_PANEL * NB) / 256;    // ... and entries of W
    constexpr int VW = MM_PANEL * NB;                    // columns of W this instantiation stages
    constexpr int FT = MM_T * (DMAX + 1);                // doubles of one feature tile
    const int tr = blockIdx.x, seg = blockIdx.y, blk = blockIdx.z;
    const int cb = blk * MM_BLOCK;
    const int t0 = seg * tps, t1 = min(t0 + tps, tiles_f);
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c16 = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* ft = reinterpret_cast<double*>(smem_raw);          // two buffers [DMAX + 1][64]: frequencies (zero for k >= d), then the phase;
                                                               // zero for features >= nf
    double* wt = ft + 2 * FT;                                   // two buffers [NB][64][16] of W, zero for features >= nf and columns >= nrhs
    // this lane's row point, in registers for the whole walk (zero for k >= d and rows >= nr)
    const int i0 = 16 * wave;
    const int gi_pt = tr * MM_T + i0 + c16;
    double xi[DMAX];
#pragma unroll
    for (int k = 0; k < DMAX; ++k) xi[k] = (k < d && gi_pt < nr) ? X[(long)gi_pt * ldx + k] : 0.0;

    // global -> registers at clamped addresses (every address is an element of the operand: gaps are not read), registers -> LDS
    double xpf[NXP], vpf[NVP], upf = 0.0;
    auto fetch = [&](int tf) {
#pragma unroll
        for (int u = 0; u < NXP; ++u) {
            const int idx = tid + 256 * u, p = idx / DMAX, k = idx % DMAX;
            const int gf = tf * MM_T + p;
            const double v = NU[(long)min(gf, nf - 1) * ldn + min(k, d - 1)];
            xpf[u] = (k < d && gf < nf) ? v : 0.0;
        }
        if (tid < MM_T) {
            const int gf = tf * MM_T + tid;
            const double v = U[min(gf, nf - 1)];
            upf = gf < nf ? v : 0.0;
        }
#pragma unroll
        for (int u = 0; u < NVP; ++u) {
            const int idx = tid + 256 * u, j = idx / VW, c = idx % VW;
            const int gf = tf * MM_T + j, gcol = cb + c;
            const double v = W[(long)min(gf, nf - 1) * ldw + min(gcol, nrhs - 1)];
            vpf[u] = (gf < nf && gcol < nrhs) ? v : 0.0;
        }
    };
    auto stash = [&](int buf) {
        double* fb = ft + buf * FT;
        double* wb = wt + buf * NB * MM_T * MM_PANEL;
#pragma unroll
        for (int u = 0; u < NXP; ++u) {
            const int idx = tid + 256 * u, p = idx / DMAX, k = idx % DMAX;
            fb[k * MM_T + p] = xpf[u];
        }
        if (tid < MM_T) fb[DMAX * MM_T + tid] = upf;
#pragma unroll
        for (int u = 0; u < NVP; ++u) {
            const int idx = tid + 256 * u, j = idx / VW, c = idx % VW;
            wb[(c / MM_PANEL) * MM_T * MM_PANEL + j * MM_PANEL + (c % MM_PANEL)] = vpf[u];
        }
    };

    pg_d4 acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[b][r] = 0.0;

    fetch(t0);
    for (int tf = t0, it = 0; tf < t1; ++tf, ++it) {
        const int buf = it & 1;
        stash(buf);
        __syncthreads();   // also orders this buffer's previous readers (two tiles ago) before the writes above
        if (tf + 1 < t1) fetch(tf + 1);
        const double* fb = ft + buf * FT;
        const double* wb = wt + buf * NB * MM_T * MM_PANEL;
#pragma unroll 1
        for (int jb = 0; jb < 4; ++jb) {
            const int j0 = 16 * jb + g;       // this lane's features: j0 + 4 r
            double t[4], pv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) t[r] = fb[DMAX * MM_T + j0 + 4 * r];
#pragma unroll
            for (int k = 0; k < DMAX; ++k)
#pragma unroll
                for (int r = 0; r < 4; ++r) t[r] = __builtin_fma(xi[k], fb[k * MM_T + j0 + 4 * r], t[r]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {      // cos(2 pi t) = 1 - 2 sin^2(pi r), r = t - rint(t): the half angle stays inside pg_sincospi's range
                double sn, cs;
                pg_sincospi(t[r], &sn, &cs);
                pv[r] = __builtin_fma(-2.0 * sn, sn, 1.0);
            }
            // (a feature past the end was staged as zero frequency and phase, and W is 0 there: its value is 1, or a NaN where the row
            // point has one -- and that row of OUT is NaN already)
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int b = 0; b < NB; ++b)
                    acc[b] = Mfma<double>::run(pv[r], wb[b * MM_T * MM_PANEL + (j0 + 4 * r) * MM_PANEL + c16], acc[b]);
        }
    }

    // register r of panel b: OUT[tr 64 + i0 + g + 4 r][cb + 16 b + c16]
    if (part) {
        const long rows_pad = (long)gridDim.x * MM_T;
        double* pp = part + (((long)seg * gridDim.z + blk) * rows_pad + tr * MM_T + i0) * MM_BLOCK;
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) pp[(long)(g + 4 * r) * MM_BLOCK + MM_PANEL * b + c16] = acc[b][r];
        return;
    }
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int gi = tr * MM_T + i0 + g + 4 * r, gcol = cb + MM_PANEL * b + c16;
            if (gi < nr && gcol < nrhs) OUT[(long)gi * ldo + gcol] = acc[b][r];
        }
}

long pg_fmatmul_worksize_impl(int nr, int nf, int nrhs) { return pg_kmatmul_worksize_impl(nr, nf, nrhs); }

template <int DMAX, int NB>
static int launch_fmatmul(hipStream_t st, const MmPlan& p, const double* X, long ldx, int nr, const double* NU, long ldn, int nf, int d,
                          const double* U, const double* W, long ldw, int nrhs, double* OUT, long ldo, double* part) {
    constexpr size_t lds = fmatmul_lds_bytes<DMAX, NB>();
    // DMAX = 32 with two panels and DMAX = 64 need more than the 64 KB a kernel gets without opting in
    if (int rc = pg_lds_opt_in<pg_fmatmul_kernel<DMAX, NB>>(lds)) return rc;
    hipLaunchKernelGGL((pg_fmatmul_kernel<DMAX, NB>), dim3(p.tiles_r, p.nseg, p.nblk), dim3(256), lds, st, X, ldx, nr, NU, ldn, nf, d, U, W, ldw,
                       nrhs, OUT, ldo, part, p.tps, p.tiles_c);
    PG_CHECK(hipGetLastError());
    return 0;
}

int pg_fmatmul_impl(hipStream_t st, const double* X, long ldx, int nr, const double* NU, long ldn, int nf, int d, const double* U,
                    const double* W, long ldw, int nrhs, double* OUT, long ldo, double* work) {
    if (nr == 0 || nrhs == 0) return 0;
    const MmPlan p = mm_plan(nr, nf, nrhs);
    double* part = p.nseg > 1 ? work : nullptr;
    if (p.nseg > 0) {
        const int rc = mm_with_nb(nrhs, [&](auto nb_c) {
            return pg_with_dmax(d, [&](auto dmax_c) {
                return launch_fmatmul<decltype(dmax_c)::value, decltype(nb_c)::value>(st, p, X, ldx, nr, NU, ldn, nf, d, U, W, ldw, nrhs, OUT, ldo,
                                                                                      part);
            });
        });
        if (rc) return rc;
    }
    if (p.nseg != 1) return pg_kmatmul_fold_plain(st, p, part, nr, nrhs, OUT, ldo);      // the segments in their order, or the empty sum
    return 0;
}
