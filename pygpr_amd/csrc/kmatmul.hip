// The matrix-free covariance product (include/pygpr_hip_matmul.h):
//   OUT[i][c] = sum_j k(xr_i, xc_j) V[j][c]  (+ shift V[i][c] in the symmetric form)
// without K ever being written.  kmfma.hip's pattern with the roles turned round: there a 16 x 16 block of G = W o K, computed in the
// accumulator layout of v_mfma_f64_16x16x4_f64, is the A operand of G^T A; here the block is K^T -- block row = column point, block
// column = row point -- so register r of a lane (g = lane >> 4, c16 = lane & 15) holds k(xr[i0 + c16], xc[j0 + g + 4 r]), which read as
// an A operand is A[i = c16][k = g]: the four column points j0 + 4 r .. j0 + 4 r + 3 of one k-step.  The B operand of that step is
// V[j0 + g + 4 r][c16] from LDS, the result OUT[i0 + g + 4 r][c16].  No LDS round trip for K, no transposition.
//   workgroup   256 threads own 64 rows of OUT, one block of up to 32 right-hand sides and one segment of the column range; wave w
//               owns rows 16 w .. 16 w + 15, its accumulators (4 or 8 doubles a lane) stay in registers for the whole walk
//   row point   a lane evaluates every one of its pairs against the SAME row point i0 + c16: its coordinates live in registers
//   column tile 64 points k-major in LDS ([k][64], sparse.hip's layout: the 16 lanes of one g read one word as a broadcast) and the
//               64 x 16 panels of V beside them, double-buffered; the next tile travels global -> registers while this one is computed
//   pair        kfun.h's forms from direct differences, four pairs interleaved (kpair.h's pair_sq is one pair at a time: not taken here)
// Bound by fp64 VALU issue on the pair evaluation: the product adds four matrix instructions per sixteen-column
// panel to four evaluations of some fifty fp64 operations each.
#include "kfun.h"
#include "kpair.h"
#include "kbuild.h"
#include "kmatmul.h"
#include <type_traits>

// (the tile constants MM_* and the plan mm_plan are in kmatmul.h: fmatmul.hip walks the same way)

// LDS of pg_kmatmul_kernel in bytes: two point tiles, two panels of V, l2 (and ipl), cpar -- the carve-up below
template <int DMAX, bool PER, int NB> static constexpr size_t kmatmul_lds_bytes() {
    return (size_t)(2 * MM_T * DMAX + 2 * NB * MM_T * MM_PANEL + (PER ? 2 : 1) * PG_MAX_COMP * DMAX + 4 * PG_MAX_COMP) * sizeof(double);
}
// partial tiles: part[seg][blk][tiles_r * 64][MM_BLOCK]
template <int DMAX, bool PER, bool PROD, int NB>
__global__ __launch_bounds__(256) void pg_kmatmul_kernel(pg_covspec spec, const double* __restrict__ hp, const double* __restrict__ Xr, long ldr,
                                                         int nr, const double* __restrict__ Xc, long ldc, int nc, int d,
                                                         const double* __restrict__ V, long ldv, int nrhs, double jitter, int sym,
                                                         double* __restrict__ OUT, long ldo, double* __restrict__ part, int tps, int tiles_c) {
    static_assert(!PROD || PER, "a product takes the instantiation that carries every kind");
    constexpr int NXP = (MM_T * DMAX) / 256;             // coordinates a thread stages per tile
    constexpr int NVP = (MM_T * MM_PANEL * NB) / 256;    // ... and entries of V
    constexpr int VW = MM_PANEL * NB;                    // columns of V this instantiation stages
    const int tr = blockIdx.x, seg = blockIdx.y, blk = blockIdx.z;
    const int cb = blk * MM_BLOCK;
    const int t0 = seg * tps, t1 = min(t0 + tps, tiles_c);
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c16 = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* xc = reinterpret_cast<double*>(smem_raw);          // two buffers [DMAX][64] of column points, zero for k >= d and points >= nc
    double* vt = xc + 2 * MM_T * DMAX;                          // two buffers [NB][64][16] of V, zero for points >= nc and columns >= nrhs
    double* l2 = vt + 2 * NB * MM_T * MM_PANEL;                 // [ncomp][DMAX] squared inverse length scales, zero for k >= d
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
    double xpf[NXP], vpf[NVP];
    auto fetch = [&](int tc) {
#pragma unroll
        for (int u = 0; u < NXP; ++u) {
            const int idx = tid + 256 * u, p = idx / DMAX, k = idx % DMAX;
            const int gc = tc * MM_T + p;
            const double v = Xc[(long)min(gc, nc - 1) * ldc + min(k, d - 1)];
            xpf[u] = (k < d && gc < nc) ? v : 0.0;
        }
#pragma unroll
        for (int u = 0; u < NVP; ++u) {
            const int idx = tid + 256 * u, j = idx / VW, c = idx % VW;
            const int gj = tc * MM_T + j, gcol = cb + c;
            const double v = V[(long)min(gj, nc - 1) * ldv + min(gcol, nrhs - 1)];
            vpf[u] = (gj < nc && gcol < nrhs) ? v : 0.0;
        }
    };
    auto stash = [&](int buf) {
        double* xb = xc + buf * MM_T * DMAX;
        double* vb = vt + buf * NB * MM_T * MM_PANEL;
#pragma unroll
        for (int u = 0; u < NXP; ++u) {
            const int idx = tid + 256 * u, p = idx / DMAX, k = idx % DMAX;
            xb[k * MM_T + p] = xpf[u];
        }
#pragma unroll
        for (int u = 0; u < NVP; ++u) {
            const int idx = tid + 256 * u, j = idx / VW, c = idx % VW;
            vb[(c / MM_PANEL) * MM_T * MM_PANEL + j * MM_PANEL + (c % MM_PANEL)] = vpf[u];
        }
    };

    pg_d4 acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[b][r] = 0.0;

    fetch(t0);
    for (int tc = t0, it = 0; tc < t1; ++tc, ++it) {
        const int buf = it & 1;
        stash(buf);
        __syncthreads();   // also orders this buffer's previous readers (two tiles ago) before the writes above, and the parameters' first readers
        if (tc + 1 < t1) fetch(tc + 1);
        const double* xb = xc + buf * MM_T * DMAX;
        const double* vb = vt + buf * NB * MM_T * MM_PANEL;
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
            // (a column point past the end was staged as the origin: its value is finite or not as the row point decides, and V is 0
            // there -- the select keeps an infinity or a NaN of that row from meeting the 0)
#pragma unroll
            for (int r = 0; r < 4; ++r) kv[r] = (j0 + 4 * r < jlim) ? kv[r] : 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int b = 0; b < NB; ++b)
                    acc[b] = Mfma<double>::run(kv[r], vb[b * MM_T * MM_PANEL + (j0 + 4 * r) * MM_PANEL + c16], acc[b]);
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
    double shift = 0.0;
    if (sym) {
        for (int q = 0; q < spec.nnoise; ++q) { const double s = hp[spec.noise_off[q]]; shift += s * s; }
        shift += jitter;
    }
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int gi = tr * MM_T + i0 + g + 4 * r, gcol = cb + MM_PANEL * b + c16;
            if (gi < nr && gcol < nrhs) {
                double s = acc[b][r];
                if (sym) s += shift * V[(long)gi * ldv + gcol];
                OUT[(long)gi * ldo + gcol] = s;
            }
        }
}

// OUT[i][c] = sum_{seg < nseg} part[seg][c / 32][i][c % 32] (+ shift V[i][c]), the segments in their order; nseg = 0: the empty sum
__global__ __launch_bounds__(256) void pg_kmatmul_fold_kernel(pg_covspec spec, const double* __restrict__ hp, const double* __restrict__ part,
                                                              int nseg, int nblk, long rows_pad, int nr, int nrhs, const double* __restrict__ V,
                                                              long ldv, double jitter, int sym, double* __restrict__ OUT, long ldo) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)nr * nrhs) return;
    const long i = e / nrhs;
    const int c = (int)(e % nrhs);
    const int blk = c / MM_BLOCK, cc = c % MM_BLOCK;
    double s = 0.0;
    for (int sg = 0; sg < nseg; ++sg) s += part[(((long)sg * nblk + blk) * rows_pad + i) * MM_BLOCK + cc];
    if (sym) {
        double shift = 0.0;
        for (int q = 0; q < spec.nnoise; ++q) { const double t = hp[spec.noise_off[q]]; shift += t * t; }
        shift += jitter;
        s += shift * V[i * ldv + c];
    }
    OUT[i * ldo + c] = s;
}

int pg_kmatmul_fold_plain(hipStream_t st, const MmPlan& p, const double* part, int nr, int nrhs, double* OUT, long ldo) {
    const long ne = (long)nr * nrhs;
    if (ne == 0) return 0;
    pg_covspec none = {};      // (no shift: neither the spec nor hp is read)
    hipLaunchKernelGGL(pg_kmatmul_fold_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, none, (const double*)nullptr, part, p.nseg,
                       p.nblk, (long)p.tiles_r * MM_T, nr, nrhs, (const double*)nullptr, 0L, 0.0, 0, OUT, ldo);
    PG_CHECK(hipGetLastError());
    return 0;
}

long pg_kmatmul_worksize_impl(int nr, int nc, int nrhs) {
    const MmPlan p = mm_plan(nr, nc, nrhs);
    return p.nseg > 1 ? (long)p.nseg * p.nblk * p.tiles_r * MM_T * MM_BLOCK : 0;
}

template <int DMAX, bool PER, bool PROD, int NB>
static int launch_kmatmul(hipStream_t st, const MmPlan& p, const pg_covspec& spec, const double* hp, const double* Xr, long ldr, int nr,
                          const double* Xc, long ldc, int nc, int d, const double* V, long ldv, int nrhs, double jitter, int sym, double* OUT,
                          long ldo, double* part) {
    constexpr size_t lds = kmatmul_lds_bytes<DMAX, PER, NB>();
    if (int rc = pg_lds_opt_in<pg_kmatmul_kernel<DMAX, PER, PROD, NB>>(lds)) return rc;   // d > 32 needs more than the 64 KB a kernel gets without opting in
    hipLaunchKernelGGL((pg_kmatmul_kernel<DMAX, PER, PROD, NB>), dim3(p.tiles_r, p.nseg, p.nblk), dim3(256), lds, st, spec, hp, Xr, ldr, nr, Xc,
                       ldc, nc, d, V, ldv, nrhs, jitter, sym, OUT, ldo, part, p.tps, p.tiles_c);
    PG_CHECK(hipGetLastError());
    return 0;
}

int pg_kmatmul_impl(hipStream_t st, const pg_covspec& spec_in, const double* hp, const double* Xr, long ldr, int nr, const double* Xc, long ldc,
                    int nc, int d, int sym, const double* V, long ldv, int nrhs, double jitter, double* OUT, long ldo, double* work) {
    if (nr == 0 || nrhs == 0) return 0;
    pg_covspec spec;
    const bool prod = pg_spec_strip(spec_in, spec);
    const MmPlan p = mm_plan(nr, nc, nrhs);
    double* part = p.nseg > 1 ? work : nullptr;
    if (p.nseg > 0) {
        const int rc = mm_with_nb(nrhs, [&](auto nb_c) {
            return pg_with_kinds(spec, prod, [&](auto per_c, auto prod_c) {
                return pg_with_dmax(d, [&](auto dmax_c) {
                    return launch_kmatmul<decltype(dmax_c)::value, decltype(per_c)::value, decltype(prod_c)::value, decltype(nb_c)::value>(
                        st, p, spec, hp, Xr, ldr, nr, Xc, ldc, nc, d, V, ldv, nrhs, jitter, sym, OUT, ldo, part);
                });
            });
        });
        if (rc) return rc;
    }
    if (p.nseg != 1) {      // the segments in their order, or the empty sum
        const long ne = (long)nr * nrhs;
        hipLaunchKernelGGL(pg_kmatmul_fold_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, spec, hp, part, p.nseg, p.nblk,
                           (long)p.tiles_r * MM_T, nr, nrhs, V, ldv, jitter, sym, OUT, ldo);
        PG_CHECK(hipGetLastError());
    }
    return 0;
}
