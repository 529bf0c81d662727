// The matrix-free product of the covariance's first-argument derivative (include/pygpr_hip_dmatmul.h):
//   OUT[i][k][c] = sum_j dk(xr_i, xc_j)/dxr_ik V[j][c]
// without dk ever being written.  kmatmul.hip's walk and layout: register r of a lane (g = lane >> 4, c16 = lane & 15) belongs to the
// pair (xr[i0 + c16], xc[j0 + g + 4 r]), which read as an A operand of v_mfma_f64_16x16x4_f64 is A[i = c16][k = g]: the four column
// points j0 + 4 r .. j0 + 4 r + 3 of one k-step against V[j0 + g + 4 r][c16] from LDS.  Where kmatmul.hip has one value per pair, this
// kernel has one per pair and coordinate,
//   dk/dxr_ik = sum_comp w l_k^2 D_k,   w = 2 kind_hcoef base(r) (times the other factors' values for a product spec),   D_k = xr_ik - xc_jk,
// (the periodic kind: sin(2 pi D_k / p_k) pi / (2 p_k) in the place of D_k and K as base -- xgrad.hip's forms), so the radial factor w
// of a pair is formed ONCE from the distance over all d coordinates and feeds one accumulator chain per coordinate.
//   workgroup   256 threads own 64 rows of OUT, one block of up to 32 right-hand sides, one segment of the column range and one CHUNK
//               of KC = 8 coordinates (4 at d <= 4): KC x NB accumulators of four doubles a lane.  The pair's distance still runs
//               over all d; a chunk's own coordinates of the row point are held a second time (xk) so that the chunk is a run-time
//               index and needs no instantiation of its own
//   row point, column tile, V panels, prefetch: kmatmul.hip's
// Registers per instantiation and what bounds the kernel: DESIGN.md 4.25.
#include "kfun.h"
#include "kpair.h"
#include "kbuild.h"
#include "kmatmul.h"
#include "dmatmul.h"
#include <type_traits>

// LDS of pg_dmatmul_kernel in bytes: kmatmul.hip's carve-up with 1 / p always beside l^2
template <int DMAX, int NB> static constexpr size_t dmatmul_lds_bytes() {
    return (size_t)(2 * MM_T * DMAX + 2 * NB * MM_T * MM_PANEL + 2 * PG_MAX_COMP * DMAX + 4 * PG_MAX_COMP) * sizeof(double);
}
// partial tiles: part[seg][tiles_r * 64][nchunk * KC][nblk * MM_BLOCK]
template <int DMAX, bool PER, bool PROD, int NB>
__global__ __launch_bounds__(256) void pg_dmatmul_kernel(pg_covspec spec, const double* __restrict__ hp, const double* __restrict__ Xr, long ldr,
                                                         int nr, const double* __restrict__ Xc, long ldc, int nc, int d,
                                                         const double* __restrict__ V, long ldv, int nrhs, double* __restrict__ OUT, long ldo,
                                                         long ldk, double* __restrict__ part, int tps, int tiles_c, int nchunk) {
    static_assert(!PROD || PER, "a product takes the instantiation that carries every kind");
    constexpr int KC = DMAX <= 4 ? 4 : DMM_KC;
    constexpr int NXP = (MM_T * DMAX) / 256;             // coordinates a thread stages per tile
    constexpr int NVP = (MM_T * MM_PANEL * NB) / 256;    // ... and entries of V
    constexpr int VW = MM_PANEL * NB;                    // columns of V this instantiation stages
    const int tr = blockIdx.x, seg = blockIdx.y, blk = blockIdx.z / nchunk, chunk = blockIdx.z % nchunk;
    const int cb = blk * MM_BLOCK, k0 = chunk * KC;
    const int t0 = seg * tps, t1 = min(t0 + tps, tiles_c);
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c16 = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* xc = reinterpret_cast<double*>(smem_raw);          // two buffers [DMAX][64] of column points, zero for k >= d and points >= nc
    double* vt = xc + 2 * MM_T * DMAX;                          // two buffers [NB][64][16] of V, zero for points >= nc and columns >= nrhs
    double* l2 = vt + 2 * NB * MM_T * MM_PANEL;                 // [ncomp][DMAX] squared inverse length scales, zero for k >= d
    double* ipl = l2 + PG_MAX_COMP * DMAX;                      // [ncomp][DMAX] reciprocal periods, zero for k >= d / other kinds
    double* cpar = ipl + PG_MAX_COMP * DMAX;                    // [ncomp][4]: sigma^2, the squared shape, its reciprocal, 2 kind_hcoef
    pair_stage_hp<double, true>(spec, hp, d, DMAX, DMAX, l2, ipl, tid, 256);
    if (tid < spec.ncomp) {
        const double sg = hp[spec.off[tid]], sh = kind_shape2(spec, hp, tid, d);
        cpar[4 * tid] = sg * sg;
        cpar[4 * tid + 1] = sh;
        cpar[4 * tid + 2] = 1.0 / sh;
        cpar[4 * tid + 3] = 2.0 * kind_hcoef(spec.kind[tid]);
    }
    // this lane's row point, in registers for the whole walk (zero for k >= d and rows >= nr), and the chunk's coordinates of it
    const int i0 = 16 * wave;
    const int gi_pt = tr * MM_T + i0 + c16;
    double xi[DMAX], xk[KC];
#pragma unroll
    for (int k = 0; k < DMAX; ++k) xi[k] = (k < d && gi_pt < nr) ? Xr[(long)gi_pt * ldr + k] : 0.0;
#pragma unroll
    for (int kk = 0; kk < KC; ++kk) xk[kk] = (k0 + kk < d && gi_pt < nr) ? Xr[(long)gi_pt * ldr + k0 + kk] : 0.0;

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

    pg_d4 acc[KC][NB];
#pragma unroll
    for (int kk = 0; kk < KC; ++kk)
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[kk][b][r] = 0.0;

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
            // component c at this lane's four pairs: the value and kfun.h's `base` (the periodic kind: K for both)
            auto eval = [&](int c, double (&val)[4], double (&bs)[4]) {
                const double* lc = l2 + c * DMAX;
                const int kind = spec.kind[c];
                const double sig2 = cpar[4 * c];
                double sq[4] = {0.0, 0.0, 0.0, 0.0};
                if constexpr (PER) {
                    if (kind == PG_KIND_PERIODIC) {      // (padding coordinates: l^2 = 1 / p = 0, so the term vanishes)
                        const double* ipc = ipl + c * DMAX;
#pragma unroll
                        for (int k = 0; k < DMAX; ++k) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) sq[r] += lc[k] * per_sin2<double>((xi[k] - xb[k * MM_T + j0 + 4 * r]) * ipc[k]);
                            if (k % 8 == 7) __builtin_amdgcn_sched_barrier(0);
                        }
#pragma unroll
                        for (int r = 0; r < 4; ++r) val[r] = bs[r] = kind_value<double, PG_KIND_RBF>(sig2, sq[r]);
                        return;
                    }
                }
#pragma unroll
                for (int k = 0; k < DMAX; ++k) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double df = xi[k] - xb[k * MM_T + j0 + 4 * r];
                        sq[r] += lc[k] * df * df;
                    }
                    // (the distance's LDS reads are taken eight coordinates at a time: hoisted together, the 4 DMAX words of a
                    // large d crowd the accumulators out of the register file)
                    if (k % 8 == 7) __builtin_amdgcn_sched_barrier(0);
                }
                if (kind == PG_KIND_RBF) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) val[r] = bs[r] = kind_value<double, PG_KIND_RBF>(sig2, sq[r]);
                } else {
                    const double sha = cpar[4 * c + 1], ish = cpar[4 * c + 2];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        double ft;
                        matern_val<double>(kind, sig2, sq[r], val[r], bs[r], sha, ish, ft);
                    }
                }
            };
            double tv[KC][4];      // dk/dxr_ik of the four pairs, the chunk's coordinates
#pragma unroll
            for (int kk = 0; kk < KC; ++kk)
#pragma unroll
                for (int r = 0; r < 4; ++r) tv[kk][r] = 0.0;
            for (int c = 0; c < spec.ncomp; ++c) {
                double w[4], val[4];
                eval(c, val, w);
#pragma unroll
                for (int r = 0; r < 4; ++r) w[r] *= cpar[4 * c + 3];
                if constexpr (PROD) {      // the other factors' values, formed explicitly: one that underflows gives 0
                    for (int c2 = 0; c2 < spec.ncomp; ++c2) {
                        if (c2 == c) continue;
                        double v2[4], b2[4];
                        eval(c2, v2, b2);
#pragma unroll
                        for (int r = 0; r < 4; ++r) w[r] *= v2[r];
                    }
                }
                const double* lc = l2 + c * DMAX + k0;
                bool done = false;
                if constexpr (PER) {
                    if (spec.kind[c] == PG_KIND_PERIODIC) {
                        const double* ipc = ipl + c * DMAX + k0;
#pragma unroll
                        for (int kk = 0; kk < KC; ++kk) {
                            const double f = lc[kk] * (0.5 * PG_PI) * ipc[kk];
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                double s2, s2w;
                                per_terms<double>((xk[kk] - xb[(k0 + kk) * MM_T + j0 + 4 * r]) * ipc[kk], s2, s2w);
                                tv[kk][r] += w[r] * (s2w * f);
                            }
                        }
                        done = true;
                    }
                }
                if (!done) {
#pragma unroll
                    for (int kk = 0; kk < KC; ++kk)
#pragma unroll
                        for (int r = 0; r < 4; ++r) tv[kk][r] += w[r] * (lc[kk] * (xk[kk] - xb[(k0 + kk) * MM_T + j0 + 4 * r]));
                }
            }
            // (a column point past the end was staged as the origin: its terms are finite or not as the row point decides, and V is 0
            // there -- the select keeps an infinity or a NaN of that row from meeting the 0; only the last tile has such points)
            if (jlim < MM_T) {
#pragma unroll
                for (int kk = 0; kk < KC; ++kk)
#pragma unroll
                    for (int r = 0; r < 4; ++r) tv[kk][r] = (j0 + 4 * r < jlim) ? tv[kk][r] : 0.0;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double vv[NB];
#pragma unroll
                for (int b = 0; b < NB; ++b) vv[b] = vb[b * MM_T * MM_PANEL + (j0 + 4 * r) * MM_PANEL + c16];
#pragma unroll
                for (int kk = 0; kk < KC; ++kk)
#pragma unroll
                    for (int b = 0; b < NB; ++b) acc[kk][b] = Mfma<double>::run(tv[kk][r], vv[b], acc[kk][b]);
            }
        }
    }

    // register r of accumulator (kk, b): OUT[tr 64 + i0 + g + 4 r][k0 + kk][cb + 16 b + c16]
    if (part) {
        const long rows_pad = (long)gridDim.x * MM_T, dpad = (long)nchunk * KC, cpad = (long)(gridDim.z / nchunk) * MM_BLOCK;
        double* pp = part + (((long)seg * rows_pad + tr * MM_T + i0) * dpad + k0) * cpad + cb;
#pragma unroll
        for (int kk = 0; kk < KC; ++kk)
#pragma unroll
            for (int b = 0; b < NB; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) pp[((long)(g + 4 * r) * dpad + kk) * cpad + MM_PANEL * b + c16] = acc[kk][b][r];
        return;
    }
#pragma unroll
    for (int kk = 0; kk < KC; ++kk)
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int gi = tr * MM_T + i0 + g + 4 * r, gcol = cb + MM_PANEL * b + c16;
                if (gi < nr && k0 + kk < d && gcol < nrhs) OUT[(long)gi * ldo + (long)(k0 + kk) * ldk + gcol] = acc[kk][b][r];
            }
}

// OUT[i][k][c] = sum_{seg < nseg} part[seg][i][k][c], the segments in their order; nseg = 0: the empty sum
__global__ __launch_bounds__(256) void pg_dmatmul_fold_kernel(const double* __restrict__ part, int nseg, long rows_pad, long dpad, long cpad, int nr,
                                                              int d, int nrhs, double* __restrict__ OUT, long ldo, long ldk) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)nr * d * nrhs) return;
    const long i = e / ((long)d * nrhs);
    const int k = (int)((e / nrhs) % d), c = (int)(e % nrhs);
    double s = 0.0;
    for (int sg = 0; sg < nseg; ++sg) s += part[(((long)sg * rows_pad + i) * dpad + k) * cpad + c];
    OUT[i * ldo + k * ldk + c] = s;
}

long pg_dmatmul_worksize_impl(int nr, int nc, int d, int nrhs) {
    const MmPlan p = mm_plan(nr, nc, nrhs);
    return p.nseg > 1 ? (long)p.nseg * p.tiles_r * MM_T * dmm_nchunk(d) * dmm_chunk(d) * p.nblk * MM_BLOCK : 0;
}

template <int DMAX, bool PER, bool PROD, int NB>
static int launch_dmatmul(hipStream_t st, const MmPlan& p, const pg_covspec& spec, const double* hp, const double* Xr, long ldr, int nr,
                          const double* Xc, long ldc, int nc, int d, const double* V, long ldv, int nrhs, double* OUT, long ldo, long ldk,
                          double* part) {
    static_assert((DMAX <= 4 ? 4 : DMM_KC) <= DMAX, "a chunk lies inside the staged coordinates");
    constexpr size_t lds = dmatmul_lds_bytes<DMAX, NB>();
    if (int rc = pg_lds_opt_in<pg_dmatmul_kernel<DMAX, PER, PROD, NB>>(lds)) return rc;   // d > 32 needs more than the 64 KB a kernel gets without opting in
    const int nchunk = dmm_nchunk(d);
    hipLaunchKernelGGL((pg_dmatmul_kernel<DMAX, PER, PROD, NB>), dim3(p.tiles_r, p.nseg, p.nblk * nchunk), dim3(256), lds, st, spec, hp, Xr, ldr,
                       nr, Xc, ldc, nc, d, V, ldv, nrhs, OUT, ldo, ldk, part, p.tps, p.tiles_c, nchunk);
    PG_CHECK(hipGetLastError());
    return 0;
}

int pg_dmatmul_impl(hipStream_t st, const pg_covspec& spec_in, const double* hp, const double* Xr, long ldr, int nr, const double* Xc, long ldc,
                    int nc, int d, const double* V, long ldv, int nrhs, double* OUT, long ldo, long ldk, double* work) {
    if (nr == 0 || nrhs == 0) return 0;
    pg_covspec spec;
    const bool prod = pg_spec_strip(spec_in, spec);
    const MmPlan p = mm_plan(nr, nc, nrhs);
    double* part = p.nseg > 1 ? work : nullptr;
    if (p.nseg > 0) {
        const int rc = mm_with_nb(nrhs, [&](auto nb_c) {
            return pg_with_kinds(spec, prod, [&](auto per_c, auto prod_c) {
                return pg_with_dmax(d, [&](auto dmax_c) {
                    return launch_dmatmul<decltype(dmax_c)::value, decltype(per_c)::value, decltype(prod_c)::value, decltype(nb_c)::value>(
                        st, p, spec, hp, Xr, ldr, nr, Xc, ldc, nc, d, V, ldv, nrhs, OUT, ldo, ldk, part);
                });
            });
        });
        if (rc) return rc;
    }
    if (p.nseg != 1) {      // the segments in their order, or the empty sum
        const long ne = (long)nr * d * nrhs;
        hipLaunchKernelGGL(pg_dmatmul_fold_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, part, p.nseg, (long)p.tiles_r * MM_T,
                           (long)dmm_nchunk(d) * dmm_chunk(d), (long)p.nblk * MM_BLOCK, nr, d, nrhs, OUT, ldo, ldk);
        PG_CHECK(hipGetLastError());
    }
    return 0;
}
