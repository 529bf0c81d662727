// The training-input gradient against a low-rank weight (include/pygpr_hip_lxgrad.h):
//   OUT[i][k] (+)= sum_j (sum_t U[i][t] V[j][t] [+ V[i][t] U[j][t]]) dk(xr_i, xc_j)/dxr_ik
// without the weight or dk ever being written.  kmatmul.hip's walk and layout: register q of a lane (g = lane >> 4, c16 = lane & 15)
// belongs to the pair (xr[i0 + c16], xc[j0 + g + 4 q]).  lowrank.hip forms a 16 x 16 block of W = U V^T on the fp64 matrix pipe with the
// rows of the block in the accumulator's rows; here the block is formed TRANSPOSED, A[m][k] = V[j0 + c16][t + g] from the column tile's
// panel in LDS and B[k][n] = U[i0 + c16][t + g] -- the lane's own row of U, in registers for the whole walk -- so that accumulator
// register q of lane (g, c16) holds W[i0 + c16][j0 + g + 4 q]: the weight of exactly the pair this lane evaluates.  The symmetric form
// adds a second chain with the panels' roles swapped (A from the column tile's U, B from the lane's own row of V).
// The pair's derivative is dmatmul.hip's,
//   dk/dxr_ik = sum_comp w l_k^2 D_k,   w = 2 kind_hcoef base(r) (times the other factors' values for a product spec),   D_k = xr_ik - xc_jk,
// (the periodic kind: sin(2 pi D_k / p_k) pi / (2 p_k) in the place of D_k and K as base), the radial factor w formed ONCE from the
// distance over all d coordinates.  The pair's weight is multiplied into w before the coordinate loop -- one multiply per pair, then one
// multiply-add per coordinate into the lane's accumulators; dmatmul.hip's tv[kk][r] values are never held (32 doubles a lane).
//   workgroup   256 threads own 64 rows of OUT, one segment of the column range and one CHUNK of KC coordinates; wave w owns rows
//               16 w .. 16 w + 15
//   row point   in registers for the whole walk, and the chunk's coordinates of it a second time (dmatmul.hip's xk)
//   column tile 64 points k-major in LDS and beside them the 64-row panels of V (and U), point-major at a stride of rp + 2 words: both
//               the staging writes and the operand reads of a half-wave meet distinct banks; double-buffered, the next tile travels
//               global -> registers while this one is computed
//   sums        at the end of the walk the four g of a row are added in the order 0, 1, 2, 3 (krowsq.hip's); column segments and the
//               passes of a rank above LXG_RC go to `work` as slabs, folded in their order by a second launch
// Registers per instantiation: profiles/lxgrad_resources.txt; what bounds the kernel: DESIGN.md 4.27.
#include "kfun.h"
#include "kpair.h"
#include "kbuild.h"
#include "kmatmul.h"
#include "dmatmul.h"
#include "lxgrad.h"
#include <type_traits>

// LDS of pg_lxgrad_kernel in bytes with rp factor columns staged: two point tiles, l2 and ipl, cpar, two buffers of one or two panels
template <int DMAX, bool SYM> static constexpr size_t lxgrad_lds_bytes(int rp) {
    return (size_t)(2 * MM_T * DMAX + 2 * PG_MAX_COMP * DMAX + 4 * PG_MAX_COMP + 2 * (SYM ? 2 : 1) * MM_T * (rp + 2)) * sizeof(double);
}
// slabs: part[slab][tiles_r * 64][nchunk * KC], slab = pass * nseg + seg
template <int DMAX, bool PER, bool PROD, bool SYM>
__global__ __launch_bounds__(256) void pg_lxgrad_kernel(pg_covspec spec, const double* __restrict__ hp, const double* __restrict__ Xr, long ldr,
                                                        int nr, const double* __restrict__ Xc, long ldc, int nc, int d,
                                                        const double* __restrict__ U, long ldu, const double* __restrict__ V, long ldv, int t0,
                                                        int rc, double* __restrict__ OUT, long ldo, int accumulate, double* __restrict__ part,
                                                        int tps, int tiles_c, int nchunk) {
    static_assert(!PROD || PER, "a product takes the instantiation that carries every kind");
    static_assert((MM_T * DMAX) % 256 == 0, "every thread stages the same number of coordinates");
    constexpr int KC = DMAX <= 4 ? 4 : DMM_KC;          // the chunk of coordinates one workgroup accumulates: dmatmul.hip's (dmm_chunk)
    constexpr int NXP = (MM_T * DMAX) / 256;             // coordinates a thread stages per tile
    constexpr int NPP = (MM_T * LXG_RC) / 256;           // ... and entries of a factor panel
    constexpr int NQ = LXG_RC / 4;                       // matrix instructions of one chain
    const int tr = blockIdx.x, seg = blockIdx.y, chunk = blockIdx.z;
    const int k0 = chunk * KC;
    const int c0 = seg * tps, c1 = min(c0 + tps, tiles_c);
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c16 = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rp = (rc + 3) & ~3;                        // factor columns staged: zero behind rc
    const int ps = rp + 2;                               // words between two points of a panel
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* xc = reinterpret_cast<double*>(smem_raw);          // two buffers [DMAX][64] of column points, zero for k >= d and points >= nc
    double* l2 = xc + 2 * MM_T * DMAX;                          // [ncomp][DMAX] squared inverse length scales, zero for k >= d
    double* ipl = l2 + PG_MAX_COMP * DMAX;                      // [ncomp][DMAX] reciprocal periods, zero for k >= d / other kinds
    double* cpar = ipl + PG_MAX_COMP * DMAX;                    // [ncomp][4]: sigma^2, the squared shape, its reciprocal, 2 kind_hcoef
    double* vp = cpar + 4 * PG_MAX_COMP;                        // two buffers [64][ps]: V of the column tile, zero for points >= nc
    double* up = vp + 2 * MM_T * ps;                            // SYM: two buffers [64][ps]: U of the column tile
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
    // ... and its rows of the factors as B operands: entry q is factor column t0 + 4 q + g (zero behind rc and for rows >= nr)
    double ub[NQ], vbr[SYM ? NQ : 1];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int t = 4 * q + g;
        const bool in = t < rc && gi_pt < nr;
        const long row = min(gi_pt, nr - 1), col = t0 + min(t, rc - 1);
        const double uv = U[row * ldu + col];
        ub[q] = in ? uv : 0.0;
        if constexpr (SYM) {
            const double vv = V[row * ldv + col];
            vbr[q] = in ? vv : 0.0;
        }
    }

    // global -> registers at clamped addresses (every address is an element of the operand: gaps are not read), registers -> LDS
    double xpf[NXP], vpf[NPP], upf[SYM ? NPP : 1];
    auto fetch = [&](int tc) {
#pragma unroll
        for (int u = 0; u < NXP; ++u) {
            const int idx = tid + 256 * u, p = idx / DMAX, k = idx % DMAX;
            const int gc = tc * MM_T + p;
            const double v = Xc[(long)min(gc, nc - 1) * ldc + min(k, d - 1)];
            xpf[u] = (k < d && gc < nc) ? v : 0.0;
        }
#pragma unroll
        for (int u = 0; u < NPP; ++u) {
            const int idx = tid + 256 * u, j = idx / LXG_RC, t = idx % LXG_RC;
            const int gj = tc * MM_T + j;
            const bool in = t < rc && gj < nc;
            const long row = min(gj, nc - 1), col = t0 + min(t, rc - 1);
            const double v = V[row * ldv + col];
            vpf[u] = in ? v : 0.0;
            if constexpr (SYM) {
                const double w = U[row * ldu + col];
                upf[u] = in ? w : 0.0;
            }
        }
    };
    auto stash = [&](int buf) {
        double* xb = xc + buf * MM_T * DMAX;
        double* vb = vp + buf * MM_T * ps;
        double* ubf = up + buf * MM_T * ps;
#pragma unroll
        for (int u = 0; u < NXP; ++u) {
            const int idx = tid + 256 * u, p = idx / DMAX, k = idx % DMAX;
            xb[k * MM_T + p] = xpf[u];
        }
#pragma unroll
        for (int u = 0; u < NPP; ++u) {
            const int idx = tid + 256 * u, j = idx / LXG_RC, t = idx % LXG_RC;
            if (t < rp) {
                vb[j * ps + t] = vpf[u];
                if constexpr (SYM) ubf[j * ps + t] = upf[u];
            }
        }
    };

    double acc[KC];
#pragma unroll
    for (int kk = 0; kk < KC; ++kk) acc[kk] = 0.0;

    fetch(c0);      // (a launch has c0 < c1 <= tiles_c, nc >= 1 and rc >= 1: the plan gives no segment to an empty sum)
    for (int tc = c0, it = 0; tc < c1; ++tc, ++it) {
        const int buf = it & 1;
        stash(buf);
        __syncthreads();   // also orders this buffer's previous readers (two tiles ago) before the writes above, and the parameters' first readers
        if (tc + 1 < c1) fetch(tc + 1);
        const double* xb = xc + buf * MM_T * DMAX;
        const double* vb = vp + buf * MM_T * ps;
        const double* ubf = up + buf * MM_T * ps;
        const int jlim = nc - tc * MM_T;      // column points of this tile that exist
#pragma unroll 1
        for (int jb = 0; jb < 4; ++jb) {
            const int j0 = 16 * jb + g;       // this lane's column points: j0 + 4 r
            // the weights of this lane's four pairs: W[i0 + c16][16 jb + g + 4 r] in register r
            pg_d4 wq = {0.0, 0.0, 0.0, 0.0};
            {
                const double* va = vb + (16 * jb + c16) * ps + g;
#pragma unroll
                for (int q = 0; q < NQ; ++q)
                    if (4 * q < rp) wq = Mfma<double>::run(va[4 * q], ub[q], wq);
                if constexpr (SYM) {
                    const double* ua = ubf + (16 * jb + c16) * ps + g;
#pragma unroll
                    for (int q = 0; q < NQ; ++q)
                        if (4 * q < rp) wq = Mfma<double>::run(ua[4 * q], vbr[q], wq);
                }
            }
            // component c at this lane's four pairs: the value and kfun.h's `base` (the periodic kind: K for both) -- dmatmul.hip's
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
                    // (the distance's LDS reads are taken eight coordinates at a time, as in dmatmul.hip)
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
            // (a column point past the end was staged as the origin and its factor rows as zero: the derivative there is finite or not as
            // the row point decides, the weight as the row's factors do -- the select keeps the weighted radial factor of such a pair at
            // zero; only the last tile has such points)
            const bool tail = jlim < MM_T;
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
                // the pair's weight meets the radial factor ONCE, before the coordinates: dk/dxr_ik W = (w W) l_k^2 D_k
#pragma unroll
                for (int r = 0; r < 4; ++r) w[r] = (tail && j0 + 4 * r >= jlim) ? 0.0 : w[r] * wq[r];
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
                                acc[kk] = fma(w[r], s2w * f, acc[kk]);
                            }
                        }
                        done = true;
                    }
                }
                if (!done) {
#pragma unroll
                    for (int kk = 0; kk < KC; ++kk)
#pragma unroll
                        for (int r = 0; r < 4; ++r) acc[kk] = fma(w[r], lc[kk] * (xk[kk] - xb[(k0 + kk) * MM_T + j0 + 4 * r]), acc[kk]);
                }
            }
        }
    }

    // the four g of a row, in their order: lane c16 + 16 g' of this wave holds the partial sums of g'
    double s[KC];
#pragma unroll
    for (int kk = 0; kk < KC; ++kk) {
        s[kk] = __shfl(acc[kk], c16, 64);
#pragma unroll
        for (int gg = 1; gg < 4; ++gg) s[kk] += __shfl(acc[kk], c16 + 16 * gg, 64);
    }
    if (g != 0) return;
    if (part) {      // (rows behind nr and coordinates behind d included: a slab holds tiles_r * 64 rows of nchunk * KC)
        const long rows_pad = (long)gridDim.x * MM_T, dpad = (long)nchunk * KC;
        double* pp = part + (((long)seg * rows_pad + gi_pt) * dpad + k0);
#pragma unroll
        for (int kk = 0; kk < KC; ++kk) pp[kk] = s[kk];
        return;
    }
    if (gi_pt < nr) {
#pragma unroll
        for (int kk = 0; kk < KC; ++kk)
            if (k0 + kk < d) {
                double* o = OUT + (long)gi_pt * ldo + k0 + kk;
                *o = accumulate ? *o + s[kk] : s[kk];
            }
    }
}

// OUT[i][k] (+)= sum_{slab < nslab} part[slab][i][k], the slabs in their order; nslab = 0: the empty sum
__global__ __launch_bounds__(256) void pg_lxgrad_fold_kernel(const double* __restrict__ part, int nslab, long rows_pad, long dpad, int nr, int d,
                                                             double* __restrict__ OUT, long ldo, int accumulate) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)nr * d) return;
    const long i = e / d;
    const int k = (int)(e % d);
    double s = 0.0;
    for (int sl = 0; sl < nslab; ++sl) s += part[((long)sl * rows_pad + i) * dpad + k];
    double* o = OUT + i * ldo + k;
    *o = accumulate ? *o + s : s;
}

long pg_lxgrad_worksize_impl(int nr, int nc, int d, int r) {
    if (d < 1) return 0;
    const MmPlan p = mm_plan(nr, nc, 1);
    const long nslab = (long)p.nseg * lxg_npass(r);
    return nslab > 1 ? nslab * p.tiles_r * MM_T * dmm_nchunk(d) * dmm_chunk(d) : 0;
}

template <int DMAX, bool PER, bool PROD, bool SYM>
static int launch_lxgrad(hipStream_t st, const MmPlan& p, const pg_covspec& spec, const double* hp, const double* Xr, long ldr, int nr,
                         const double* Xc, long ldc, int nc, int d, const double* U, long ldu, const double* V, long ldv, int r, double* OUT,
                         long ldo, int accumulate, double* part) {
    static_assert((DMAX <= 4 ? 4 : DMM_KC) <= DMAX, "a chunk lies inside the staged coordinates");
    // d > 32, or a full pass of the symmetric form at d = 32, needs more than the 64 KB a kernel gets without opting in
    if (int rc = pg_lds_opt_in<pg_lxgrad_kernel<DMAX, PER, PROD, SYM>>(lxgrad_lds_bytes<DMAX, SYM>(LXG_RC))) return rc;
    const int nchunk = dmm_nchunk(d);
    const long slab = (long)p.tiles_r * MM_T * nchunk * dmm_chunk(d);
    for (int ps = 0; ps < lxg_npass(r); ++ps) {      // passes over the factor columns, each into slabs of its own
        const int t0 = ps * LXG_RC, rc = std::min(LXG_RC, r - t0);
        const size_t lds = lxgrad_lds_bytes<DMAX, SYM>((rc + 3) & ~3);
        hipLaunchKernelGGL((pg_lxgrad_kernel<DMAX, PER, PROD, SYM>), dim3(p.tiles_r, p.nseg, nchunk), dim3(256), lds, st, spec, hp, Xr, ldr, nr,
                           Xc, ldc, nc, d, U, ldu, V, ldv, t0, rc, OUT, ldo, accumulate, part ? part + (long)ps * p.nseg * slab : nullptr, p.tps,
                           p.tiles_c, nchunk);
        PG_CHECK(hipGetLastError());
    }
    return 0;
}

int pg_lxgrad_impl(hipStream_t st, const pg_covspec& spec_in, const double* hp, const double* Xr, long ldr, int nr, const double* Xc, long ldc,
                   int nc, int d, int sym, const double* U, long ldu, const double* V, long ldv, int r, double* OUT, long ldo, int accumulate,
                   double* work) {
    if (nr == 0) return 0;
    pg_covspec spec;
    const bool prod = pg_spec_strip(spec_in, spec);
    const MmPlan p = mm_plan(nr, nc, 1);
    const int nslab = p.nseg * lxg_npass(r);
    double* part = nslab > 1 ? work : nullptr;
    if (nslab > 0) {
        const int rc = pg_with_kinds(spec, prod, [&](auto per_c, auto prod_c) {
            return pg_with_dmax(d, [&](auto dmax_c) {
                constexpr int DM = decltype(dmax_c)::value;
                constexpr bool PE = decltype(per_c)::value, PR = decltype(prod_c)::value;
                return sym ? launch_lxgrad<DM, PE, PR, true>(st, p, spec, hp, Xr, ldr, nr, Xc, ldc, nc, d, U, ldu, V, ldv, r, OUT, ldo, accumulate, part)
                           : launch_lxgrad<DM, PE, PR, false>(st, p, spec, hp, Xr, ldr, nr, Xc, ldc, nc, d, U, ldu, V, ldv, r, OUT, ldo, accumulate, part);
            });
        });
        if (rc) return rc;
    }
    if (nslab == 0 && accumulate) return 0;      // the empty sum added: OUT as it is
    if (nslab != 1) {      // the slabs in their order, or the empty sum
        const long ne = (long)nr * d;
        hipLaunchKernelGGL(pg_lxgrad_fold_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, part, nslab, (long)p.tiles_r * MM_T,
                           (long)dmm_nchunk(d) * dmm_chunk(d), nr, d, OUT, ldo, accumulate);
        PG_CHECK(hipGetLastError());
    }
    return 0;
}
