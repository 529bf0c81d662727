// The matrix-free hyper-parameter contraction against a low-rank weight (include/pygpr_hip_lowrank.h):
//   grad[p] (+)= sum_{i, j} (sum_{t < r} U[i][t] V[j][t]) dk(xr_i, xc_j)/dtheta_p
// The contraction of pg_kernel_cross_grad (sparse.hip) with the weight formed on the fly.  kmatmul.hip's pattern with the roles turned once more: there a 16 x 16
// block of covariance values is the A operand of a product; here the 16 x 16 block of W = U V^T is the RESULT of r / 4 steps of
// v_mfma_f64_16x16x4_f64 on the factor panels, A[i][k] = U[i0 + c16][t0 + g] and B[k][j] = V[j0 + c16][t0 + g], and arrives in the
// accumulator layout: register q of lane (g = lane >> 4, c16 = lane & 15) holds W[i0 + g + 4 q][j0 + c16].  The pair derivatives are
// evaluated right there, one weight register against one pair, and folded into per-lane accumulators: the per-pair body and the fold
// are pg_cross_grad_kernel's text (see sparse.hip's header on why three kernels carry it), the product rule's factor is kpair.h's.
//   workgroup   256 threads own one tile of 64 column points and a segment of the row tiles; wave w owns columns 16 w .. 16 w + 15
//   column      a lane evaluates every one of its pairs against the SAME column point j0 + c16: its coordinates live in registers;
//               the 64-row panels of V (and of U in the symmetric form) of the column tile sit in LDS for the whole walk
//   row tile    64 points k-major in LDS ([k][64]: the 16 lanes of one g read one word as a broadcast) and the panels of U (and V)
//               beside them, t-major at a stride of 80 words: the four g of an operand read meet distinct banks
//   symmetric   only tiles on and below the diagonal are walked; off the diagonal the weight is W_ij + W_ji, a second chain of matrix
//               instructions with the panels swapped (A from the row tile's V, B from the column tile's U)
//   sums        per-lane accumulators -> wave_sum -> one slot row of `work` per workgroup, folded by pg_cross_grad_reduce_kernel
// More than LR_RC factor columns are taken in passes of LR_RC (the panels of 64 columns, four of them in the symmetric form, do not
// fit the LDS beside a 64-dimensional point tile); every pass has slot rows of its own and the one reduce folds them all.
// Bound by fp64 VALU issue on the pair evaluation, like pg_kernel_matmul.
#include "kfun.h"
#include "kpair.h"
#include "kbuild.h"
#include "sparse.h"
#include "lowrank.h"
#include <type_traits>

#define LR_T 64          // tile edge
#define LR_RC 32         // factor columns of one pass over the pairs
#define LR_PS 80         // words between two factor columns of a panel in LDS
#define LR_SEGMIN 4      // row tiles a segment holds at least
#define LR_WGCAP 32768   // workgroups of one pass beyond which the segments grow: a constant, so the order of the sum depends on the shape alone

struct LrPlan {
    int tiles_r, tiles_c, tps, nseg, nchunk;      // tps: row tiles per segment; nchunk: passes over the factor columns
    long nblk;                                    // slot rows: nseg * tiles_c * nchunk
};
static inline LrPlan lr_plan(int nr, int nc, int r) {
    LrPlan p;
    p.tiles_r = (nr + LR_T - 1) / LR_T;
    p.tiles_c = (nc + LR_T - 1) / LR_T;
    p.nchunk = (r + LR_RC - 1) / LR_RC;
    p.tps = p.nseg = 0;
    p.nblk = 0;
    if (p.tiles_r > 0 && p.tiles_c > 0 && p.nchunk > 0) {
        const long tot = (long)p.tiles_r * p.tiles_c;
        const long t = std::max<long>(LR_SEGMIN, (tot + LR_WGCAP - 1) / LR_WGCAP);
        p.tps = (int)std::min<long>(t, p.tiles_r);
        p.nseg = (p.tiles_r + p.tps - 1) / p.tps;
        p.nblk = (long)p.nseg * p.tiles_c * p.nchunk;
    }
    return p;
}

// LDS of pg_lowrank_grad_kernel in bytes with rp factor columns staged: red, the row tile (d > 16: and the column tile), l2 (and ipl),
// four panels -- the carve-up below
template <int DMAX, bool PER> static constexpr size_t lowrank_lds_bytes(int rp) {
    return (size_t)(4 * kind_nparam(PER ? PG_KIND_PERIODIC : PG_KIND_RQ, DMAX) + (DMAX <= 16 ? 1 : 2) * LR_T * DMAX +
                    (PER ? 2 : 1) * PG_MAX_COMP * DMAX + 4 * rp * LR_PS) * sizeof(double);
}
// slot rows: part[(seg * tiles_c + tc)][pw], the layout of pg_cross_grad_kernel's
template <int DMAX, bool PER, bool PROD>
__global__ __launch_bounds__(256) void pg_lowrank_grad_kernel(pg_covspec spec, const double* __restrict__ hp, const double* __restrict__ Xr, long ldr,
                                                              int nr, const double* __restrict__ Xc, long ldc, int nc, int d,
                                                              const double* __restrict__ U, long ldu, const double* __restrict__ V, long ldv,
                                                              int t0, int rc, int sym, double* __restrict__ part, int pw, int tps, int tiles_r) {
    static_assert(!PROD || PER, "a product takes the instantiation that carries every kind");
    const int tc = blockIdx.x, seg = blockIdx.y;
    const long blk = (long)seg * gridDim.x + tc;
    int r0 = seg * tps;
    const int r1 = min(r0 + tps, tiles_r);
    if (sym) r0 = max(r0, tc);                     // tiles on and below the diagonal; an empty range writes zeros into its slots
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c16 = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rp = (rc + 3) & ~3;                  // factor columns staged: zero behind rc
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int RS = kind_nparam(PER ? PG_KIND_PERIODIC : PG_KIND_RQ, DMAX);      // slots of the widest block this kernel folds
    double* red = reinterpret_cast<double*>(smem_raw);             // [4 waves][RS]: sigma, l_1..l_DMAX, the shape | the periods
    double* xr = red + 4 * RS;                                      // the row points' tile [DMAX][64], zero for k >= d
    double* l2 = xr + LR_T * DMAX;                                  // [ncomp][DMAX] squared inverse length scales, zero for k >= d
    double* ipl = l2 + PG_MAX_COMP * DMAX;                          // PER: [ncomp][DMAX] reciprocal periods, zero for k >= d / other kinds
    double* vc = ipl + (PER ? PG_MAX_COMP * DMAX : 0);              // [rp][LR_PS]: V of the column tile
    double* ur = vc + rp * LR_PS;                                   // U of the row tile
    double* uc = ur + rp * LR_PS;                                   // symmetric form: U of the column tile
    double* vr = uc + rp * LR_PS;                                   // ... and V of the row tile
    double* xcl = vr + rp * LR_PS;                                  // d > 16: the column points' tile [DMAX][64]
    pair_stage_hp<double, PER>(spec, hp, d, DMAX, DMAX, l2, ipl, tid, 256);
    // a 64-row panel of F (global rows first .. first + 63 of `rows`, factor columns t0 .. t0 + rc - 1) -> LDS [t][LR_PS], zero behind the
    // rows and the columns; every address read is an element of the operand (clamped): gaps are not read
    auto stage_panel = [&](double* dst, const double* __restrict__ F, long ldf, int first, int rows) {
        for (int idx = tid; idx < LR_T * rp; idx += 256) {
            const int p = idx / rp, t = idx % rp;
            const int gi = first + p;
            const double v = F[(long)min(gi, rows - 1) * ldf + t0 + min(t, rc - 1)];
            dst[t * LR_PS + p] = (gi < rows && t < rc) ? v : 0.0;
        }
    };
    stage_panel(vc, V, ldv, tc * LR_T, nc);
    if (sym) stage_panel(uc, U, ldu, tc * LR_T, nc);
    // this lane's column point, for the whole walk: in registers up to d = 16, in LDS beyond (with the accumulators of 32 dimensions the
    // registers do not hold it).  A point past the end is a copy of the last one (its weight is zero): its pairs are finite exactly when
    // that point's are.
    constexpr bool XJ_REG = DMAX <= 16;
    const int j0 = 16 * wave;
    double xj[XJ_REG ? DMAX : 1];
    if constexpr (XJ_REG) {
        const int gj = min(tc * LR_T + j0 + c16, nc - 1);
#pragma unroll
        for (int k = 0; k < DMAX; ++k) xj[k] = (k < d) ? Xc[(long)gj * ldc + min(k, d - 1)] : 0.0;
    } else {
        for (int idx = tid; idx < LR_T * DMAX; idx += 256) {
            const int p = idx / DMAX, k = idx % DMAX;
            const int gc = min(tc * LR_T + p, nc - 1);
            xcl[k * LR_T + p] = (k < d) ? Xc[(long)gc * ldc + k] : 0.0;
        }
    }
    const double* xcj = xcl + j0 + c16;
    auto cj = [&](int k) -> double {
        if constexpr (XJ_REG) return xj[k];
        else return xcj[k * LR_T];
    };


    for (int cp = 0; cp < spec.ncomp; ++cp) {
        const int o = spec.off[cp];
        const double sg = hp[o];
        const double sig2 = sg * sg;
        const double* lc = l2 + cp * DMAX;
        const int kind = spec.kind[cp];
        const double sha = kind_shape2(spec, hp, cp, d), ish = 1.0 / sha;      // rational quadratic: alpha^2, 1 / alpha^2
        double accf = 0.0;                            // ... and its shape entry, sum W K fs
        double acc[DMAX + 1];                         // sigma: sum W K;  l_k: sum W base D_k^2 (the periodic kind: sum W K sin^2)
#pragma unroll
        for (int k = 0; k <= DMAX; ++k) acc[k] = 0.0;
        double accp[PER ? DMAX : 1];                  // the periodic kind's period entries, sum W K sin(2 pi t_k) t_k
#pragma unroll
        for (int k = 0; k < (PER ? DMAX : 1); ++k) accp[k] = 0.0;
        for (int tr = r0; tr < r1; ++tr) {
            __syncthreads();                          // the previous tile's readers (and the previous component's fold) are done
            for (int idx = tid; idx < LR_T * DMAX; idx += 256) {
                const int p = idx / DMAX, k = idx % DMAX;
                const int gr = min(tr * LR_T + p, nr - 1);      // (a row past the end: a copy of the last one, weight zero)
                xr[k * LR_T + p] = (k < d) ? Xr[(long)gr * ldr + k] : 0.0;
            }
            stage_panel(ur, U, ldu, tr * LR_T, nr);
            const bool both = sym && tr != tc;        // off the diagonal of the symmetric form: W_ij + W_ji
            if (both) stage_panel(vr, V, ldv, tr * LR_T, nr);
            __syncthreads();
#pragma unroll 1
            for (int ib = 0; ib < 4; ++ib) {
                const int i0 = 16 * ib;
                pg_d4 wq = {0.0, 0.0, 0.0, 0.0};
                for (int s = 0; s < rp; s += 4)
                    wq = Mfma<double>::run(ur[(s + g) * LR_PS + i0 + c16], vc[(s + g) * LR_PS + j0 + c16], wq);
                if (both)
                    for (int s = 0; s < rp; s += 4)
                        wq = Mfma<double>::run(vr[(s + g) * LR_PS + i0 + c16], uc[(s + g) * LR_PS + j0 + c16], wq);
                // (one pair at a time from d = 9 on: four in flight hold 4 DMAX differences and spill the accumulators)
#pragma unroll(DMAX <= 8 ? 2 : 1)
                for (int q = 0; q < 4; ++q) {
                    const int row = i0 + g + 4 * q;
                    double w = q == 0 ? wq[0] : (q == 1 ? wq[1] : (q == 2 ? wq[2] : wq[3]));
                    if constexpr (PROD) {      // the product rule: the others' values weigh this component's element
                        auto xa = [&](int k) { return xr[k * LR_T + row]; };
                        for (int c2 = 0; c2 < spec.ncomp; ++c2)
                            if (c2 != cp) w *= pair_value<double, DMAX>(spec, hp, c2, d, l2 + c2 * DMAX, ipl + c2 * DMAX, xa, cj);
                    }
                    if constexpr (PER) {
                        if (kind == PG_KIND_PERIODIC) {      // (padding coordinates: l^2 = 1 / p = 0, so t = 0 and both terms vanish)
                            const double* ipc = ipl + cp * DMAX;
                            double sp = 0.0;
#pragma unroll
                            for (int k = 0; k < DMAX; ++k) sp += lc[k] * per_sin2<double>((xr[k * LR_T + row] - cj(k)) * ipc[k]);
                            const double wk = w * kind_value<double, PG_KIND_RBF>(sig2, sp);
                            acc[0] += wk;
#pragma unroll
                            for (int k = 0; k < DMAX; ++k) {
                                const double t = (xr[k * LR_T + row] - cj(k)) * ipc[k];
                                double s2, s2w;
                                per_terms<double>(t, s2, s2w);
                                acc[1 + k] += wk * s2;
                                accp[k] += wk * s2w * t;
                            }
                            continue;
                        }
                    }
                    double sq = 0.0;
#pragma unroll
                    for (int k = 0; k < DMAX; ++k) {
                        const double df = xr[k * LR_T + row] - cj(k);
                        sq += lc[k] * df * df;
                    }
                    double kv, base;   // dK/dl_k = base * l_k * D_k^2 (sign and constants applied in the reduce)
                    if (kind == PG_KIND_RBF) {
                        kv = kind_value<double, PG_KIND_RBF>(sig2, sq);
                        base = kv;
                    } else {
                        double ft;
                        matern_val<double>(kind, sig2, sq, kv, base, sha, ish, ft);
                        accf += w * ft;
                    }
                    acc[0] += w * kv;
                    const double wb = w * base;
#pragma unroll
                    for (int k = 0; k < DMAX; ++k) {
                        const double df = xr[k * LR_T + row] - cj(k);
                        acc[1 + k] += wb * df * df;
                    }
                }
            }
        }
        __syncthreads();                              // (`red` of the previous component has been read)
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
    }
}

long pg_lowrank_grad_worksize_impl(int nr, int nc, int r, int nhp) { return lr_plan(nr, nc, r).nblk * nhp; }

template <int DMAX, bool PER, bool PROD>
static int launch_lowrank_grad(hipStream_t st, const LrPlan& p, const pg_covspec& spec, const double* hp, const double* Xr, long ldr, int nr,
                               const double* Xc, long ldc, int nc, int d, const double* U, long ldu, const double* V, long ldv, int r, int sym,
                               double* part, int pw) {
    // the panels of a full pass need more than the 64 KB a kernel gets without opting in
    if (int rc = pg_lds_opt_in<pg_lowrank_grad_kernel<DMAX, PER, PROD>>(lowrank_lds_bytes<DMAX, PER>(LR_RC))) return rc;
    const long per_chunk = (long)p.nseg * p.tiles_c;
    for (int ch = 0; ch < p.nchunk; ++ch) {      // passes over the factor columns, each into slot rows of its own
        const int t0 = ch * LR_RC, rc = std::min(LR_RC, r - t0);
        const size_t lds = lowrank_lds_bytes<DMAX, PER>((rc + 3) & ~3);
        hipLaunchKernelGGL((pg_lowrank_grad_kernel<DMAX, PER, PROD>), dim3(p.tiles_c, p.nseg), dim3(256), lds, st, spec, hp, Xr, ldr, nr, Xc, ldc,
                           nc, d, U, ldu, V, ldv, t0, rc, sym, part + ch * per_chunk * pw, pw, p.tps, p.tiles_r);
        PG_CHECK(hipGetLastError());
    }
    return 0;
}

int pg_lowrank_grad_impl(hipStream_t st, const pg_covspec& spec_in, const double* hp, const double* Xr, long ldr, int nr, const double* Xc, long ldc,
                         int nc, int d, int sym, const double* U, long ldu, const double* V, long ldv, int r, double* grad, int accumulate,
                         double* work) {
    pg_covspec spec;
    const bool prod = pg_spec_strip(spec_in, spec);
    const int pw = pg_cross_grad_extent(spec, d);
    if (pw == 0) return 0;                            // no stationary component: no entry is this call's
    const LrPlan p = lr_plan(nr, nc, r);
    if (p.nblk > 0) {
        const int rc = pg_with_kinds(spec, prod, [&](auto per_c, auto prod_c) {
            return pg_with_dmax(d, [&](auto dmax_c) {
                return launch_lowrank_grad<decltype(dmax_c)::value, decltype(per_c)::value, decltype(prod_c)::value>(
                    st, p, spec, hp, Xr, ldr, nr, Xc, ldc, nc, d, U, ldu, V, ldv, r, sym, work, pw);
            });
        });
        if (rc) return rc;
    }
    // (r == 0 or an empty point set: an empty sum -- the reduce alone zeroes the spec's entries, or leaves them when accumulating)
    return pg_cross_grad_reduce(st, spec, hp, work, p.nblk, pw, d, grad, accumulate);
}
