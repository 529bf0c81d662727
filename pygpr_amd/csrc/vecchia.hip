// The nearest-neighbour (Vecchia) GP (include/pygpr_hip_vecchia.h): the brute-force neighbour search and the per-target blocks.
//
// pg_knn_kernel       one wavefront per query, VC_KW of them a workgroup.  The candidates travel through LDS 64 at a time, k-major
//                     ([k][64]: lane j reads word j), shared by the workgroup's wavefronts; the query and the scales are read from LDS
//                     as broadcasts.  A wavefront keeps its m best in REGISTERS: lane l holds entry l of the list sorted by (distance,
//                     index); the lanes whose candidate beats entry m - 1 are found by ballot and inserted lowest lane first -- every
//                     lane behind the insertion point takes its left neighbour's entry (one cross-lane move).  No atomics.
//                     Bound by fp64 VALU issue on the distances (three operations a coordinate and pair).
// pg_vecchia_kernel   one wavefront per target, WPB of them a workgroup (as many as 80 KB of LDS hold: two workgroups a CU), each
//                     walking its share of the workgroup's targets.  Per wavefront in LDS: the block's points k-major, the packed lower
//                     triangle of A_B (64 * 65 / 2 doubles), y_B, c, a and the wavefront's running sums.  The pairs (p, q <= p) are
//                     dealt to the lanes in packed order, 64 a step, so a block of b points costs b (b + 1) / 128 evaluations a lane
//                     whatever b is.  Cholesky is left-looking by columns, lane p owning row p; the three substitutions keep their
//                     right-hand side one entry a lane.  The gradient walks the pairs again with the rank-two weight W: a component's
//                     sigma and shape slots are summed in registers, w * base goes back into the triangle (the factor is dead by
//                     then) and the per-coordinate slots are folded from it coordinate by coordinate.  The per-pair forms are kfun.h's
//                     from direct differences, the staging and the slot scales kpair.h's (the NLML's reduce halves them).
//                     Sums over targets: lane 0 of a wavefront adds into its LDS row in target order, the workgroup adds its rows in
//                     wavefront order into its row of `work`, pg_vecchia_fold_kernel adds those in workgroup order.  No atomics.
//                     Bound by LDS latency in the factorisation (b^2 / 2 dependent two-read steps) at b = 64 and by fp64 VALU issue
//                     on the pair evaluations at small b.
#include "kfun.h"
#include "kpair.h"
#include "kbuild.h"
#include "vecchia.h"
#include <climits>

#define VC_KW 4                 // wavefronts (queries) of a pg_knn workgroup
#define VC_TRI 2080             // 64 * 65 / 2: the packed lower triangle of a full block
#define VC_LDS_BYTES 81920      // what a workgroup of the block kernel may take: two of them share a CU's 160 KB
#define VC_MAX_BLOCKS 4096      // workgroups (rows of `work`) of one block-kernel launch

// LDS traffic between the lanes of ONE wavefront: the hardware serves a wavefront's LDS instructions in order; this keeps the
// compiler from moving them across the point
__device__ __forceinline__ void vc_wsync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// the next pair of this lane in packed order: 64 entries further
__device__ __forceinline__ void vc_advance(int& p, int& q) {
    q += 64;
    while (q > p) {
        q -= p + 1;
        ++p;
    }
}

// ------------------------------------------------------------------------------------------------------------------ neighbour search
// (d, j) < (bd, bi) in the order of the list
__device__ __forceinline__ bool vc_less(double d, int j, double bd, int bi) { return d < bd || (d == bd && j < bi); }

__global__ __launch_bounds__(64 * VC_KW) void pg_knn_kernel(const double* __restrict__ Xq, long ldq, int nq, const double* __restrict__ Xc,
                                                             long ldc, int n, int d, const double* __restrict__ s, int m, int causal,
                                                             int* __restrict__ nbr, long ldn) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* xc = reinterpret_cast<double*>(smem_raw);      // [d][64] candidate tile, k-major
    double* xq = xc + 64 * d;                              // [VC_KW][d] the queries
    double* sc = xq + VC_KW * d;                           // [d] the scales
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i0 = blockIdx.x * VC_KW, i = i0 + wave;
    for (int idx = tid; idx < VC_KW * d; idx += 64 * VC_KW) {
        const int w = idx / d, k = idx % d;
        xq[idx] = Xq[(long)min(i0 + w, nq - 1) * ldq + k];
    }
    for (int k = tid; k < d; k += 64 * VC_KW) sc[k] = s ? s[k] : 1.0;
    // candidates of this wavefront: j < lim; of the workgroup: j < wlim
    const int lim = i < nq ? (causal ? min(i, n) : n) : 0;
    const int wlim = causal ? min(min(i0 + VC_KW, nq) - 1, n) : n;
    const int tiles = (wlim + 63) / 64;
    double bd = __builtin_inf();      // entry `lane` of the sorted list; (inf, INT_MAX) = empty
    int bi = INT_MAX;
    const double* myq = xq + wave * d;
    for (int tc = 0; tc < tiles; ++tc) {
        __syncthreads();      // the previous tile's readers (and, the first time, the queries' writers)
        for (int idx = tid; idx < 64 * d; idx += 64 * VC_KW) {
            const int p = idx / d, k = idx % d;
            xc[k * 64 + p] = Xc[(long)min(tc * 64 + p, n - 1) * ldc + k];      // (clamped: a point behind the end is never a candidate)
        }
        __syncthreads();
        const int j = tc * 64 + lane;
        if (tc * 64 >= lim) continue;      // (wave-uniform; the barriers above are met by every wavefront all the same)
        double dist = 0.0;
        for (int k = 0; k < d; ++k) {
            const double df = sc[k] * (myq[k] - xc[k * 64 + lane]);
            dist += df * df;
        }
        double td = __shfl(bd, m - 1, 64);
        int ti = __shfl(bi, m - 1, 64);
        unsigned long long mask = __ballot(j < lim && vc_less(dist, j, td, ti));      // (a NaN distance compares false)
        while (mask) {
            const int b = __builtin_ctzll(mask);
            mask &= mask - 1;
            const double cd = __shfl(dist, b, 64);
            const int cj = tc * 64 + b;
            if (!vc_less(cd, cj, td, ti)) continue;      // the threshold moved since the ballot
            const double ud = __shfl_up(bd, 1, 64);
            const int ui = __shfl_up(bi, 1, 64);
            const bool before = vc_less(bd, bi, cd, cj);                 // this lane's entry stays in front of the candidate
            const bool ubefore = lane == 0 || vc_less(ud, ui, cd, cj);   // ... and so does its left neighbour's
            if (!before) {
                bd = ubefore ? cd : ud;
                bi = ubefore ? cj : ui;
            }
            td = __shfl(bd, m - 1, 64);
            ti = __shfl(bi, m - 1, 64);
        }
    }
    if (i < nq && lane < m) nbr[(long)i * ldn + lane] = bi == INT_MAX ? -1 : bi;
}

int pg_knn_impl(hipStream_t st, const double* Xq, long ldq, int q, const double* Xc, long ldc, int n, int d, const double* s, int m, int causal,
                int* nbr, long ldn) {
    if (q == 0) return 0;
    const size_t lds = (size_t)(64 * d + VC_KW * d + d) * sizeof(double);
    hipLaunchKernelGGL(pg_knn_kernel, dim3((unsigned)((q + VC_KW - 1) / VC_KW)), dim3(64 * VC_KW), lds, st, Xq, ldq, q, Xc, ldc, n, d, s, m, causal,
                       nbr, ldn);
    PG_CHECK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------- the block kernel
// LDS of one wavefront in doubles: the triangle, the points, y_B / c / a, the compacted indices (64 ints), the running sums
// (nhp slots, the loss, the failed index)
static inline int vc_wave_doubles(int d, int nhp) { return VC_TRI + 64 * d + 3 * 64 + 32 + ((nhp + 2 + 1) & ~1); }
static inline int vc_shared_doubles(int d) { return 2 * PG_MAX_COMP * d + 4 * PG_MAX_COMP; }
static inline int vc_wpb(int d, int nhp) {
    const int w = (VC_LDS_BYTES / 8 - vc_shared_doubles(d)) / vc_wave_doubles(d, nhp);
    return std::max(1, std::min(4, w));
}
struct VcPlan {
    int wpb, tpb, nblk, pw;      // wavefronts and targets a workgroup, workgroups, width of a row of `work`
};
static inline VcPlan vc_plan(int count, int d, int nhp) {
    VcPlan p;
    p.wpb = vc_wpb(d, nhp);
    p.pw = nhp + 2;
    const long per = ((long)count + (long)p.wpb * VC_MAX_BLOCKS - 1) / ((long)p.wpb * VC_MAX_BLOCKS);      // targets a wavefront
    p.tpb = (int)std::max(1L, per) * p.wpb;
    p.nblk = (count + p.tpb - 1) / p.tpb;
    return p;
}
long pg_vecchia_worksize_impl(int count, int d, int nhp) {
    const VcPlan p = vc_plan(count, d, nhp);
    return (long)p.nblk * p.pw;
}

// kv, base and fs (kfun.h: kind_eval) of component c at the pair (p, q) of the block's points xs [k][64]
template <bool PER>
__device__ __forceinline__ void vc_eval(const pg_covspec& spec, const double* __restrict__ l2, const double* __restrict__ ipl,
                                        const double* __restrict__ cpar, int c, int d, const double* __restrict__ xs, int p, int q, double& kv,
                                        double& base, double& fs) {
    const double* lc = l2 + c * d;
    const int kind = spec.kind[c];
    const double sig2 = cpar[4 * c];
    fs = 0.0;
    if constexpr (PER) {
        if (kind == PG_KIND_PERIODIC) {
            const double* ipc = ipl + c * d;
            double sq = 0.0;
            for (int k = 0; k < d; ++k) sq += lc[k] * per_sin2<double>((xs[k * 64 + p] - xs[k * 64 + q]) * ipc[k]);
            kv = base = kind_value<double, PG_KIND_RBF>(sig2, sq);
            return;
        }
    }
    double sq = 0.0;
    for (int k = 0; k < d; ++k) {
        const double df = xs[k * 64 + p] - xs[k * 64 + q];
        sq += lc[k] * df * df;
    }
    if (kind == PG_KIND_RBF) kv = base = kind_value<double, PG_KIND_RBF>(sig2, sq);
    else matern_val<double>(kind, sig2, sq, kv, base, cpar[4 * c + 1], cpar[4 * c + 2], fs);
}

// PREDICT: the target's point is row t of Xq, y_last = 0, no jitter on the last diagonal entry, no gradient and no loss
template <bool PER, bool PROD, bool PREDICT>
__global__ __launch_bounds__(256) void pg_vecchia_kernel(pg_covspec spec, const double* __restrict__ hp, int nhp, const double* __restrict__ X,
                                                         long ldx, int n, int d, const double* __restrict__ Y, const double* __restrict__ Xq,
                                                         long ldq, const int* __restrict__ nbr, long ldn, int m, int first, int count,
                                                         double jitter, int want_grad, double* __restrict__ cmean, double* __restrict__ cvar,
                                                         double* __restrict__ part, int tpb, int wave_dbl) {
    static_assert(!PROD || PER, "a product takes the instantiation that carries every kind");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63, nthr = blockDim.x, wpb = nthr >> 6;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pw = nhp + 2;
    double* l2 = reinterpret_cast<double*>(smem_raw);      // [ncomp][d] squared inverse length scales
    double* ipl = l2 + PG_MAX_COMP * d;                    // [ncomp][d] reciprocal periods (0 for the other kinds)
    double* cpar = ipl + PG_MAX_COMP * d;                  // [ncomp][4]: sigma^2, the squared shape, its reciprocal
    double* mine = cpar + 4 * PG_MAX_COMP + (long)wave * wave_dbl;
    double* L = mine;                                      // the packed lower triangle: entry (p, q <= p) at p (p + 1) / 2 + q
    double* xs = L + VC_TRI;                               // [d][64] the block's points
    double* yb = xs + 64 * d;                              // [64] y_B
    double* cs = yb + 64;                                  // [64] c
    double* as = cs + 64;                                  // [64] a
    int* idxs = reinterpret_cast<int*>(as + 64);           // [64] the valid neighbours, compacted
    double* gacc = as + 64 + 32;                           // [pw] this wavefront's sums: hp slots, the loss, the lowest failed index
    if constexpr (PER) pair_stage_hp<double, true>(spec, hp, d, d, d, l2, ipl, tid, nthr);
    else pair_stage_hp<double, false>(spec, hp, d, d, d, l2, ipl, tid, nthr);
    if (tid < spec.ncomp) {
        const double sg = hp[spec.off[tid]], sh = kind_shape2(spec, hp, tid, d);
        cpar[4 * tid] = sg * sg;
        cpar[4 * tid + 1] = sh;
        cpar[4 * tid + 2] = 1.0 / sh;
    }
    for (int u = lane; u < pw; u += 64) gacc[u] = u == nhp + 1 ? 1.0e300 : 0.0;
    double noise2 = 0.0;
    for (int u = 0; u < spec.nnoise; ++u) noise2 += hp[spec.noise_off[u]] * hp[spec.noise_off[u]];
    __syncthreads();

    const int t0 = blockIdx.x * tpb, t1 = min(t0 + tpb, count);
    for (int t = t0 + wave; t < t1; t += wpb) {
        // ---- the block: valid neighbours in their order, then the target
        const int jn = lane < m ? nbr[(long)t * ldn + lane] : -1;
        const bool valid = jn >= 0 && jn < n;
        const unsigned long long vm = __ballot(valid);
        const int nv = __builtin_popcountll(vm), b = nv + 1;
        if (valid) idxs[__builtin_popcountll(vm & ((1ull << lane) - 1ull))] = jn;
        vc_wsync();
        if (lane < b) {
            const double* src = lane < nv ? X + (long)idxs[lane] * ldx : (PREDICT ? Xq + (long)t * ldq : X + (long)(first + t) * ldx);
            for (int k = 0; k < d; ++k) xs[k * 64 + lane] = src[k];
            yb[lane] = lane < nv ? Y[idxs[lane]] : (PREDICT ? 0.0 : Y[first + t]);
        }
        vc_wsync();
        // ---- A_B, 64 pairs a step
        const int npair = b * (b + 1) / 2;
        {
            int p = 0, q = lane;
            while (q > p) { q -= p + 1; ++p; }
            for (int e = lane; e < npair; e += 64) {
                double val = PROD ? 1.0 : 0.0;
                for (int c = 0; c < spec.ncomp; ++c) {
                    double kv, bs, fs;
                    vc_eval<PER>(spec, l2, ipl, cpar, c, d, xs, p, q, kv, bs, fs);
                    val = PROD ? val * kv : val + kv;
                }
                if (spec.ncomp == 0) val = 0.0;
                if (p == q) val += (PREDICT && p == nv) ? noise2 : noise2 + jitter;
                L[e] = val;
                vc_advance(p, q);
            }
        }
        vc_wsync();
        // ---- Cholesky in place, left-looking: lane p owns row p
        double* rowp = L + lane * (lane + 1) / 2;
        bool failed = false;
        for (int j = 0; j < b; ++j) {
            const double* rowj = L + j * (j + 1) / 2;
            double acc = 0.0;
            if (lane >= j && lane < b) {
                acc = rowp[j];
#pragma unroll 4
                for (int k = 0; k < j; ++k) acc -= rowp[k] * rowj[k];
            }
            const double piv = __shfl(acc, j, 64);
            failed = failed || !(piv > 0.0);
            const double sd = sqrt(piv);
            if (lane >= j && lane < b) rowp[j] = lane == j ? sd : acc / sd;
            vc_wsync();
        }
        const double lll = L[nv * (nv + 1) / 2 + nv];      // L_last,last: v = its square
        const double v = lll * lll;
        // ---- c: L^T c = L_ll e_last, so c_last = 1
        double cl = 0.0, al = 0.0;
        {
            double rhs = lane == nv ? lll : 0.0;
            for (int j = nv; j >= 0; --j) {
                const double* rowj = L + j * (j + 1) / 2;
                const double cj = __shfl(rhs, j, 64) / rowj[j];
                if (lane == j) cl = cj;
                if (lane < j) rhs -= rowj[lane] * cj;
            }
        }
        // ---- a = [A_NN^-1 y_N ; 0]: the leading block of the same factor, forward then backward
        if (PREDICT ? false : want_grad != 0) {
            double rhs = lane < nv ? yb[lane] : 0.0, w = 0.0;
            for (int j = 0; j < nv; ++j) {
                const double wj = __shfl(rhs, j, 64) / L[j * (j + 1) / 2 + j];
                if (lane == j) w = wj;
                if (lane > j && lane < nv) rhs -= rowp[j] * wj;
            }
            rhs = w;
            for (int j = nv - 1; j >= 0; --j) {
                const double* rowj = L + j * (j + 1) / 2;
                const double aj = __shfl(rhs, j, 64) / rowj[j];
                if (lane == j) al = aj;
                if (lane < j) rhs -= rowj[lane] * aj;
            }
        }
        const double r = wave_sum(lane < b ? cl * yb[lane] : 0.0);
        const double nanv = __builtin_nan("");
        if (lane == 0) {
            const double ylast = yb[nv];
            cmean[t] = failed ? nanv : ylast - r;
            if (cvar) cvar[t] = failed ? nanv : v;
            if (failed) gacc[nhp + 1] = fmin(gacc[nhp + 1], (double)(first + t));
            if constexpr (!PREDICT) gacc[nhp] += failed ? nanv : 0.5 * (log(v) + r * r / v + 1.8378770664093454836);
        }
        // ---- the gradient: W = alpha c c^T - beta (a c^T + c a^T) against the per-pair derivative forms
        if constexpr (!PREDICT) {
            if (want_grad) {
                const double beta = failed ? nanv : r / v, alpha = 1.0 / v - beta * beta;
                cs[lane] = lane < b ? cl : 0.0;
                as[lane] = lane < b ? al : 0.0;
                const double wpp = wave_sum(lane < b ? alpha * cl * cl - 2.0 * beta * al * cl : 0.0);      // sum_p W_pp: the noise entries
                if (lane == 0)
                    for (int u = 0; u < spec.nnoise; ++u) gacc[spec.noise_off[u]] += wpp;
                vc_wsync();      // (also: the factor's last readers are done, the triangle is free)
                for (int cp = 0; cp < spec.ncomp; ++cp) {
                    const int o = spec.off[cp], kind = spec.kind[cp];
                    double acc0 = 0.0, accf = 0.0;      // sum W K (sigma), sum W K fs (the shape)
                    int p = 0, q = lane;
                    while (q > p) { q -= p + 1; ++p; }
                    for (int e = lane; e < npair; e += 64) {
                        double w = alpha * cs[p] * cs[q] - beta * (as[p] * cs[q] + cs[p] * as[q]);
                        w = p == q ? w : 2.0 * w;      // the pair and its mirror image
                        if constexpr (PROD) {          // the product rule: the others' values weigh this component's element
                            for (int c2 = 0; c2 < spec.ncomp; ++c2)
                                if (c2 != cp) {
                                    double k2, b2, f2;
                                    vc_eval<PER>(spec, l2, ipl, cpar, c2, d, xs, p, q, k2, b2, f2);
                                    w *= k2;
                                }
                        }
                        double kv, bs, fs;
                        vc_eval<PER>(spec, l2, ipl, cpar, cp, d, xs, p, q, kv, bs, fs);
                        acc0 += w * kv;
                        accf += w * fs;
                        L[e] = w * bs;      // (the periodic kind: base = K)
                        vc_advance(p, q);
                    }
                    acc0 = wave_sum(acc0);
                    accf = wave_sum(accf);
                    if (lane == 0) {
                        gacc[o] += acc0;
                        if (kind == PG_KIND_RQ) gacc[o + d + 1] += accf;
                    }
                    vc_wsync();
                    for (int k = 0; k < d; ++k) {      // l_k: sum W base D_k^2 (periodic: sum W K sin^2; its period: sum W K sin(2 pi t) t)
                        double sl = 0.0, sp = 0.0;
                        p = 0, q = lane;
                        while (q > p) { q -= p + 1; ++p; }
                        for (int e = lane; e < npair; e += 64) {
                            const double df = xs[k * 64 + p] - xs[k * 64 + q];
                            bool done = false;
                            if constexpr (PER) {
                                if (kind == PG_KIND_PERIODIC) {
                                    const double tt = df * ipl[cp * d + k];
                                    double s2, s2w;
                                    per_terms<double>(tt, s2, s2w);
                                    sl += L[e] * s2;
                                    sp += L[e] * s2w * tt;
                                    done = true;
                                }
                            }
                            if (!done) sl += L[e] * df * df;
                            vc_advance(p, q);
                        }
                        sl = wave_sum(sl);
                        if (lane == 0) gacc[o + 1 + k] += sl;
                        if constexpr (PER) {
                            if (kind == PG_KIND_PERIODIC) {
                                sp = wave_sum(sp);
                                if (lane == 0) gacc[o + d + 1 + k] += sp;
                            }
                        }
                    }
                    vc_wsync();
                }
            }
        }
        vc_wsync();      // this target's readers before the next one's writers
    }
    __syncthreads();
    // the wavefronts' rows in their order
    for (int u = tid; u < pw; u += nthr) {
        const double* g0 = cpar + 4 * PG_MAX_COMP + (VC_TRI + 64 * d + 3 * 64 + 32);
        double sum = g0[u];
        for (int w = 1; w < wpb; ++w) {
            const double x = g0[(long)w * wave_dbl + u];
            sum = u == nhp + 1 ? fmin(sum, x) : sum + x;
        }
        part[(long)blockIdx.x * pw + u] = sum;
    }
}

// out, grad, info from the workgroups' rows in workgroup order; the slot scales are kpair.h's, halved (the NLML's 1/2), a noise
// entry's is sigma_n (1/2 * 2 sigma_n); an entry of hp that nothing owns gets 0
__global__ __launch_bounds__(256) void pg_vecchia_fold_kernel(pg_covspec spec, const double* __restrict__ hp, int nhp, int d,
                                                              const double* __restrict__ part, int nblk, double* __restrict__ out,
                                                              double* __restrict__ grad, int* __restrict__ info) {
    const int pw = nhp + 2;
    for (int u = threadIdx.x; u < pw; u += 256) {
        if (u < nhp && !grad) continue;
        if (u == nhp && !out) continue;
        double s = u == nhp + 1 ? 1.0e300 : 0.0;
        for (int b = 0; b < nblk; ++b) {
            const double x = part[(long)b * pw + u];
            s = u == nhp + 1 ? fmin(s, x) : s + x;
        }
        if (u == nhp + 1) info[0] = s < 1.0e299 ? 1 + (int)s : 0;
        else if (u == nhp) out[0] = s;
        else {
            double scale = 0.0;
            bool mine = false;
            for (int c = 0; c < spec.ncomp; ++c) {
                bool hit = false;
                const double sc = kind_entry_scale(spec, hp, c, u, d, hit);
                if (hit) { scale = 0.5 * sc; mine = true; }
            }
            for (int c = 0; c < spec.nnoise; ++c)
                if (spec.noise_off[c] == u) { scale = hp[u]; mine = true; }
            grad[u] = mine ? scale * s : 0.0;
        }
    }
}

template <bool PER, bool PROD, bool PREDICT>
static int launch_vecchia(hipStream_t st, const VcPlan& p, const pg_covspec& spec, const double* hp, int nhp, const double* X, long ldx, int n, int d,
                          const double* Y, const double* Xq, long ldq, const int* nbr, long ldn, int m, int first, int count, double jitter,
                          int want_grad, double* cmean, double* cvar, double* part) {
    if (int rc = pg_lds_opt_in<pg_vecchia_kernel<PER, PROD, PREDICT>>(VC_LDS_BYTES)) return rc;      // beyond the 64 KB a kernel gets without opting in
    const int wave_dbl = vc_wave_doubles(d, nhp);
    const size_t lds = (size_t)(vc_shared_doubles(d) + (long)p.wpb * wave_dbl) * sizeof(double);
    hipLaunchKernelGGL((pg_vecchia_kernel<PER, PROD, PREDICT>), dim3(p.nblk), dim3(64 * p.wpb), lds, st, spec, hp, nhp, X, ldx, n, d, Y, Xq, ldq,
                       nbr, ldn, m, first, count, jitter, want_grad, cmean, cvar, part, p.tpb, wave_dbl);
    PG_CHECK(hipGetLastError());
    return 0;
}

template <bool PREDICT>
static int vecchia_run(hipStream_t st, const pg_covspec& spec_in, const double* hp, int nhp, const double* X, long ldx, int n, int d, const double* Y,
                       const double* Xq, long ldq, const int* nbr, long ldn, int m, int first, int count, double jitter, int want_grad,
                       double* cmean, double* cvar, double* out, double* grad, int* info, double* work) {
    pg_covspec spec;
    const bool prod = pg_spec_strip(spec_in, spec);
    const VcPlan p = vc_plan(count, d, nhp);
    if (p.nblk > 0) {
        const int rc = pg_with_kinds(spec, prod, [&](auto per_c, auto prod_c) {
            return launch_vecchia<decltype(per_c)::value, decltype(prod_c)::value, PREDICT>(st, p, spec, hp, nhp, X, ldx, n, d, Y, Xq, ldq, nbr, ldn, m,
                                                                                             first, count, jitter, want_grad, cmean, cvar, work);
        });
        if (rc) return rc;
    }
    hipLaunchKernelGGL(pg_vecchia_fold_kernel, dim3(1), dim3(256), 0, st, spec, hp, nhp, d, work, p.nblk, out, want_grad ? grad : nullptr, info);
    PG_CHECK(hipGetLastError());
    return 0;
}

int pg_vecchia_nlml_grad_impl(hipStream_t st, const pg_covspec& spec, const double* hp, int nhp, const double* X, long ldx, int n, int d,
                              const double* Y, const int* nbr, long ldn, int m, int first, int count, double jitter, int want_grad,
                              double* cmean, double* cvar, double* out, double* grad, int* info, double* work) {
    return vecchia_run<false>(st, spec, hp, nhp, X, ldx, n, d, Y, nullptr, 0, nbr, ldn, m, first, count, jitter, want_grad, cmean, cvar, out, grad,
                              info, work);
}

int pg_vecchia_predict_impl(hipStream_t st, const pg_covspec& spec, const double* hp, const double* X, long ldx, int n, int d, const double* Y,
                            const double* Xq, long ldq, int q, const int* nbr, long ldn, int m, double jitter, double* mean, double* var,
                            int* info, double* work) {
    return vecchia_run<true>(st, spec, hp, 0, X, ldx, n, d, Y, Xq, ldq, nbr, ldn, m, 0, q, jitter, 0, mean, var, nullptr, nullptr, info, work);
}
