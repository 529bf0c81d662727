// Greedy conditional-variance selection of inducing points (include/pygpr_hip_select.h): the partial pivoted Cholesky factorisation of
// k(X, X).  Step j forms, for every point i,  l_i = (k(x_i, x_p) - sum_{t < j} L[i][t] L[p][t]) / sqrt(r_p)  against the pivot p, updates
// the residual r_i -= l_i^2 and finds the next pivot, the largest residual.  Strictly sequential in j; per step a mat-vec against the
// factor so far, bound by the factor's traffic (8 n j bytes): no matrix-pipe work.
//   factor   L[t][i], one column per pivot with the points contiguous, columns ldl = n rounded up to even apart and 16-byte aligned: a
//            wave reads two points per lane, 1 KB of consecutive words per column
//   step     one workgroup per 128 points, four waves: wave w takes the columns t = w, w + 4, ... of the inner product (eight loads in
//            flight per lane), the four partial sums meet in LDS in wave order, then one thread per point evaluates k from direct
//            differences (kfun.h; sel_value: kpair.h's pair_value with loops to the run-time d), stores l_i and the residual, and the
//            workgroup writes its (max, index, sum)
//   fold     one workgroup folds the partials (tie: lowest index; a NaN is never a maximum; sums in a fixed order), records piv[j],
//            trace[j] and count, tests the next pivot against the floor and gathers its row of the factor for the next step
// The steps are ordinary launches on one stream: no flags, no spinning, no atomics.  All m_max steps are enqueued at once; after the
// stop the remaining launches see the stop word and return.
#include "kfun.h"
#include "kpair.h"
#include "kbuild.h"
#include "select.h"
#include <climits>
#include <cmath>

#define SEL_PTS 128      // points of one workgroup (64 lanes x 2)
#define SEL_WG 256       // its threads: four waves split the columns of the inner product
#define SEL_UN 8         // column loads one lane keeps in flight

typedef double pg_d2 __attribute__((ext_vector_type(2)));

// state words behind the pivot row (doubles): the pivot of the coming step, its residual, the stop word
#define SEL_PIVOT 0
#define SEL_RP 1
#define SEL_STOP 2
#define SEL_NSTATE 8

struct SelWork {
    double* L; long ldl;                    // the factor [m_max][ldl]
    double* r;                              // the residuals [n]
    double *pmax, *pidx, *psum; int nwg;    // per-workgroup partials
    double* prow;                           // the pivot's row of the factor [m_max]
    double* state;
};

__device__ __forceinline__ void sel_take(double& v, int& i, double v2, int i2) {      // the larger value; a tie takes the lower index
    if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
}

// (max, index, sum) of one workgroup from every thread's (v, vi, s); threads without a point bring (-inf, INT_MAX, 0).  All SEL_WG
// threads call it.
__device__ __forceinline__ void sel_partials(double v, int vi, double s, double* __restrict__ pmax, double* __restrict__ pidx,
                                             double* __restrict__ psum) {
    __shared__ double sv[4], ss[4];
    __shared__ int si[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sel_take(v, vi, __shfl_xor(v, o, 64), __shfl_xor(vi, o, 64));
    s = wave_sum(s);
    if (lane == 0) { sv[wave] = v; si[wave] = vi; ss[wave] = s; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) sel_take(v, vi, sv[w], si[w]);
        pmax[blockIdx.x] = v;
        pidx[blockIdx.x] = (double)vi;
        psum[blockIdx.x] = ((ss[0] + ss[1]) + ss[2]) + ss[3];
    }
}

// r_i = kdiag, the first partials, the stop word cleared
__global__ __launch_bounds__(SEL_WG) void pg_select_init_kernel(pg_covspec spec, int prod, const double* __restrict__ hp, int n, SelWork w) {
    double kdiag = prod ? 1.0 : 0.0;
    for (int c = 0; c < spec.ncomp; ++c) {
        const double sg = hp[spec.off[c]];
        kdiag = prod ? kdiag * (sg * sg) : kdiag + sg * sg;
    }
    const int tid = threadIdx.x;
    if (blockIdx.x == 0 && tid == 0) w.state[SEL_STOP] = 0.0;
    const long i = (long)blockIdx.x * SEL_PTS + tid;
    double v = -INFINITY, s = 0.0;
    int vi = INT_MAX;
    if (tid < SEL_PTS && i < n) {
        w.r[i] = kdiag;
        s = kdiag;
        if (kdiag > v) { v = kdiag; vi = (int)i; }
    }
    sel_partials(v, vi, s, w.pmax, w.pidx, w.psum);
}

// component c at (x_i, the pivot): kpair.h's pair_value on a point in global memory and the pivot in LDS, with loops to the run-time d
// (one kernel for every dimension: the step is bound by the factor's traffic, not by these d operations per point)
__device__ __forceinline__ double sel_value(const pg_covspec& spec, const double* __restrict__ hp, int c, int d, const double* __restrict__ xi,
                                            const double* xp, const double* lc, const double* ipc) {
    const int kind = spec.kind[c];
    const double sg = hp[spec.off[c]];
    const double sig2 = sg * sg;
    double sq = 0.0;
    if (kind == PG_KIND_PERIODIC) {
        for (int k = 0; k < d; ++k) sq += lc[k] * per_sin2<double>((xi[k] - xp[k]) * ipc[k]);
        return kind_value<double, PG_KIND_RBF>(sig2, sq);
    }
    for (int k = 0; k < d; ++k) {
        const double df = xi[k] - xp[k];
        sq += lc[k] * df * df;
    }
    if (kind == PG_KIND_RBF) return kind_value<double, PG_KIND_RBF>(sig2, sq);
    const double sh = kind_shape2(spec, hp, c, d);
    double kt, bt, ft;
    matern_val<double>(kind, sig2, sq, kt, bt, sh, 1.0 / sh, ft);
    return kt;
}

__global__ __launch_bounds__(SEL_WG) void pg_select_step_kernel(pg_covspec spec, int prod, const double* __restrict__ hp,
                                                                const double* __restrict__ X, long ldx, int n, int d, int j, SelWork w) {
    if (w.state[SEL_STOP] != 0.0) return;
    __shared__ double xp[PG_MAX_DIM];                       // the pivot's coordinates
    __shared__ double l2[PG_MAX_COMP * PG_MAX_DIM];         // squared inverse length scales per component
    __shared__ double ipl[PG_MAX_COMP * PG_MAX_DIM];        // reciprocal periods of the periodic components
    __shared__ double red[4 * SEL_PTS];                     // the waves' partial inner products
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int p = (int)w.state[SEL_PIVOT];
    const double rp = w.state[SEL_RP];
    for (int k = tid; k < d; k += SEL_WG) xp[k] = X[(long)p * ldx + k];
    pair_stage_hp<double, true>(spec, hp, d, d, PG_MAX_DIM, l2, ipl, tid, SEL_WG);
    // sum_{t < j, t = wave mod 4} L[t][i] L[t][p] for the lane's two points (n odd: the last lane's second point is padding, read and dropped)
    const long i0 = (long)blockIdx.x * SEL_PTS + 2 * lane;
    double ax = 0.0, ay = 0.0;
    if (i0 < n) {
        const double* col = w.L + i0;
        const double* __restrict__ prow = w.prow;
        int t = wave;
        for (; t + 4 * (SEL_UN - 1) < j; t += 4 * SEL_UN) {
            pg_d2 v[SEL_UN];
            double q[SEL_UN];
#pragma unroll
            for (int u = 0; u < SEL_UN; ++u) {
                v[u] = *reinterpret_cast<const pg_d2*>(col + (long)(t + 4 * u) * w.ldl);
                q[u] = prow[t + 4 * u];
            }
#pragma unroll
            for (int u = 0; u < SEL_UN; ++u) {
                ax = __builtin_fma(v[u].x, q[u], ax);
                ay = __builtin_fma(v[u].y, q[u], ay);
            }
        }
        for (; t < j; t += 4) {
            const pg_d2 v = *reinterpret_cast<const pg_d2*>(col + (long)t * w.ldl);
            const double q = prow[t];
            ax = __builtin_fma(v.x, q, ax);
            ay = __builtin_fma(v.y, q, ay);
        }
    }
    red[wave * SEL_PTS + 2 * lane] = ax;
    red[wave * SEL_PTS + 2 * lane + 1] = ay;
    __syncthreads();
    // one thread per point: the column entry, the residual, the candidate
    const long i = (long)blockIdx.x * SEL_PTS + tid;
    double v = -INFINITY, s = 0.0;
    int vi = INT_MAX;
    if (tid < SEL_PTS && i < n) {
        const double dot = ((red[tid] + red[SEL_PTS + tid]) + red[2 * SEL_PTS + tid]) + red[3 * SEL_PTS + tid];
        const double* xi = X + i * ldx;
        double kv = prod ? 1.0 : 0.0;
        for (int c = 0; c < spec.ncomp; ++c) {
            const double val = sel_value(spec, hp, c, d, xi, xp, l2 + c * PG_MAX_DIM, ipl + c * PG_MAX_DIM);
            kv = prod ? kv * val : kv + val;
        }
        const double li = (kv - dot) / sqrt(rp);
        w.L[(long)j * w.ldl + i] = li;
        double rn = w.r[i] - li * li;
        if (i == p) rn = 0.0;
        w.r[i] = rn;
        s = rn;
        if (rn > v) { v = rn; vi = (int)i; }
    }
    sel_partials(v, vi, s, w.pmax, w.pidx, w.psum);
}

// j >= 0: record step j (piv, trace, count), then -- unless it was the last -- test the next pivot against the floor and gather its row;
// j = -1: the first pivot from the initial partials (count = 0, nothing to record or gather)
__global__ __launch_bounds__(256) void pg_select_fold_kernel(int j, int last, double floor, SelWork w, int* __restrict__ piv,
                                                             int* __restrict__ count, double* __restrict__ trace) {
    if (w.state[SEL_STOP] != 0.0) return;
    __shared__ double sv[4], ss[4];
    __shared__ int si[4];
    __shared__ int next;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double v = -INFINITY, s = 0.0;
    int vi = INT_MAX;
    for (int b = tid; b < w.nwg; b += 256) {
        sel_take(v, vi, w.pmax[b], (int)w.pidx[b]);
        s += w.psum[b];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sel_take(v, vi, __shfl_xor(v, o, 64), __shfl_xor(vi, o, 64));
    s = wave_sum(s);
    if (lane == 0) { sv[wave] = v; si[wave] = vi; ss[wave] = s; }
    __syncthreads();
    if (tid == 0) {
        for (int q = 1; q < 4; ++q) sel_take(v, vi, sv[q], si[q]);
        if (j >= 0) {
            piv[j] = (int)w.state[SEL_PIVOT];
            trace[j] = ((ss[0] + ss[1]) + ss[2]) + ss[3];
            count[0] = j + 1;
        } else {
            count[0] = 0;
        }
        int nx = -1;
        if (!last) {
            if (vi != INT_MAX && v > floor) {
                w.state[SEL_PIVOT] = (double)vi;
                w.state[SEL_RP] = v;
                nx = vi;
            } else {
                w.state[SEL_STOP] = 1.0;
            }
        }
        next = nx;
    }
    __syncthreads();
    const int p = next;
    if (p < 0) return;
    for (int t = tid; t <= j; t += 256) w.prow[t] = w.L[(long)t * w.ldl + p];
}

__global__ __launch_bounds__(256) void pg_select_resid_kernel(int n, const double* __restrict__ r, double* __restrict__ resid) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) resid[i] = r[i];
}

static inline long sel_ldl(int n) { return ((long)n + 1) & ~1L; }
static inline long sel_nwg(int n) { return ((long)n + SEL_PTS - 1) / SEL_PTS; }

long pg_greedy_select_worksize_impl(int n, int m_max) {
    // one word to align the columns, the factor, the residuals, three partials per workgroup, the pivot row, the state words
    return 1 + (long)m_max * sel_ldl(n) + n + 3 * sel_nwg(n) + m_max + SEL_NSTATE;
}

int pg_greedy_select_impl(hipStream_t st, const pg_covspec& spec_in, const double* hp, const double* X, long ldx, int n, int d, int m_max,
                          double floor, int* piv, int* count, double* trace, double* resid, double* work) {
    pg_covspec spec;
    const int prod = pg_spec_strip(spec_in, spec) ? 1 : 0;
    spec.nnoise = 0;
    if (m_max == 0) {      // (n == 0 included) no pivot: count alone
        PG_CHECK(hipMemsetAsync(count, 0, sizeof(int), st));
        return 0;
    }
    SelWork w;
    w.ldl = sel_ldl(n);
    w.nwg = (int)sel_nwg(n);
    w.L = work + ((reinterpret_cast<uintptr_t>(work) & 15) ? 1 : 0);
    w.r = w.L + (long)m_max * w.ldl;
    w.pmax = w.r + n;
    w.pidx = w.pmax + w.nwg;
    w.psum = w.pidx + w.nwg;
    w.prow = w.psum + w.nwg;
    w.state = w.prow + m_max;
    hipLaunchKernelGGL(pg_select_init_kernel, dim3(w.nwg), dim3(SEL_WG), 0, st, spec, prod, hp, n, w);
    PG_CHECK(hipGetLastError());
    hipLaunchKernelGGL(pg_select_fold_kernel, dim3(1), dim3(256), 0, st, -1, 0, floor, w, piv, count, trace);
    PG_CHECK(hipGetLastError());
    for (int j = 0; j < m_max; ++j) {
        hipLaunchKernelGGL(pg_select_step_kernel, dim3(w.nwg), dim3(SEL_WG), 0, st, spec, prod, hp, X, ldx, n, d, j, w);
        PG_CHECK(hipGetLastError());
        hipLaunchKernelGGL(pg_select_fold_kernel, dim3(1), dim3(256), 0, st, j, j == m_max - 1 ? 1 : 0, floor, w, piv, count, trace);
        PG_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(pg_select_resid_kernel, dim3((unsigned)(((long)n + 255) / 256)), dim3(256), 0, st, n, w.r, resid);
    PG_CHECK(hipGetLastError());
    return 0;
}
