#pragma once
#include "common.h"
#include "pygpr_hip_matmul.h"
#include <algorithm>

// kmatmul.hip: OUT = k(Xr, Xc) V (+ shift V in the symmetric form) without writing K; see pg_kernel_matmul
long pg_kmatmul_worksize_impl(int nr, int nc, int nrhs);
int pg_kmatmul_impl(hipStream_t st, const pg_covspec& spec, const double* hp, const double* Xr, long ldr, int nr, const double* Xc, long ldc,
                    int nc, int d, int sym, const double* V, long ldv, int nrhs, double jitter, double* OUT, long ldo, double* work);

// The tiling and the plan, shared with fmatmul.hip (pg_feature_matmul: the same walk with a feature as the "column point")
#define MM_T 64          // tile edge: rows of OUT per workgroup, column points per step of the walk
#define MM_PANEL 16      // right-hand sides of one matrix instruction
#define MM_BLOCK 32      // right-hand sides of one pass over the pairs (two panels)
#define MM_TARGET 512    // workgroups wanted before the column range is left whole: two per compute unit of a 256-CU part, a constant so
                         // that the order of the sum depends on the shape alone
#define MM_SEGMIN 4      // column tiles a segment holds at least

struct MmPlan {
    int tiles_r, tiles_c, nblk, nseg, tps;      // tps: column tiles per segment
};
static inline MmPlan mm_plan(int nr, int nc, int nrhs) {
    MmPlan p;
    p.tiles_r = (nr + MM_T - 1) / MM_T;
    p.tiles_c = (nc + MM_T - 1) / MM_T;
    p.nblk = (nrhs + MM_BLOCK - 1) / MM_BLOCK;
    p.nseg = p.tiles_c > 0 ? 1 : 0;
    p.tps = p.tiles_c;
    const long wg = (long)p.tiles_r * p.nblk;
    if (wg > 0 && wg < MM_TARGET && p.tiles_c >= 2 * MM_SEGMIN) {
        const long want = (MM_TARGET + wg - 1) / wg;
        const long s = std::min<long>(want, p.tiles_c / MM_SEGMIN);
        p.tps = (int)((p.tiles_c + s - 1) / s);
        p.nseg = (p.tiles_c + p.tps - 1) / p.tps;
    }
    return p;
}

// one panel when sixteen columns hold every right-hand side, two otherwise: f(std::integral_constant<int, NB>{})
template <class F> static inline int mm_with_nb(int nrhs, F f) {
    return nrhs <= MM_PANEL ? f(std::integral_constant<int, 1>{}) : f(std::integral_constant<int, 2>{});
}

// OUT[i][c] = sum_{seg < p.nseg} part[seg][c / 32][i][c % 32] for i < nr, c < nrhs, the segments in their order (nseg = 0: zeros);
// part is laid out [nseg][nblk][tiles_r * 64][MM_BLOCK] as the product kernels write it
int pg_kmatmul_fold_plain(hipStream_t st, const MmPlan& p, const double* part, int nr, int nrhs, double* OUT, long ldo);
