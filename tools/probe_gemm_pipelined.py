"""The software-pipelined four-wave fp64 tile (variants 14-17, _lib.PIPELINED) against today's form of the same launch, in one process:
uniform NT / NN / TN / TT at 8192^3, the five large products of an N = 16384 evaluation (tools/probe_big_products.py) and a K sweep of
the lower-tile update.  Old and new alternate, REPS times each; per row: the old form's min / median / spread (max - min), the new
form's, and whether the two results are the same bits.  TFLOP/s over the tile-granular flop of the launch, from the minimum.

    python tools/probe_gemm_pipelined.py [pad] [reps]        (leading dimension 16384 + pad, default 16; reps default 5)"""
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pygpr_amd import _lib
from pygpr_amd._lib import GEMM_NN, GEMM_NT, GEMM_TN, GEMM_TT
from pygpr_amd._ops import get_ops

ops = get_ops()
PAD = int(sys.argv[1]) if len(sys.argv) > 1 else 16
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5


def raw(var, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc, tri=0, klo=0, khi=0):
    _lib.check(ops.lib.pg_gemm_raw(ops.h, _lib.PG_F64, var, m, n, k, float(alpha), C.c_void_p(a), lda, C.c_void_p(b), ldb, float(beta),
                                   C.c_void_p(c), ldc, tri, klo, khi, ops._st()), "gemm_raw")


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b)


def row(name, flop, call, out, var, lower=False):
    """call(variant, klo_bits): one launch with beta = 0 into `out` (a tensor view); old form first, then alternating."""
    old, new = (lambda: call(var, 8)), (lambda: call(_lib.PIPELINED[var], 0))      # (klo | 8: the variant's own form, no routing)
    low = (lambda x: x.tril()) if lower else (lambda x: x)      # (tri: what lies above the diagonal inside diagonal tiles is unspecified)
    old(); torch.cuda.synchronize(); ref = low(out).clone()
    new(); torch.cuda.synchronize(); same = torch.equal(ref.view(torch.int64), low(out).view(torch.int64))
    del ref
    to, tn = [], []
    for _ in range(REPS):
        to.append(once(old)); tn.append(once(new))
    f = lambda ts: "%7.3f %7.3f %6.3f" % (min(ts), statistics.median(ts), max(ts) - min(ts))
    print("%-46s old %s  %5.1f TF | new %s  %5.1f TF | gain %+5.1f %%  bits %s" % (
        name, f(to), flop / min(to) / 1e9, f(tn), flop / min(tn) / 1e9, 100.0 * (min(to) / min(tn) - 1.0), "same" if same else "DIFFER"), flush=True)


print("columns: min ms, median ms, max - min ms over %d alternating repeats; ld = 16384 + %d" % (REPS, PAD), flush=True)
N, h = 16384, 8192
ld = N + PAD
A = torch.randn(N, ld, device="cuda", dtype=torch.float64) * 1e-3
M = torch.randn(N, ld, device="cuda", dtype=torch.float64) * 1e-3
a, m = A.data_ptr(), M.data_ptr()
off = lambda r, c: (r * ld + c) * 8

# uniform 8192^3: operands the top-left blocks of M, result the top-left block of A
for name, var in (("NT", GEMM_NT), ("NN", GEMM_NN), ("TN", GEMM_TN), ("TT", GEMM_TT)):
    row("uniform %s 8192^3" % name, 2.0 * h ** 3, lambda v, x: raw(v, h, h, h, 1.0, m, ld, m + off(h, 0), ld, 0.0, a, ld, 0, x, 0), A[:h, :h], var)

M.tril_()    # (the K-range modes multiply triangular operands: the per-wave skip inside diagonal tiles relies on the zeros)
t = h // 128
fl_tri_k = 2.0 * 128 ** 3 * sum(j + 1 for j in range(t)) * t
T = N // 128
fl_lauum = 2.0 * 128 ** 3 * sum((T - i) * (i + 1) for i in range(T))
row("panel L21 = K21 M11^T (NT khi=2)", fl_tri_k, lambda v, x: raw(v, h, h, h, 1.0, m + off(h, 0), ld, m, ld, 0.0, a + off(h, 0), ld, 0, x, 2), A[h:, :h], GEMM_NT)
row("S = (L21 M11)^T (TT klo=1, krev)", fl_tri_k, lambda v, x: raw(v, h, h, h, 1.0, m, ld, m + off(h, 0), ld, 0.0, a + off(0, h), ld, 0, 5 | x, 0), A[:h, h:N], GEMM_TT)
row("M21 = -M22 S^T (NT khi=1)", fl_tri_k, lambda v, x: raw(v, h, h, h, -1.0, m + off(h, h), ld, m + off(0, h), ld, 0.0, a + off(h, 0), ld, 0, x, 1), A[h:, :h], GEMM_NT)
row("K^-1 = M^T M (TN tri klo=1 krev, n = 16384)", fl_lauum, lambda v, x: raw(v, N, N, N, 1.0, m, ld, m, ld, 0.0, a, ld, 1, 5 | x, 0), A[:, :N], GEMM_TN, lower=True)
# K sweeps of the lower-tile update, for the selection threshold: the NT form (the factorisation's update; beta = 0 here so that repeats
# do not accumulate -- the library's has beta = 1 and the atomic epilogue; today's form is the mixed launch) and the TN form
SWEEP = (384, 768, 1024, 2048, 4096, 8192)
for K in SWEEP:
    row("update tri NT h = 8192, K = %d" % K, 2.0 * 128 * 128 * K * (t * (t + 1) // 2),
        lambda v, x: raw(v, h, h, K, -1.0, m + off(h, 0), ld, m + off(h, 0), ld, 0.0, a + off(h, h), ld, 1, x, 0), A[h:, h:N], GEMM_NT, lower=True)
for K in SWEEP:
    row("update tri TN h = 8192, K = %d" % K, 2.0 * 128 * 128 * K * (t * (t + 1) // 2),
        lambda v, x: raw(v, h, h, K, -1.0, m + off(h, 0), ld, m + off(h, 0), ld, 0.0, a + off(h, h), ld, 1, x, 0), A[h:, h:N], GEMM_TN, lower=True)
for K in SWEEP:
    row("uniform NN 8192 x 8192, K = %d" % K, 2.0 * h * h * K, lambda v, x: raw(v, h, h, K, 1.0, m + off(h, 0), ld, m + off(h, 0), ld, 0.0, a, ld, 0, x, 0), A[:h, :h], GEMM_NN)
# the K-range launches of the two routed forms at the sizes the library meets, and launches of less than one round of workgroup slots
for n in (4096, 8192):
    tt = n // 128
    row("K^-1 = M^T M (TN tri klo=1 krev, n = %d)" % n, 2.0 * 128 ** 3 * sum((tt - i) * (i + 1) for i in range(tt)),
        lambda v, x: raw(v, n, n, n, 1.0, m, ld, m, ld, 0.0, a, ld, 1, 5 | x, 0), A[:n, :n], GEMM_TN, lower=True)
for n, r in ((8192, 8192), (8192, 1024), (16384, 2048), (16384, 256)):
    tt = n // 128
    fl = 2.0 * 128 * 128 * 128 * sum(j + 1 for j in range(tt)) * (r // 128)
    row("V = M B (NN khi=1, n = %d, %d columns)" % (n, r), fl, lambda v, x: raw(v, n, r, n, 1.0, m, ld, m + off(0, h), ld, 0.0, a, ld, 0, x, 1), A[:n, :r], GEMM_NN)
    row("X = M^T V (TN klo=1, n = %d, %d columns)" % (n, r), fl, lambda v, x: raw(v, n, r, n, 1.0, m, ld, m + off(0, h), ld, 0.0, a, ld, 0, 1 | x, 0), A[:n, :r], GEMM_TN)
