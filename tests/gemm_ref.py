"""NumPy statement of what one pg_gemm_raw call must do (include/pygpr_hip.h, pygpr_amd/csrc/gemm.h):

    C[M x N] = beta * C + alpha * opA * opB      over the output tiles the call covers,

with each tile's product restricted to the tile's own useful K range [kbeg, kend):

    klo = 1 / 2   kbeg = the tile's row / column origin            (0 otherwise)
    khi = 1 / 2   kend = min(K, row origin + BM / column origin + BN)   (K otherwise)

tri = 1 covers the tiles on and below the diagonal only (N < M: the leading N x N triangle and the full tile rows below it); the
elements strictly above the diagonal INSIDE the diagonal tiles are unspecified afterwards, everything else outside the covered tiles
keeps the caller's bits.

The operands are given in their logical orientation, opA [M x K] and opB [K x N]; `store` lays them out the way the variant reads them.
Host only: no GPU, no torch."""
import numpy as np

F64, F32 = "float64", "float32"


def _v(ta, tb, bm, bn, bkt64=16, bkt32=None):
    return (ta, tb, bm, bn, {F64: bkt64, F32: bkt64 if bkt32 is None else bkt32})


# name of the constant in pygpr_amd/_lib.py -> (TA, TB, BM, BN, {dtype: BKT}); from gemm.h and pg_gemm's switch
VARIANTS = {
    "GEMM_NT": _v(False, True, 128, 128),
    "GEMM_NT_RP": _v(False, True, 64, 256),
    "GEMM_NN": _v(False, False, 128, 128),
    "GEMM_TN": _v(True, False, 128, 128),
    "GEMM_TT": _v(True, True, 128, 128),
    "GEMM_NT_64": _v(False, True, 64, 64),
    "GEMM_NT_64x128": _v(False, True, 64, 128),
    "GEMM_NT_32x64": _v(False, True, 32, 64, 32),
    "GEMM_NT_32x128": _v(False, True, 32, 128, 16, 32),
    "GEMM_TT_64": _v(True, True, 64, 64),
    "GEMM_NT_32x32": _v(False, True, 32, 32, 64),
    "GEMM_TN_64": _v(True, False, 64, 64),
}


def tiling(variant):
    """(TA, TB, BM, BN, {dtype: BKT}) of a variant name, or the tuple itself (tests of this helper use tiny tiles)."""
    return VARIANTS[variant] if isinstance(variant, str) else variant


def store(variant, opA, opB):
    """The arrays the call is given: A holds opA as M x K, or K x M when the variant transposes A; B holds opB as K x N, or N x K when
    the variant transposes B."""
    ta, tb = tiling(variant)[:2]
    return np.ascontiguousarray(opA.T if ta else opA), np.ascontiguousarray(opB.T if tb else opB)


def k_range(K, origin_m, origin_n, bm, bn, klo, khi):
    kbeg = {0: 0, 1: origin_m, 2: origin_n}[klo]
    kend = {0: K, 1: min(K, origin_m + bm), 2: min(K, origin_n + bn)}[khi]
    return kbeg, kend


def k_modes_allowed(variant, dtype, klo, khi):
    """A K range that follows the tile rows (columns) needs the row (column) tile to be a whole number of K tiles."""
    _, _, bm, bn, bkt = tiling(variant)
    return all((bm if mode == 1 else bn) % bkt[dtype] == 0 for mode in (klo, khi) if mode)


def covered_tiles(variant, M, N, tri):
    _, _, bm, bn, _ = tiling(variant)
    assert M % bm == 0 and N % bn == 0 and (not tri or (bm == bn and N <= M))
    return [(ti, tj) for ti in range(M // bm) for tj in range(N // bn) if not tri or tj <= ti]


def unspecified_mask(variant, M, N, tri):
    """tri = 1: strictly above the diagonal inside the diagonal tiles (some tilings update it, some do not)."""
    mask = np.zeros((M, N), dtype=bool)
    if tri:
        bm = tiling(variant)[2]
        for t in range(N // bm):
            blk = mask[t * bm:(t + 1) * bm, t * bm:(t + 1) * bm]
            blk[np.triu_indices(bm, 1)] = True
    return mask


def expected(variant, M, N, K, alpha, opA, opB, beta, C0, tri=0, klo=0, khi=0):
    """(C_expected, written_mask): per covered tile a slice of a float64 matmul over the tile's K range.  beta == 0 does not read C0
    (it may hold NaN).  Outside written_mask C_expected is C0; the unspecified elements are in neither set."""
    _, _, bm, bn, _ = tiling(variant)
    opA, opB = np.asarray(opA, dtype=np.float64), np.asarray(opB, dtype=np.float64)
    assert opA.shape == (M, K) and opB.shape == (K, N) and C0.shape == (M, N)
    out = np.array(C0, dtype=np.float64)
    written = np.zeros((M, N), dtype=bool)
    for ti, tj in covered_tiles(variant, M, N, tri):
        r, c = slice(ti * bm, (ti + 1) * bm), slice(tj * bn, (tj + 1) * bn)
        kbeg, kend = k_range(K, ti * bm, tj * bn, bm, bn, klo, khi)
        prod = opA[r, kbeg:kend] @ opB[kbeg:kend, c] if kend > kbeg else np.zeros((bm, bn))
        out[r, c] = alpha * prod + (beta * out[r, c] if beta != 0 else 0.0)
        written[r, c] = True
    written &= ~unspecified_mask(variant, M, N, tri)
    return out, written


def abs_bound(variant, M, N, K, alpha, opA, opB, beta, C0, tri=0, klo=0, khi=0):
    """S = |alpha| |opA| |opB| + |beta| |C0| per element, over the same tiles and K ranges: the scale of the textbook rounding bound."""
    return expected(variant, M, N, K, abs(alpha), np.abs(opA), np.abs(opB), abs(beta), np.abs(C0), tri, klo, khi)[0]


def shape_triangular(opA, opB, klo, khi):
    """Make the operands triangular at element level the way the K-range modes assume: mode 1 speaks about opA (klo: zero for k < row,
    khi: zero for k > row), mode 2 about opB (klo: zero for k < column, khi: zero for k > column)."""
    M, K = opA.shape
    N = opB.shape[1]
    a, b = opA.copy(), opB.copy()
    i, ka = np.arange(M)[:, None], np.arange(K)[None, :]
    kb, j = np.arange(K)[:, None], np.arange(N)[None, :]
    if klo == 1: a[ka < i] = 0
    if khi == 1: a[ka > i] = 0
    if klo == 2: b[kb < j] = 0
    if khi == 2: b[kb > j] = 0
    return a, b


def poison_unread(variant, opA, opB, klo, khi, value=np.nan):
    """Fill what a K-range mode says is never read: the blocks strictly beyond the diagonal blocks of the triangular operand, a block
    being 128 rows / columns or the variant's own tile where that is larger."""
    _, _, bm, bn, _ = tiling(variant)
    M, K = opA.shape
    N = opB.shape[1]
    a, b = opA.copy(), opB.copy()
    ga, gb = max(128, bm), max(128, bn)
    i, ka = np.arange(M)[:, None], np.arange(K)[None, :]
    kb, j = np.arange(K)[:, None], np.arange(N)[None, :]
    if klo == 1: a[ka < (i // ga) * ga] = value
    if khi == 1: a[ka >= (i // ga + 1) * ga] = value
    if klo == 2: b[kb < (j // gb) * gb] = value
    if khi == 2: b[kb >= (j // gb + 1) * gb] = value
    return a, b
