"""The MFMA GEMM core (pygpr_amd/csrc/gemm.hip) through pg_gemm_raw, every exposed variant in fp64 and fp32, against tests/gemm_ref.py.

The main instrument is exactness.  Operands are integer valued (A, B in -4..4, C0 in -64..64), alpha in {1, -1, -0.5, 2}, beta in {0, 1, 2}
and K <= 2176, so every partial sum is an integer or half-integer below 2^20: exact in fp32 and fp64 in ANY summation order.  The float64
NumPy reference is then exact too, and the comparison is np.array_equal on what the call must write, and the caller's bits everywhere
else.  One test per variant and dtype uses normal data against the textbook rounding bound instead (small integers are also exact in a
reduced-precision matrix format, which exactness alone would not notice)."""
import itertools

import numpy as np
import pytest
import torch

from pygpr_amd import _lib

import gemm_ref as gr

pytestmark = pytest.mark.gpu

NAMES = sorted(gr.VARIANTS)
SQUARE = [n for n in NAMES if gr.VARIANTS[n][2] == gr.VARIANTS[n][3]]
DTYPES = [torch.float64, torch.float32]
NP = {torch.float64: np.float64, torch.float32: np.float32}
BITS = {torch.float64: np.uint64, torch.float32: np.uint32}
ALPHAS = (1.0, -1.0, -0.5, 2.0)
BETAS = (0.0, 1.0, 2.0)
MODES = list(itertools.product((0, 1, 2), (0, 1, 2)))

every_variant = pytest.mark.parametrize("name", NAMES)
square_variant = pytest.mark.parametrize("name", SQUARE)
both_dtypes = pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])


@pytest.fixture(scope="module")
def ops():
    from pygpr_amd._ops import get_ops

    return get_ops()


def _dims(name, dtype):
    _, _, bm, bn, bkt = gr.VARIANTS[name]
    return bm, bn, bkt[gr.F64 if dtype == torch.float64 else gr.F32]


def _ints(rng, M, N, K, beta):
    """Integer-valued operands; a C that beta == 0 must not read is NaN throughout."""
    a = rng.integers(-4, 5, (M, K)).astype(np.float64)
    b = rng.integers(-4, 5, (K, N)).astype(np.float64)
    c0 = rng.integers(-64, 65, (M, N)).astype(np.float64) if beta != 0 else np.full((M, N), np.nan)
    return a, b, c0


def _run(ops, name, dtype, M, N, K, alpha, opA, opB, beta, C0, tri=0, klo=0, khi=0):
    """One pg_gemm_raw call on operands rounded to dtype; returns C afterwards and C as it was given, both in dtype on the host."""
    A, B = gr.store(name, opA, opB)
    before = np.ascontiguousarray(C0.astype(NP[dtype]))
    a, b, c = (torch.from_numpy(x.astype(NP[dtype])).cuda() for x in (A, B, before))
    try:
        ops.gemm_raw(getattr(_lib, name), M, N, K, alpha, a, b, beta, c, tri=tri, klo=klo, khi=khi)
    finally:
        got = c.cpu().numpy()
    return got, before


def _tiles(mask, bm, bn):
    return sorted({(int(i) // bm, int(j) // bn) for i, j in zip(*np.nonzero(mask))})[:12]


def _exact(ops, name, dtype, M, N, K, alpha, opA, opB, beta, C0, tri=0, klo=0, khi=0):
    bm, bn, _ = _dims(name, dtype)
    what = "%s %s M=%d N=%d K=%d alpha=%g beta=%g tri=%d klo=%d khi=%d" % (name, dtype, M, N, K, alpha, beta, tri, klo, khi)
    exp, written = gr.expected(name, M, N, K, alpha, opA, opB, beta, C0, tri, klo & 3, khi)
    assert np.isfinite(exp[written]).all(), "the reference itself read a poisoned element: " + what
    got, before = _run(ops, name, dtype, M, N, K, alpha, opA, opB, beta, C0, tri, klo, khi)
    wrong = written & ~((got.astype(np.float64) == exp) & np.isfinite(got))
    assert not wrong.any(), "%s: %d wrong elements, tiles (row, column) %s" % (what, wrong.sum(), _tiles(wrong, bm, bn))
    keep = ~written & ~gr.unspecified_mask(name, M, N, tri)
    touched = keep & (got.view(BITS[dtype]) != before.view(BITS[dtype]))
    assert not touched.any(), "%s: wrote outside its tiles, tiles %s" % (what, _tiles(touched, bm, bn))


def _refused(ops, name, dtype, M, N, K, opA, opB, C0, tri=0, klo=0, khi=0):
    """The call must return a status and leave a text and C as it was; returns (status, text)."""
    A, B = (torch.from_numpy(x.astype(NP[dtype])).cuda() for x in gr.store(name, opA, opB))
    before = np.ascontiguousarray(C0.astype(NP[dtype]))
    c = torch.from_numpy(before).cuda()
    rc = ops.lib.pg_gemm_raw(ops.h, _lib.PG_F64 if dtype == torch.float64 else _lib.PG_F32, getattr(_lib, name), M, N, K, 1.0, A.data_ptr(),
                             A.stride(0), B.data_ptr(), B.stride(0), 1.0, c.data_ptr(), c.stride(0), tri, klo, khi, ops._st())
    text = _lib.last_error()
    assert rc != 0 and text, "%s tri=%d klo=%d khi=%d was not refused" % (name, tri, klo, khi)
    assert np.array_equal(c.cpu().numpy().view(BITS[dtype]), before.view(BITS[dtype]))
    return rc, text


# --------------------------------------------------------------------------- K tiles and epilogues
@both_dtypes
@every_variant
def test_k_tile_counts_and_epilogues(ops, name, dtype):
    """2 x 2 tiles with one K tile (prologue only, nothing prefetched), two, three (odd: the double buffer ends on its first half) and
    thirteen; each with beta = 0 on a C full of NaN (must not be read), beta = 1 (fp64: the atomic epilogue) and beta = 2."""
    bm, bn, bkt = _dims(name, dtype)
    rng = np.random.default_rng(1)
    alphas = itertools.cycle(ALPHAS)
    for nk, beta in itertools.product((1, 2, 3, 13), BETAS):
        M, N, K = 2 * bm, 2 * bn, nk * bkt
        a, b, c0 = _ints(rng, M, N, K, beta)
        _exact(ops, name, dtype, M, N, K, next(alphas), a, b, beta, c0)


# --------------------------------------------------------------------------- the tile walk
@both_dtypes
@every_variant
def test_every_tile_once_full_launch(ops, name, dtype):
    """tri = 0 on tile grids around the band of eight tile rows: each tile computed exactly once (a tile never computed keeps NaN under
    beta = 0, one computed twice adds its product twice under beta = 1 and 2)."""
    bm, bn, bkt = _dims(name, dtype)
    rng = np.random.default_rng(2)
    alphas = itertools.cycle(ALPHAS)
    for (tm, tn), beta in itertools.product([(1, 1), (7, 3), (8, 1), (9, 3), (17, 2)], BETAS):
        M, N, K = tm * bm, tn * bn, 3 * bkt
        a, b, c0 = _ints(rng, M, N, K, beta)
        _exact(ops, name, dtype, M, N, K, next(alphas), a, b, beta, c0)


@both_dtypes
@square_variant
def test_every_tile_once_triangular_launch(ops, name, dtype):
    """tri = 1: squares of 1 .. 19 tile rows (full bands, a ragged last band, the diagonal patches) and trapezoids; tiles above the
    diagonal keep the caller's bits."""
    bm, bn, bkt = _dims(name, dtype)
    rng = np.random.default_rng(3)
    alphas = itertools.cycle(ALPHAS)
    shapes = [(t, t) for t in (1, 2, 8, 9, 16, 19)] + [(5, 3), (9, 8), (20, 3)]
    for (tm, tn), beta in itertools.product(shapes, BETAS):
        M, N, K = tm * bm, tn * bn, 2 * bkt
        a, b, c0 = _ints(rng, M, N, K, beta)
        if beta == 0:                                        # the tiles the call must leave alone need bits to keep
            c0 = np.where(gr.expected(name, M, N, K, 1.0, a, b, 1.0, np.zeros((M, N)), 1)[1], np.nan, 7.0)
        _exact(ops, name, dtype, M, N, K, next(alphas), a, b, beta, c0, tri=1)


@both_dtypes
@every_variant
def test_tri_is_refused_where_it_has_no_meaning(ops, name, dtype):
    """tri = 1 on a tiling that is not square, or with N > M: a status, a text, and C as it was."""
    bm, bn, bkt = _dims(name, dtype)
    rng = np.random.default_rng(4)
    M, N, K = 2 * bm, (2 if bm != bn else 3) * bn, bkt
    a, b, c0 = _ints(rng, M, N, K, 1.0)
    rc, text = _refused(ops, name, dtype, M, N, K, a, b, c0, tri=1)
    assert rc == -2 and text.startswith("pg_gemm:")


# --------------------------------------------------------------------------- K ranges from triangular operands
def _k_range_case(rng, name, M, N, K, beta, klo, khi):
    """Operands that are triangular element by element where the mode says so (the per-wave skip inside diagonal tiles may rely on it),
    with NaN in every block the mode says is never read."""
    a, b, c0 = _ints(rng, M, N, K, beta)
    a, b = gr.shape_triangular(a, b, klo & 3, khi)
    return (*gr.poison_unread(name, a, b, klo & 3, khi), c0)


@both_dtypes
@every_variant
def test_k_range_modes(ops, name, dtype):
    """Every (klo, khi) on 5 x 3 and 3 x 5 tiles: K = max(M, N), and a K of two tiles (kend = min(K, ...), and tiles whose range is
    empty: C = beta C).  Among them the combinations the library uses: TT / TT_64 klo = 1 (triangular inverse), NT / NT_64 khi = 1,
    NT khi = 2 over several tile columns (the column-major walk), NN khi = 1 and klo = 2, the panel solves' khi = 2.
    A tiling whose tile is no multiple of its K tile (32 x 32, K tile 64) must refuse klo / khi: it would shorten every range."""
    bm, bn, bkt = _dims(name, dtype)
    rng = np.random.default_rng(5)
    alphas, betas = itertools.cycle(ALPHAS), itertools.cycle(BETAS)
    for (klo, khi), (tm, tn, short) in itertools.product(MODES, [(5, 3, False), (3, 5, False), (5, 3, True), (3, 5, True)]):
        M, N = tm * bm, tn * bn
        K = 2 * max(bm, bn, bkt) if short else -(-max(M, N) // bkt) * bkt          # (32 x 32 tiles, K tile 64: rounded up to a K tile)
        alpha, beta = next(alphas), next(betas)
        a, b, c0 = _k_range_case(rng, name, M, N, K, beta, klo, khi)
        if gr.k_modes_allowed(name, gr.F64 if dtype == torch.float64 else gr.F32, klo, khi):
            _exact(ops, name, dtype, M, N, K, alpha, a, b, beta, c0, klo=klo, khi=khi)
            continue
        assert name == "GEMM_NT_32x32"
        rc, text = _refused(ops, name, dtype, M, N, K, a, b, np.nan_to_num(c0), klo=klo, khi=khi)
        assert rc == -2 and "GEMM_NT_32x32" in text


def test_refused_k_range_leaves_c_untouched(ops):
    """The 32 x 32 tiling with khi = 2 (tile column 0 would end at k = 32 < its K tile of 64 and compute nothing): refused with -2 and a
    text that names the variant, before anything is enqueued."""
    rng = np.random.default_rng(6)
    M, N, K = 160, 96, 192
    for dtype, (klo, khi) in itertools.product(DTYPES, [(0, 2), (0, 1), (1, 0), (2, 0), (1, 2)]):
        a, b, c0 = _k_range_case(rng, "GEMM_NT_32x32", M, N, K, 1.0, klo, khi)
        rc, text = _refused(ops, "GEMM_NT_32x32", dtype, M, N, K, a, b, c0, klo=klo, khi=khi)
        assert rc == -2 and "GEMM_NT_32x32" in text and "K tile" in text


@both_dtypes
@pytest.mark.parametrize("name", [n for n in SQUARE if n != "GEMM_NT_32x32"])
def test_triangular_launch_with_k_from_the_tile_row(ops, name, dtype):
    """tri = 1 with klo = 1 (L^T L on GEMM_TN), walked forwards and from the end of each range downwards (klo | 4, which also rotates
    the tile columns of a row): 3, 9 and 17 tile rows and a trapezoid.  Exact sums do not depend on the order."""
    bm, bn, bkt = _dims(name, dtype)
    rng = np.random.default_rng(7)
    alphas, betas = itertools.cycle(ALPHAS), itertools.cycle(BETAS)
    for (tm, tn), klo in itertools.product([(3, 3), (9, 9), (17, 17), (5, 3)], (1, 5)):
        M, N = tm * bm, tn * bn
        for K in (M, 2 * bm):
            alpha, beta = next(alphas), next(betas)
            a, b, c0 = _k_range_case(rng, name, M, N, K, beta, klo, 0)
            if beta == 0:
                c0 = np.where(gr.expected(name, M, N, K, 1.0, a, b, 1.0, np.zeros((M, N)), 1, 1)[1], np.nan, 7.0)
            _exact(ops, name, dtype, M, N, K, alpha, a, b, beta, c0, tri=1, klo=klo)


# --------------------------------------------------------------------------- rounding
@both_dtypes
@every_variant
def test_rounding_stays_within_the_textbook_bound(ops, name, dtype):
    """Standard-normal data rounded to the dtype, 2 x 2 tiles, K = 13 K tiles.  For any order of the K products and sums, and the
    alpha / beta arithmetic after them, |got - exact| <= (K + 3) u S with S = |alpha| |opA| |opB| + |beta| |C0| (Higham, Accuracy and
    Stability of Numerical Algorithms, section 3.5) and u = 2^-53 / 2^-24; the float64 reference gets the same bound at 2^-53."""
    bm, bn, bkt = _dims(name, dtype)
    rng = np.random.default_rng(8)
    M, N, K = 2 * bm, 2 * bn, 13 * bkt
    u = 2.0 ** -53 if dtype == torch.float64 else 2.0 ** -24
    for alpha, beta in [(-0.5, 2.0), (1.0, 1.0), (2.0, 0.0)]:
        a, b, c0 = (rng.standard_normal(s).astype(NP[dtype]).astype(np.float64) for s in ((M, K), (K, N), (M, N)))
        ref, _ = gr.expected(name, M, N, K, alpha, a, b, beta, c0)
        S = gr.abs_bound(name, M, N, K, alpha, a, b, beta, c0)
        got, _ = _run(ops, name, dtype, M, N, K, alpha, a, b, beta, c0)
        err = np.abs(got.astype(np.float64) - ref)
        bound = (K + 3) * u * S + (K + 3) * 2.0 ** -53 * S
        print("%s %s alpha=%g beta=%g: max err / bound = %.3g" % (name, dtype, alpha, beta, (err / bound).max()))
        assert (err <= bound).all()


# --------------------------------------------------------------------------- EPI = 1: column sums of squares
@both_dtypes
@pytest.mark.parametrize("kt_form", [False, True], ids=["NN_128_SS", "NT_128_SS"])
@pytest.mark.parametrize("n_pad,m_pad", [(256, 256), (768, 512), (768, 256), (256, 512)])
def test_column_sums_of_squares_epilogue(ops, n_pad, m_pad, kt_form, dtype):
    """The epilogue that pg_gemm_raw cannot reach, through pg_predict_mean_q (GEMM_NN_128_SS) and pg_predict_mean_q_kt
    (GEMM_NT_128_SS): var[j] = kss - sum_i (Minv Ks)[i][j]^2 with integer data whose sums of squares stay below 2^24, so mean and
    variance are exact in both dtypes; Minv's 128-blocks above the diagonal blocks (khi = 1: never read) hold NaN."""
    rng = np.random.default_rng(n_pad + m_pad)
    minv = np.tril(rng.integers(-2, 3, (n_pad, n_pad))).astype(np.float64)
    ks = rng.integers(-1, 2, (n_pad, m_pad)).astype(np.float64)
    alpha = rng.integers(-3, 4, n_pad).astype(np.float64)
    kss = 5.0
    v = minv @ ks
    mean_ref, q_ref = ks.T @ alpha, kss - (v * v).sum(0)
    assert np.abs(v).max() < 2 ** 24 and (v * v).sum(0).max() < 2 ** 24                   # (of the inputs: what makes the result exact)
    blocks = np.arange(n_pad) // 128
    minv[blocks[None, :] > blocks[:, None]] = np.nan
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).astype(NP[dtype])).cuda()
    mean, q = (torch.full((m_pad,), float("nan"), dtype=dtype, device="cuda") for _ in range(2))
    work = torch.full(((n_pad // 64) * m_pad,), float("nan"), dtype=dtype, device="cuda")
    if kt_form:
        ops.predict_mean_q_kt(dev(ks.T), dev(minv), dev(alpha), mean, q, kss, work)
    else:
        ops.predict_mean_q(dev(ks), dev(minv), dev(alpha), mean, q, kss, work)
    assert np.array_equal(mean.cpu().numpy().astype(np.float64), mean_ref)
    assert np.array_equal(q.cpu().numpy().astype(np.float64), q_ref)
