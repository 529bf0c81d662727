"""The software-pipelined four-wave fp64 tile (gemm.hip: PlTile; variants 14-17, _lib.PIPELINED) through pg_gemm_raw, against
tests/gemm_ref.py and against the eight-wave form of the same variant, bit for bit.

Operands are integer valued (A, B in -4..4, C0 in -64..64) with alpha in {1, -1, -0.5, 2} and beta in {0, 1, 2}: every partial sum is
an integer or a half-integer far below 2^53, exact in any order, so the float64 NumPy reference is exact and the comparison is equality.
NaN stands wherever a call must not read: in C under beta = 0 and in the operand blocks a K-range mode never touches.  The shapes are
the pipeline's own cases: one to five K tiles (prologue only; prologue + last tile; both buffer parities; the first steady-state tile),
K ranges that start and end inside the matrix, diagonal tiles in which half the waves skip, walked forwards and from the end."""
import itertools

import numpy as np
import pytest
import torch

from pygpr_amd import _lib

import gemm_ref as gr

pytestmark = pytest.mark.gpu

FORMS = ["GEMM_NT", "GEMM_NN", "GEMM_TN", "GEMM_TT"]
ALPHAS = (1.0, -1.0, -0.5, 2.0)
BETAS = (0.0, 1.0, 2.0)
every_form = pytest.mark.parametrize("name", FORMS)


@pytest.fixture(scope="module")
def ops():
    from pygpr_amd._ops import get_ops

    return get_ops()


def _ints(rng, M, N, K, beta):
    a = rng.integers(-4, 5, (M, K)).astype(np.float64)
    b = rng.integers(-4, 5, (K, N)).astype(np.float64)
    c0 = rng.integers(-64, 65, (M, N)).astype(np.float64) if beta != 0 else np.full((M, N), np.nan)
    return a, b, c0


def _call(ops, variant, name, M, N, K, alpha, opA, opB, beta, C0, tri=0, klo=0, khi=0, pad=0):
    """One pg_gemm_raw call; every array sits in rows `pad` elements longer than the matrix, the bands filled with a marker.  Returns C
    and the three bands afterwards."""
    A, B = gr.store(name, opA, opB)
    devs = []
    for x in (A, B, np.ascontiguousarray(C0)):
        full = torch.full((x.shape[0], x.shape[1] + pad), -7.25, dtype=torch.float64, device="cuda")
        full[:, :x.shape[1]] = torch.from_numpy(x).cuda()
        devs.append(full)
    a, b, c = (d[:, :d.shape[1] - pad] for d in devs)
    if pad == 0:
        ops.gemm_raw(variant, M, N, K, alpha, a, b, beta, c, tri=tri, klo=klo, khi=khi)
    else:                                                    # (ops.gemm_raw takes contiguous tensors only)
        _lib.check(ops.lib.pg_gemm_raw(ops.h, _lib.PG_F64, variant, M, N, K, float(alpha), a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0),
                                       float(beta), c.data_ptr(), c.stride(0), tri, klo, khi, ops._st()), "pg_gemm_raw")
    return c.cpu().numpy(), [d[:, d.shape[1] - pad:].cpu().numpy() for d in devs]


def _check(ops, name, M, N, K, alpha, opA, opB, beta, C0, tri=0, klo=0, khi=0, pad=0):
    what = "%s pipelined M=%d N=%d K=%d alpha=%g beta=%g tri=%d klo=%d khi=%d pad=%d" % (name, M, N, K, alpha, beta, tri, klo, khi, pad)
    exp, written = gr.expected(name, M, N, K, alpha, opA, opB, beta, C0, tri, klo & 3, khi)
    assert np.isfinite(exp[written]).all(), "the reference itself read a poisoned element: " + what
    got, bands = _call(ops, _lib.PIPELINED[getattr(_lib, name)], name, M, N, K, alpha, opA, opB, beta, C0, tri, klo, khi, pad)
    wrong = written & ~((got == exp) & np.isfinite(got))
    assert not wrong.any(), "%s: %d wrong elements" % (what, wrong.sum())
    keep = ~written & ~gr.unspecified_mask(name, M, N, tri)
    assert np.array_equal(got[keep].view(np.uint64), np.ascontiguousarray(C0)[keep].view(np.uint64)), what + ": wrote outside its tiles"
    assert all((band == -7.25).all() for band in bands), what + ": wrote into a guard band"
    ref, _ = _call(ops, getattr(_lib, name), name, M, N, K, alpha, opA, opB, beta, C0, tri, klo | 8, khi, pad)      # (| 8: never routed)
    assert np.array_equal(got[written].view(np.uint64), ref[written].view(np.uint64)), what + ": differs from the eight-wave form"


@every_form
def test_one_to_five_k_tiles(ops, name):
    """One tile, K = 16 .. 80: nk = 1 (prologue and last tile only), 2 (one staged tile, buffer 0 -> 1), 3 and 4 (both parities of the
    last buffer), 5; each with every beta (1: the atomic epilogue; 0: C full of NaN) and alpha in turn."""
    rng = np.random.default_rng(11)
    alphas = itertools.cycle(ALPHAS)
    for K, beta in itertools.product((16, 32, 48, 64, 80), BETAS):
        a, b, c0 = _ints(rng, 128, 128, K, beta)
        _check(ops, name, 128, 128, K, next(alphas), a, b, beta, c0)


def _k_range_case(rng, name, M, N, K, beta, klo, khi):
    a, b, c0 = _ints(rng, M, N, K, beta)
    a, b = gr.shape_triangular(a, b, klo & 3, khi)
    return (*gr.poison_unread(name, a, b, klo & 3, khi), c0)


@every_form
@pytest.mark.parametrize("tri", [0, 1])
def test_k_ranges_at_384(ops, name, tri):
    """M = N = K = 384 with klo = 1, 2 and khi = 1, 2, forwards and (klo) from the end: tiles whose range is one 128-block, diagonal
    tiles where half the waves skip, ranges that start and end inside the matrix; NaN in the blocks the mode never reads."""
    rng = np.random.default_rng(12 + tri)
    alphas, betas = itertools.cycle(ALPHAS), itertools.cycle(BETAS)
    for klo, khi in [(1, 0), (5, 0), (2, 0), (6, 0), (0, 1), (0, 2), (1, 2), (5, 2), (2, 1), (6, 1), (0, 0)]:
        alpha, beta = next(alphas), next(betas)
        a, b, c0 = _k_range_case(rng, name, 384, 384, 384, beta, klo, khi)
        if tri and beta == 0:                                # the tiles the call must leave alone need bits to keep
            c0 = np.where(gr.expected(name, 384, 384, 384, 1.0, a, b, 1.0, np.zeros((384, 384)), 1, klo & 3, khi)[1], np.nan, 7.0)
        _check(ops, name, 384, 384, 384, alpha, a, b, beta, c0, tri=tri, klo=klo, khi=khi)


@every_form
def test_trapezoid(ops, name):
    """tri = 1 with N < M (M = 384, N = 256): the leading triangle and the full tile rows below it, plain and with klo = 1 reversed."""
    rng = np.random.default_rng(14)
    for (klo, K), (alpha, beta) in zip([(0, 96), (5, 384), (1, 384)], [(-1.0, 1.0), (2.0, 0.0), (-0.5, 2.0)]):
        a, b, c0 = _k_range_case(rng, name, 384, 256, K, beta, klo, 0)
        if beta == 0:
            c0 = np.where(gr.expected(name, 384, 256, K, 1.0, a, b, 1.0, np.zeros((384, 256)), 1, klo & 3, 0)[1], np.nan, 7.0)
        _check(ops, name, 384, 256, K, alpha, a, b, beta, c0, tri=1, klo=klo)


@every_form
def test_every_alpha_and_beta(ops, name):
    """2 x 2 tiles, K = 112 (seven K tiles), all twelve (alpha, beta)."""
    rng = np.random.default_rng(15)
    for alpha, beta in itertools.product(ALPHAS, BETAS):
        a, b, c0 = _ints(rng, 256, 256, 112, beta)
        _check(ops, name, 256, 256, 112, alpha, a, b, beta, c0)


@every_form
def test_leading_dimensions_and_guard_bands(ops, name):
    """Rows 48 and 1040 elements longer than the matrix (the second moves every row to another 8 KB page): the bands come back untouched."""
    rng = np.random.default_rng(16)
    for pad, beta in [(48, 1.0), (1040, 0.0), (48, 2.0)]:
        a, b, c0 = _ints(rng, 256, 128, 96, beta)
        _check(ops, name, 256, 128, 96, -0.5, a, b, beta, c0, pad=pad)


def test_fp32_is_refused(ops):
    a = torch.zeros(128, 128, dtype=torch.float32, device="cuda")
    c = torch.full((128, 128), 3.0, dtype=torch.float32, device="cuda")
    rc = ops.lib.pg_gemm_raw(ops.h, _lib.PG_F32, _lib.PIPELINED[_lib.GEMM_NT], 128, 128, 128, 1.0, a.data_ptr(), 128, a.data_ptr(), 128, 0.0,
                             c.data_ptr(), 128, 0, 0, 0, ops._st())
    assert rc == -2 and "fp64" in _lib.last_error()
    assert (c == 3.0).all()


@every_form
def test_rounding_and_bit_equality_on_normal_data(ops, name):
    """Standard-normal data, M = N = 256, K = 512: within (K + 3) u |A||B| of the float64 reference (itself within the same bound at
    2^-53: Higham, Accuracy and Stability of Numerical Algorithms, section 3.5), and the same bits as the eight-wave form."""
    rng = np.random.default_rng(17)
    M, N, K = 256, 256, 512
    for alpha, beta in [(-0.5, 2.0), (1.0, 1.0), (2.0, 0.0)]:
        a, b, c0 = (rng.standard_normal(s) for s in ((M, K), (K, N), (M, N)))
        ref, _ = gr.expected(name, M, N, K, alpha, a, b, beta, c0)
        S = gr.abs_bound(name, M, N, K, alpha, a, b, beta, c0)
        got, _ = _call(ops, _lib.PIPELINED[getattr(_lib, name)], name, M, N, K, alpha, a, b, beta, c0)
        old, _ = _call(ops, getattr(_lib, name), name, M, N, K, alpha, a, b, beta, c0, klo=8)
        bound = 2 * (K + 3) * 2.0 ** -53 * S
        print("%s alpha=%g beta=%g: max err / bound = %.3g" % (name, alpha, beta, (np.abs(got - ref) / bound).max()))
        assert (np.abs(got - ref) <= bound).all()
        assert np.array_equal(got.view(np.uint64), old.view(np.uint64))


def _stacked(ops, variant, name, M, N, K, alpha, beta, probs, levels, flags=None, pad=0):
    """One launch over len(probs) stacked problems (tri | 2: batch = 2, | 4: nexp = 2, | 8: status flags in front of C); returns the C
    blocks afterwards.  Rows are `pad` elements longer than the matrices."""
    stack = lambda xs: np.concatenate([np.pad(x, ((0, 0), (0, pad)), constant_values=-7.25) for x in xs], 0)
    stored = [gr.store(name, a, b) for a, b, _ in probs]
    a = torch.from_numpy(stack([s[0] for s in stored])).cuda()
    b = torch.from_numpy(stack([s[1] for s in stored])).cuda()
    buf = torch.zeros(2 + len(probs) * M * (N + pad), dtype=torch.float64, device="cuda")      # 16 bytes of flags, then C
    if flags is not None:
        buf[:2].view(torch.int32)[:len(flags)] = torch.tensor(flags, dtype=torch.int32, device="cuda")
    c = buf[2:].view(len(probs) * M, N + pad)
    c.copy_(torch.from_numpy(stack([c0 for _, _, c0 in probs])).cuda())
    _lib.check(ops.lib.pg_gemm_raw(ops.h, _lib.PG_F64, variant, M, N, K, float(alpha), a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0),
                                   float(beta), c.data_ptr(), c.stride(0), levels | (8 if flags is not None else 0), 8, 0, ops._st()), "pg_gemm_raw")
    out = c.cpu().numpy()
    assert (out[:, N:] == -7.25).all(), "wrote into a guard band"
    return [out[i * M:(i + 1) * M, :N] for i in range(len(probs))]


@every_form
def test_batch_and_experts_with_strides(ops, name):
    """batch = 2, nexp = 2 and both (four problems: z -> (z % batch, z / batch)) in one launch, 256 x 128 x 80 each in rows 16 longer
    than the matrix: every problem gets its own product, equal to the reference and to the eight-wave form's."""
    rng = np.random.default_rng(18)
    M, N, K = 256, 128, 80
    for levels, count, (alpha, beta) in [(2, 2, (-1.0, 1.0)), (4, 2, (2.0, 0.0)), (6, 4, (-0.5, 2.0))]:
        probs = [_ints(rng, M, N, K, beta) for _ in range(count)]
        got = _stacked(ops, _lib.PIPELINED[getattr(_lib, name)], name, M, N, K, alpha, beta, probs, levels, pad=16)
        old = _stacked(ops, getattr(_lib, name), name, M, N, K, alpha, beta, probs, levels, pad=16)
        for (a, b, c0), g, o in zip(probs, got, old):
            exp, _ = gr.expected(name, M, N, K, alpha, a, b, beta, c0)
            assert np.array_equal(g, exp) and np.array_equal(g.view(np.uint64), o.view(np.uint64))


@every_form
def test_a_raised_status_flag_leaves_c_untouched(ops, name):
    """Two experts with a flag each: the expert whose flag is not zero keeps C bit for bit (NaN operands: nothing may be computed
    from them), the other is computed; both flags zero: both computed."""
    rng = np.random.default_rng(19)
    M, N, K = 128, 128, 48
    for flags in ([0, 3], [-1, 0], [0, 0], [5, 5]):
        probs = [_ints(rng, M, N, K, 1.0) for _ in flags]
        probs = [(a * np.nan, b, c0) if f else (a, b, c0) for (a, b, c0), f in zip(probs, flags)]
        got = _stacked(ops, _lib.PIPELINED[getattr(_lib, name)], name, M, N, K, -1.0, 1.0, probs, 4, flags=flags)
        for (a, b, c0), f, g in zip(probs, flags, got):
            want = c0 if f else gr.expected(name, M, N, K, -1.0, a, b, 1.0, c0)[0]
            assert np.array_equal(g.view(np.uint64), np.ascontiguousarray(want).view(np.uint64)), (name, flags)
