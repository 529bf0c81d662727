"""tests/gemm_ref.py (the NumPy statement of one pg_gemm_raw call) against a brute-force loop over elements, and its variant table
against the constants of pygpr_amd/_lib.py: no GPU needed."""
import itertools
import re

import numpy as np
import pytest

from pygpr_amd import _lib

import gemm_ref as gr

MODES = list(itertools.product((0, 1, 2), (0, 1, 2)))


def _brute(bm, bn, M, N, K, alpha, a, b, beta, c0, tri, klo, khi):
    """Element by element, each with the K range of the tile it lies in; None marks what the call does not write."""
    out = [[None] * N for _ in range(M)]
    for i in range(M):
        for j in range(N):
            ti, tj = i // bm, j // bn
            if tri and tj > ti:
                continue
            kbeg = 0 if klo == 0 else (ti * bm if klo == 1 else tj * bn)
            kend = K if khi == 0 else min(K, (ti + 1) * bm if khi == 1 else (tj + 1) * bn)
            s = 0.0
            for k in range(kbeg, kend):
                s += a[i][k] * b[k][j]
            out[i][j] = alpha * s + (beta * c0[i][j] if beta != 0 else 0.0)
    return out


def _case(rng, M, N, K):
    a = rng.integers(-4, 5, (M, K)).astype(np.float64)
    b = rng.integers(-4, 5, (K, N)).astype(np.float64)
    c0 = rng.integers(-64, 65, (M, N)).astype(np.float64)
    return a, b, c0


def _compare(variant, bm, bn, M, N, K, alpha, beta, tri, klo, khi, rng):
    a, b, c0 = _case(rng, M, N, K)
    if beta == 0:
        c0[:] = np.nan
    exp, written = gr.expected(variant, M, N, K, alpha, a, b, beta, c0, tri, klo, khi)
    ref = _brute(bm, bn, M, N, K, alpha, a.tolist(), b.tolist(), beta, c0.tolist(), tri, klo, khi)
    unspec = gr.unspecified_mask(variant, M, N, tri)
    for i in range(M):
        for j in range(N):
            if ref[i][j] is None:                       # a tile the call does not cover: the caller's value, and not marked written
                assert not written[i, j] and not unspec[i, j]
                assert exp[i, j] == c0[i, j] or (np.isnan(exp[i, j]) and np.isnan(c0[i, j]))
            else:
                assert exp[i, j] == ref[i][j]
                assert written[i, j] != unspec[i, j]
                assert unspec[i, j] == bool(tri and i // bm == j // bn and j > i)


@pytest.mark.parametrize("klo,khi", MODES)
@pytest.mark.parametrize("tiles", [(4, 4), (4, 8), (8, 4)])
def test_expected_against_the_element_loop_on_tiny_tiles(tiles, klo, khi):
    """Every K-range mode on 5 x 3 and 3 x 5 tiles, K = max(M, N) and K shorter than M (empty ranges, kend = K), all epilogues."""
    bm, bn = tiles
    variant = (False, True, bm, bn, {gr.F64: 4, gr.F32: 4})
    rng = np.random.default_rng(100 * klo + 10 * khi + bm)
    for (tm, tn), (alpha, beta) in zip([(5, 3), (3, 5), (5, 3)], [(1.0, 0.0), (-0.5, 1.0), (2.0, 2.0)]):
        M, N = tm * bm, tn * bn
        for K in (max(M, N), 2 * bm, 4):
            _compare(variant, bm, bn, M, N, K, alpha, beta, 0, klo, khi, rng)


@pytest.mark.parametrize("klo,khi", [(0, 0), (1, 0), (0, 2), (1, 2)])
@pytest.mark.parametrize("tm,tn", [(1, 1), (3, 3), (5, 3), (4, 1)])
def test_expected_tri_covers_the_triangle_and_the_rows_below_it(tm, tn, klo, khi):
    bm = 4
    variant = (True, False, bm, bm, {gr.F64: 4, gr.F32: 4})
    rng = np.random.default_rng(7 * tm + tn)
    for alpha, beta in [(-1.0, 0.0), (1.0, 1.0), (2.0, 2.0)]:
        _compare(variant, bm, bm, tm * bm, tn * bm, 3 * bm, alpha, beta, 1, klo, khi, rng)
    a, b, c0 = _case(rng, tm * bm, tn * bm, bm)
    exp, written = gr.expected(variant, tm * bm, tn * bm, bm, 1.0, a, b, 1.0, c0, tri=1)
    tiles = tn * (tn + 1) // 2 + (tm - tn) * tn
    assert written.sum() == tiles * bm * bm - tn * (bm * (bm - 1) // 2)


@pytest.mark.parametrize("name", sorted(gr.VARIANTS))
def test_expected_on_the_variants_own_tiles(name):
    """Each named variant at its own tile size (2 x 2 tiles, K = one row tile + one K tile): the element loop with NumPy's dot over
    each element's own K range."""
    _, _, bm, bn, bkt = gr.VARIANTS[name]
    M, N = 2 * bm, 2 * bn
    rng = np.random.default_rng(len(name))
    for dtype, (klo, khi) in itertools.product((gr.F64, gr.F32), MODES):
        if not gr.k_modes_allowed(name, dtype, klo, khi):
            continue
        K = bm + bkt[dtype]
        a, b, c0 = _case(rng, M, N, K)
        exp, written = gr.expected(name, M, N, K, -0.5, a, b, 2.0, c0, 0, klo, khi)
        assert written.all()
        for i, j in itertools.product(range(0, M, 7), range(0, N, 5)):
            kbeg, kend = gr.k_range(K, i // bm * bm, j // bn * bn, bm, bn, klo, khi)
            assert exp[i, j] == -0.5 * np.dot(a[i, kbeg:kend], b[kbeg:kend, j]) + 2.0 * c0[i, j]


def test_variant_table_names_the_library_constants():
    consts = {k for k in vars(_lib) if k.startswith("GEMM_")}
    assert consts == set(gr.VARIANTS)
    assert len({getattr(_lib, k) for k in consts}) == len(consts)
    # the tile sizes the names carry, and the K tiles gemm.h documents
    for name, (ta, tb, bm, bn, bkt) in gr.VARIANTS.items():
        m = re.fullmatch(r"GEMM_([NT])([NT])(?:_(\d+)(?:x(\d+))?|_(RP))?", name)
        assert m, name
        assert (ta, tb) == (m.group(1) == "T", m.group(2) == "T")
        if m.group(5):
            assert (bm, bn) == (64, 256)
        elif m.group(3):
            assert (bm, bn) == (int(m.group(3)), int(m.group(4) or m.group(3)))
        else:
            assert (bm, bn) == (128, 128)
        want = {"GEMM_NT_32x64": (32, 32), "GEMM_NT_32x128": (16, 32), "GEMM_NT_32x32": (64, 64)}.get(name, (16, 16))
        assert (bkt[gr.F64], bkt[gr.F32]) == want


def test_k_modes_refused_where_the_tile_is_no_multiple_of_the_k_tile():
    bad = [(n, d, klo, khi) for n in gr.VARIANTS for d in (gr.F64, gr.F32) for klo, khi in MODES if not gr.k_modes_allowed(n, d, klo, khi)]
    assert bad and {n for n, *_ in bad} == {"GEMM_NT_32x32"}
    assert all(klo or khi for _, _, klo, khi in bad)


def test_shape_and_poison_leave_every_tile_range_clean():
    """shape_triangular + poison_unread: the product over each tile's K range is finite and equals the full product of the triangular
    operands, for every variant and mode that is allowed."""
    rng = np.random.default_rng(5)
    for name in sorted(gr.VARIANTS):
        _, _, bm, bn, _ = gr.VARIANTS[name]
        M, N = 3 * bm, 2 * bn
        K = max(M, N)
        for klo, khi in MODES:
            if not gr.k_modes_allowed(name, gr.F64, klo, khi):
                continue
            a, b, c0 = _case(rng, M, N, K)
            a, b = gr.shape_triangular(a, b, klo, khi)
            full = a @ b
            ap, bp = gr.poison_unread(name, a, b, klo, khi)
            if (klo or khi) and K > 256:
                assert np.isnan(ap).any() or np.isnan(bp).any()
            exp, _ = gr.expected(name, M, N, K, 1.0, ap, bp, 0.0, c0, 0, klo, khi)
            assert np.array_equal(exp, full)
