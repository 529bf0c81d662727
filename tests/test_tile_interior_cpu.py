"""The strip map of the covariance build kernels, restated on the host, and the shapes of tests/test_tile_interior_gpu.py held against it.

pg_kbuild_kernel (csrc/kbuild.hip) and pg_kbuild_mfma_kernel (csrc/kmfma.hip) give a workgroup a STRIP of up to S = 6 tiles of one
tile row (kb_strip_of, csrc/kfun.h) and choose ONE body for the whole strip: the checked body (per-element fix-ups for the diagonal,
the padding and accumulate passes) or the interior body (none), the latter when

    interior = !accumulate && (!symmetric || tcl < tr) && (tr + 1) * 64 <= nr && (tcl + 1) * 64 <= nc

with tr the tile row and tcl the strip's last tile.  A value test reaches the interior body -- the six-tile walk over both column
buffers, the fast body's norm refresh, the re-use of the transpose buffer, a strip that starts at tile 6 -- only at a shape that
HOLDS interior strips.  This file

  * restates kb_strips_before / kb_strip_of (the float32 square-root decode included) and the predicate, and checks the restatement
    against the definition: every tile of the window on or below the diagonal (symmetric) or of the rectangle (cross) exactly once,
    strips never longer than S and never across a row;
  * reads S's default and the tile edge from the sources, so that a changed default fails HERE instead of hollowing the GPU file;
  * holds SHAPES, the one table the GPU file takes its shapes from, and asserts of every entry what makes it worth running;
  * records the gap: the shapes of the value tests that existed before hold no interior strip at all (but for one test of one body).

No GPU and no library: the sources are read as text."""
import os
import re

import numpy as np
import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pygpr_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def strip_default():
    """S: the default of PG_KB_STRIP in pg_kbuild (csrc/kbuild.hip)."""
    m = re.search(r'getenv\("PG_KB_STRIP"\)\s*\?\s*atoi\(getenv\("PG_KB_STRIP"\)\)\s*:\s*(\d+)\s*;', _src("kbuild.hip"))
    assert m, "the default of PG_KB_STRIP is no longer where this file looks for it"
    return int(m.group(1))


def tile_edges():
    """{source: KT} of every source that defines the tile edge."""
    out = {}
    for name in sorted(os.listdir(CSRC)):
        m = re.search(r"^#define\s+KT\s+(\d+)\s*$", _src(name), re.M)
        if m:
            out[name] = int(m.group(1))
    return out


S = strip_default()
KT = 64
COUPLED_PANEL = 384      # the outer panel of a factorisation of at most 8192 rows (csrc/linalg.hip); checked below


# ---- the strip map (csrc/kfun.h) ------------------------------------------------------------------------------------------------------
def strips_before(rp, s):
    """Strips in triangle rows 0 .. rp - 1 (kb_strips_before)."""
    q, rem = divmod(rp, s)
    return s * q * (q + 1) // 2 + rem * (q + 1)


def n_strips(symmetric, tr_count, c0, c1, s):
    """The grid of a build over the tile-column window [c0, c1) of tr_count tile rows (pg_kbuild)."""
    w = c1 - c0
    sw = (w + s - 1) // s
    return strips_before(w, s) + (tr_count - c1) * sw if symmetric else tr_count * sw


def strip_of(b, symmetric, c0, c1, s):
    """(tr, tcs, ntile) of workgroup b (kb_strip_of), its arithmetic in the device's types: the first guess of the triangle's block
    comes from a float32 square root and is then corrected in integers."""
    w = c1 - c0
    sw = (w + s - 1) // s
    if not symmetric:
        tcs = c0 + (b % sw) * s
        return b // sw, tcs, min(s, c1 - tcs)
    ntri = strips_before(w, s)
    if b < ntri:
        f = np.float32
        q = int((np.sqrt(f(1) + f(8) * f(b) / f(s)) - f(1)) * f(0.5))
        while q > 0 and s * q * (q + 1) // 2 > b:
            q -= 1
        while s * (q + 1) * (q + 2) // 2 <= b:
            q += 1
        within = b - s * q * (q + 1) // 2
        rem, sidx = divmod(within, q + 1)
        rp = s * q + rem
        return c0 + rp, c0 + sidx * s, min(s, rp + 1 - sidx * s)
    j = b - ntri
    tcs = c0 + (j % sw) * s
    return c1 + j // sw, tcs, min(s, c1 - tcs)


def is_interior(tr, tcs, ntile, nr, nc, symmetric, accumulate=False):
    tcl = tcs + ntile - 1
    return (not accumulate) and (not symmetric or tcl < tr) and (tr + 1) * KT <= nr and (tcl + 1) * KT <= nc


def strips(symmetric, nr, nc, rows_pad, cols_pad, col0=0, col1=0, s=None):
    """[(tr, tcs, ntile, interior)] of one launch: a symmetric build on nr = nc points, a cross build nr x nc, the column window
    [col0, col1) of a lower-only build (col1 = 0: every column)."""
    s = S if s is None else s
    col1 = col1 or cols_pad
    assert rows_pad % KT == 0 and cols_pad % KT == 0 and col0 % KT == 0 and col1 % KT == 0 and (not symmetric or rows_pad == cols_pad)
    c0, c1, trs = col0 // KT, col1 // KT, rows_pad // KT
    out = []
    for b in range(n_strips(symmetric, trs, c0, c1, s)):
        tr, tcs, nt = strip_of(b, symmetric, c0, c1, s)
        out.append((tr, tcs, nt, is_interior(tr, tcs, nt, nr, nc, symmetric)))
    return out


def interior_of(strip_list):
    return [q for q in strip_list if q[3]]


def windows_of(n_pad):
    """The column windows of the build folded into a factorisation of n_pad <= 8192 rows on its default schedule: one window up to two
    panels, else the first panel and the rest (pg_potrf_t, csrc/linalg.hip: the look-ahead schedule needs three panels)."""
    panels = -(-n_pad // COUPLED_PANEL)
    return [(0, n_pad)] if panels < 3 else [(0, COUPLED_PANEL), (COUPLED_PANEL, n_pad)]


# ---- the shapes of tests/test_tile_interior_gpu.py ------------------------------------------------------------------------------------
N, NPAD = 840, 1024              # thirteen full tile rows, a ragged one (8 real points), two of padding
NLONG, NLONG_PAD = 4000, 4096    # W = 64: the triangle's decode well past the small cases
ROLL = 197                       # the shift of the position-independence check: 3 tiles + 5 points
REC_SPLIT = 512                  # pg_set_recursive_split in the factorisation tests
SHAPES = {
    # name: (symmetric, nr, nc, rows_pad, cols_pad)
    "sym": (1, N, N, NPAD, NPAD),
    "cross_wide": (0, 200, N, 256, NPAD),
    "cross_tall": (0, N, 512, NPAD, 512),
    "long": (1, NLONG, NLONG, NLONG_PAD, NLONG_PAD),
    # what pg_set_recursive_split(512) makes of "sym": the trailing points against the leading half, and among themselves
    "rec_cross": (0, N - REC_SPLIT, REC_SPLIT, NPAD - REC_SPLIT, REC_SPLIT),
    "rec_sym": (1, N - REC_SPLIT, N - REC_SPLIT, NPAD - REC_SPLIT, NPAD - REC_SPLIT),
}
# the value tests of a build that existed before, by their shapes (real / padded): test_hip_kernels, test_framed*_gpu, test_rq_gpu,
# test_periodic_gpu, test_product_gpu, test_matern_family_gpu
OLD_SHAPES = [(1, n, n, p, p) for n, p in ((70, 256), (130, 256), (200, 256), (300, 512), (330, 512), (333, 512), (410, 512))] + [
    (0, 37, 300, 256, 512), (0, 300, 1, 512, 256), (0, 300, 37, 512, 256), (0, 1, 37, 256, 256), (0, 200, 333, 256, 512),
    (0, 70, 330, 256, 512), (0, 70, 130, 256, 256)]


def _shape(name):
    sym, nr, nc, rp, cp = SHAPES[name]
    return strips(sym, nr, nc, rp, cp)


# ---- the restatement against the definition -------------------------------------------------------------------------------------------
def test_constants_are_the_sources_own():
    assert S == 6, "PG_KB_STRIP's default changed: re-derive SHAPES (every assertion of this file is about strips of six)"
    edges = tile_edges()
    assert set(edges) >= {"kbuild.hip", "kmfma.hip"} and set(edges.values()) == {KT}, edges
    for name in ("kbuild.hip", "kmfma.hip"):      # both kernels decode their strip through the one routine and state the one predicate
        src = _src(name)
        assert "kb_strip_of(blockIdx.x, symmetric, ctile0, ctile1, S, tr, tcs, ntile);" in src
        assert re.search(r"interior = (!accumulate && )?\(!symmetric \|\| tcl < tr\) && \(tr \+ 1\) \* KT <= nr && \(tcl \+ 1\) \* KT <= nc;", src)
    lin = _src("linalg.hip")
    assert re.search(r"^#define\s+COUPLED_PANEL\s+%d\b" % COUPLED_PANEL, lin, re.M)
    assert re.search(r"return n <= 10240 \? 512 :", lin)      # pg_nbo: the panel is min(512, COUPLED_PANEL) at these sizes


@pytest.mark.parametrize("s", [1, 2, 5, 6, 7, 16])
def test_strips_partition_their_window(s):
    """Every tile the build owns exactly once -- symmetric: on or below the diagonal, inside the window's columns; cross: the rectangle
    -- for whole builds and for every window [c0, c1) of up to 20 tile rows; strips stay in one row and hold 1 .. s tiles."""
    for trs in (1, 2, 6, 7, 13, 16, 20):
        for c0 in range(trs):
            for c1 in range(c0 + 1, trs + 1):
                for symmetric in (0, 1):
                    seen = np.zeros((trs, trs), int)
                    for b in range(n_strips(symmetric, trs, c0, c1, s)):
                        tr, tcs, nt = strip_of(b, symmetric, c0, c1, s)
                        assert 1 <= nt <= s and c0 <= tcs and tcs + nt <= c1 and 0 <= tr < trs, (trs, c0, c1, symmetric, b)
                        assert (tcs - c0) % s == 0
                        seen[tr, tcs:tcs + nt] += 1
                    want = np.zeros((trs, trs), int)
                    want[:, c0:c1] = 1
                    if symmetric:
                        want = np.tril(want)
                    assert np.array_equal(seen, want), (trs, c0, c1, symmetric)


def test_long_triangle_decodes_in_float32():
    """W = 64 (n_pad = 4096): the float32 first guess of the triangle's block, corrected in integers, lands on the right strip for every
    workgroup -- and at W = 1024, S = 1 (half a million strips), past where float32 holds b exactly divided."""
    for w, s in ((64, S), (1024, 1), (1000, 3)):
        b = 0
        for rp in range(w):
            for sidx in range(rp // s + 1):
                if b % 97 == 0 or sidx == rp // s or w == 64:
                    assert strip_of(b, 1, 0, w, s) == (rp, sidx * s, min(s, rp + 1 - sidx * s)), (w, s, b)
                b += 1
        assert b == strips_before(w, s)


# ---- what makes each shape worth running ----------------------------------------------------------------------------------------------
def test_symmetric_shape_reaches_both_strip_positions_and_both_buffers():
    sym = _shape("sym")
    inner = interior_of(sym)
    assert len(sym) == 30 and len(inner) == 8
    assert {(tr, tcs) for tr, tcs, _, _ in inner} == {(tr, 0) for tr in range(6, 13)} | {(12, 6)}
    assert all(nt == S for _, _, nt, _ in inner)                   # six tiles: cur = 0, 1, 0, 1, 0, 1 -- both buffer parities, five prefetches
    assert any(tcs == S for _, tcs, _, _ in inner)                 # an interior strip that starts at tile 6
    assert N % KT and N // KT == 13                                # tile row 13 is ragged ...
    assert any(tr == 13 and not inn for tr, _, _, inn in sym)
    assert {tr for tr, _, _, _ in sym} >= {14, 15}                 # ... and rows 14, 15 are padding only
    # checked strips of six tiles run beside them (the diagonal's row 5, the ragged row), so both bodies walk whole strips
    assert any(nt == S and not inn for _, _, nt, inn in sym)


def test_cross_shapes_reach_the_interior_body():
    wide = _shape("cross_wide")
    assert len(wide) == 12 and len(interior_of(wide)) == 6
    assert {(tr, tcs, nt) for tr, tcs, nt, _ in interior_of(wide)} == {(tr, tcs, S) for tr in range(3) for tcs in (0, 6)}
    assert any(nt == 4 and not inn for _, _, nt, inn in wide)      # the last strip of a row: four tiles, the last one ragged
    assert any(tr == 3 and not inn for tr, _, _, inn in wide)      # a ragged tile row (200 = 3 x 64 + 8)
    tall = _shape("cross_tall")
    assert len(tall) == 32 and len(interior_of(tall)) == 26
    assert {nt for _, tcs, nt, inn in tall if inn and tcs == 6} == {2}      # an interior strip shorter than S, at the second position
    assert {nt for _, tcs, nt, inn in tall if inn and tcs == 0} == {S}


def test_windowed_build_of_the_factorisation():
    """n_pad = 1024: panels of 384, 384 and 256 columns, so the folded build runs as the windows [0, 384) and [384, 1024); each holds
    interior strips, the second as a triangle that starts at tile column 6 (c0 > 0)."""
    assert windows_of(NPAD) == [(0, 384), (384, 1024)] and windows_of(512) == [(0, 512)] and windows_of(768) == [(0, 768)]
    assert [len(strips(1, N, N, NPAD, NPAD, c0, c1)) for c0, c1 in windows_of(NPAD)] == [16, 14]
    whole = {(tr, tc) for tr, tcs, nt, _ in _shape("sym") for tc in range(tcs, tcs + nt)}
    tiles, inner = set(), []
    for c0, c1 in windows_of(NPAD):
        part = strips(1, N, N, NPAD, NPAD, c0, c1)
        for tr, tcs, nt, inn in part:
            new = {(tr, tc) for tc in range(tcs, tcs + nt)}
            assert not (new & tiles)
            tiles |= new
        inner.append(interior_of(part))
    assert tiles == whole                                           # the two windows build the lower tiles once each
    assert {(tr, tcs, nt) for tr, tcs, nt, _ in inner[0]} == {(tr, 0, S) for tr in range(6, 13)}      # the rectangle below the first panel
    assert {(tr, tcs, nt) for tr, tcs, nt, _ in inner[1]} == {(12, 6, S)}                             # the triangle of the second window
    # under pg_set_recursive_split(512): a 328 x 512 cross build and a 328-point symmetric build; the leading half is one window
    sym, nr, nc, rp, cp = SHAPES["rec_cross"]
    assert (sym, nr, nc, rp, cp) == (0, 328, 512, 512, 512)
    rc = _shape("rec_cross")
    assert {(tr, tcs, nt) for tr, tcs, nt, _ in interior_of(rc)} == {(tr, tcs, nt) for tr in range(5) for tcs, nt in ((0, 6), (6, 2))}
    assert not interior_of(_shape("rec_sym"))                       # five full rows of a 512 triangle: every strip touches the diagonal
    assert len(interior_of(strips(1, REC_SPLIT, REC_SPLIT, REC_SPLIT, REC_SPLIT))) == 2      # the leading half: rows 6, 7


def test_long_triangle_shape():
    long = _shape("long")
    assert NLONG_PAD // KT == 64 and len(long) == strips_before(64, S) == 374
    inner = interior_of(long)
    assert len(inner) == 290                                       # three strips in four
    assert {nt for _, _, nt, _ in inner} == {S}
    assert max(tcs for _, tcs, _, _ in inner) == 54                 # strips at every start tile 0, 6, .., 54
    assert NLONG % KT and any(tr == 62 and not inn for tr, _, _, inn in long) and any(tr == 63 for tr, _, _, _ in long)


def test_roll_moves_pairs_between_the_bodies():
    """The position-independence check builds K for X and for X rolled by 197 points: pairs then change tile (197 is no multiple of 64),
    strip position and buffer parity, and pairs of interior tiles land in diagonal and ragged tiles and back."""
    assert ROLL % KT and (ROLL // KT) % 2 == 1
    body = np.zeros((NPAD // KT, NPAD // KT), int)                  # 1: interior, 2: checked (lower tiles; the upper ones mirror them)
    for tr, tcs, nt, inn in _shape("sym"):
        body[tr, tcs:tcs + nt] = 1 if inn else 2
    body = np.maximum(body, body.T)
    i = np.arange(N)
    src = body[np.ix_(i // KT, i // KT)]
    j = (i + ROLL) % N
    dst = body[np.ix_(j // KT, j // KT)]
    assert ((src == 1) & (dst == 2)).any() and ((src == 2) & (dst == 1)).any() and ((src == 1) & (dst == 1)).any()
    par = ((i // KT) % S) % 2                                       # the column buffer a pair's column tile sits in
    assert (par != ((j // KT) % S) % 2).any()


# ---- the record of the gap ------------------------------------------------------------------------------------------------------------
def test_the_older_value_tests_hold_no_interior_strip():
    for sym, nr, nc, rp, cp in OLD_SHAPES:
        assert not interior_of(strips(sym, nr, nc, rp, cp)), (sym, nr, nc)
    assert [len(strips(1, n, n, p, p)) for n, p in ((200, 256), (410, 512))] == [4, 10]
    assert len(strips(0, 37, 300, 256, 512)) == 8
    assert len(interior_of(strips(1, 448, 448, 512, 512))) == 1    # the first shape with any
    # the one older value test past that: test_kernel_build_fast_body_on_uncentred_data, n = 700 in 768 -- four interior strips of the
    # FAST body (fp64 squared exponential, d = 3), all at the first position of a row
    fast = strips(1, 700, 700, 768, 768)
    assert len(fast) == 18 and {(tr, tcs, nt) for tr, tcs, nt, _ in interior_of(fast)} == {(tr, 0, S) for tr in range(6, 10)}
    assert len(strips(0, N, 200, NPAD, 256)) == 16 and not interior_of(strips(0, N, 200, NPAD, 256))     # a four-tile strip, last tile ragged
