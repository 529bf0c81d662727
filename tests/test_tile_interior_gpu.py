"""Covariance builds at shapes that reach the INTERIOR bodies of pg_kbuild_kernel (csrc/kbuild.hip) and pg_kbuild_mfma_kernel
(csrc/kmfma.hip): the strips that lie strictly below the diagonal and inside the real points, which run without per-element fix-ups --
the six-tile walk over both column buffers, the fast body's norm refresh per tile, the transpose buffer re-used by consecutive tiles of
a mirrored build, strips that start at tile 6.  The older value tests of a build hold no such strip (tests/test_tile_interior_cpu.py,
which also checks every shape used here against a restatement of the strip map: SHAPES is that file's table).

Plain `ops` calls on packed operands; K itself against tests/kernel_ref.py in fp64, never another GPU call.  Models: the eight rows of
test_framed_kinds_gpu.MODELS and the base routes they leave out (BASE), each with one white-noise term; both dtypes; PG_KB_MFMA unset,
"0" and "2" wherever pg_kbuild's routing depends on it (route()).  Data in [0, 1)^d and the hyper-parameters of
test_framed_kinds_gpu.hp_of (sigma 1.2, inverse length scales 0.4 .. 1.2, periods 0.7 .. 2.5, alpha 0.8, noise 0.05 .. 0.15; 0.3 where
a matrix is factored), so that the allowances of the small-shape tests apply unchanged -- element-wise error does not grow with n:

  MODELS                 test_framed_kinds_gpu.k_tol: 1e-13; fp32 4e-6, F x 4e-6 / 1.44 of max|K| for F >= 3 factors, per pass
  BASE on the pipe       atol = rtol = 2e-14 / 4e-6   test_matrix_pipe_bodies_against_the_valu_bodies_and_the_oracle (se, m52) and
                                                      test_matern_family_gpu::test_entry_points_against_the_restatement (m32)
  BASE se, m52, se + se  atol = rtol = 1e-14          test_kernel_build, test_kernel_build_large_d (VALU bodies, fp64)
  BASE m32, m12          atol = rtol = 2e-14          test_matern_family_gpu (VALU: m12 always, m32 under PG_KB_MFMA = 0)
  BASE fp32 on the VALU  atol = rtol = 4e-6           the same two tests; se + se: 4e-6 absolute, k_tol's rule for a sum
  sqd (PG_KIND_SQDIST)   atol 1e-14                   test_sqdist_kind_and_centres_any_d; fp32 has no older test: u d L^2 (7 + d) with
                                                      u = 2^-24, L = max l -- each (l a - l b)^2 carries at most 7 u L^2 (two staged
                                                      roundings, the difference, the square), the d - 1 additions u d L^2 each
Every allowance is first held against kernel_ref's own fp64 error on 64 of the case's points (test_product_gpu.allowance), and the
measured error is printed beside it.

The position-independence check (c) needs neither: the VALU bodies form a pair's value from its two points alone, so K of the rolled
points is K rolled, bit for bit."""
import functools

import numpy as np
import pytest
import torch

import kernel_ref as kr
from kind_tools import dev, host, ops, specs_of  # noqa: F401  (ops: the fixture)
from pygpr_amd import _lib
from pygpr_amd._ops import make_spec
from test_framed_gpu import F32, F64, both
from test_framed_kinds_gpu import MODELS, hp_of, k_tol, passes_of
from test_product_gpu import allowance
from test_tile_interior_cpu import KT, N, NLONG, NLONG_PAD, NPAD, REC_SPLIT, ROLL, SHAPES

pytestmark = pytest.mark.gpu

# id -> (terms, d): the routes MODELS leaves out.  "sqd" is PG_KIND_SQDIST, the scaled squared distance itself (block [sigma, l_1..l_d],
# sigma unused), which tests/kernel_ref.py has as kr.sqdist
BASE = {
    "se3": (["se", "wn"], 3),           # FAST in fp64, the matrix pipe in fp32
    "se13": (["se", "wn"], 13),         # the matrix pipe, DP = 16
    "m52": (["m52", "wn"], 5),
    "m32": (["m32", "wn"], 16),
    "m12": (["m12", "wn"], 8),          # PRESC on the VALU, never the matrix pipe
    "se2": (["se", "se", "wn"], 8),     # the general body, presc = 0
    "se40": (["se", "wn"], 40),         # NPF = 16, more than 64 KB of LDS
    "sqd": (["sqd", "wn"], 5),
}
ALL = list(MODELS) + list(BASE)
ONE_PASS = [m for m in ALL if m != "C1"]
FACTORED = [m for m in ONE_PASS if m != "sqd"]      # a distance matrix is not positive definite: nothing to factor
PIPE_KINDS = ("se", "m52", "m32", "rq")
JIT = 1e-7


def model_of(mid):
    return MODELS[mid] if mid in MODELS else BASE[mid]


def specs(mid):
    """The passes of a model as ops.kernel_build takes them."""
    model, d = model_of(mid)
    if mid == "sqd":
        return [make_spec([_lib.PG_KIND_SQDIST], [0], [d + 1])]
    return [sp for sp, _, _ in passes_of(mid)] if mid in MODELS else specs_of(model, d)


def one_spec(mid):
    sp = specs(mid)
    assert len(sp) == 1
    return sp[0]


def hp_for(mid, rng, noise=None):
    model, d = model_of(mid)
    return hp_of(["se", "wn"] if mid == "sqd" else model, d, rng, noise)


def ref_kernel(mid, hp, x, xp=None, dtype=np.float64):
    """K [n, n] with the noise on its diagonal, or the cross kernel with the points xp as ROWS."""
    model, _ = model_of(mid)
    if mid != "sqd":
        return kr.kernel(model, hp, x, xp, dtype=dtype)
    hp, x = np.asarray(hp, dtype), np.asarray(x, dtype)
    sq = kr.sqdist(hp, x, None if xp is None else np.asarray(xp, dtype))
    return sq + hp[-1] ** 2 * np.eye(x.shape[0], dtype=dtype) if xp is None else sq


def pipe_eligible(mid):
    model, d = model_of(mid)
    return len(model) == 2 and model[0] in PIPE_KINDS and d <= 16


def route(mid, dtype, mode):
    """The body pg_kbuild gives a first pass of this model (csrc/kbuild.hip): "pipe", or the VALU instantiation."""
    model, d = model_of(mid)
    stat = [t for t in model if t != "wn"]
    fast = len(stat) == 1 and stat[0] == "se" and dtype == F64
    if pipe_eligible(mid):
        env = 1 if mode is None else int(mode)
        if env and (env >= 2 or not fast or d > 8):
            return "pipe"
    if mid == "C1":
        return "passes"      # (the plain child on PRESC, then the product with accumulate = 1: always the checked body)
    if any(isinstance(t, tuple) for t in stat):
        return "prod"
    if "per" in stat:
        return "per"
    return "fast" if fast else ("presc" if len(stat) == 1 else "general")


CASES = [(m, mode) for m in ALL for mode in ((None, "0", "2") if pipe_eligible(m) else (None,))]
by_mode = pytest.mark.parametrize("mid,mode", CASES, ids=["%s-kb%s" % (m, "_" if mode is None else mode) for m, mode in CASES])
by_mode_one_pass = pytest.mark.parametrize("mid,mode", [c for c in CASES if c[0] != "C1"],
                                           ids=["%s-kb%s" % (m, "_" if mode is None else mode) for m, mode in CASES if m != "C1"])


def set_mode(monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv("PG_KB_MFMA", raising=False)
    else:
        monkeypatch.setenv("PG_KB_MFMA", mode)


def name(dtype):
    return "f64" if dtype == F64 else "f32"


def tol_of(mid, dtype, body, ref, hp, x, xp=None):
    """(atol, rtol) of K for this model, dtype and body: the table of the module docstring."""
    if mid in MODELS:
        return k_tol(mid, dtype, ref, hp, x, xp), 0.0
    model, d = model_of(mid)
    if mid == "sqd":
        atol, rtol = (1e-14, 0.0) if dtype == F64 else (2.0 ** -24 * d * float(hp[1:1 + d].max()) ** 2 * (7 + d), 0.0)
    elif dtype == F32:
        atol, rtol = (4e-6, 0.0) if mid == "se2" else (4e-6, 4e-6)
    elif body == "pipe" or model[0] in ("m32", "m12"):
        atol, rtol = 2e-14, 2e-14
    else:
        atol, rtol = 1e-14, 1e-14
    s, sp = x[:64], (None if xp is None else xp[:32])
    atol, err = allowance(atol, ref_kernel(mid, hp, s, sp), ref_kernel(mid, hp, s, sp, dtype=np.longdouble))
    print("%s %s %s K: allowance %.2e + %.0e |K|, kernel_ref's own error %.2e" % (mid, name(dtype), body, atol, rtol, err))
    return atol, rtol


def close(what, got, ref, tol, mask=None):
    """|got - ref| <= atol + rtol |ref| on the mask, the largest error printed beside the bound; NaN fails."""
    atol, rtol = tol
    err, bound = np.abs(got - ref), atol + rtol * np.abs(ref)
    if mask is not None:
        err, bound = err[mask], bound[mask]
    print("%-44s err %.2e (allowance %.2e + %.0e |K|)" % (what, float(np.nanmax(err)), atol, rtol))
    assert not np.isnan(err).any() and (err <= bound).all(), (what, float(np.nanmax(err)), atol, rtol)


def tile_lower(npad):
    t = np.arange(npad) // KT
    return t[:, None] >= t[None, :]


def nan_filled(ops, *shape, dtype):
    out = ops.empty(*shape, dtype=dtype)
    out.fill_(float("nan"))
    return out


def diag_value(mid, hp, dtype):
    """(value, exact) of a symmetric build's real diagonal: every term's product of sigma^2, rounded as the body forms it, plus
    (jitter + sigma_n^2).  Exact for a lone periodic child and for a product spec (test_periodic_gpu, test_product_gpu); the other
    kinds to 1e-15 / 2e-7 relative (test_matrix_pipe_bodies_*, test_matern_family_gpu, test_rq_gpu)."""
    model, d = model_of(mid)
    ft = np.float64 if dtype == F64 else np.float32
    vals, noise, o = [], 0.0, 0
    for t in model:
        if t == "wn":
            noise += hp[o] ** 2
            o += 1
            continue
        v = None
        for q in kr.factors(t):
            s2 = ft(hp[o] * hp[o]) if q != "sqd" else ft(0)
            v = s2 if v is None else ft(v * s2)
            o += kr.width("se" if q == "sqd" else q, d)
        vals.append(v)
    exact = len(vals) == 1 and (isinstance(model[0], tuple) or model[0] == "per")
    if exact:
        return np.float64(ft(vals[0] + ft(JIT + noise))), True
    return float(sum(np.float64(v) for v in vals) + (JIT + noise)), False


def build(ops, mid, hp, x, dtype, lower_only=False, xc=None, shape=(NPAD, NPAD)):
    """One build of the model (all its passes in order, as Ops.kernel_build runs them) into a NaN-filled matrix, on the host."""
    out = nan_filled(ops, *shape, dtype=dtype)
    sp = specs(mid)
    ops.kernel_build(sp if len(sp) > 1 else sp[0], dev(hp), dev(x, dtype), None if xc is None else dev(xc, dtype), out, lower_only=lower_only,
                     jitter=JIT if xc is None else 0.0)
    return host(out)


# ------------------------------------------------------------------------------------------- a. symmetric, 840 in 1024
@functools.lru_cache(maxsize=None)
def sym_inputs(mid, n=N, npad=NPAD):
    _, d = model_of(mid)
    rng = np.random.default_rng(1000 * n + d + 17 * ALL.index(mid))
    x, hp = rng.random((n, d)), hp_for(mid, rng)
    ref = np.eye(npad)
    ref[:n, :n] = ref_kernel(mid, hp, x) + JIT * np.eye(n)
    ref.setflags(write=False)
    return x, hp, ref


@both
@by_mode
def test_symmetric_build(ops, monkeypatch, mid, mode, dtype):
    """n = 840 in 1024, mirrored and lower-only: eight interior strips of six tiles at the first and the second position of a row, a
    ragged row, two rows of padding.  The whole padded matrix against kernel_ref + 1e-7 I with identity padding; the lower-only build
    on a NaN-filled matrix leaves no NaN in the 64-tiles on or below the diagonal and every NaN above them, and equals the mirrored one
    bit for bit there; the mirrored matrix is exactly symmetric; the diagonal has the value the small tests assert."""
    assert SHAPES["sym"] == (1, N, N, NPAD, NPAD)
    x, hp, ref = sym_inputs(mid)
    set_mode(monkeypatch, mode)
    body = route(mid, dtype, mode)
    tol = tol_of(mid, dtype, body, ref[:N, :N], hp, x)
    full, low = build(ops, mid, hp, x, dtype), build(ops, mid, hp, x, dtype, lower_only=True)
    close("%s %s %s mirrored" % (mid, name(dtype), body), full, ref, tol)
    assert np.array_equal(full, full.T)
    pad = np.eye(NPAD)
    pad[:N, :N] = full[:N, :N]
    assert np.array_equal(full, pad)                                    # identity padding, exactly
    tl = tile_lower(NPAD)
    assert not np.isnan(low[tl]).any() and np.isnan(low[~tl]).all()
    assert np.array_equal(low[tl], full[tl])
    dgv, exact = diag_value(mid, hp, dtype)
    if exact:
        assert (np.diag(full)[:N] == dgv).all()
    else:
        np.testing.assert_allclose(np.diag(full)[:N], dgv, rtol=1e-15 if dtype == F64 else 2e-7, atol=0)


# ------------------------------------------------------------------------------------------- b. cross builds
@functools.lru_cache(maxsize=None)
def cross_inputs(mid, shape):
    _, nr, nc, rp, cp = SHAPES[shape]
    _, d = model_of(mid)
    rng = np.random.default_rng(100 * nr + nc + d + 17 * ALL.index(mid))
    xr, xc, hp = rng.random((nr, d)), rng.random((nc, d)), hp_for(mid, rng)
    ref = np.zeros((rp, cp))
    ref[:nr, :nc] = ref_kernel(mid, hp, xc, xr)
    ref.setflags(write=False)
    return xr, xc, hp, ref


@both
@pytest.mark.parametrize("shape", ["cross_wide", "cross_tall"])
@by_mode
def test_cross_build(ops, monkeypatch, mid, mode, shape, dtype):
    """200 x 840 in 256 x 1024 (six interior strips of six tiles, a four-tile strip with a ragged last tile) and 840 x 512 in 1024 x 512
    (26 interior strips, every second one two tiles long): values, and padding that is exactly zero."""
    _, nr, nc, rp, cp = SHAPES[shape]
    xr, xc, hp, ref = cross_inputs(mid, shape)
    set_mode(monkeypatch, mode)
    body = route(mid, dtype, mode)
    tol = tol_of(mid, dtype, body, ref[:nr, :nc], hp, xc, xr)
    got = build(ops, mid, hp, xr, dtype, xc=xc, shape=(rp, cp))
    close("%s %s %s %s" % (mid, name(dtype), body, shape), got, ref, tol)
    assert not got[nr:, :].any() and not got[:, nc:].any() and not np.isnan(got).any()


# ------------------------------------------------------------------------------------------- c. position independence
@both
@pytest.mark.parametrize("mid", ALL)
def test_position_independence_of_the_valu_bodies(ops, monkeypatch, mid, dtype):
    """PG_KB_MFMA = 0: every model on its VALU body (FAST, PRESC, the general body and its PER and PROD instantiations, NPF 2, 4, 16).
    Those bodies form a pair's value from the two points alone -- the same products in the same order wherever the pair sits, and the
    same with the roles of row and column point exchanged -- so the mirrored K of the points rolled by 197 is K rolled, BIT FOR BIT:
    K2[(i + 197) % n, (j + 197) % n] == K[i, j] for all i, j.  The roll moves pairs between interior, diagonal and ragged tiles, between
    the two column buffers and between the computed and the mirrored half.  No tolerance, no reference.  (The matrix-pipe bodies take
    coordinates relative to the expert's first point, which the roll changes: they get the value checks only.)"""
    x, hp, _ = sym_inputs(mid)
    monkeypatch.setenv("PG_KB_MFMA", "0")
    assert route(mid, dtype, "0") != "pipe"
    k1 = build(ops, mid, hp, x, dtype)[:N, :N]
    k2 = build(ops, mid, hp, np.roll(x, ROLL, axis=0), dtype)[:N, :N]
    back = np.roll(k2, (-ROLL, -ROLL), axis=(0, 1))                     # back[i, j] = k2[(i + ROLL) % n, (j + ROLL) % n]
    diff = back != k1
    if diff.any():
        i, j = np.nonzero(diff)
        ulp = np.abs(back - k1)[diff] / np.spacing(np.abs(k1[diff]).astype(np.float64 if dtype == F64 else np.float32)).astype(np.float64)
        print("%s %s: %d of %d pairs differ, at most %.1f ulp; tiles (row, column) of the first: %s" % (
            mid, name(dtype), diff.sum(), diff.size, ulp.max(), sorted({(int(a) // KT, int(b) // KT) for a, b in zip(i[:2000], j[:2000])})[:12]))
    assert not diff.any()


# ------------------------------------------------------------------------------------------- d. batched
@both
@by_mode_one_pass
def test_batched_experts_equal_their_single_builds(ops, monkeypatch, mid, mode, dtype):
    """pg_kernel_build_batched, three experts of 840 points with their own points and hyper-parameters (blockIdx.y = expert): a symmetric
    build and a cross build with shared row points (200 x 840).  Each expert equals its one-expert call bit for bit, padding included."""
    _, d = model_of(mid)
    _, m, _, mp, _ = SHAPES["cross_wide"]
    rng = np.random.default_rng(5 + d + ALL.index(mid))
    xs, xq = rng.random((3, N, d)), rng.random((m, d))
    hps = np.stack([hp_for(mid, rng) for _ in range(3)])
    spec = one_spec(mid)
    set_mode(monkeypatch, mode)
    xd, qd, hd = dev(xs, dtype), dev(xq, dtype), dev(hps)
    sym, cross = nan_filled(ops, 3, NPAD, NPAD, dtype=dtype), nan_filled(ops, 3, mp, NPAD, dtype=dtype)
    ops.kernel_build_batched(spec, hd, xd, None, sym, jitter=JIT)
    ops.kernel_build_batched(spec, hd, qd, xd, cross)
    assert not torch.isnan(sym).any() and not torch.isnan(cross).any()
    for e in range(3):
        one, onec = nan_filled(ops, NPAD, NPAD, dtype=dtype), nan_filled(ops, mp, NPAD, dtype=dtype)
        ops.kernel_build(spec, hd[e], xd[e], None, one, jitter=JIT)
        ops.kernel_build(spec, hd[e], qd, xd[e], onec)
        assert torch.equal(sym[e], one) and torch.equal(cross[e], onec), (mid, e)
    assert not torch.equal(sym[0], sym[1]) and not torch.equal(cross[1], cross[2])      # (the experts are not one another's copies)


# ------------------------------------------------------------------------------------------- e. inside the factorisation
@functools.lru_cache(maxsize=None)
def fit_inputs(mid):
    """Points, hyper-parameters with noise 0.3, the padded K + 1e-7 I and its Cholesky factor (LAPACK)."""
    from scipy.linalg import lapack

    _, d = model_of(mid)
    rng = np.random.default_rng(50 + N + d + ALL.index(mid))
    x, hp = rng.random((N, d)), hp_for(mid, rng, noise=0.3)
    k = np.eye(NPAD)
    k[:N, :N] = ref_kernel(mid, hp, x) + JIT * np.eye(N)
    chol, info = lapack.dpotrf(k, lower=1)
    assert info == 0
    return x, hp, np.tril(chol)


def factor(ops, mid, dtype, with_inv, folded):
    """(L, L^-1 or None) on the host, lower triangles: the build folded into the factorisation, or the lower-only build and then the
    factorisation, both into a NaN-filled matrix."""
    x, hp, _ = fit_inputs(mid)
    spec, hpd, xd = one_spec(mid), dev(hp), dev(x, dtype)
    a = nan_filled(ops, NPAD, NPAD, dtype=dtype)
    invd = ops.potrf_workspace(NPAD, dtype)
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    minv = ops.zeros(NPAD, NPAD, dtype=dtype) if with_inv else None
    if folded:
        ops.build_factor(spec, hpd, xd, a, invd, info, minv, jitter=JIT)
    else:
        ops.kernel_build(spec, hpd, xd, None, a, lower_only=True, jitter=JIT)
        (ops.potrf_trtri(a, invd, info, minv) if with_inv else ops.potrf(a, invd, info))
    assert int(info.item()) == 0
    return np.tril(host(a)), (np.tril(host(minv)) if with_inv else None)


@both
@pytest.mark.parametrize("with_inv", [False, True], ids=["factor", "factor+inverse"])
@pytest.mark.parametrize("mid", FACTORED)
def test_build_inside_the_factorisation(ops, mid, with_inv, dtype):
    """pg_build_potrf_trtri at n_pad = 1024 builds K in the column windows [0, 384) and [384, 1024) (three panels): the rectangle below
    the first panel and a triangle that starts at tile column 6, both with interior strips.  Factor (and inverse) equal those of
    pg_kernel_build(lower_only) followed by pg_potrf / pg_potrf_trtri bit for bit -- test_build_folded_into_the_factorisation's
    assertion, on every one-pass model that can be factored."""
    l0, m0 = factor(ops, mid, dtype, with_inv, folded=False)
    l1, m1 = factor(ops, mid, dtype, with_inv, folded=True)
    assert not np.isnan(l1).any()
    np.testing.assert_array_equal(l0, l1)
    if with_inv:
        np.testing.assert_array_equal(m0, m1)
    if dtype == F64:
        np.testing.assert_allclose(l1, fit_inputs(mid)[2], atol=1e-10)      # (as that test: the factor against LAPACK's of the reference K)


@both
@pytest.mark.parametrize("mid", FACTORED)
def test_build_inside_the_recursive_split(ops, mid, dtype):
    """pg_set_recursive_split(512): the factor-and-invert call builds the leading 512 points, then K21 as a 328 x 512 cross build (its
    second strip two tiles long) and K22 as a symmetric build of 328 points.  What test_recursive_split_matches_one_level_schedule asserts
    of its built case: factor and inverse against the one-level schedule and LAPACK, 1e-11 / 2e-3."""
    assert SHAPES["rec_cross"][1:3] == (N - REC_SPLIT, REC_SPLIT)
    tol = 1e-11 if dtype == F64 else 2e-3
    want = fit_inputs(mid)[2]
    try:
        ops.set_recursive_split(REC_SPLIT)
        l_rec, m_rec = factor(ops, mid, dtype, True, folded=True)
        ops.set_recursive_split(0)
        l_one, m_one = factor(ops, mid, dtype, True, folded=True)
    finally:
        ops.set_recursive_split(16384)
    print("%s %s: L against LAPACK %.2e, against one level %.2e (bound %.0e); L^-1 %.2e (bound %.1e); L^-1 L - I %.2e (bound %.0e)" % (
        mid, name(dtype), np.abs(l_rec - want).max(), np.abs(l_rec - l_one).max(), tol, np.abs(m_rec - m_one).max(),
        tol * 10 * np.abs(m_one).max(), np.abs(m_rec @ l_rec - np.eye(NPAD)).max(), tol * 100))
    np.testing.assert_allclose(l_rec, want, atol=tol)
    np.testing.assert_allclose(l_rec, l_one, atol=tol)
    np.testing.assert_allclose(m_rec, m_one, atol=tol * 10 * np.abs(m_one).max())
    np.testing.assert_allclose(m_rec @ l_rec, np.eye(NPAD), atol=tol * 100)


# ------------------------------------------------------------------------------------------- f. a long triangle
@pytest.mark.parametrize("mid", ["se3", "X1", "R1"])
def test_long_triangle(ops, monkeypatch, mid):
    """n = 4000 in 4096, lower-only, fp64: 64 tile rows, 374 strips (290 interior, at every start tile 0 .. 54) -- kb_strip_of's square-root
    decode well past the small cases -- on FAST (se3), PROD (X1) and the matrix pipe (R1).  Every lower 64-tile against kernel_ref; no
    NaN there and nothing written above."""
    assert SHAPES["long"] == (1, NLONG, NLONG, NLONG_PAD, NLONG_PAD)
    x, hp, ref = sym_inputs(mid, NLONG, NLONG_PAD)
    monkeypatch.delenv("PG_KB_MFMA", raising=False)
    body = route(mid, F64, None)
    assert body == {"se3": "fast", "X1": "prod", "R1": "pipe"}[mid]
    tol = tol_of(mid, F64, body, ref[:NLONG, :NLONG], hp, x)
    low = build(ops, mid, hp, x, F64, lower_only=True, shape=(NLONG_PAD, NLONG_PAD))
    tl = tile_lower(NLONG_PAD)
    assert np.isnan(low[~tl]).all()
    close("%s f64 %s long triangle" % (mid, body), low, ref, tol, mask=tl)
