"""VarianceCache on the host: the dense restatement (tests/varcache_ref.py) shows the projection's properties on the project's n = 700
problems -- an upper bound, monotone in steps and in added anchors, bracketed from below by the certified gap, exact at full span --
and the class itself (pygpr_amd/varcache.py) runs on oracle ops against that restatement.  No GPU.

slack: sr.tol_of(err) * k**, err the disagreement of the restatement's two orthonormalisations (eigen-decomposition of the block's
Gram matrix, pivoted QR) relative to k**: the variance depends on the span alone, so that disagreement is the restatement's own error.
Every case prints what it measured."""
import functools

import numpy as np
import pytest
import torch

import iterative_ref as ir
import kernel_ref as kr
import matmul_ref as mr
import pygpr_amd as pg
import rowsq_ref as rr
import select_ref as sel
import sparse_ref as sr
import varcache_ref as vr
from kind_tools import cov_of
from oracle_ops import _np
from pygpr_amd import _lib, _ops, varcache
from pygpr_amd import iterative as it_mod
from test_dmatmul_cpu import DxOracleOps

MODELS = {"se+wn": ["se", "wn"], "m32+rq+wn": ["m32", "rq", "wn"], "se*per+wn": [("se", "per"), "wn"]}
T = torch.from_numpy


def test_the_public_surface():
    assert "VarianceCache" in pg.__all__ and pg.VarianceCache is varcache.VarianceCache
    assert callable(getattr(pg.Iterative_GP, "variance_cache", None)) and hasattr(_ops.HipOps, "kernel_rowsq")
    for name in ("variance", "covariance", "variance_grad", "check"):
        assert callable(getattr(pg.VarianceCache, name))
    assert "snapshot" in pg.Iterative_GP.variance_cache.__doc__.lower() and "variance_cache" in it_mod.__doc__
    assert varcache.NOVELTY_TOL == vr.NOVELTY_TOL and varcache._FLOOR1 == vr.FLOOR1
    for n, r in ((700, 123), (150, 150), (20000, 303)):
        assert varcache.floor_multiple(n, r) == vr.floor_multiple(n, r) == 4 * (n + 2 * r + 66)


# ------------------------------------------------------------------------------------------- the restatement's properties
@functools.lru_cache(maxsize=None)
def problem(name):
    terms = MODELS[name]
    hp, x, y, _ = sr.problem(terms, n=700, m=40)
    xp = np.random.default_rng(9).random((70, x.shape[1]))
    anchors = np.random.default_rng(10).random((64, x.shape[1]))
    return terms, hp, x, y, xp, anchors, ir.operator(terms, hp, x)


@functools.lru_cache(maxsize=None)
def walk(name, rank, with_anchors):
    """Steps 0 to 3 of one start block: per step (excess, upper - lower, lower - exact, err, rank, dropped)."""
    terms, hp, x, y, xp, anchors, a = problem(name)
    anc = anchors if with_anchors else None
    b0 = vr.start_block(terms, hp, x, y, rank, anc)
    out = []
    for steps in range(4):
        ce, cq, err = vr.own_error(terms, hp, x, y, rank, steps, xp, anc, a, b0)
        exact = ce.exact(xp)
        upper, lower = ce.variance(xp, bounds=True)
        out.append((upper - exact, upper - lower, lower - exact, err, ce.rank, ce.dropped, ce.kss, ce.floor_multiple))
    return out


@pytest.mark.parametrize("rank", [40, 100])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_upper_bound_monotone_bracketed(name, rank):
    plain, anch = walk(name, rank, False), walk(name, rank, True)
    for label, rows in (("no anchors", plain), ("64 anchors", anch)):
        for steps, (excess, gap, low, err, r, dropped, kss, fm) in enumerate(rows):
            slack = sr.tol_of(err) * kss
            ratio = float(np.max(gap / np.maximum(excess, slack)))
            print("%-10s rank %3d %s steps %d: r %3d dropped %3d  excess [%.1e, %.1e]  gap max %.1e (<= %.1f x excess)  lower - exact max %.1e  "
                  "err %.1e  floor multiple %d" % (name, rank, label, steps, r, dropped, excess.min(), excess.max(), gap.max(), ratio, low.max(), err, fm))
            assert np.all(excess >= -slack)                              # never under-reports
            assert np.all(low <= slack)                                  # the certified bracket
            assert np.all(gap > 0)
            if steps:
                slack2 = slack + sr.tol_of(rows[steps - 1][3]) * kss
                assert np.all(excess <= rows[steps - 1][0] + slack2)     # monotone in steps
    for steps in range(4):
        slack = (sr.tol_of(plain[steps][3]) + sr.tol_of(anch[steps][3])) * plain[steps][6]
        assert np.all(anch[steps][0] <= plain[steps][0] + slack)         # ... and in added anchors


def test_exact_once_the_span_is_everything():
    """n = 150, rank 49, steps 2: three blocks of 50 columns span R^150 and the cache is the dense answer, to the dense yardstick
    tests/test_iterative_gpu.py holds variances to (1e-11 absolute)."""
    terms = MODELS["se+wn"]
    hp, x, y, _ = sr.problem(terms, n=150, m=40)
    xp = np.random.default_rng(9).random((70, 3))
    ce, cq, err = vr.own_error(terms, hp, x, y, 49, 2, xp)
    cond = float(np.linalg.cond(ce.a))
    upper, lower = ce.variance(xp, bounds=True)
    dev = float(np.max(np.abs(upper - ce.exact(xp))))
    print("n = 150: rank %d, dropped %d, cond(A) %.0f, |var - exact| %.1e, gap max %.1e, err %.1e" % (ce.rank, ce.dropped, cond, dev,
                                                                                                 float((upper - lower).max()), err))
    assert ce.rank == cq.rank == 150 and ce.dropped == 0
    assert dev <= 1e-11
    assert np.all(lower <= ce.exact(xp) + 1e-11)


# ------------------------------------------------------------------------------------------- the class on oracle ops
class VcOracleOps(DxOracleOps):
    """DxOracleOps plus what the preconditioner and the cache call beyond it: the raw products, the matrix solve, the greedy
    selection and the squared row norms, in NumPy."""

    def gemm_raw(self, variant, m, n, k, alpha, a, b, beta, c, tri=0, klo=0, khi=0):
        assert tri == klo == khi == 0 and m % 128 == n % 128 == k % 128 == 0
        if variant in (_lib.GEMM_TN, _lib.GEMM_TN_64):
            prod = _np(a)[:k, :m].T @ _np(b)[:k, :n]
        elif variant == _lib.GEMM_NN:
            prod = _np(a)[:m, :k] @ _np(b)[:k, :n]
        else:
            assert variant == _lib.GEMM_NT
            prod = _np(a)[:m, :k] @ _np(b)[:n, :k].T
        assert np.isfinite(prod).all(), "a product read padding that nobody initialised"
        _np(c)[:m, :n] = alpha * prod + (beta * _np(c)[:m, :n] if beta != 0 else 0.0)

    def potrs(self, chol, invd, b, minv=None, triangular_only=False):
        import scipy.linalg as sla

        assert not triangular_only
        return torch.from_numpy(sla.cho_solve((np.tril(_np(chol)), True), _np(b), check_finite=False))

    def greedy_select_worksize(self, n, m_max):
        return 1

    def greedy_select(self, spec, hp, x, m_max, floor, work=None, out=None):
        model, h, _ = self._model(spec, _np(hp), x.shape[1])
        run = sel.greedy(model, h, _np(x), m_max, floor)
        c = len(run.piv)
        piv, trace = torch.full((m_max,), -77, dtype=torch.int32), torch.full((m_max,), float("nan"), dtype=torch.float64)
        piv[:c], trace[:c] = torch.from_numpy(run.piv.astype(np.int32)), torch.from_numpy(run.trace)
        return piv, torch.tensor([c], dtype=torch.int32), trace, torch.from_numpy(run.resid.copy())

    def kernel_rowsq_worksize(self, nr, nc):
        return 0

    def kernel_rowsq(self, spec, hp, xr, xc, out=None, work=None):
        x = _np(xr)
        model, h, _ = self._model(spec, _np(hp), x.shape[1])
        res = torch.from_numpy(np.ascontiguousarray(rr.rowsq(model, h, x, _np(xc))))
        return res if out is None else out.copy_(res)


@pytest.fixture
def vc_ops(monkeypatch):
    ops = VcOracleOps()
    monkeypatch.setattr(_ops, "_OPS", ops)
    monkeypatch.setattr(it_mod, "_RHS_BLOCK", 32)
    return ops


@functools.lru_cache(maxsize=None)
def small(name, n=180):
    terms = MODELS[name]
    hp, x, y, _ = sr.problem(terms, n=700, m=40)
    rng = np.random.default_rng(12)
    return terms, hp, x[:n], y[:n], rng.random((37, 3)), rng.random((9, 3))


def fit(terms, hp, x, y, rank, tol=1e-9):
    model = pg.Iterative_GP(T(x), T(y), cov_of(terms), rank=rank, tol=tol)
    model.set_params(T(hp))
    return model


@pytest.mark.parametrize("name,rank,steps,with_anchors", [("se+wn", 12, 2, False), ("m32+rq+wn", 12, 1, True), ("se*per+wn", 0, 2, True),
                                                          ("se+wn", 12, 0, True)])
def test_the_class_on_oracle_ops_against_the_restatement(vc_ops, name, rank, steps, with_anchors):
    terms, hp, x, y, xp, anchors = small(name)
    anc = anchors if with_anchors else None
    model = fit(terms, hp, x, y, rank)
    vc = model.variance_cache(steps=steps, anchors=None if anc is None else T(anc))
    ce, cq, err = vr.own_error(terms, hp, x, y, rank, steps, xp, anc)
    tol = sr.tol_of(err) * ce.kss
    print("%s rank %d steps %d anchors %s: cache rank %d, info %s, err %.1e" % (name, rank, steps, with_anchors, vc.rank, vc.info, err))
    assert vc.rank == ce.rank and vc.info["dropped"] == ce.dropped == 0 and vc.info["width"] == rank + 1 + (9 if with_anchors else 0)
    assert vc.info["products"] == vc.rank and vc.info["orthogonality"] <= 1e-12 and vc.info["floor_multiple"] == ce.floor_multiple
    assert vc.info["bytes"] == 8 * (2 * 256 * 256 + 2 * 256 * 256)
    assert vc.info["pinned_bytes"] >= 8 * (180 * 3 + 180 + (2 * 256 * 256 if rank else 0))       # the points, alpha, and L and C at rank > 0
    var = vc.variance(T(xp))
    upper, lower = vc.variance(T(xp), bounds=True)
    ru, rl = ce.variance(xp, bounds=True)
    assert torch.equal(var, upper) and var.shape == (37,) and var.dtype == torch.float64
    for label, got, ref in (("upper", upper, ru), ("lower", lower, rl), ("covariance", vc.covariance(T(xp)), ce.covariance(xp))):
        e = float(np.max(np.abs(got.numpy() - ref)))
        print("  %-10s err %.2e (tol %.2e)" % (label, e, tol))
        assert e <= tol
    cov = vc.covariance(T(xp)).numpy()
    assert np.array_equal(cov, cov.T) and np.max(np.abs(np.diag(cov) - var.numpy())) <= tol
    # the gradient: the value's bits, and central differences of the restatement
    v2, dvar = vc.variance_grad(T(xp))
    assert torch.equal(v2, var) and dvar.shape == (37, 3)
    fd = {}
    for h in (1e-5, 2e-5):
        cols = []
        for k in range(3):
            e = np.zeros(3)
            e[k] = h
            cols.append((ce.variance(xp + e) - ce.variance(xp - e)) / (2 * h))
        fd[h] = np.stack(cols, 1)
    trunc = float(np.max(np.abs(fd[2e-5] - fd[1e-5]))) * 4.0 / 3.0      # the h^2 term of the coarser step: above the finer step's
    e = float(np.max(np.abs(dvar.numpy() - fd[1e-5])))
    bound = trunc + tol
    print("  gradient   err %.2e (truncation estimate %.2e, bound %.2e)" % (e, trunc, bound))
    assert e <= bound
    # check(): the model's own block solve
    res = vc.check(T(xp[:32]))
    exact = ce.exact(xp[:32])
    cond = float(np.linalg.cond(ce.a))
    slack = tol + 2 * cond * 1e-9 * ce.kss + 1e-11                        # (the model's solves stop at 1e-9 here)
    assert abs(res["excess"] - float(np.max(ru[:32] - exact))) <= slack and abs(res["gap"] - float(np.max((ru - rl)[:32]))) <= tol
    with pytest.raises(ValueError, match="at most 32"):
        vc.check(T(xp))


def test_snapshot_refusals_and_a_duplicated_anchor(vc_ops):
    terms, hp, x, y, xp, anchors = small("se+wn")
    model = fit(terms, hp, x, y, 12)
    before = model.predict(T(xp[:5]), var="diag")
    vc = model.variance_cache(steps=1, anchors=T(anchors), bounds=False)
    assert all(torch.equal(a, b) for a, b in zip(before, model.predict(T(xp[:5]), var="diag")))      # predict keeps its solves and bits
    assert vc.info["bytes"] == 8 * 256 * 256
    var = vc.variance(T(xp))
    with pytest.raises(ValueError, match="bounds=False"):
        vc.variance(T(xp), bounds=True)
    assert vc.check(T(xp[:5]))["gap"] is None
    # a duplicated anchor is dropped, not kept at tiny norm; the variances are those of the cache without it
    dup = model.variance_cache(steps=1, anchors=T(np.concatenate([anchors, anchors[3:4]])), bounds=False)
    assert dup.info["dropped"] >= 1 and dup.rank == vc.rank
    d2 = dup.variance(T(xp))
    assert bool(torch.isfinite(d2).all()) and float((d2 - var).abs().max()) <= 1e-10 * 2.0
    # the snapshot: other parameters on the model, the same bits from the old cache
    model.set_params(T(hp * 1.1))
    assert model.need_upd
    model.update()
    assert torch.equal(vc.variance(T(xp)), var)
    assert not torch.equal(model.variance_cache(steps=1, anchors=T(anchors), bounds=False).variance(T(xp)), var)
    # refusals
    with pytest.raises(ValueError, match="max_columns"):
        model.variance_cache(steps=2, anchors=T(anchors), max_columns=3 * (12 + 1 + 9) - 1)
    model.variance_cache(steps=2, anchors=T(anchors), max_columns=3 * (12 + 1 + 9), bounds=False)
    with pytest.raises(ValueError, match="steps"):
        model.variance_cache(steps=-1)
    with pytest.raises(TypeError, match="float64 only"):
        vc.variance(T(xp).float())
    with pytest.raises(NotImplementedError, match="no batches"):
        vc.variance(T(xp)[None])
    with pytest.raises(NotImplementedError, match="no batches"):
        model.variance_cache(anchors=T(anchors[:, :2]))
    with pytest.raises(TypeError, match="float64 only"):
        model.variance_cache(anchors=T(anchors).float())


def test_full_span_on_oracle_ops(vc_ops):
    """n = 150, rank 49, steps 2 through the class: three blocks of 50 columns, rank 150, the dense answer."""
    terms = MODELS["se+wn"]
    hp, x, y, _ = sr.problem(terms, n=150, m=40)
    xp = np.random.default_rng(9).random((70, 3))
    model = fit(terms, hp, x, y, 49)
    vc = model.variance_cache(steps=2)
    _, cov = kr.predict(terms, hp, x, y, xp, var="full")
    upper, lower = vc.variance(T(xp), bounds=True)
    dev = float(np.max(np.abs(upper.numpy() - np.diag(cov))))
    print("n = 150 through the class: rank %d, |var - exact| %.1e, gap max %.1e, info %s" % (vc.rank, dev, float((upper - lower).max()), vc.info))
    assert vc.rank == 150 and vc.info["dropped"] == 0 and dev <= 1e-11
    more = model.variance_cache(steps=3)                                  # the span is everything: a further step adds nothing
    assert more.rank == 150 and more.info["products"] == 150
