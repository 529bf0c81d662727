"""VarianceCache on the MI355X: the device's variances, covariances and certified bounds against the dense restatement
(tests/varcache_ref.py) on the same start block, against the dense answer (tests/kernel_ref.py), against the model's own block solve,
its gradient, its snapshot semantics, its refusals and the memory claim.

Setup: tests/test_iterative_gpu.py's -- n = 700, d = 3, 70 test points from default_rng(9), tol = 1e-10, _RHS_BLOCK lowered to 32 --
plus 64 anchors from default_rng(10).

Bounds (none is fitted; every test prints what it measured):
  restatement  tol = sr.tol_of(err) * k**: err is the disagreement of the restatement's two orthonormalisations relative to k** (the
               variance depends on the span alone, so that is the restatement's own error); the rule's floor is 1e-10 relative.  The
               cases keep every direction (dropped == 0 is asserted: a drop is a decision at a threshold, which two roundings may take
               differently); the se+wn problem at rank 100 with 64 anchors drops only from steps = 3 on.
  dense        slack = tol + 2 cond(A) TOL max|ref| + 1e-11: test_iterative_gpu.py's variance yardstick for what a solve at TOL leaves
               (the cache solves nothing, the yardstick covers kernel_ref's own factorisation and the device's covariance values).
  gradient     central differences of the restatement's variance at h = 1e-5: their truncation, estimated from a second step 2 h
               (4/3 |fd(2h) - fd(h)|, the h^2 term at the coarser step, an upper estimate of the finer step's), plus tol.
  monotone     two device values, each within slack of its own exact figure, whose exact figures are ordered: upper_s <= upper_s-1 +
               slack_s + slack_s-1."""
import functools

import numpy as np
import pytest
import torch

import iterative_ref as ir
import kernel_ref as kr
import pygpr_amd as pg
import sparse_ref as sr
import varcache_ref as vr
from kind_tools import N, T, cov_of, ops  # noqa: F401  (ops: the module's fixture)
from pygpr_amd import iterative as it_mod

pytestmark = pytest.mark.gpu

MODELS = {"se+wn": ["se", "wn"], "m32+rq+wn": ["m32", "rq", "wn"], "se*per+wn": [("se", "per"), "wn"]}
TOL = 1e-10


@functools.lru_cache(maxsize=None)
def case(name, n=700):
    """The problem and the dense answers, computed once per model."""
    terms = MODELS[name]
    hp, x, y, _ = sr.problem(terms, n=n, m=40)
    xp = np.random.default_rng(9).random((70, x.shape[1]))
    anchors = np.random.default_rng(10).random((64, x.shape[1]))
    a = ir.operator(terms, hp, x)
    _, cov = kr.predict(terms, hp, x, y, xp, var="full")
    return terms, hp, x, y, xp, anchors, a, float(np.linalg.cond(a)), np.diag(cov).copy()


@functools.lru_cache(maxsize=None)
def fitted(name, rank, n=700):
    terms, hp, x, y, *_ = case(name, n)
    model = pg.Iterative_GP(T(x), T(y), cov_of(terms), rank=rank, tol=TOL)
    model.set_params(T(hp))
    model.update()
    return model


@functools.lru_cache(maxsize=None)
def start(name, rank, with_anchors, n=700):
    terms, hp, x, y, xp, anchors, *_ = case(name, n)
    return vr.start_block(terms, hp, x, y, rank, anchors if with_anchors else None)


@functools.lru_cache(maxsize=None)
def restated(name, rank, steps, with_anchors, n=700):
    """(the restatement's cache, its own error), computed once per case."""
    terms, hp, x, y, xp, anchors, a, *_ = case(name, n)
    ce, _, err = vr.own_error(terms, hp, x, y, rank, steps, xp, anchors if with_anchors else None, a, start(name, rank, with_anchors, n))
    return ce, err


def build(name, rank, steps, with_anchors, n=700, **kw):
    anchors = case(name, n)[5]
    return fitted(name, rank, n).variance_cache(steps=steps, anchors=T(anchors) if with_anchors else None, **kw)


@pytest.fixture(autouse=True)
def small_blocks(monkeypatch):
    monkeypatch.setattr(it_mod, "_RHS_BLOCK", 32)


def dense_slack(name, tol):
    *_, cond, exact = case(name)
    return tol + 2 * cond * TOL * float(np.max(np.abs(exact))) + 1e-11


GRID = [(name, rank, steps, anc) for name in sorted(MODELS) for rank in (40, 100) for steps in (0, 2) for anc in (False, True)]


@pytest.mark.parametrize("name,rank,steps,with_anchors", GRID, ids=["%s-%d-%d-%s" % (c[:3] + ("anchors" if c[3] else "plain",)) for c in GRID])
def test_against_the_restatement(ops, name, rank, steps, with_anchors):
    xp = case(name)[4]
    ce, err = restated(name, rank, steps, with_anchors)
    tol = sr.tol_of(err) * ce.kss
    vc = build(name, rank, steps, with_anchors)
    print("%s rank %d steps %d anchors %s: cache rank %d, err %.1e, tol %.1e, info %s" % (name, rank, steps, with_anchors, vc.rank, err, tol, vc.info))
    assert ce.dropped == 0 and vc.info["dropped"] == 0 and vc.rank == ce.rank == (steps + 1) * (rank + 1 + (64 if with_anchors else 0))
    assert vc.info["products"] == vc.rank and vc.info["floor_multiple"] == ce.floor_multiple and vc.info["orthogonality"] <= 1e-12
    var = N(vc.variance(T(xp)))
    upper, lower = (N(t) for t in vc.variance(T(xp), bounds=True))
    cov = N(vc.covariance(T(xp)))
    ru, rl = ce.variance(xp, bounds=True)
    assert var.tobytes() == upper.tobytes() and var.shape == (70,)
    for label, got, ref in (("upper", upper, ru), ("lower", lower, rl), ("covariance", cov, ce.covariance(xp)), ("its diagonal", np.diag(cov), var)):
        e = float(np.max(np.abs(got - ref)))
        print("  %-12s err %.2e (tol %.2e)" % (label, e, tol))
        assert e <= tol, (label, e, tol)
    assert np.array_equal(cov, cov.T)                               # mirrored: exactly symmetric
    assert np.all(lower < upper)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_from_above_bracketed_and_monotone_against_the_dense_answer(ops, name):
    *_, xp, _, _, cond, exact = case(name)
    prev = prev_slack = None
    for steps in (0, 1, 2):
        ce, err = restated(name, 40, steps, False)
        slack = dense_slack(name, sr.tol_of(err) * ce.kss)
        upper, lower = (N(t) for t in build(name, 40, steps, False).variance(T(xp), bounds=True))
        excess, gap = upper - exact, upper - lower
        print("%-10s steps %d: excess [%.1e, %.1e]  gap max %.1e (<= %.1f x excess)  lower - exact max %.1e  (slack %.1e, cond %.0f)"
              % (name, steps, excess.min(), excess.max(), gap.max(), float(np.max(gap / np.maximum(excess, slack))), float((lower - exact).max()),
                 slack, cond))
        assert np.all(upper >= exact - slack)                       # from above
        assert np.all(lower <= exact + slack)                       # the bracket
        if prev is not None:
            assert np.all(upper <= prev + slack + prev_slack)       # monotone in steps: one slack for each of the two values
        prev, prev_slack = upper, slack


def test_exact_at_full_span(ops):
    """n = 150, rank 49, steps 2: three blocks of 50 columns are R^150."""
    name, n = "se+wn", 150
    *_, xp, _, _, cond, exact = case(name, n)
    vc = build(name, 49, 2, False, n=n)
    upper, lower = (N(t) for t in vc.variance(T(xp), bounds=True))
    bound = 2 * cond * TOL * float(np.max(np.abs(exact))) + 1e-11
    dev = float(np.max(np.abs(upper - exact)))
    print("n = 150: rank %d, cond(A) %.0f, |var - exact| %.1e (bound %.1e), gap max %.1e, info %s" % (vc.rank, cond, dev, bound,
                                                                                                float((upper - lower).max()), vc.info))
    assert vc.rank == 150 and vc.info["dropped"] == 0
    assert dev <= bound and np.all(lower <= exact + bound)


def test_a_duplicated_anchor_is_dropped(ops):
    name = "se+wn"
    terms, hp, x, y, xp, anchors, *_ = case(name)
    ce, err = restated(name, 40, 2, True)
    tol = sr.tol_of(err) * ce.kss
    model = fitted(name, 40)
    dup = model.variance_cache(steps=2, anchors=T(np.concatenate([anchors, anchors[7:8]])))
    upper, lower = (N(t) for t in dup.variance(T(xp), bounds=True))
    ref_u, ref_l = (N(t) for t in build(name, 40, 2, True).variance(T(xp), bounds=True))
    print("duplicated anchor: dropped %d, rank %d (without it %d), |upper - upper'| %.1e, |lower - lower'| %.1e (tol %.1e)"
          % (dup.info["dropped"], dup.rank, ce.rank, np.max(np.abs(upper - ref_u)), np.max(np.abs(lower - ref_l)), tol))
    assert dup.info["dropped"] >= 1 and dup.info["width"] == 40 + 1 + 65
    assert np.isfinite(upper).all() and np.isfinite(lower).all() and np.isfinite(N(dup.covariance(T(xp)))).all()
    assert np.max(np.abs(upper - ref_u)) <= tol and np.max(np.abs(lower - ref_l)) <= tol


def test_the_gradient(ops):
    name = "se+wn"
    xp = case(name)[4]
    ce, err = restated(name, 40, 2, True)
    tol = sr.tol_of(err) * ce.kss
    vc = build(name, 40, 2, True)
    var, dvar = vc.variance_grad(T(xp))
    assert N(var).tobytes() == N(vc.variance(T(xp))).tobytes() and dvar.shape == (70, 3) and dvar.dtype == torch.float64
    h, fd = 1e-5, {}
    for step in (h, 2 * h):
        cols = []
        for k in range(3):
            e = np.zeros(3)
            e[k] = step
            cols.append((ce.variance(xp + e) - ce.variance(xp - e)) / (2 * step))
        fd[step] = np.stack(cols, 1)
    trunc = 4.0 / 3.0 * float(np.max(np.abs(fd[2 * h] - fd[h])))
    bound = trunc + tol
    e = float(np.max(np.abs(N(dvar) - fd[h])))
    print("gradient: err %.2e of max %.2e (bound %.2e: truncation estimate %.2e, tol %.2e)" % (e, np.abs(fd[h]).max(), bound, trunc, tol))
    assert e <= bound


def test_check_is_the_models_own_block_solve(ops):
    name = "se+wn"
    xp = case(name)[4]
    ce, err = restated(name, 40, 2, False)
    slack = dense_slack(name, sr.tol_of(err) * ce.kss)
    vc = build(name, 40, 2, False)
    res = vc.check(T(xp[:32]))
    solved = N(fitted(name, 40).predict(T(xp[:32]), var="diag")[1])
    upper, lower = (N(t) for t in vc.variance(T(xp[:32]), bounds=True))
    print("check: excess %.3e (from predict %.3e), gap %.3e (slack %.1e)" % (res["excess"], float(np.max(upper - solved)), res["gap"], slack))
    assert abs(res["excess"] - float(np.max(upper - solved))) <= slack
    assert abs(res["gap"] - float(np.max(upper - lower))) <= slack and res["excess"] <= res["gap"] + slack
    with pytest.raises(ValueError, match="at most 32"):
        vc.check(T(xp))


def test_a_cache_is_a_snapshot_and_leaves_predict_alone(ops):
    name = "se+wn"
    terms, hp, x, y, xp, *_ = case(name)
    model = pg.Iterative_GP(T(x), T(y), cov_of(terms), rank=40, tol=TOL)
    model.set_params(T(hp))
    before = [N(t) for t in model.predict(T(xp), var="diag")]
    vc = model.variance_cache(steps=1)
    after = [N(t) for t in model.predict(T(xp), var="diag")]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
    old = [N(t) for t in vc.variance(T(xp), bounds=True)]
    model.set_params(T(hp * 1.15))
    model.update()
    again = [N(t) for t in vc.variance(T(xp), bounds=True)]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(old, again))
    fresh = N(model.variance_cache(steps=1).variance(T(xp)))
    assert np.max(np.abs(fresh - old[0])) > 1e-6                   # ... while a new cache sees the new parameters


def test_refusals_and_rank_zero(ops):
    name = "se+wn"
    terms, hp, x, y, xp, anchors, *_ = case(name)
    model = fitted(name, 40)
    with pytest.raises(ValueError, match="max_columns"):
        model.variance_cache(steps=2, anchors=T(anchors), max_columns=3 * 105 - 1)
    plain = model.variance_cache(steps=0, bounds=False)
    with pytest.raises(ValueError, match="bounds=False"):
        plain.variance(T(xp), bounds=True)
    assert plain.check(T(xp[:4]))["gap"] is None
    for call in (plain.variance, plain.covariance, plain.variance_grad, plain.check):
        with pytest.raises(NotImplementedError):
            call(T(xp[:, :2]))
        with pytest.raises(TypeError):
            call(T(xp).float())
    with pytest.raises(TypeError):
        model.variance_cache(anchors=T(anchors).float())
    # rank 0: no factor, the start block is [y | k(X, anchors)]
    ce, err = restated(name, 0, 1, True)
    vc = build(name, 0, 1, True)
    tol = sr.tol_of(err) * ce.kss
    upper, lower = (N(t) for t in vc.variance(T(xp), bounds=True))
    ru, rl = ce.variance(xp, bounds=True)
    print("rank 0: cache rank %d, upper err %.1e, lower err %.1e (tol %.1e)" % (vc.rank, np.max(np.abs(upper - ru)), np.max(np.abs(lower - rl)), tol))
    assert vc.info["width"] == 65 and vc.rank == ce.rank == 130
    assert np.max(np.abs(upper - ru)) <= tol and np.max(np.abs(lower - rl)) <= tol


def test_no_n_by_n_array_at_n_20000(ops):
    """update() plus a cache of rank 100, steps 2 with bounds at n = 20000 raises the peak of allocated device memory by less than
    8 n^2 / 8 bytes (400 MB, DESIGN 4.21's condition for the solver's buffers) plus the two n x r arrays the cache keeps."""
    n, d = 20000, 3
    rng = np.random.default_rng(2)
    x = rng.random((n, d))
    y = np.sin(3.0 * x.sum(1)) + 0.1 * rng.standard_normal(n)
    hp = np.array([1.0, 2.6, 2.8, 2.7, 0.3])
    xp = rng.random((64, d))
    xt, yt, xpt = T(x).cuda(), T(y).cuda(), T(xp).cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    model = pg.Iterative_GP(xt, yt, cov_of(["se", "wn"]), rank=100, tol=1e-8)
    model.set_params(T(hp))
    vc = model.variance_cache(steps=2, bounds=True)
    upper, lower = vc.variance(xpt, bounds=True)
    torch.cuda.synchronize()
    used = torch.cuda.max_memory_allocated() - before
    kept = 2 * 8 * n * vc.rank
    print("n = %d: cache rank %d, peak memory + %.1f MB (bound %.0f MB = 400 + %.0f), held %.1f MB, gap max %.1e, info %s"
          % (n, vc.rank, used / 1e6, (8 * n * n // 8 + kept) / 1e6, kept / 1e6, vc.info["bytes"] / 1e6, float((upper - lower).max()), vc.info))
    assert used < 8 * n * n // 8 + kept
    assert bool(torch.isfinite(upper).all()) and bool((upper > 0).all()) and bool((lower < upper).all())
