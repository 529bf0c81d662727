"""Iterative_GP on the MI355X: the fitted weights and every prediction against the dense NumPy restatement (tests/kernel_ref.py) and
against Exact_GP on the device, the solver's iteration counts against its restatement (tests/iterative_ref.py), its failure path, the
refusals, and the memory claim.

Setup: n = 700, d = 3, 70 test points, _RHS_BLOCK lowered to 32 (three blocks of test points, the last of 6), tol = 1e-10.

Bounds (none is fitted; every test prints what it measured):
  residual   ||y - A alpha|| / ||y||, formed in NumPy from the device's alpha and the dense A, is at most 2 tol.
  accuracy   a solve stopped at relative residual tol is within cond(A) tol of the solution; twice that, relative to the largest
             reference entry, plus the dense yardstick tests/test_parity_gpu.py holds Exact_GP to at this size: weights rtol 1e-8, mean
             atol 1e-10, variance and covariance atol 1e-11.  cond(A) is computed here, by NumPy, per model.
  iterations at most the restatement's count plus max(2, 10 %): the device's sums run in another order."""
import functools

import numpy as np
import pytest
import torch

import iterative_ref as ir
import kernel_ref as kr
import pygpr_amd as pg
import sparse_ref as sr
from kind_tools import N, T, cov_of, ops  # noqa: F401  (ops: the module's fixture)
from pygpr_amd import iterative as it_mod

pytestmark = pytest.mark.gpu

MODELS = {"se+wn": ["se", "wn"], "m32+rq+wn": ["m32", "rq", "wn"], "se*per+wn": [("se", "per"), "wn"]}
TOL = 1e-10
RANK = 40


@functools.lru_cache(maxsize=None)
def case(name):
    """The problem and the dense answers, computed once per model."""
    terms = MODELS[name]
    hp, x, y, _ = sr.problem(terms, n=700, m=40)
    xp = np.random.default_rng(9).random((70, x.shape[1]))
    a = ir.operator(terms, hp, x)
    cond = float(np.linalg.cond(a))
    _, alpha = kr.factor(terms, hp, x, y)
    mu, cov = kr.predict(terms, hp, x, y, xp, var="full")
    return terms, hp, x, y, xp, a, cond, alpha, mu, cov


@functools.lru_cache(maxsize=None)
def fitted(name, rank=RANK):
    terms, hp, x, y, *_ = case(name)
    model = pg.Iterative_GP(T(x), T(y), cov_of(terms), rank=rank, tol=TOL)
    model.set_params(T(hp))
    model.update()
    return model


@pytest.fixture(autouse=True)
def small_blocks(monkeypatch):
    monkeypatch.setattr(it_mod, "_RHS_BLOCK", 32)


def held(label, got, ref, cond, yard_abs=0.0, yard_rel=0.0):
    scale = float(np.max(np.abs(ref)))
    bound = 2 * cond * TOL * scale + yard_abs + yard_rel * scale
    err = float(np.max(np.abs(got - ref)))
    print("%-34s err %.2e  (bound %.2e: cond %.2e)" % (label, err, bound, cond))
    assert err <= bound, (label, err, bound)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_weights_and_predictions_against_the_dense_restatement(ops, name):
    terms, hp, x, y, xp, a, cond, alpha, mu, cov = case(name)
    model = fitted(name)
    got = N(model.alpha)
    res = float(np.linalg.norm(y - a @ got) / np.linalg.norm(y))
    info = model.cg_info
    print("%s: %d iterations at rank %d, residual reported %.2e, recomputed %.2e" % (name, info["iterations"], info["rank"], info["residual"], res))
    assert res <= 2 * TOL and info["residual"] <= 2 * TOL and info["rank"] == RANK
    held(name + " alpha", got, alpha, cond, yard_rel=1e-8)
    m0, none = model.predict(T(xp), var="none")
    assert none is NotImplemented
    m1, vd = model.predict(T(xp), var="diag")
    m2, vf = model.predict(T(xp), var="full")
    assert N(m0).tobytes() == N(m1).tobytes() == N(m2).tobytes()
    held(name + " mean", N(m1), mu, cond, yard_abs=1e-10)
    held(name + " variance", N(vd), np.diag(cov), cond, yard_abs=1e-11)
    held(name + " covariance", N(vf), cov, cond, yard_abs=1e-11)
    assert np.array_equal(N(vf), N(vf).T)                       # mirrored over the blocks: exactly symmetric
    assert N(model.predict_var(T(xp))).tobytes() == N(vd).tobytes() and N(model.predict_covar(T(xp))).tobytes() == N(vf).tobytes()


@pytest.mark.parametrize("name", sorted(MODELS))
def test_agreement_with_exact_gp_on_the_device(ops, name):
    terms, hp, x, y, xp, a, cond, *_ = case(name)
    exact = pg.Exact_GP(T(x), T(y), cov_of(terms))
    exact.set_params(T(hp))
    mu_e, var_e = exact.predict(T(xp), var="diag")
    mu_i, var_i = fitted(name).predict(T(xp), var="diag")
    held(name + " mean vs Exact_GP", N(mu_i), N(mu_e), cond, yard_abs=1e-10)
    held(name + " variance vs Exact_GP", N(var_i), N(var_e), cond, yard_abs=1e-11)


def test_the_preconditioner_cuts_the_iterations_as_the_restatement_says(ops):
    terms, hp, x, y, *_ = case("se+wn")
    with_pre, plain = fitted("se+wn").cg_info, fitted("se+wn", 0).cg_info
    _, it_pre, _ = ir.fit(terms, hp, x, y, RANK, TOL)
    _, it_plain, _ = ir.fit(terms, hp, x, y, 0, TOL)
    print("iterations  device: rank %d %d, rank 0 %d;  restatement: %d, %d" % (RANK, with_pre["iterations"], plain["iterations"], it_pre, it_plain))
    assert plain["rank"] == 0 and with_pre["iterations"] < plain["iterations"]
    assert with_pre["iterations"] <= it_pre + max(2, 0.1 * it_pre)
    assert plain["iterations"] <= it_plain + max(2, 0.1 * it_plain)


def test_a_solve_that_does_not_converge_raises_and_leaves_the_model_dirty(ops):
    terms, hp, x, y, xp, a, cond, alpha, mu, cov = case("se+wn")
    model = pg.Iterative_GP(T(x), T(y), cov_of(terms), rank=RANK, tol=TOL, max_iter=2)
    model.set_params(T(hp))
    with pytest.raises(pg.NotConverged) as e:
        model.update()
    assert isinstance(e.value, torch.linalg.LinAlgError) and e.value.iterations == 2 and e.value.residual > TOL
    assert model.need_upd
    with pytest.raises(pg.NotConverged):          # a dirty model refits on predict, as Exact_GP does: the same failure
        model.predict(T(xp), var="diag")
    model.max_iter = 1000
    model.update()
    assert not model.need_upd
    held("after raising max_iter: mean", N(model.predict(T(xp), var="none")[0]), mu, cond, yard_abs=1e-10)


def test_refusals(ops):
    terms, hp, x, y, xp, *_ = case("se+wn")
    cov = cov_of(terms)
    with pytest.raises(NotImplementedError):
        pg.Iterative_GP(T(x).reshape(2, 350, 3), T(y).reshape(2, 350), cov)
    with pytest.raises(TypeError):
        pg.Iterative_GP(T(x).float(), T(y).float(), cov)
    with pytest.raises(NotImplementedError):
        pg.Iterative_GP(T(x), T(y), pg.Compose([pg.Squared_exponential() for _ in range(5)] + [pg.White_noise()]))
    model = pg.Iterative_GP(T(x), T(y), cov, rank=RANK, tol=TOL)
    model.set_params(T(np.stack([hp, hp])))
    with pytest.raises(NotImplementedError):      # batched hyper-parameters
        model.update()
    model.set_params(T(hp))
    with pytest.raises(TypeError):
        model.predict(T(xp).float(), var="diag")
    with pytest.raises(NotImplementedError):
        model.predict(T(xp).reshape(2, 35, 3), var="diag")
    with pytest.raises(NotImplementedError):
        model.predict(T(xp).clone().requires_grad_(True), var="diag")
    for call in (lambda: model.append(T(x[:2]), T(y[:2])), model.loo_predict, lambda: model.sampler(T(xp)), lambda: pg.MLE(model),
                 lambda: pg.LOO(model)):
        with pytest.raises(NotImplementedError):
            call()


def test_a_covariance_without_noise_is_legal(ops):
    """The shift is JITTER alone: A = k(x, x) + JITTER I, here for a rough kernel whose spectrum keeps A within reach of the solver."""
    rng = np.random.default_rng(4)
    x = rng.random((120, 3))
    y = np.sin(3 * x.sum(1))
    hp = np.array([1.0, 2.5, 2.5, 2.5])
    model = pg.Iterative_GP(T(x), T(y), pg.Matern12(), rank=30, tol=1e-8)
    model.set_params(T(hp))
    model.update()
    a = ir.operator(["m12"], hp, x)
    res = float(np.linalg.norm(y - a @ N(model.alpha)) / np.linalg.norm(y))
    print("m12 without noise: %d iterations at rank %d, residual %.2e" % (model.cg_info["iterations"], model.cg_info["rank"], res))
    assert res <= 2e-8


def test_no_n_by_n_array_at_n_20000(ops):
    """update() plus predict(64 points, "diag") at n = 20000, rank 100 raises the peak of allocated device memory by less than
    8 n^2 / 8 bytes (400 MB): one eighth of ONE n x n matrix.  Expected: L (n x 256), six n x 128 solver buffers, the selection's
    factor -- some 200 MB."""
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
    model.update()
    mu, var = model.predict(xpt, var="diag")
    torch.cuda.synchronize()
    used = torch.cuda.max_memory_allocated() - before
    print("n = %d: %d iterations, residual %.2e, peak memory + %.1f MB (bound %.0f MB)" % (n, model.cg_info["iterations"], model.cg_info["residual"],
                                                                                       used / 1e6, n * n / 1e6))
    assert used < 8 * n * n // 8
    assert model.cg_info["residual"] <= 2e-8 and bool(torch.isfinite(mu).all()) and bool((var > 0).all())
