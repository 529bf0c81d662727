"""Iterative_GP.function_samples on the MI355X: the features against their restatement, the samples against the dense pathwise formula
(tests/pathwise_ref.py), reproducibility, the prior, the first two moments, the memory claim and the interface.

Setup: tests/test_iterative_gpu.py's -- n = 700, d = 3, 70 test points, tol = 1e-10, rank 40 -- with _RHS_BLOCK lowered to 4, so that
five samples span two block solves.

Bounds (none is fitted; every test prints what it measured):
  features   2e-13 of the largest frequency: tests/test_sample_gpu.py's 5e-14 for the device's normals against the restatement's, times
             4 for the square sum, the root and the quotient that follow.
  identity   a solve stopped at relative residual tol is within cond(A) tol of the solution; twice that, relative to the largest
             reference entry, plus atol 1e-10: test_iterative_gpu.held's bound for the mean.  The reported true residual is <= 2 tol.
  moments    given the frequencies the samples are exactly Gaussian with predict's mean and pathwise_ref.sampler_cov's variance v_j:
             over S samples the empirical mean is within 6 sqrt(v_j / S), the empirical variance within 6 v_j sqrt(2 / (S - 1)) --
             140 comparisons at six standard deviations."""
import functools

import numpy as np
import pytest
import torch

import feature_ref as fr
import iterative_ref as ir
import kernel_ref as kr
import pathwise_ref as pr
import pygpr_amd as pg
import sparse_ref as sr
from kind_tools import N, T, cov_of, ops  # noqa: F401  (ops: the module's fixture)
from pygpr_amd import iterative as it_mod
from test_iterative_gpu import held

pytestmark = pytest.mark.gpu

MODELS = {"se+wn": ["se", "wn"], "m32+m52+wn": ["m32", "m52", "wn"]}
TOL = 1e-10
RANK = 40
SEED = 11


@functools.lru_cache(maxsize=None)
def case(name):
    """The problem and the dense answers, computed once per model."""
    terms = MODELS[name]
    hp, x, y, _ = sr.problem(terms, n=700, m=40)
    xp = np.random.default_rng(9).random((70, x.shape[1]))
    cond = float(np.linalg.cond(ir.operator(terms, hp, x)))
    mu, _ = kr.predict(terms, hp, x, y, xp, var="diag")
    return terms, hp, x, y, xp, cond, mu


@functools.lru_cache(maxsize=None)
def fitted(name):
    terms, hp, x, y, *_ = case(name)
    model = pg.Iterative_GP(T(x), T(y), cov_of(terms), rank=RANK, tol=TOL)
    model.set_params(T(hp))
    model.update()
    return model


@functools.lru_cache(maxsize=None)
def drawn(name, n_samples, features, seed=SEED):
    """(FunctionSamples, its values at the 70 test points [n_samples, 70]) at _RHS_BLOCK = 4."""
    saved, it_mod._RHS_BLOCK = it_mod._RHS_BLOCK, 4
    try:
        fs = fitted(name).function_samples(n_samples, features, seed)
    finally:
        it_mod._RHS_BLOCK = saved
    return fs, N(fs(T(case(name)[4])))


@pytest.fixture(autouse=True)
def small_blocks(monkeypatch):
    monkeypatch.setattr(it_mod, "_RHS_BLOCK", 4)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_the_features_are_the_restatements(ops, name):
    terms, hp, x, *_ = case(name)
    fs, _ = drawn(name, 5, 64)
    nu, u, amp = pr.spectral_features(terms, hp, 3, 64, SEED)
    err = float(np.max(np.abs(fs.frequencies - nu)) / np.max(np.abs(nu)))
    print("%-12s frequencies: %.2e of the largest  (bound 2e-13)" % (name, err))
    assert fs.frequencies.shape == nu.shape and err <= 2e-13
    assert np.array_equal(fs.phases, u)
    w = pr.weights(SEED, nu.shape[0], 5, amp)
    assert float(np.max(np.abs(fs.weights - w))) <= 2e-13 * float(np.max(np.abs(w)))
    assert (fs.n_samples, fs.features, fs.seed) == (5, 64, SEED)
    direct = pg.spectral_features(cov_of(terms), hp, 3, 64, SEED)
    assert np.array_equal(direct[0], fs.frequencies) and np.array_equal(direct[1], u) and np.allclose(direct[2], amp, rtol=1e-15)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_the_samples_are_the_dense_pathwise_formula(ops, name):
    terms, hp, x, y, xp, cond, mu = case(name)
    fs, got = drawn(name, 5, 64)
    nu, u, amp = pr.spectral_features(terms, hp, 3, 64, SEED)
    ref = pr.samples(terms, hp, x, y, xp, nu, u, amp, pr.weights(SEED, nu.shape[0], 5, amp), pr.noise_draws(SEED, 700, 5))
    info = fs.cg_info
    print("%s: %d solves, at most %d iterations, worst true residual %.2e" % (name, info["solves"], info["iterations"], info["residual"]))
    assert got.shape == (5, 70) and info["solves"] == 2 and info["residual"] <= 2 * TOL
    held(name + " five samples", got, ref, cond, yard_abs=1e-10)


def test_reproducibility(ops):
    """Sample 0 is the same bits whether one sample is drawn or five (full-width solves with columns frozen at convergence); the same
    seed gives the same bits, another seed others.  Evaluating the 70 points as 35 + 35 gives the bits of one call HERE because both
    products take the same plan at 70 and at 35 rows: the feature product has 2 or 4 feature tiles (no segments below 8), and the cross
    product's 11 column tiles are cut into 2 segments either way (the cut is capped at tiles / 4 long before the row count matters).
    At other shapes the plan may differ with the row count, and the halves then agree to the kernels' bound only."""
    name = "m32+m52+wn"
    xp = case(name)[4]
    fs5, a5 = drawn(name, 5, 64)
    fs1, a1 = drawn(name, 1, 64)
    assert a1[0].tobytes() == a5[0].tobytes()
    again = N(fitted(name).function_samples(5, 64, SEED)(T(xp)))
    assert again.tobytes() == a5.tobytes()
    other = N(fitted(name).function_samples(5, 64, SEED + 1)(T(xp)))
    assert not np.array_equal(other, a5)
    halves = np.concatenate([N(fs5(T(xp[:35]))), N(fs5(T(xp[35:])))], axis=1)
    assert ops.kernel_matmul_worksize(70, 700, 5) == 2 * ops.kernel_matmul_worksize(35, 700, 5) > 0      # two row tiles against one: the same segments
    assert halves.tobytes() == a5.tobytes()


def test_a_snapshot_does_not_follow_the_model(ops):
    terms, hp, x, y, xp, *_ = case("se+wn")
    model = pg.Iterative_GP(T(x), T(y), cov_of(terms), rank=RANK, tol=TOL)
    model.set_params(T(hp))
    fs = model.function_samples(2, 64, SEED)
    before = N(fs(T(xp)))
    model.set_params(T(hp * 1.3))
    model.update()
    assert N(fs(T(xp))).tobytes() == before.tobytes()
    assert before.tobytes() == drawn("se+wn", 5, 64)[1][:2].tobytes()      # and another model object draws the same functions


@pytest.mark.parametrize("name", sorted(MODELS))
def test_the_prior_needs_no_fit(ops, name):
    terms, hp, x, y, xp, *_ = case(name)
    model = pg.Iterative_GP(T(x), T(y), cov_of(terms), rank=RANK, tol=TOL)
    model.set_params(T(hp))
    fs = model.function_samples(3, 64, SEED, prior=True)
    assert model.need_upd and fs.cg_info is None and fs.prior
    got = N(fs(T(xp)))
    # Phi(xp) W of the sample's own frequencies and weights (held to the restatement's by the first test), to the feature kernel's bound
    nu, u, w = fs.frequencies, fs.phases, fs.weights
    ref, scale = fr.matmul(xp, nu, u, w, np.longdouble)
    bound = (16 * fr.own_phi(xp, nu, u) + (nu.shape[0] + 2) * 2.0 ** -53) * np.asarray(scale.T, np.float64)
    err = np.asarray(np.abs(got - ref.T), np.float64)
    print("%-12s prior: %.2e  (bound %.2e)" % (name, float(err.max()), float(bound.max())))
    assert got.shape == (3, 70) and np.all(err <= bound)
    assert N(model.sample(T(xp), 3, SEED, features=64, prior=True)).tobytes() == got.tobytes() and model.need_upd


@pytest.mark.parametrize("name", sorted(MODELS))
def test_the_first_two_moments(ops, name, monkeypatch):
    monkeypatch.setattr(it_mod, "_RHS_BLOCK", 64)
    terms, hp, x, y, xp, cond, mu = case(name)
    S = 512
    fs = fitted(name).function_samples(S, 256, SEED)
    got = N(fs(T(xp)))
    nu, u, amp = fs.frequencies, fs.phases, pr.spectral_features(terms, hp, 3, 256, SEED)[2]
    v = np.diag(pr.sampler_cov(terms, hp, x, xp, lambda a, b: pr.feature_kernel(a, b, nu, u, amp)))
    mean_dev = np.abs(got.mean(0) - mu) / np.sqrt(v / S)
    var_dev = np.abs(got.var(0, ddof=1) - v) / (v * np.sqrt(2.0 / (S - 1)))
    print("%-12s mean: worst %.2f standard deviations, variance: worst %.2f  (bound 6; %d solves)" % (name, mean_dev.max(), var_dev.max(),
                                                                                                 fs.cg_info["solves"]))
    assert got.shape == (S, 70) and np.all(v > 0)
    assert np.all(mean_dev <= 6) and np.all(var_dev <= 6)


def test_no_n_by_nf_array_at_n_20000(ops, monkeypatch):
    """function_samples(8 samples, 8192 frequencies: nf = 16384) plus one call at 64 points at n = 20000, rank 100 raises the peak of
    allocated device memory by at most 400 MB (DESIGN 4.21's condition); ONE n x nf slab of features would be 2.6 GB."""
    monkeypatch.setattr(it_mod, "_RHS_BLOCK", 64)
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
    fs = model.function_samples(8, 8192, SEED)
    out = fs(xpt)
    torch.cuda.synchronize()
    used = torch.cuda.max_memory_allocated() - before
    print("n = %d, nf = %d: %d iterations, residual %.2e, peak memory + %.1f MB (bound 400 MB)" % (n, fs.frequencies.shape[0], fs.cg_info["iterations"],
                                                                                               fs.cg_info["residual"], used / 1e6))
    assert used <= 400e6
    assert out.shape == (8, 64) and out.is_cuda and bool(torch.isfinite(out).all()) and fs.cg_info["residual"] <= 2e-8


def test_the_interface(ops):
    terms, hp, x, y, xp, *_ = case("se+wn")
    model = fitted("se+wn")
    s = model.sample(T(xp), 3)
    assert tuple(s.shape) == (3, 70) and s.dtype == torch.float64 and not s.is_cuda
    assert N(s).tobytes() == N(model.function_samples(3)(T(xp))).tobytes()      # seed 0, 1024 features: the defaults of both
    with pytest.raises(NotImplementedError, match="function_samples"):
        model.sampler(T(xp))
    for bad in (lambda: model.function_samples(0), lambda: model.function_samples(2, features=0), lambda: model.function_samples(2, seed=1.5)):
        with pytest.raises(ValueError):
            bad()
    fs = model.function_samples(2, 16)
    with pytest.raises(TypeError):
        fs(T(xp).float())
    with pytest.raises(NotImplementedError):
        fs(T(xp).reshape(2, 35, 3))
    for tms, name in ((["rq", "wn"], "Rational_quadratic"), (["per", "wn"], "Periodic"), ([("se", "m32"), "wn"], "Product")):
        other = pg.Iterative_GP(T(x), T(y), cov_of(tms), rank=RANK, tol=TOL)
        with pytest.raises(NotImplementedError, match=name):
            other.function_samples(2, 16)
        assert other.need_upd                                                     # refused before anything was fitted
    slow = pg.Iterative_GP(T(x), T(y), cov_of(terms), rank=RANK, tol=TOL, max_iter=1)
    slow.set_params(T(hp))
    with pytest.raises(pg.NotConverged):
        slow.function_samples(2, 16)
