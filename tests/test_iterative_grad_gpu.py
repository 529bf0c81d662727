"""Derivatives in the test points of Iterative_GP on the MI355X: predict_grad against the dense restatement, FunctionSamples.grad against
the exact restatement of a sample from the snapshot's own host arrays, reproducibility, the prior and the refusals.

Setup: tests/test_iterative_gpu.py's -- n = 700, d = 3, 70 test points, tol = 1e-10, rank 40, its three covariances, _RHS_BLOCK lowered
to 32 (three blocks of test points, the last of 6).  The function samples take tests/test_pathwise_gpu.py's two covariances (the ones
with a spectral law) at _RHS_BLOCK = 4.

Reference of predict_grad: the dense factor.  tests/xgrad_ref.predict_grads (torch autograd through the dense prediction) knows the
squared exponential and the Matern family only, so it is the reference of `se+wn`; kernel_ref.predict_grads -- the same two
quantities from the closed-form derivative on the same dense factor -- is the reference of all three models, and the two references
are held to each other where both exist.

Bounds (none is fitted; every test prints what it measured):
  predict_grad  test_iterative_gpu.held: 2 cond(A) tol of the largest reference entry, plus the dense yardstick tests/test_xgrad_gpu.py
                holds Exact_GP.predict_grad to -- 1e-9 of the largest reference entry -- for dmean and dvar alike.
  grad          the sum of the two kernels' bounds, per entry: (16 own_dK + (n + 2) 2^-53) S_data of tests/test_dmatmul_gpu.py for the
                data part and (16 own_Phi + (nf + 2 + 2) 2^-53) S_feature of tests/test_feature_matmul_gpu.py for the feature part, the
                extra 2 x 2^-53 for the two roundings of a weight 2 pi nu_fk w_fs formed in float64."""
import functools

import numpy as np
import pytest
import torch

import dmatmul_ref as dr
import feature_ref as fr
import kernel_ref as kr
import pygpr_amd as pg
import xgrad_ref as xr
from kind_tools import N, T, cov_of, ops  # noqa: F401  (ops: the module's fixture)
from pygpr_amd import iterative as it_mod
from test_dmatmul_gpu import bound_of
from test_iterative_gpu import MODELS, RANK, TOL, case, fitted, held
from test_pathwise_gpu import MODELS as SAMPLE_MODELS
from test_pathwise_gpu import SEED
from test_pathwise_gpu import case as sample_case
from test_pathwise_gpu import fitted as sample_fitted

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def small_blocks(monkeypatch):
    monkeypatch.setattr(it_mod, "_RHS_BLOCK", 32)


@functools.lru_cache(maxsize=None)
def dense_grads(name):
    terms, hp, x, y, xp, *_ = case(name)
    return kr.predict_grads(terms, hp, x, y, xp)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_predict_grad_against_the_dense_factor(ops, name):
    terms, hp, x, y, xp, a, cond, alpha, mu, cov = case(name)
    model = fitted(name)
    mean, var, dmean, dvar = model.predict_grad(T(xp), var="diag")
    m0, v0 = model.predict(T(xp), var="diag")
    assert N(mean).tobytes() == N(m0).tobytes() and N(var).tobytes() == N(v0).tobytes()       # predict's own: same path, same bits
    assert dmean.shape == dvar.shape == (70, 3) and dmean.dtype == dvar.dtype == torch.float64 and dmean.device == T(xp).device
    rdm, rdv = dense_grads(name)
    held(name + " dmean", N(dmean), rdm, cond, yard_rel=1e-9)
    held(name + " dvar", N(dvar), rdv, cond, yard_rel=1e-9)
    if all(t in ("se", "m52", "m32", "m12", "wn") for t in terms):
        _, _, tdm, tdv = xr.predict_grads(terms, T(hp), T(x), T(y), T(xp))
        held(name + " dmean (autograd)", N(dmean), N(tdm), cond, yard_rel=1e-9)
        held(name + " dvar (autograd)", N(dvar), N(tdv), cond, yard_rel=1e-9)
        held(name + " the two references, dvar", rdv, N(tdv), 0.0, yard_rel=1e-9)


def test_var_none_does_no_variance_solve(ops, monkeypatch):
    terms, hp, x, y, xp, *_ = case("se+wn")
    model = fitted("se+wn")
    full = model.predict_grad(T(xp), var="diag")
    calls = []
    solve = model._solve
    monkeypatch.setattr(model, "_solve", lambda *a, **k: calls.append(1) or solve(*a, **k))
    mean, dmean = model.predict_grad(T(xp), var="none")
    assert calls == []
    assert N(mean).tobytes() == N(full[0]).tobytes() and N(dmean).tobytes() == N(full[2]).tobytes()
    model.predict_grad(T(xp), var="diag")
    assert len(calls) == 3                                    # 70 points in blocks of 32: the variance and its derivative share each solve


def restated(fs, terms, hp, x, xp):
    """(grad [S, q, d] in longdouble, its bound per entry) of the snapshot's own frequencies, phases, weights and data weights."""
    nu, u, w, v = fs.frequencies, fs.phases, fs.weights, fs.data_weights
    nf, d = nu.shape
    S = w.shape[1]
    two_pi = 8 * np.arctan(np.longdouble(1))
    wk = (two_pi * np.asarray(nu, np.longdouble)[:, :, None] * np.asarray(w, np.longdouble)[:, None, :]).reshape(nf, d * S)
    ref, scale = fr.matmul(xp, nu, u + 0.25, wk, np.longdouble)
    q = xp.shape[0]
    ref = ref.reshape(q, d, S)
    bound = (16 * fr.own_phi(xp, nu, u + 0.25) + (nf + 4) * 2.0 ** -53) * np.asarray(scale, np.float64).reshape(q, d, S)
    if v is not None:
        stationary = [t for t in terms if t != "wn"]
        keep = np.concatenate([np.arange(a, b) for t, blocks in kr._chunks(terms, d) if t != "wn" for _, a, b in blocks])
        dref, dscale = dr.matmul_dx(stationary, hp[keep], xp, x, v, np.longdouble)
        ref = ref + dref
        bound = bound + bound_of(dr.own_dk(stationary, hp[keep], xp, x), x.shape[0]) * np.asarray(dscale, np.float64)
    return np.transpose(ref, (2, 0, 1)), np.transpose(bound, (2, 0, 1))


@functools.lru_cache(maxsize=None)
def drawn(name, n_samples, prior=False):
    saved, it_mod._RHS_BLOCK = it_mod._RHS_BLOCK, 4
    try:
        if prior:
            terms, hp, x, y, *_ = sample_case(name)
            model = pg.Iterative_GP(T(x), T(y), cov_of(terms), rank=RANK, tol=TOL)
            model.set_params(T(hp))
            return model.function_samples(n_samples, 64, SEED, prior=True), model
        return sample_fitted(name).function_samples(n_samples, 64, SEED), None
    finally:
        it_mod._RHS_BLOCK = saved


@pytest.mark.parametrize("name", sorted(SAMPLE_MODELS))
def test_grad_is_the_derivative_of_the_restated_sample(ops, name):
    terms, hp, x, y, xp, cond, mu = sample_case(name)
    fs, _ = drawn(name, 5)
    got = N(fs.grad(T(xp)))
    assert got.shape == (5, 70, 3) and fs.data_weights.shape == (700, 5)
    ref, bound = restated(fs, terms, hp, x, xp)
    err = np.asarray(np.abs(got - ref), np.float64)
    print("%-12s grad of five samples: err %.2e of max|grad| %.2e  (largest bound %.2e, err / bound %.2e)"
          % (name, float(err.max()), float(np.abs(ref).max()), float(bound.max()), float((err / bound).max())))
    assert np.isfinite(got).all() and np.all(err <= bound)
    # ... and of what __call__ returns: central differences of the device's own values, to their truncation and rounding
    h = 1e-5
    k = 1
    e = np.zeros(3)
    e[k] = h
    fd = (N(fs(T(xp + e))) - N(fs(T(xp - e)))) / (2 * h)
    assert float(np.max(np.abs(fd - got[:, :, k]))) <= 1e-5 * max(1.0, float(np.abs(got).max()))


def test_sample_s_does_not_depend_on_n_samples(ops):
    name = "m32+m52+wn"
    xp = sample_case(name)[4]
    g5, g1 = N(drawn(name, 5)[0].grad(T(xp))), N(drawn(name, 1)[0].grad(T(xp)))
    assert g1.shape == (1, 70, 3) and g1[0].tobytes() == g5[0].tobytes()
    assert N(drawn(name, 5)[0].grad(T(xp))).tobytes() == g5.tobytes()


@pytest.mark.parametrize("name", sorted(SAMPLE_MODELS))
def test_a_priors_grad_is_the_feature_part_alone(ops, name):
    terms, hp, x, y, xp, *_ = sample_case(name)
    fs, model = drawn(name, 3, prior=True)
    assert fs.prior and fs.data_weights is None and model.need_upd
    got = N(fs.grad(T(xp)))
    ref, bound = restated(fs, terms, hp, x, xp)
    err = np.asarray(np.abs(got - ref), np.float64)
    print("%-12s prior grad: err %.2e  (largest bound %.2e)" % (name, float(err.max()), float(bound.max())))
    assert got.shape == (3, 70, 3) and np.all(err <= bound) and model.need_upd


def test_refusals(ops):
    terms, hp, x, y, xp, *_ = case("se+wn")
    model = fitted("se+wn")
    with pytest.raises(ValueError, match="'diag' or 'none'"):
        model.predict_grad(T(xp), var="full")
    with pytest.raises(NotImplementedError, match="no batches"):
        model.predict_grad(T(xp).reshape(2, 35, 3))
    with pytest.raises(NotImplementedError, match="no batches"):
        model.predict_grad(T(xp)[:, :2])
    with pytest.raises(TypeError, match="float64 only"):
        model.predict_grad(T(xp).float())
    with pytest.raises(NotImplementedError, match="use an Exact_GP for derivatives in the test points"):      # predict stays closed to autograd
        model.predict(T(xp).requires_grad_(True), var="none")
    with pytest.raises(NotImplementedError, match="no joint sampler"):
        model.sampler(T(xp))
    mean, dmean = model.predict_grad(T(xp).requires_grad_(True), var="none")      # ... predict_grad needs none
    assert not dmean.requires_grad
    fs, _ = drawn("se+wn", 5)
    with pytest.raises(NotImplementedError, match="no batches"):
        fs.grad(T(xp).reshape(2, 35, 3))
    with pytest.raises(TypeError, match="float64 only"):
        fs.grad(T(xp).float())
    with pytest.raises(NotImplementedError):
        fs.grad(xp)
