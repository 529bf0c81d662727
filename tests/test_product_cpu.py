"""CPU tier of Product: the NumPy restatement of tests/kernel_ref.py against central differences of itself; the Python and ctypes side
of a product spec (PG_SPEC_PRODUCT in ncomp, the pass plan of spec_of, the refusals, the memo key); and the public surface on a CPU
double of the device ops backed by the restatement."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pygpr_amd as pg
from pygpr_amd import _lib, _ops
from pygpr_amd.covar import layout, spec_of, terms
from oracle import pygpr_oracle as orc

import kernel_ref as kr
from kind_tools import N, T, cov_of
from oracle_ops import fake_ops  # noqa: F401  (fake_ops: the fixture)

# Central differences with step h: truncation h^2 |f'''| / 6, rounding eps |f| / h.  The step and the bound are those of
# tests/test_periodic_cpu.py (|D| <= 2, periods in [0.7, 2.5]: |f'''| <= ~1e4 for the periodic factor, 2e-9 of truncation and 3e-10 of
# rounding at h = 1e-6, bound 1e-8).  The factors here have sigma <= 1, so the other factors of a product are <= 1 and the product rule's
# leading term K_{-c} f_c''' keeps that bound; the cross terms carry lower derivatives of the periodic factor (|f''| <= ~4e2).
H, FD_ATOL = 1.0e-6, 1.0e-8


def hp_of(model, d, rng, sigma=(0.7, 1.0)):
    blocks = []
    for p in kr.flat(model):
        if p == "wn":
            blocks.append([0.2])
        else:
            blocks.append(np.concatenate([[rng.uniform(*sigma)], 0.5 + rng.random(d),
                                          rng.uniform(0.7, 2.5, d) if p == "per" else ([0.8] if p == "rq" else [])]))
    return np.concatenate(blocks)


def _data(n=40, m=9, d=3, seed=0):
    rng = np.random.default_rng(seed)
    x, xp = rng.uniform(-1, 1, (n, d)), rng.uniform(-1, 1, (m, d))      # |D| <= 2
    x[5] = x[2]                                                 # an exact duplicate: sq = 0 off the diagonal
    return x, xp, rng


MODELS = [[("se", "per")], [("m52", "per"), "wn"], ["se", ("m32", "per"), "wn"], [("rq", "m12", "per"), ("se", "m32"), "wn"],
          [("se", "m32", "rq", "per")]]


@pytest.mark.parametrize("model", MODELS, ids=str)
def test_restatement_gradient_matches_central_differences(model):
    x, xp, rng = _data()
    d = x.shape[1]
    hp = hp_of(model, d, rng)
    k, dk = kr.kernel_and_grad(model, hp, x)
    assert dk.shape == (hp.size,) + k.shape and hp.size == kr.nhp_of(model, d) and np.isfinite(dk).all()
    assert np.array_equal(k, kr.kernel(model, hp, x))
    for p in range(hp.size):
        e = np.zeros(hp.size)
        e[p] = H
        fd = (kr.kernel(model, hp + e, x) - kr.kernel(model, hp - e, x)) / (2 * H)
        np.testing.assert_allclose(dk[p], fd, rtol=0, atol=FD_ATOL)
    dks = kr.kernel_xgrad(model, hp, x, xp)
    for kk in range(d):
        e = np.zeros_like(xp)
        e[:, kk] = H
        fd = (kr.kernel(model, hp, x, xp + e) - kr.kernel(model, hp, x, xp - e)) / (2 * H)
        np.testing.assert_allclose(dks[kk], fd, rtol=0, atol=FD_ATOL)


def test_restatement_is_the_product_of_the_parts():
    x, xp, rng = _data()
    d = x.shape[1]
    hp = hp_of([("se", "per"), "m32", "wn"], d, rng)
    a, b, c = d + 1, 3 * d + 2, 4 * d + 3
    for q in (None, xp):
        want = kr.kernel(["se"], hp[:a], x, q) * kr.kernel(["per"], hp[a:b], x, q) + kr.kernel(["m32", "wn"], hp[b:], x, q)
        assert np.array_equal(kr.kernel([("se", "per"), "m32", "wn"], hp, x, q), want)
        assert np.array_equal(want, kr.stationary("se", hp[:a], x, q) * kr.stationary("per", hp[a:b], x, q)
                              + (kr.stationary("m32", hp[b:c], x, q) + (hp[c] ** 2 * np.eye(x.shape[0]) if q is None else 0.0)))
    # a product of one factor is the factor; the dK stack of a list without tuples is the lone parts' slabs at their offsets
    assert np.array_equal(kr.kernel([("per",)], hp[a:b], x), kr.kernel(["per"], hp[a:b], x))
    assert np.array_equal(kr.kernel_and_grad([("per",)], hp[a:b], x)[1], kr.kernel_and_grad(["per"], hp[a:b], x)[1])
    singles = [kr.kernel_and_grad([p], hp[i:j], x)[1] for p, i, j in (("se", 0, a), ("per", a, b), ("m32", b, c), ("wn", c, c + 1))]
    assert np.array_equal(kr.kernel_and_grad(["se", "per", "m32", "wn"], hp, x)[1], np.concatenate(singles))
    # the same formulas in extended precision agree with themselves to a few float64 ulps of the values (|K| <= 1.3)
    k64, k80 = kr.kernel([("se", "per"), "m32", "wn"], hp, x), kr.kernel([("se", "per"), "m32", "wn"], hp, x, dtype=np.longdouble)
    assert k80.dtype == np.longdouble and np.abs(k64 - k80).max() <= 32 * np.finfo(np.float64).eps


def test_restatement_nlml_and_prediction_derivatives_match_central_differences():
    rng = np.random.default_rng(3)
    x, y = orc.synth(40, 3, seed=2)
    xp = rng.random((5, 3))
    model = [("se", "per"), "m32", "wn"]
    hp = hp_of(model, 3, rng)
    loss, g = kr.nlml_and_grad(model, hp, x, y)
    np.testing.assert_allclose(loss, kr.nlml(model, hp, x, y), rtol=1e-14)
    # the NLML of 40 points: |f| ~ 50 and K^-1 ~ 1 / sigma_n^2 = 25 in every derivative -- the step and bounds of the periodic kernel's own test
    h = 1e-6
    for p in range(hp.size):
        e = np.zeros(hp.size)
        e[p] = h
        np.testing.assert_allclose(g[p], (kr.nlml(model, hp + e, x, y) - kr.nlml(model, hp - e, x, y)) / (2 * h), rtol=1e-5, atol=1e-6)
    dmean, dvar = kr.predict_grads(model, hp, x, y, xp)
    g_mu, g_f = rng.standard_normal(5), rng.standard_normal((5, 5))
    vjp = kr.predict_vjp(model, hp, x, y, xp, "full", g_mu, g_f)
    for p in range(xp.shape[0]):
        for kk in range(3):
            e = np.zeros_like(xp)
            e[p, kk] = 1e-5
            hi, lo = kr.predict(model, hp, x, y, xp + e), kr.predict(model, hp, x, y, xp - e)
            assert abs((hi[0][p] - lo[0][p]) / 2e-5 - dmean[p, kk]) <= 1e-7 and abs((hi[1][p] - lo[1][p]) / 2e-5 - dvar[p, kk]) <= 1e-7
            hi, lo = kr.predict(model, hp, x, y, xp + e, var="full"), kr.predict(model, hp, x, y, xp - e, var="full")
            fd = (g_mu @ (hi[0] - lo[0]) + np.sum(g_f * (hi[1] - lo[1]))) / 2e-5
            assert abs(fd - vjp[p, kk]) <= 1e-6


def test_flag_struct_and_make_spec():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "pygpr_hip.h")).read()
    assert re.findall(r"#define\s+PG_SPEC_PRODUCT\s+(\w+)", text) == ["0x100"] and _lib.PG_SPEC_PRODUCT == 0x100
    assert _lib.PG_SPEC_PRODUCT > _lib.PG_MAX_COMP                           # the count keeps the low byte
    sp = _ops.make_spec([_lib.PG_KIND_RBF, _lib.PG_KIND_PERIODIC], [0, 4], [11], product=True)
    assert ctypes.sizeof(sp) == (2 + 3 * _lib.PG_MAX_COMP) * ctypes.sizeof(ctypes.c_int)      # pg_covspec did not grow
    assert (sp.ncomp, sp.kind[0], sp.kind[1], sp.off[1], sp.nnoise, sp.noise_off[0]) == (0x102, 0, 8, 4, 1, 11)
    assert _ops.make_spec([0, 8], [0, 4], [11]).ncomp == 2 == _ops.make_spec([0, 8], [0, 4], [11], product=False).ncomp
    with pytest.raises(ValueError):
        _ops.make_spec([], [], [3], product=True)
    with pytest.raises(ValueError):
        _ops.make_spec([0] * 5, list(range(5)), [], product=True)
    _lib.load(check_symbols=True)


def _plan(cov, d):
    specs, nhp = spec_of(cov, d)
    out = []
    for sp in specs:
        n = sp.ncomp & 0xFF
        out.append((bool(sp.ncomp & _lib.PG_SPEC_PRODUCT), list(sp.kind[:n]), list(sp.off[:n]), list(sp.noise_off[: sp.nnoise])))
    return out, nhp


def test_pass_plan():
    d = 3
    se, m32, per, wn = pg.Squared_exponential, pg.Matern32, pg.Periodic, pg.White_noise
    assert "Product" in pg.__all__
    # a bare product: one flagged spec
    assert _plan(pg.Product([se(), per()]), d) == ([(True, [0, 8], [0, d + 1], [])], 3 * d + 2)
    # product + noise: still one flagged spec, the noise in it (the fused, batched and checked paths take one spec)
    assert _plan(pg.Compose([pg.Product([se(), per()]), wn()]), d) == ([(True, [0, 8], [0, d + 1], [3 * d + 2])], 3 * d + 3)
    assert _plan(pg.Compose([wn(), pg.Product([se(), per()]), wn()]), d) == ([(True, [0, 8], [1, d + 2], [0, 3 * d + 3])], 3 * d + 4)
    # a plain child beside the product: the sum pass of today with the noise, then the product's own pass without
    cov = pg.Compose([se(), pg.Product([m32(), per()]), wn()])
    assert _plan(cov, d) == ([(False, [0], [0], [4 * d + 3]), (True, [3, 8], [d + 1, 2 * d + 2], [])], 4 * d + 4)
    assert layout(cov, d) == ([0, 3, 8], [0, d + 1, 2 * d + 2], [4 * d + 3], 4 * d + 4)            # layout keeps its 4-tuple
    assert terms(cov, d) == (((False, (0,), (0,)), (True, (3, 8), (d + 1, 2 * d + 2))), [4 * d + 3], 4 * d + 4)
    # two products: the noise pass first, then one flagged pass each
    cov = pg.Compose([pg.Product([se(), per()]), pg.Product([se(), m32()]), wn()])
    assert _plan(cov, d) == ([(False, [], [], [5 * d + 4]), (True, [0, 8], [0, d + 1], []), (True, [0, 3], [3 * d + 2, 4 * d + 3], [])], 5 * d + 5)
    assert _plan(pg.Compose([pg.Product([se(), per()]), pg.Product([se(), m32()])]), d)[0] == \
        [(True, [0, 8], [0, d + 1], []), (True, [0, 3], [3 * d + 2, 4 * d + 3], [])]
    # plain children in the order they always had, products behind them wherever they stood
    cov = pg.Compose([pg.Product([se(), per()]), m32(), wn(), se()])
    assert _plan(cov, d)[0] == [(False, [3, 0], [3 * d + 2, 4 * d + 4], [4 * d + 3]), (True, [0, 8], [0, d + 1], [])]
    # sums without a product are planned as before
    assert _plan(pg.Compose([se(), per(), wn()]), d) == ([(False, [0, 8], [0, d + 1], [3 * d + 2])], 3 * d + 3)
    assert [len(spec_of(pg.Compose([se()] * k + [wn()]), d)[0]) for k in (4, 5)] == [1, 2]
    # shapes and initial parameters follow the children
    prod = pg.Product([se(), per()])
    assert prod.get_params_shape(torch.empty(7, d)) == [3 * d + 2] and prod.get_params_shape(torch.empty(4, 7, d)) == [4, 3 * d + 2]
    assert torch.equal(prod.init_params(torch.empty(7, d)), torch.ones(3 * d + 2, dtype=torch.float64))
    full = pg.Compose([prod, wn()]).init_params(torch.empty(5, 7, d))
    assert full.shape == (5, 3 * d + 3) and float(full[0, -1]) == 1e-4


def test_refusals_at_construction():
    se, per, wn = pg.Squared_exponential, pg.Periodic, pg.White_noise
    for bad in (wn(), pg.Compose([se(), wn()]), pg.Product([se(), per()])):
        with pytest.raises(TypeError):
            pg.Product([se(), bad])
    for count in (0, 1, _lib.PG_MAX_COMP + 1):
        with pytest.raises(ValueError):
            pg.Product([se() for _ in range(count)])
    assert len(pg.Product([se() for _ in range(_lib.PG_MAX_COMP)]).covars) == _lib.PG_MAX_COMP
    for cls in (pg.Squared_exponential, pg.Matern52, pg.Matern32, pg.Matern12, pg.Rational_quadratic, pg.Periodic):
        pg.Product([cls(), se()])


# ---- the public surface on a CPU double of the device ops, backed by the restatement ------------------------------------------------
@pytest.mark.parametrize("model", [[("se", "per")], [("se", "per"), "wn"], ["wn", ("rq", "per"), "m32"], [("m52", "per"), ("se", "m32"), "wn"]], ids=str)
def test_public_surface_on_the_cpu_double(fake_ops, model):
    """Every block is read by its offset: a product in front of, behind and between plain children and the noise."""
    rng = np.random.default_rng(7)
    n, m, d = 50, 11, 3
    x, y = orc.synth(n, d, seed=4)
    xp = rng.random((m, d))
    hp = hp_of(model, d, rng, sigma=(0.7, 1.3))
    cov = cov_of(model)
    assert hp.size == kr.nhp_of(model, d) == cov.get_params_shape(T(x))[0]
    np.testing.assert_allclose(N(cov.kernel(T(hp), T(x))), kr.kernel(model, hp, x), rtol=0, atol=1e-14)
    np.testing.assert_allclose(N(cov.kernel(T(hp), T(x), T(xp))), kr.kernel(model, hp, x, xp), rtol=0, atol=1e-14)
    k, dk = cov.kernel_and_grad(T(hp), T(x))
    assert k.shape == (n, n) and dk.shape == (hp.size, n, n)
    np.testing.assert_allclose(N(dk), kr.kernel_and_grad(model, hp, x)[1], rtol=0, atol=1e-14)
    if "wn" not in model:
        return                                                  # (a noise-free model on 50 clustered points is not a fit to rely on)
    gp = pg.Exact_GP(T(x), T(y), cov)
    gp.set_params(T(hp))
    mu, var = gp.predict(T(xp), var="diag")
    mu_ref, var_ref = kr.predict(model, hp, x, y, xp)
    np.testing.assert_allclose(N(mu), mu_ref, rtol=0, atol=1e-10)
    np.testing.assert_allclose(N(var), var_ref, rtol=0, atol=1e-10)      # the prior variance of a product term is prod sigma_c^2
    _, cov_f = gp.predict(T(xp), var="full")
    np.testing.assert_allclose(N(cov_f), kr.predict(model, hp, x, y, xp, var="full")[1], rtol=0, atol=1e-10)
    loss, grad = pg.MLE(gp).loss_and_grad(hp.copy())
    loss_ref, grad_ref = kr.nlml_and_grad(model, hp, x, y)
    np.testing.assert_allclose(loss, loss_ref, rtol=1e-11)
    np.testing.assert_allclose(grad, grad_ref, rtol=1e-9, atol=1e-9 * np.abs(grad_ref).max())
    with pytest.raises(AssertionError):
        cov.kernel(T(hp[:-1]), T(x))                            # one value short: the length assertion of covar.py


def test_memo_key_tells_a_product_from_a_sum(fake_ops):
    """Product([a, b]) and Compose([a, b]) have the same layout; MLE's memo must not return one's loss for the other."""
    x, y = orc.synth(30, 2, seed=1)
    rng = np.random.default_rng(2)
    hp = hp_of([("se", "per"), "wn"], 2, rng)
    se, per, wn = pg.Squared_exponential(), pg.Periodic(), pg.White_noise()
    c_sum, c_prod = pg.Compose([se, per, wn]), pg.Compose([pg.Product([se, per]), wn])
    assert layout(c_sum, 2) == layout(c_prod, 2) and terms(c_sum, 2)[0] != terms(c_prod, 2)[0]
    gp = pg.Exact_GP(T(x), T(y), c_sum)
    gp.set_params(T(hp))
    mle = pg.MLE(gp)
    keys = []
    real = mle._evaluate_device
    mle._evaluate_device = lambda params, want_grad, key, reuse: (keys.append(key), real(params, want_grad, key, reuse))[1]
    l_sum = mle.loss(hp.copy())
    gp.cov = c_prod
    l_prod = mle.loss(hp.copy())
    # apart from id(cov), only the terms differ (same kinds, offsets and noise: the layouts are the same)
    assert len(keys) == 2 and keys[0][:-2] == keys[1][:-2] and keys[0][-1] != keys[1][-1] and keys[0][-1][1] == keys[1][-1][1]
    np.testing.assert_allclose(l_sum, kr.nlml(["se", "per", "wn"], hp, x, y), rtol=1e-11)
    np.testing.assert_allclose(l_prod, kr.nlml([("se", "per"), "wn"], hp, x, y), rtol=1e-11)


def test_batched_experts_on_the_cpu_double(fake_ops):
    rng = np.random.default_rng(8)
    nc, n, m, d = 3, 30, 7, 2
    model = [("se", "per"), "wn"]
    x = rng.random((nc, n, d))
    y = np.sin(-x.sum(-1)) + 0.1 * rng.standard_normal((nc, n))
    xp = rng.random((nc, m, d))
    hp = np.stack([hp_of(model, d, rng, sigma=(0.7, 1.3)) for _ in range(nc)])
    gp = pg.Exact_GP(T(x), T(y), cov_of(model))
    assert list(gp.cov.get_params_shape(T(x))) == [nc, 3 * d + 3]
    gp.set_params(T(hp))
    mu, var = gp.predict(T(xp), var="diag")
    loss, grad = pg.MLE(gp).loss_and_grad(hp.copy())
    for c in range(nc):
        mu_ref, var_ref = kr.predict(model, hp[c], x[c], y[c], xp[c])
        np.testing.assert_allclose(N(mu[c]), mu_ref, rtol=0, atol=1e-10)
        np.testing.assert_allclose(N(var[c]).ravel(), var_ref, rtol=0, atol=1e-10)
        l_ref, g_ref = kr.nlml_and_grad(model, hp[c], x[c], y[c])
        np.testing.assert_allclose(loss[c], l_ref, rtol=1e-11)
        np.testing.assert_allclose(grad[c], g_ref, rtol=1e-9, atol=1e-9 * np.abs(g_ref).max())
