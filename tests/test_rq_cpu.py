"""CPU tier of the rational quadratic: the NumPy restatement of tests/kernel_ref.py against central differences of itself and against the
squared exponential it tends to, the Python side of the new kind (its d + 2 wide block through layout / spec_of), and the public surface
on a CPU double of the device ops backed by the restatement."""
import os
import re

import numpy as np
import pytest
import torch

import pygpr_amd as pg
from pygpr_amd import _lib
from oracle import pygpr_oracle as orc

import kernel_ref as kr
from kind_tools import N, T, compose
from oracle_ops import fake_ops  # noqa: F401  (fake_ops: the fixture)

# Central differences with step h: truncation h^2 |f'''| / 6, rounding eps |f| / h.  The kernel and its derivatives of every order are
# O(1) here (sigma, l, alpha in [0.5, 1.5], points in the unit cube, |f'''| <= ~60 from the chain rule through the squares):
# h = 1e-5 gives 1e-9 + 2e-11, and the bound below is ten times that.
H, FD_ATOL = 1.0e-5, 1.0e-8


def _data(n=40, m=9, d=3, seed=0, alpha=0.8):
    rng = np.random.default_rng(seed)
    x, xp = rng.random((n, d)), rng.random((m, d))
    x[5] = x[2]                                                 # an exact duplicate: sq = 0 off the diagonal
    hp = np.concatenate([[1.3], 0.5 + rng.random(d), [alpha]])
    return x, xp, hp


@pytest.mark.parametrize("alpha", [0.6, 1.0, 3.0])
def test_restatement_gradient_matches_central_differences(alpha):
    x, xp, hp = _data(alpha=alpha)
    parts = ["rq", "wn"]
    hp = np.append(hp, 0.3)
    k, dk = kr.kernel_and_grad(parts, hp, x)
    assert dk.shape == (hp.size,) + k.shape and hp.size == 3 + 2 + 1 and np.isfinite(dk).all()
    for p in range(hp.size):
        e = np.zeros(hp.size)
        e[p] = H
        fd = (kr.kernel(parts, hp + e, x) - kr.kernel(parts, hp - e, x)) / (2 * H)
        np.testing.assert_allclose(dk[p], fd, rtol=0, atol=FD_ATOL)
    shape = dk[3 + 1]
    assert not np.diag(shape).any() and shape[2, 5] == 0.0 and (shape <= 0.0).all()      # 0 at sq = 0; t/(1+t) <= log1p(t)
    # x*-derivative of the cross kernel
    dks = kr.kernel_xgrad(parts, hp, x, xp)
    for kk in range(x.shape[1]):
        e = np.zeros_like(xp)
        e[:, kk] = H
        fd = (kr.kernel(parts, hp, x, xp + e) - kr.kernel(parts, hp, x, xp - e)) / (2 * H)
        np.testing.assert_allclose(dks[kk], fd, rtol=0, atol=FD_ATOL)


def test_restatement_prediction_derivatives_match_central_differences():
    x, xp, hp = _data()
    parts = ["rq", "se", "wn"]
    hp = np.concatenate([hp, [0.7, 0.9, 1.1, 0.6], [0.3]])
    y = np.sin(3 * x.sum(1))
    rng = np.random.default_rng(1)
    m = xp.shape[0]
    g_mu, g_d, g_f = rng.standard_normal(m), rng.standard_normal(m), rng.standard_normal((m, m))
    dmean, dvar = kr.predict_grads(parts, hp, x, y, xp)

    def loss(q, var, g2):
        mu, v = kr.predict(parts, hp, x, y, q, var=var)
        return float(g_mu @ mu + np.sum(g2 * v))

    # (K^-1 multiplies the rounding term: 1 / (sigma_n^2 + jitter) ~ 11, so ten times the kernel's bound)
    for p in range(m):
        for kk in range(x.shape[1]):
            e = np.zeros_like(xp)
            e[p, kk] = H
            fd_mu = (kr.predict(parts, hp, x, y, xp + e)[0][p] - kr.predict(parts, hp, x, y, xp - e)[0][p]) / (2 * H)
            fd_v = (kr.predict(parts, hp, x, y, xp + e)[1][p] - kr.predict(parts, hp, x, y, xp - e)[1][p]) / (2 * H)
            assert abs(fd_mu - dmean[p, kk]) <= 10 * FD_ATOL and abs(fd_v - dvar[p, kk]) <= 10 * FD_ATOL
            for var, g2 in (("diag", g_d), ("full", g_f)):
                fd = (loss(xp + e, var, g2) - loss(xp - e, var, g2)) / (2 * H)
                assert abs(fd - kr.predict_vjp(parts, hp, x, y, xp, var, g_mu, g2)[p, kk]) <= 100 * FD_ATOL


def test_restatement_nlml_gradient_matches_central_differences():
    rng = np.random.default_rng(3)
    x, y = orc.synth(40, 3, seed=2)
    parts = ["rq", "m32", "wn"]
    hp = np.concatenate([[1.1], 0.5 + rng.random(3), [0.7], [0.7], 0.5 + rng.random(3), [0.2]])
    loss, g = kr.nlml_and_grad(parts, hp, x, y)
    k, dk = kr.kernel_and_grad(parts, hp, x)
    k[np.diag_indices_from(k)] += kr.JITTER
    kinv = np.linalg.inv(k)
    a = kinv @ y
    np.testing.assert_allclose(g, -0.5 * (np.einsum("i,kij,j->k", a, dk, a) - np.einsum("ij,kji->k", kinv, dk)), rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(loss, kr.nlml(parts, hp, x, y), rtol=1e-14)
    # the NLML of 40 points: |f| ~ 50 and K^-1 ~ 1 / sigma_n^2 = 25 in every derivative -- the step and bounds of the Matern family's own test
    h = 1e-6
    for p in range(hp.size):
        e = np.zeros(hp.size)
        e[p] = h
        np.testing.assert_allclose(g[p], (kr.nlml(parts, hp + e, x, y) - kr.nlml(parts, hp - e, x, y)) / (2 * h), rtol=1e-5, atol=1e-6)


def test_se_limit():
    """alpha = 1e4 (a = 1e8): 0 <= K_RQ - K_SE <= K_SE (exp(sq^2 / (2 a)) - 1), entry by entry; the lower side within the rounding of
    the two exponentials (a few ulp of K_SE)."""
    x, xp, hp = _data()
    hp[-1] = 1.0e4
    for q in (None, xp):
        k_rq = kr.kernel(["rq"], hp, x, q)
        k_se = kr.kernel(["se"], hp[:-1], x, q)
        sq = kr.sqdist(hp, x, q)
        assert (k_rq - k_se >= -4 * np.finfo(float).eps * k_se).all()
        assert (k_rq - k_se <= k_se * np.expm1(sq * sq / 2.0e8) + 4 * np.finfo(float).eps * k_se).all()
    assert (kr.kernel(["rq"], hp, x) - kr.kernel(["se"], hp[:-1], x)).max() > 0.0


def test_layout_of_the_new_kind():
    from pygpr_amd.covar import layout, spec_of

    d = 3
    assert "Rational_quadratic" in pg.__all__
    assert pg.Rational_quadratic().get_params_shape(torch.empty(7, d)) == [d + 2]
    assert pg.Rational_quadratic().get_params_shape(torch.empty(4, 7, d)) == [4, d + 2]
    assert torch.equal(pg.Rational_quadratic().init_params(torch.empty(7, d)), torch.ones(d + 2, dtype=torch.float64))
    cov = pg.Compose([pg.Rational_quadratic(), pg.Squared_exponential(), pg.White_noise()])
    kinds, offs, noise, nhp = layout(cov, d)
    assert kinds == [6, 0] and offs == [0, d + 2] and noise == [2 * d + 3] and nhp == 2 * d + 4
    specs, nhp2 = spec_of(cov, d)
    assert nhp2 == nhp and len(specs) == 1
    sp = specs[0]
    assert (sp.ncomp, list(sp.kind[:2]), list(sp.off[:2]), sp.nnoise, sp.noise_off[0]) == (2, [6, 0], [0, d + 2], 1, 2 * d + 3)
    assert cov.get_params_shape(torch.empty(5, 7, d)) == [5, nhp]          # batched [nc, nhp]
    assert cov.init_params(torch.empty(5, 7, d)).shape == (5, nhp)


def test_kind_constant_matches_the_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "pygpr_hip.h")).read()
    found = re.findall(r"#define\s+PG_KIND_RQ\s+\(?(\d+)\)?", text)
    assert found == ["6"] and _lib.PG_KIND_RQ == 6
    assert not re.search(r"#define\s+PG_KIND_\w+\s+\(?5\)?\s", text)       # 5 stays unassigned


# ---- the public surface on a CPU double of the device ops, backed by the restatement ------------------------------------------------
@pytest.mark.parametrize("parts", [["rq", "wn"], ["wn", "rq", "m32"]], ids=lambda p: "+".join(p))
def test_public_surface_on_the_cpu_double(fake_ops, parts):
    rng = np.random.default_rng(7)
    n, m, d = 50, 11, 3
    x, y = orc.synth(n, d, seed=4)
    xp = rng.random((m, d))
    hp = np.concatenate([[0.2] if p == "wn" else np.concatenate([[1.1], 0.5 + rng.random(d), [0.8] if p == "rq" else []]) for p in parts])
    cov = compose(parts)
    assert hp.size == kr.nhp_of(parts, d) == cov.get_params_shape(T(x))[0]
    np.testing.assert_allclose(N(cov.kernel(T(hp), T(x))), kr.kernel(parts, hp, x), rtol=0, atol=1e-14)
    np.testing.assert_allclose(N(cov.kernel(T(hp), T(x), T(xp))), kr.kernel(parts, hp, x, xp), rtol=0, atol=1e-14)
    k, dk = cov.kernel_and_grad(T(hp), T(x))
    np.testing.assert_allclose(N(dk), kr.kernel_and_grad(parts, hp, x)[1], rtol=0, atol=1e-14)
    gp = pg.Exact_GP(T(x), T(y), cov)
    gp.set_params(T(hp))
    mu, var = gp.predict(T(xp), var="diag")
    mu_ref, var_ref = kr.predict(parts, hp, x, y, xp)
    np.testing.assert_allclose(N(mu), mu_ref, rtol=0, atol=1e-10)
    np.testing.assert_allclose(N(var), var_ref, rtol=0, atol=1e-10)
    _, cov_f = gp.predict(T(xp), var="full")
    np.testing.assert_allclose(N(cov_f), kr.predict(parts, hp, x, y, xp, var="full")[1], rtol=0, atol=1e-10)
    loss, grad = pg.MLE(gp).loss_and_grad(hp.copy())
    loss_ref, grad_ref = kr.nlml_and_grad(parts, hp, x, y)
    np.testing.assert_allclose(loss, loss_ref, rtol=1e-11)
    np.testing.assert_allclose(grad, grad_ref, rtol=1e-9, atol=1e-9 * np.abs(grad_ref).max())
    with pytest.raises(AssertionError):
        cov.kernel(T(hp[:-1]), T(x))                            # one value short: the length assertion of covar.py


def test_batched_experts_on_the_cpu_double(fake_ops):
    rng = np.random.default_rng(8)
    nc, n, m, d = 3, 30, 7, 2
    parts = ["rq", "wn"]
    x = rng.random((nc, n, d))
    y = np.sin(-x.sum(-1)) + 0.1 * rng.standard_normal((nc, n))
    xp = rng.random((nc, m, d))
    hp = np.concatenate([0.8 + 0.4 * rng.random((nc, 1)), 0.5 + rng.random((nc, d)), 0.6 + rng.random((nc, 1)), np.full((nc, 1), 0.2)], axis=1)
    gp = pg.Exact_GP(T(x), T(y), compose(parts))
    assert list(gp.cov.get_params_shape(T(x))) == [nc, d + 3]
    gp.set_params(T(hp))
    mu, var = gp.predict(T(xp), var="diag")
    loss, grad = pg.MLE(gp).loss_and_grad(hp.copy())
    for c in range(nc):
        mu_ref, var_ref = kr.predict(parts, hp[c], x[c], y[c], xp[c])
        np.testing.assert_allclose(N(mu[c]), mu_ref, rtol=0, atol=1e-10)
        np.testing.assert_allclose(N(var[c]).ravel(), var_ref, rtol=0, atol=1e-10)
        l_ref, g_ref = kr.nlml_and_grad(parts, hp[c], x[c], y[c])
        np.testing.assert_allclose(loss[c], l_ref, rtol=1e-11)
        np.testing.assert_allclose(grad[c], g_ref, rtol=1e-9, atol=1e-9 * np.abs(g_ref).max())
