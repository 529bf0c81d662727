"""CPU tier of the periodic kernel: the NumPy restatement of tests/kernel_ref.py against central differences of itself, against
MacKay's form and against the properties the definition promises (even in p, periodic, positive definite); the Python and ctypes side of
kind 8 (its 2 d + 1 wide block through layout / spec_of); and the public surface on a CPU double of the device ops backed by the
restatement."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pygpr_amd as pg
from pygpr_amd import _lib, _ops
from oracle import pygpr_oracle as orc

import kernel_ref as kr
from kind_tools import N, T, compose
from oracle_ops import fake_ops  # noqa: F401  (fake_ops: the fixture)

# Central differences with step h: truncation h^2 |f'''| / 6, rounding eps |f| / h.  sigma, l in [0.5, 1.5], periods in [0.7, 2.5]: a
# derivative in p_k brings a factor pi D / p^2 each time, so the kernel test scales its points to |D| <= 2 (|f'''| <= ~1e4); h = 1e-6
# then gives 2e-9 of truncation and 3e-10 of rounding.  The bound is the 1e-8 the formulas were first checked to.
H, FD_ATOL = 1.0e-6, 1.0e-8


def _data(n=40, m=9, d=3, seed=0):
    rng = np.random.default_rng(seed)
    x, xp = rng.uniform(-3, 3, (n, d)), rng.uniform(-3, 3, (m, d))
    x[5] = x[2]                                                 # an exact duplicate: sq = 0 off the diagonal
    hp = np.concatenate([[1.3], 0.5 + rng.random(d), rng.uniform(0.7, 2.5, d)])
    return x, xp, hp


def test_restatement_gradient_matches_central_differences():
    x, xp, hp = _data()
    x, xp = x / 3.0, xp / 3.0                                    # |D| <= 2: third derivatives in p stay below ~1e4 (h^2 f''' / 6 < 2e-9)
    parts = ["per", "wn"]
    hp = np.append(hp, 0.3)
    d = x.shape[1]
    k, dk = kr.kernel_and_grad(parts, hp, x)
    assert dk.shape == (hp.size,) + k.shape and hp.size == 2 * d + 1 + 1 and np.isfinite(dk).all()
    for p in range(hp.size):
        e = np.zeros(hp.size)
        e[p] = H
        fd = (kr.kernel(parts, hp + e, x) - kr.kernel(parts, hp - e, x)) / (2 * H)
        np.testing.assert_allclose(dk[p], fd, rtol=0, atol=FD_ATOL)
    for kk in range(d):                                          # the period slabs vanish where D = 0
        assert not np.diag(dk[d + 1 + kk]).any() and dk[d + 1 + kk][2, 5] == 0.0 and dk[d + 1 + kk].any()
    dks = kr.kernel_xgrad(parts, hp, x, xp)
    for kk in range(d):
        e = np.zeros_like(xp)
        e[:, kk] = H
        fd = (kr.kernel(parts, hp, x, xp + e) - kr.kernel(parts, hp, x, xp - e)) / (2 * H)
        np.testing.assert_allclose(dks[kk], fd, rtol=0, atol=FD_ATOL)


def test_restatement_in_a_sum_delegates_to_the_other_kinds():
    """A sum is its terms evaluated apart: K the sum of the sub-models' K, each dK slab the lone part's own slab at its offset, the
    x*-gradient the sum of theirs -- whichever widths stand in front of a block."""
    x, xp, hp = _data()
    d = x.shape[1]
    parts = ["rq", "per", "se", "wn"]
    hp_rq, hp_se = np.concatenate([[0.9], 0.5 + np.arange(d) / d, [0.8]]), np.concatenate([[1.1], 0.6 + np.arange(d) / d])
    full = np.concatenate([hp_rq, hp, hp_se, [0.2]])
    assert full.size == kr.nhp_of(parts, d) == (d + 2) + (2 * d + 1) + (d + 1) + 1
    k, dk = kr.kernel_and_grad(parts, full, x)
    k_rq, dk_rq = kr.kernel_and_grad(["rq", "se", "wn"], np.concatenate([hp_rq, hp_se, [0.2]]), x)
    k_p, dk_p = kr.kernel_and_grad(["per"], hp, x)
    np.testing.assert_allclose(k, k_rq + k_p, rtol=0, atol=1e-15)
    assert np.array_equal(dk[: d + 2], dk_rq[: d + 2]) and np.array_equal(dk[d + 2: 3 * d + 3], dk_p) and np.array_equal(dk[3 * d + 3:], dk_rq[d + 2:])
    singles = [kr.kernel_and_grad([q], h, x)[1] for q, h in (("rq", hp_rq), ("per", hp), ("se", hp_se), ("wn", np.array([0.2])))]
    assert np.array_equal(dk, np.concatenate(singles))
    np.testing.assert_allclose(kr.kernel_xgrad(parts, full, x, xp),
                               kr.kernel_xgrad(["rq", "se"], np.concatenate([hp_rq, hp_se]), x, xp) + kr.kernel_xgrad(["per"], hp, x, xp),
                               rtol=0, atol=1e-14)


def test_restatement_nlml_and_prediction_derivatives_match_central_differences():
    rng = np.random.default_rng(3)
    x, y = orc.synth(40, 3, seed=2)
    xp = rng.random((5, 3))
    parts = ["per", "m32", "wn"]
    hp = np.concatenate([[1.1], 0.5 + rng.random(3), rng.uniform(0.7, 2.5, 3), [0.7], 0.5 + rng.random(3), [0.2]])
    loss, g = kr.nlml_and_grad(parts, hp, x, y)
    np.testing.assert_allclose(loss, kr.nlml(parts, hp, x, y), rtol=1e-14)
    # the NLML of 40 points: |f| ~ 50 and K^-1 ~ 1 / sigma_n^2 = 25 in every derivative -- the step and bounds of the Matern family's own test
    h = 1e-6
    for p in range(hp.size):
        e = np.zeros(hp.size)
        e[p] = h
        np.testing.assert_allclose(g[p], (kr.nlml(parts, hp + e, x, y) - kr.nlml(parts, hp - e, x, y)) / (2 * h), rtol=1e-5, atol=1e-6)
    dmean, dvar = kr.predict_grads(parts, hp, x, y, xp)
    g_mu, g_f = rng.standard_normal(5), rng.standard_normal((5, 5))
    vjp = kr.predict_vjp(parts, hp, x, y, xp, "full", g_mu, g_f)
    for p in range(xp.shape[0]):
        for kk in range(3):
            e = np.zeros_like(xp)
            e[p, kk] = 1e-5
            hi, lo = kr.predict(parts, hp, x, y, xp + e), kr.predict(parts, hp, x, y, xp - e)
            assert abs((hi[0][p] - lo[0][p]) / 2e-5 - dmean[p, kk]) <= 1e-7 and abs((hi[1][p] - lo[1][p]) / 2e-5 - dvar[p, kk]) <= 1e-7
            hi, lo = kr.predict(parts, hp, x, y, xp + e, var="full"), kr.predict(parts, hp, x, y, xp - e, var="full")
            fd = (g_mu @ (hi[0] - lo[0]) + np.sum(g_f * (hi[1] - lo[1]))) / 2e-5
            assert abs(fd - vjp[p, kk]) <= 1e-6


def test_mackay_correspondence():
    """MacKay's exp(-2 sin^2(pi D / p) / ell^2), one dimension at a time, is this kernel with l^2 = 2 / ell^2."""
    x, xp, hp = _data(d=1)
    ell, p = 0.8, 1.7
    hp = np.array([1.0, np.sqrt(2.0) / ell, p])
    for q in (None, xp):
        dd = (x if q is None else q)[:, 0][:, None] - x[:, 0][None, :]
        np.testing.assert_allclose(kr.kernel(["per"], hp, x, q), np.exp(-2.0 * np.sin(np.pi * dd / p) ** 2 / ell ** 2), rtol=0, atol=4e-16)


def test_even_in_the_period_and_periodic_in_the_input():
    x, xp, hp = _data()
    d = x.shape[1]
    neg = hp.copy()
    neg[d + 1:] *= -1.0
    assert np.array_equal(kr.kernel(["per"], hp, x, xp), kr.kernel(["per"], neg, x, xp))
    # K(x, x + p e_k) = K(x, x) = sigma^2 to rounding: the shifted point's phase is pi (D + p) / p, off pi by a few ulps of pi |D + p| / p
    for k in range(d):
        shifted = x.copy()
        shifted[:, k] += hp[d + 1 + k]
        kd = np.diag(kr.kernel(["per"], hp, x, shifted))
        np.testing.assert_allclose(kd, hp[0] ** 2, rtol=0, atol=1e-15 * 9)
        np.testing.assert_allclose(kr.kernel(["per"], hp, x, shifted), kr.kernel(["per"], hp, x, x), rtol=0, atol=1e-14)


def test_positive_definite_on_random_points():
    for seed, d in ((0, 1), (1, 2), (2, 3), (3, 8)):
        rng = np.random.default_rng(seed)
        x = rng.uniform(-3, 3, (120, d))
        hp = np.concatenate([[1.2], 0.3 + rng.random(d), rng.uniform(0.7, 2.5, d)])
        k = kr.kernel(["per"], hp, x)
        assert np.array_equal(k, k.T) and (np.diag(k) == hp[0] ** 2).all()
        assert np.linalg.eigvalsh(k).min() >= -1e-13 * 120 * hp[0] ** 2      # (backward error of the symmetric eigensolver: eps n |K|)
        np.linalg.cholesky(k + 1e-10 * np.eye(120))


def test_layout_of_the_new_kind():
    from pygpr_amd.covar import layout, spec_of

    d = 3
    assert "Periodic" in pg.__all__
    assert pg.Periodic().get_params_shape(torch.empty(7, d)) == [2 * d + 1]
    assert pg.Periodic().get_params_shape(torch.empty(4, 7, d)) == [4, 2 * d + 1]
    assert torch.equal(pg.Periodic().init_params(torch.empty(7, d)), torch.ones(2 * d + 1, dtype=torch.float64))
    cov = pg.Compose([pg.Rational_quadratic(), pg.Periodic(), pg.Squared_exponential(), pg.White_noise()])
    kinds, offs, noise, nhp = layout(cov, d)
    assert kinds == [6, 8, 0] and offs == [0, d + 2, 3 * d + 3] and noise == [4 * d + 4] and nhp == 4 * d + 5
    specs, nhp2 = spec_of(cov, d)
    assert nhp2 == nhp and len(specs) == 1
    sp = specs[0]
    assert (sp.ncomp, list(sp.kind[:3]), list(sp.off[:3]), sp.nnoise, sp.noise_off[0]) == (3, [6, 8, 0], [0, d + 2, 3 * d + 3], 1, 4 * d + 4)
    assert cov.get_params_shape(torch.empty(5, 7, d)) == [5, nhp]
    assert cov.init_params(torch.empty(5, 7, d)).shape == (5, nhp)
    with pytest.raises(TypeError):
        pg.Periodic().distance(torch.empty(7, d))              # the squared exponential's Euclidean distance is not this kind's


def test_kind_constant_struct_and_symbols():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "pygpr_hip.h")).read()
    assert re.findall(r"#define\s+PG_KIND_PERIODIC\s+\(?(\d+)\)?", text) == ["8"] and _lib.PG_KIND_PERIODIC == 8
    assert not re.search(r"#define\s+PG_KIND_\w+\s+\(?[57]\)?\s", text)    # 5 and 7 stay unassigned
    assert re.search(r"periods.*\n.*off\[c\] \+ d \+ 1 \.\. off\[c\] \+ 2 d", text)      # pg_covspec.off says where the periods sit
    # no new entry point and no change to pg_covspec: the periods are found from off[c] and d
    sp = _ops.make_spec([_lib.PG_KIND_PERIODIC, _lib.PG_KIND_RBF], [0, 7], [11])
    assert ctypes.sizeof(sp) == (2 + 3 * _lib.PG_MAX_COMP) * ctypes.sizeof(ctypes.c_int)
    assert (sp.ncomp, sp.kind[0], sp.kind[1], sp.off[1], sp.nnoise, sp.noise_off[0]) == (2, 8, 0, 7, 1, 11)
    _lib.load(check_symbols=True)
    for name in ("pg_kernel_build", "pg_kernel_build_batched", "pg_kernel_grad_build", "pg_nlml_grad", "pg_nlml_grad_worksize", "pg_kernel_xgrad"):
        assert name in _lib.header_symbols()


# ---- the public surface on a CPU double of the device ops, backed by the restatement ------------------------------------------------
def _hp(parts, d, rng):
    blocks = []
    for p in parts:
        if p == "wn":
            blocks.append([0.2])
        else:
            blocks.append(np.concatenate([[1.1], 0.5 + rng.random(d), rng.uniform(0.7, 2.5, d) if p == "per" else ([0.8] if p == "rq" else [])]))
    return np.concatenate(blocks)


@pytest.mark.parametrize("parts", [["per", "wn"], ["wn", "per", "m32"], ["rq", "per", "wn"]], ids=lambda p: "+".join(p))
def test_public_surface_on_the_cpu_double(fake_ops, parts):
    """A wide block in front of a later child (and of the noise): Exact_GP reads every child's sigma by its layout offset."""
    rng = np.random.default_rng(7)
    n, m, d = 50, 11, 3
    x, y = orc.synth(n, d, seed=4)
    xp = rng.random((m, d))
    hp = _hp(parts, d, rng)
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
    parts = ["per", "wn"]
    x = rng.random((nc, n, d))
    y = np.sin(-x.sum(-1)) + 0.1 * rng.standard_normal((nc, n))
    xp = rng.random((nc, m, d))
    hp = np.stack([_hp(parts, d, rng) for _ in range(nc)])
    gp = pg.Exact_GP(T(x), T(y), compose(parts))
    assert list(gp.cov.get_params_shape(T(x))) == [nc, 2 * d + 2]
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
