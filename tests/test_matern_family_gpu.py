"""GPU tier of the Matern family: Matern-1/2 and Matern-3/2 through every covariance path (C ABI entry points, the dK stack, the
fused gradient, Exact_GP / MLE / batched experts / GRBCM / SK_WRAP) against the direct-difference restatement of tests/kernel_ref.py.
Matern-3/2 takes the matrix-pipe bodies where Matern-5/2 does; Matern-1/2 never does (its K is 1 - r near r = 0, so the expansion's
error in the squared distance would reach K as a square root): the near-duplicate test below is the one that says so."""
import numpy as np
import pytest
import torch

import pygpr_amd as pg
from oracle import pygpr_oracle as orc

import kernel_ref as kr
from kind_tools import N, T, builds, compose, dev, grad_inputs, host, near_duplicates, one_spec, ops  # noqa: F401  (ops: the fixture)

pytestmark = pytest.mark.gpu


# --------------------------------------------------------------------------- 1. entry points
@pytest.mark.parametrize("part", ["m12", "m32"])
@pytest.mark.parametrize("d", [2, 5, 8, 13, 16, 24])
def test_entry_points_against_the_restatement(ops, monkeypatch, part, d):
    """Mirrored, lower-only and cross builds and the fused gradient, fp64 / fp32, with the matrix pipe forced on and off: Matern-3/2
    at d <= 16 takes kmfma.hip and must agree with the VALU bodies; Matern-1/2 stays on the VALU bodies either way (the same bits)."""
    from pygpr_amd._ops import pad_to

    rng = np.random.default_rng(10 * d + len(part))
    n, m = 333, 200
    x, y = orc.synth(n, d, seed=d)
    xp = rng.random((m, d))
    parts = [part, "wn"]
    hp = np.concatenate([[1.2], 0.4 + 0.8 * rng.random(d), [0.1]])
    spec, npad = one_spec(parts, d), pad_to(n)
    ref = kr.kernel(parts, hp, x) + 1e-7 * np.eye(n)
    ref_x = kr.kernel(parts, hp, x, xp)
    for dtype, tol in ((torch.float64, 2e-14), (torch.float32, 4e-6)):
        out = {}
        for mode in ("2", "0"):
            monkeypatch.setenv("PG_KB_MFMA", mode)
            out[mode] = builds(ops, spec, hp, x, xp, dtype)
        monkeypatch.delenv("PG_KB_MFMA")
        full, low, cross = out["2"]
        np.testing.assert_allclose(full[:n, :n], ref, atol=tol, rtol=tol)
        np.testing.assert_allclose(cross[:m, :n], ref_x, atol=tol, rtol=tol)
        if part == "m12" or d > 16:
            for a, b in zip(out["2"], out["0"]):
                assert np.array_equal(a, b)                                       # no matrix-pipe body: the same kernel either way
        else:
            np.testing.assert_allclose(full, out["0"][0], atol=tol, rtol=tol)
            np.testing.assert_allclose(cross, out["0"][2], atol=tol, rtol=tol)
        assert np.array_equal(full[:n, :n], full[:n, :n].T)                       # exactly symmetric
        pad_ref = np.eye(npad)
        pad_ref[:n, :n] = full[:n, :n]
        assert np.array_equal(full, pad_ref)                                      # identity padding
        assert not cross[m:, :].any() and not cross[:, n:].any()                  # zero padding of a cross build
        tl = np.tril_indices(npad)
        assert np.array_equal(low[tl], full[tl])                                  # lower-only == mirrored on the lower triangle
        dgv = np.float64(np.float32(1.2 ** 2 + 0.1 ** 2 + 1e-7)) if dtype == torch.float32 else 1.2 ** 2 + 0.1 ** 2 + 1e-7
        np.testing.assert_allclose(np.diag(full)[:n], dgv, rtol=2e-7 if dtype == torch.float32 else 1e-15)
    _, grad_ref = kr.nlml_and_grad(parts, hp, x, y)
    scale = np.abs(grad_ref).max()
    for dtype, rtol in ((torch.float64, 1e-9), (torch.float32, 3e-3)):
        hpd, xd, kinv, alpha = grad_inputs(ops, spec, hp, x, y, dtype)
        work = ops.empty(ops.nlml_grad_worksize(n, hp.size))
        got = {}
        for mode in ("1", "0"):
            monkeypatch.setenv("PG_GRAD_MFMA", mode)
            g = ops.zeros(hp.size)
            ops.nlml_grad(spec, hpd, xd, n, kinv, alpha, g, work)
            got[mode] = host(g)
        monkeypatch.delenv("PG_GRAD_MFMA")
        assert np.isfinite(got["1"]).all()
        if part == "m12" or d > 16:
            assert np.array_equal(got["1"], got["0"])
        else:
            np.testing.assert_allclose(got["1"], got["0"], rtol=rtol, atol=rtol * scale)
        # (fp32: K^-1 itself carries cond(K) x 6e-8; the same allowance as the Matern-5/2 test of test_hip_kernels.py)
        tol_ref = rtol if dtype == torch.float64 else 3 * rtol
        np.testing.assert_allclose(got["1"], grad_ref, rtol=tol_ref, atol=tol_ref * scale)


# --------------------------------------------------------------------------- 2. near-duplicates
def test_matern12_near_duplicates_on_offset_data(ops, monkeypatch):
    """Near-duplicate pairs on data offset by 1e3.  Direct differences keep K to rounding (the matrix pipe's expansion would be off by
    ~sqrt(u) |x|: 1e-8 in fp64), and the gradient's factor 1/r stays bounded.  The inverse length scales are powers of two, so the
    scaled coordinates the VALU body stages are exact and the 1e-13 below measures the arithmetic alone."""
    rng = np.random.default_rng(12)
    d = 5
    l = np.array([0.5, 1.0, 2.0, 0.25, 1.0])
    hp = np.concatenate([[1.2], l, [0.1]])
    parts = ["m12", "wn"]
    x, y = near_duplicates(rng, d, l, 1.0e3)
    n = x.shape[0]
    spec = one_spec(parts, d)
    for mode in ("1", "2"):
        monkeypatch.setenv("PG_KB_MFMA", mode)
        monkeypatch.setenv("PG_GRAD_MFMA", mode)
        for dtype, tol in ((torch.float64, 1e-13), (torch.float32, 4e-6)):
            xt = x if dtype == torch.float64 else x.astype(np.float32).astype(np.float64)     # the fp32 run's own inputs
            ref = kr.kernel(parts, hp, xt)
            k = ops.empty(256, 256, dtype=dtype)
            ops.kernel_build(spec, dev(hp), dev(xt, dtype), None, k)
            np.testing.assert_allclose(host(k)[:n, :n], ref, rtol=0, atol=tol)
            kx = ops.empty(128, 256, dtype=dtype)
            ops.kernel_build(spec, dev(hp), dev(xt[::-1].copy(), dtype), dev(xt, dtype), kx)     # a cross build meets the same pairs
            np.testing.assert_allclose(host(kx)[:n, :n], kr.kernel(parts, hp, xt, xt[::-1].copy()), rtol=0, atol=tol)
        loss_ref, grad_ref = kr.nlml_and_grad(parts, hp, x, y)
        gp = pg.Exact_GP(T(x), T(y), compose(parts))
        loss, grad = pg.MLE(gp).loss_and_grad(hp.copy())
        assert np.isfinite(grad).all()
        np.testing.assert_allclose(loss, loss_ref, rtol=1e-10)
        np.testing.assert_allclose(grad, grad_ref, rtol=1e-9, atol=1e-9 * np.abs(grad_ref).max())
        _, dk = compose(parts).kernel_and_grad(T(hp), T(x))
        assert np.isfinite(N(dk)).all()
        np.testing.assert_allclose(N(dk), kr.kernel_and_grad(parts, hp, x)[1], rtol=0, atol=1e-12)
        # prediction AT the training points: every pair of the cross build is a near-duplicate or a duplicate
        gp = pg.Exact_GP(T(x), T(y), compose(parts))
        gp.set_params(T(hp))
        mu, var = gp.predict(T(x), var="diag")
        mu_ref, var_ref = kr.predict(parts, hp, x, y, x)
        np.testing.assert_allclose(N(mu), mu_ref, rtol=0, atol=1e-10)
        np.testing.assert_allclose(N(var), var_ref, rtol=0, atol=1e-10)


# --------------------------------------------------------------------------- 3. several components
@pytest.mark.parametrize("parts", [["m12", "m32", "wn"], ["m32", "se", "wn"]])
def test_multi_component(parts):
    rng = np.random.default_rng(len(parts[0]) + 7)
    n, m, d = 200, 50, 3
    x, y = orc.synth(n, d, seed=5)
    xp = rng.random((m, d))
    hp = np.concatenate([[1.1], 0.5 + rng.random(d), [0.8], 0.5 + rng.random(d), [0.1]])
    cov = compose(parts)
    np.testing.assert_allclose(N(cov.kernel(T(hp), T(x))), kr.kernel(parts, hp, x), rtol=0, atol=1e-13)
    np.testing.assert_allclose(N(cov.kernel(T(hp), T(x), T(xp))), kr.kernel(parts, hp, x, xp), rtol=0, atol=1e-13)
    k, dk = cov.kernel_and_grad(T(hp), T(x))
    k_ref, dk_ref = kr.kernel_and_grad(parts, hp, x)
    np.testing.assert_allclose(N(k), k_ref, rtol=0, atol=1e-13)
    np.testing.assert_allclose(N(dk), dk_ref, rtol=0, atol=1e-12)
    loss, grad = pg.MLE(pg.Exact_GP(T(x), T(y), cov)).loss_and_grad(hp.copy())
    loss_ref, grad_ref = kr.nlml_and_grad(parts, hp, x, y)
    np.testing.assert_allclose(loss, loss_ref, rtol=1e-10)
    np.testing.assert_allclose(grad, grad_ref, rtol=1e-8, atol=1e-8 * np.abs(grad_ref).max())


# --------------------------------------------------------------------------- 4. NaN
@pytest.mark.parametrize("part", ["m12", "m32"])
def test_nan_coordinate_gives_a_nan_row_and_column(ops, monkeypatch, part):
    rng = np.random.default_rng(4)
    n, d = 70, 3
    x = rng.random((n, d))
    x[23, 1] = np.nan
    hp = np.array([1.0, 0.7, 0.8, 0.9, 0.1])
    for mode in ("2", "0"):
        monkeypatch.setenv("PG_KB_MFMA", mode)
        for dt in (torch.float64, torch.float32):
            k = ops.empty(256, 256, dtype=dt)
            ops.kernel_build(one_spec([part, "wn"], d), dev(hp), dev(x, dt), None, k, jitter=1e-7)
            got = host(k)
            assert np.isnan(got[23, :n]).all() and np.isnan(got[:n, 23]).all()
            assert np.isfinite(np.delete(np.delete(got[:n, :n], 23, 0), 23, 1)).all()


# --------------------------------------------------------------------------- 5. public surface
@pytest.mark.parametrize("part", ["m12", "m32"])
def test_exact_gp_and_mle(part):
    rng = np.random.default_rng(len(part))
    n, m, d = 1000, 60, 5
    x, y = orc.synth(n, d, seed=9)
    xp = rng.random((m, d))
    parts = [part, "wn"]
    hp = np.concatenate([[1.1], 0.5 + rng.random(d), [0.1]])
    gp = pg.Exact_GP(T(x), T(y), compose(parts))
    gp.set_params(T(hp))
    gp.update()
    mu, var = gp.predict(T(xp), var="diag")
    mu_ref, var_ref = kr.predict(parts, hp, x, y, xp)
    np.testing.assert_allclose(N(mu), mu_ref, rtol=0, atol=1e-10)
    np.testing.assert_allclose(N(var), var_ref, rtol=0, atol=1e-10)
    mu_f, cov_f = gp.predict(T(xp), var="full")
    _, cov_ref = kr.predict(parts, hp, x, y, xp, var="full")
    np.testing.assert_allclose(N(mu_f), mu_ref, rtol=0, atol=1e-10)
    np.testing.assert_allclose(N(cov_f), cov_ref, rtol=0, atol=1e-10)
    loss, grad = pg.MLE(gp).loss_and_grad(hp.copy())
    loss_ref, grad_ref = kr.nlml_and_grad(parts, hp, x, y)
    np.testing.assert_allclose(loss, loss_ref, rtol=1e-10)
    np.testing.assert_allclose(grad, grad_ref, rtol=1e-8, atol=1e-8 * np.abs(grad_ref).max())


@pytest.mark.parametrize("part", ["m12", "m32"])
def test_batched_experts_match_their_loop(part):
    rng = np.random.default_rng(20 + len(part))
    nc, n, m, d = 4, 250, 30, 4
    x = rng.random((nc, n, d))
    y = np.sin(-x.sum(-1)) + 0.1 * rng.standard_normal((nc, n))
    xp = rng.random((nc, m, d))
    parts = [part, "wn"]
    hp = np.concatenate([0.8 + 0.4 * rng.random((nc, 1)), 0.5 + rng.random((nc, d)), np.full((nc, 1), 0.1)], axis=1)
    gp = pg.Exact_GP(T(x), T(y), compose(parts))
    gp.set_params(T(hp))
    mu, var = gp.predict(T(xp), var="diag")
    loss, grad = pg.MLE(pg.Exact_GP(T(x), T(y), compose(parts))).loss_and_grad(hp.copy())
    for c in range(nc):
        one = pg.Exact_GP(T(x[c]), T(y[c]), compose(parts))
        one.set_params(T(hp[c]))
        mu1, var1 = one.predict(T(xp[c]), var="diag")
        np.testing.assert_allclose(N(mu[c]), N(mu1), rtol=0, atol=1e-11)
        np.testing.assert_allclose(N(var[c]).ravel(), N(var1).ravel(), rtol=0, atol=1e-11)
        l1, g1 = pg.MLE(one).loss_and_grad(hp[c].copy())
        np.testing.assert_allclose(loss[c], l1, rtol=1e-11)
        np.testing.assert_allclose(grad[c], g1, rtol=1e-9, atol=1e-9 * np.abs(g1).max())
        l_ref, g_ref = kr.nlml_and_grad(parts, hp[c], x[c], y[c])
        np.testing.assert_allclose(l1, l_ref, rtol=1e-10)
        np.testing.assert_allclose(g1, g_ref, rtol=1e-8, atol=1e-8 * np.abs(g_ref).max())


def test_grbcm_with_matern32():
    rng = np.random.default_rng(33)
    nc, nsc, ng, m, d = 3, 120, 40, 25, 3
    xl, xg, xs = rng.random((nc, nsc, d)), rng.random((ng, d)), rng.random((m, d))
    yl, yg = np.sin(-xl.sum(-1)), np.sin(-xg.sum(-1))
    parts = ["m32", "wn"]
    hp_g = np.concatenate([[1.0], 0.6 + rng.random(d), [0.1]])
    hp_l = np.concatenate([0.9 + 0.2 * rng.random((nc, 1)), 0.6 + rng.random((nc, d)), np.full((nc, 1), 0.1)], axis=1)
    model = pg.GRBCM(T(xl), T(yl), T(xg), T(yg), compose(parts))
    model.gpg.set_params(T(hp_g))
    model.gpl.set_params(T(hp_l))
    mu, var = model.predict(T(xs), var="diag")
    mu_ref, var_ref = kr.grbcm_predict(parts, hp_g, hp_l, xl, yl, xg, yg, xs)
    np.testing.assert_allclose(N(mu), mu_ref, rtol=0, atol=1e-9)
    np.testing.assert_allclose(N(var).ravel(), var_ref, rtol=1e-9, atol=1e-11)


def test_sk_wrap_with_matern12():
    rng = np.random.default_rng(44)
    n, m, d = 900, 40, 3
    x, y = orc.synth(n, d, seed=44)
    xp = rng.random((m, d))
    parts = ["m12", "wn"]
    hp = np.concatenate([[1.0], 0.5 + rng.random(d), [0.1]])
    gp = pg.Exact_GP(T(x[:10]), T(y[:10]), compose(parts))
    gp.set_params(T(hp))
    sk = pg.SK_WRAP(gp).fit(T(x), T(y))
    np.testing.assert_allclose(N(sk.predict(T(xp))), kr.predict(parts, hp, x, y, xp)[0], rtol=0, atol=1e-10)


# --------------------------------------------------------------------------- 6. at size
@pytest.mark.parametrize("part", ["m32", "m12"])
def test_nlml_and_gradient_at_n4096(part):
    n, d = 4096, 8
    x, y = orc.synth(n, d, seed=41)
    parts = [part, "wn"]
    hp = np.concatenate([[1.0], np.linspace(0.6, 1.4, d), [0.1]])
    loss, grad = pg.MLE(pg.Exact_GP(T(x), T(y), compose(parts))).loss_and_grad(hp.copy())
    loss_ref, grad_ref = kr.nlml_and_grad(parts, hp, x, y)
    np.testing.assert_allclose(loss, loss_ref, rtol=1e-10)
    np.testing.assert_allclose(grad, grad_ref, rtol=1e-8, atol=1e-8 * np.abs(grad_ref).max())


# --------------------------------------------------------------------------- 7. refusals
def test_unknown_kind_is_still_refused(ops):
    from pygpr_amd._ops import make_spec

    x = dev(np.random.default_rng(1).random((10, 2)))
    with pytest.raises(RuntimeError, match="unknown kernel kind 5"):
        ops.kernel_build(make_spec([5], [0], []), dev(np.ones(3)), x, None, ops.empty(64, 64))
    with pytest.raises(RuntimeError, match="unknown kernel kind 5"):
        ops.kernel_grad_build(make_spec([5], [0], []), dev(np.ones(3)), x, ops.empty(3, 10, 10))
