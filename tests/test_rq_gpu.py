"""GPU tier of the rational quadratic: the kind whose block is d + 2 wide through every covariance path (C ABI entry points, the dK stack
with its shape slab, the fused gradient with its shape entry, Exact_GP / MLE / LOO / predict_grad / append / batched experts / GRBCM /
SK_WRAP) against the direct-difference restatement of tests/kernel_ref.py.  K is smooth in the squared distance (|dK/dsq| <= sigma^2), so the
kind takes the matrix-pipe bodies where Matern-3/2 does; the tolerances are those tests/test_matern_family_gpu.py uses for the same
quantities."""
import numpy as np
import pytest
import torch

import pygpr_amd as pg
from oracle import pygpr_oracle as orc

import kernel_ref as kr
import loo_ref
from kind_tools import N, T, builds, check, compose, dev, grad_inputs, host, near_duplicates, one_spec, ops  # noqa: F401  (ops: the fixture)

pytestmark = pytest.mark.gpu


# --------------------------------------------------------------------------- 1. entry points
@pytest.mark.parametrize("d,alpha", [(2, 0.6), (5, 1.0), (8, 3.0), (13, 0.6), (16, 3.0), (24, 0.6)])
def test_entry_points_against_the_restatement(ops, monkeypatch, d, alpha):
    """Mirrored, lower-only and cross builds and the fused gradient with its shape entry, fp64 / fp32, the matrix pipe forced on and off:
    at d <= 16 the kind takes kmfma.hip and must agree with the VALU bodies; beyond, the same kernel serves either way (the same bits).
    Bounds: test_matern_family_gpu.py::test_entry_points_against_the_restatement (2e-14 / 4e-6 on K; 1e-9 and 3 x 3e-3 on the gradient)."""
    from pygpr_amd._ops import pad_to

    rng = np.random.default_rng(10 * d + 2)
    n, m = 333, 200
    x, y = orc.synth(n, d, seed=d)
    xp = rng.random((m, d))
    parts = ["rq", "wn"]
    hp = np.concatenate([[1.2], 0.4 + 0.8 * rng.random(d), [alpha], [0.1]])
    spec, npad = one_spec(parts, d), pad_to(n)
    ref = kr.kernel(parts, hp, x) + 1e-7 * np.eye(n)
    ref_x = kr.kernel(parts, hp, x, xp)
    for dtype, tol in ((torch.float64, 2e-14), (torch.float32, 4e-6)):
        out = {}
        for mode in ("2", "0"):
            monkeypatch.setenv("PG_KB_MFMA", mode)
            out[mode] = builds(ops, spec, hp, x, xp, dtype)
        monkeypatch.delenv("PG_KB_MFMA")
        for mode in ("2", "0"):
            full, low, cross = out[mode]
            print("d=%d %s PG_KB_MFMA=%s: K err %.2e, cross err %.2e (bound %.0e)" % (
                d, dtype, mode, np.abs(full[:n, :n] - ref).max(), np.abs(cross[:m, :n] - ref_x).max(), tol))
        for mode in ("2", "0"):
            full, low, cross = out[mode]
            np.testing.assert_allclose(full[:n, :n], ref, atol=tol, rtol=tol)
            np.testing.assert_allclose(cross[:m, :n], ref_x, atol=tol, rtol=tol)
            assert np.array_equal(full[:n, :n], full[:n, :n].T)                       # exactly symmetric
            pad_ref = np.eye(npad)
            pad_ref[:n, :n] = full[:n, :n]
            assert np.array_equal(full, pad_ref)                                      # identity padding
            assert not cross[m:, :].any() and not cross[:, n:].any()                  # zero padding of a cross build
            tl = np.tril_indices(npad)
            assert np.array_equal(low[tl], full[tl])                                  # lower-only == mirrored on the lower triangle
            dgv = np.float64(np.float32(1.2 ** 2 + 0.1 ** 2 + 1e-7)) if dtype == torch.float32 else 1.2 ** 2 + 0.1 ** 2 + 1e-7
            np.testing.assert_allclose(np.diag(full)[:n], dgv, rtol=2e-7 if dtype == torch.float32 else 1e-15)
        full, low, cross = out["2"]
        if d > 16:
            for a, b in zip(out["2"], out["0"]):
                assert np.array_equal(a, b)                                           # no matrix-pipe body: the same kernel either way
        else:
            np.testing.assert_allclose(full, out["0"][0], atol=tol, rtol=tol)
            np.testing.assert_allclose(cross, out["0"][2], atol=tol, rtol=tol)
    _, grad_ref = kr.nlml_and_grad(parts, hp, x, y)
    scale = np.abs(grad_ref).max()
    assert grad_ref[d + 1] != 0.0
    for dtype, rtol in ((torch.float64, 1e-9), (torch.float32, 3e-3)):
        hpd, xd, kinv, alpha_v = grad_inputs(ops, spec, hp, x, y, dtype)
        work = ops.empty(ops.nlml_grad_worksize(n, hp.size))
        got = {}
        for mode in ("1", "0"):
            monkeypatch.setenv("PG_GRAD_MFMA", mode)
            g = ops.zeros(hp.size)
            ops.nlml_grad(spec, hpd, xd, n, kinv, alpha_v, g, work)
            got[mode] = host(g)
        monkeypatch.delenv("PG_GRAD_MFMA")
        tol_ref = rtol if dtype == torch.float64 else 3 * rtol
        for mode in ("1", "0"):
            print("d=%d %s PG_GRAD_MFMA=%s: gradient err / max %.2e, shape entry %.2e (bound %.0e)" % (
                d, dtype, mode, np.abs(got[mode] - grad_ref).max() / scale, abs(got[mode][d + 1] - grad_ref[d + 1]) / scale, tol_ref))
        assert np.isfinite(got["1"]).all()
        if d > 16:
            assert np.array_equal(got["1"], got["0"])
        else:
            np.testing.assert_allclose(got["1"], got["0"], rtol=rtol, atol=rtol * scale)
        # (fp32: K^-1 itself carries cond(K) x 6e-8; the same allowance as the Matern tests)
        for mode in ("1", "0"):
            np.testing.assert_allclose(got[mode], grad_ref, rtol=tol_ref, atol=tol_ref * scale)      # (the shape entry is entry d + 1)


# --------------------------------------------------------------------------- 2. near-duplicates
def test_near_duplicates_on_offset_data(ops, monkeypatch):
    """Near-duplicate pairs on data offset by 1e3.  VALU path (direct differences): K, the dK stack and the shape slab to the Matern
    test's absolute bounds (1e-13 / 4e-6 on K, 1e-12 on dK; the inverse length scales are powers of two, so the staged coordinates are
    exact).  Matrix-pipe path: that file grants Matern-3/2 no bound under this offset, so Matern-3/2's own error on this data is measured
    in the same run and the rational quadratic is allowed twice that."""
    rng = np.random.default_rng(12)
    d = 5
    l = np.array([0.5, 1.0, 2.0, 0.25, 1.0])
    hp = np.concatenate([[1.2], l, [0.7], [0.1]])
    hp_m = np.concatenate([[1.2], l, [0.1]])
    parts = ["rq", "wn"]
    x, y = near_duplicates(rng, d, l, 1.0e3)
    n = x.shape[0]
    spec, spec_m = one_spec(parts, d), one_spec(["m32", "wn"], d)
    for dtype, tol in ((torch.float64, 1e-13), (torch.float32, 4e-6)):
        xt = x if dtype == torch.float64 else x.astype(np.float32).astype(np.float64)     # the fp32 run's own inputs
        ref, ref_m = kr.kernel(parts, hp, xt), kr.kernel(["m32", "wn"], hp_m, xt)
        err = {}
        for mode in ("0", "2"):
            monkeypatch.setenv("PG_KB_MFMA", mode)
            k, km = ops.empty(256, 256, dtype=dtype), ops.empty(256, 256, dtype=dtype)
            ops.kernel_build(spec, dev(hp), dev(xt, dtype), None, k)
            ops.kernel_build(spec_m, dev(hp_m), dev(xt, dtype), None, km)
            assert np.isfinite(host(k)).all()
            err[mode] = (np.abs(host(k)[:n, :n] - ref).max(), np.abs(host(km)[:n, :n] - ref_m).max())
            kx = ops.empty(128, 256, dtype=dtype)
            ops.kernel_build(spec, dev(hp), dev(xt[::-1].copy(), dtype), dev(xt, dtype), kx)     # a cross build meets the same pairs
            errx = np.abs(host(kx)[:n, :n] - kr.kernel(parts, hp, xt, xt[::-1].copy())).max()
            print("%s PG_KB_MFMA=%s: K err rq %.2e, Matern-3/2 %.2e; cross rq %.2e" % (dtype, mode, err[mode][0], err[mode][1], errx))
            if mode == "0":
                assert err[mode][0] <= tol and errx <= tol
            else:
                assert err[mode][0] <= 2 * err[mode][1] and errx <= 2 * err[mode][1]
        monkeypatch.delenv("PG_KB_MFMA")
    k_ref, dk_ref = kr.kernel_and_grad(parts, hp, x)
    _, dk = compose(parts).kernel_and_grad(T(hp), T(x))
    assert np.isfinite(N(dk)).all()
    np.testing.assert_allclose(N(dk), dk_ref, rtol=0, atol=1e-12)                        # (the shape slab is dk[d + 1])
    loss_ref, grad_ref = kr.nlml_and_grad(parts, hp, x, y)
    _, gm_ref = kr.nlml_and_grad(["m32", "wn"], hp_m, x, y)
    errs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("PG_KB_MFMA", mode)
        monkeypatch.setenv("PG_GRAD_MFMA", mode)
        loss, grad = pg.MLE(pg.Exact_GP(T(x), T(y), compose(parts))).loss_and_grad(hp.copy())
        _, gm = pg.MLE(pg.Exact_GP(T(x), T(y), compose(["m32", "wn"]))).loss_and_grad(hp_m.copy())
        assert np.isfinite(grad).all()
        errs[mode] = (np.abs(grad - grad_ref).max() / np.abs(grad_ref).max(), np.abs(gm - gm_ref).max() / np.abs(gm_ref).max())
        print("PG_*_MFMA=%s: gradient err / max rq %.2e, Matern-3/2 %.2e" % (mode, errs[mode][0], errs[mode][1]))
    assert errs["0"][0] <= 1e-9                                                          # VALU: the Matern test's bound
    assert errs["1"][0] <= 2 * max(errs["1"][1], 1e-9)                                   # matrix pipe: twice Matern-3/2's, measured here


# --------------------------------------------------------------------------- 3. dK stack, several components
@pytest.mark.parametrize("parts", [["rq", "wn"], ["rq", "se", "wn"]], ids=lambda p: "+".join(p))
def test_dk_stack_and_compose(parts):
    """atol 1e-13 on K, 1e-12 on dK: test_matern_family_gpu.py::test_multi_component."""
    rng = np.random.default_rng(len(parts) + 7)
    n, m, d = 200, 50, 3
    x, y = orc.synth(n, d, seed=5)
    xp = rng.random((m, d))
    hp = np.concatenate([[0.1] if p == "wn" else np.concatenate([[1.1], 0.5 + rng.random(d), [0.6] if p == "rq" else []]) for p in parts])
    cov = compose(parts)
    np.testing.assert_allclose(N(cov.kernel(T(hp), T(x))), kr.kernel(parts, hp, x), rtol=0, atol=1e-13)
    np.testing.assert_allclose(N(cov.kernel(T(hp), T(x), T(xp))), kr.kernel(parts, hp, x, xp), rtol=0, atol=1e-13)
    k, dk = cov.kernel_and_grad(T(hp), T(x))
    k_ref, dk_ref = kr.kernel_and_grad(parts, hp, x)
    assert dk.shape == (kr.nhp_of(parts, d), n, n) and dk_ref[d + 1].any()
    np.testing.assert_allclose(N(k), k_ref, rtol=0, atol=1e-13)
    np.testing.assert_allclose(N(dk), dk_ref, rtol=0, atol=1e-12)
    loss, grad = pg.MLE(pg.Exact_GP(T(x), T(y), cov)).loss_and_grad(hp.copy())
    loss_ref, grad_ref = kr.nlml_and_grad(parts, hp, x, y)
    np.testing.assert_allclose(loss, loss_ref, rtol=1e-10)
    np.testing.assert_allclose(grad, grad_ref, rtol=1e-8, atol=1e-8 * np.abs(grad_ref).max())


def test_compose_longer_than_one_pass():
    """Six stationary children (PG_MAX_COMP = 4): two passes, the rational quadratic in each, beside SE and Matern children and noise."""
    parts = ["rq", "se", "m32", "rq", "wn", "se", "rq"]
    rng = np.random.default_rng(3)
    n, m, d = 150, 40, 3
    x, y = orc.synth(n, d, seed=6)
    xp = rng.random((m, d))
    hp = np.concatenate([[0.2] if p == "wn" else np.concatenate([[0.7], 0.5 + rng.random(d), [0.5 + rng.random()] if p == "rq" else []]) for p in parts])
    cov = compose(parts)
    from pygpr_amd.covar import spec_of
    assert len(spec_of(cov, d)[0]) == 2
    np.testing.assert_allclose(N(cov.kernel(T(hp), T(x))), kr.kernel(parts, hp, x), rtol=0, atol=1e-13)
    np.testing.assert_allclose(N(cov.kernel(T(hp), T(x), T(xp))), kr.kernel(parts, hp, x, xp), rtol=0, atol=1e-13)
    np.testing.assert_allclose(N(cov.kernel_and_grad(T(hp), T(x))[1]), kr.kernel_and_grad(parts, hp, x)[1], rtol=0, atol=1e-12)
    loss, grad = pg.MLE(pg.Exact_GP(T(x), T(y), cov)).loss_and_grad(hp.copy())
    loss_ref, grad_ref = kr.nlml_and_grad(parts, hp, x, y)
    np.testing.assert_allclose(loss, loss_ref, rtol=1e-10)
    np.testing.assert_allclose(grad, grad_ref, rtol=1e-8, atol=1e-8 * np.abs(grad_ref).max())


# --------------------------------------------------------------------------- 4. NaN
def test_nan_coordinate_and_nan_shape(ops, monkeypatch):
    rng = np.random.default_rng(4)
    n, d = 70, 3
    x = rng.random((n, d))
    xn = x.copy()
    xn[23, 1] = np.nan
    hp = np.array([1.0, 0.7, 0.8, 0.9, 0.8, 0.1])
    hp_nan = hp.copy()
    hp_nan[d + 1] = np.nan
    for mode in ("2", "0"):
        monkeypatch.setenv("PG_KB_MFMA", mode)
        for dt in (torch.float64, torch.float32):
            k = ops.empty(256, 256, dtype=dt)
            ops.kernel_build(one_spec(["rq", "wn"], d), dev(hp), dev(xn, dt), None, k, jitter=1e-7)
            got = host(k)
            assert np.isnan(got[23, :n]).all() and np.isnan(got[:n, 23]).all()
            assert np.isfinite(np.delete(np.delete(got[:n, :n], 23, 0), 23, 1)).all()
            ops.kernel_build(one_spec(["rq", "wn"], d), dev(hp_nan), dev(x, dt), None, k, jitter=1e-7)
            assert np.isnan(host(k)[:n, :n]).all()                                     # a NaN shape: every entry


# --------------------------------------------------------------------------- 5. public surface
@pytest.mark.parametrize("n,d", [(1000, 5), (2049, 8)])
def test_exact_gp_and_mle(n, d):
    """n = 2049: an odd tile count, padded to 2304.  Bounds: test_matern_family_gpu.py::test_exact_gp_and_mle."""
    rng = np.random.default_rng(n)
    m = 60
    x, y = orc.synth(n, d, seed=9)
    xp = rng.random((m, d))
    parts = ["rq", "wn"]
    hp = np.concatenate([[1.1], 0.5 + rng.random(d), [0.8], [0.1]])
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


def test_loo_loss_and_grad():
    """LOO(model).loss_and_grad against loo_ref's closed forms (R&W 5.10 - 5.13) on kernel_ref's kernel and slabs; the relative bounds of
    tests/test_loo_gpu.py's own comparison are not assumed: loss 1e-10 and gradient 1e-8 of its largest entry, as for the NLML above."""
    parts = ["rq", "wn"]
    n, d = 300, 4
    x, y = orc.synth(n, d, seed=21)
    hp = np.concatenate([[1.1], np.linspace(0.6, 1.2, d), [0.7], [0.3]])
    k = kr.kernel(parts, hp, x) + kr.JITTER * np.eye(n)
    kinv = np.linalg.inv(k)
    kinv = 0.5 * (kinv + kinv.T)
    alpha, c = kinv @ y, np.diag(kinv).copy()
    loss_ref = loo_ref.loss_from(y - alpha / c, 1.0 / c, y)
    g_ref = loo_ref.grad_from(parts, hp, x, kinv, alpha, c)
    gp = pg.Exact_GP(T(x), T(y), compose(parts))
    gp.set_params(T(hp))
    loss, grad = pg.LOO(gp).loss_and_grad(hp.copy())
    print("LOO loss err %.2e, gradient err / max %.2e" % (abs(loss - loss_ref) / abs(loss_ref), np.abs(grad - g_ref).max() / np.abs(g_ref).max()))
    np.testing.assert_allclose(loss, loss_ref, rtol=1e-10)
    np.testing.assert_allclose(grad, g_ref, rtol=1e-8, atol=1e-8 * np.abs(g_ref).max())
    mu, var = gp.loo_predict()
    np.testing.assert_allclose(N(mu), y - alpha / c, rtol=0, atol=1e-9)
    np.testing.assert_allclose(N(var), 1.0 / c, rtol=1e-9, atol=0)


@pytest.mark.parametrize("parts", [["rq", "wn"], ["rq", "m32", "wn"]], ids=lambda p: "+".join(p))
def test_predict_grad_and_autograd(parts):
    """predict_grad and autograd in xp against kernel_ref's x*-derivatives: 1e-9 relative to the largest entry, tests/test_xgrad_gpu.py."""
    rng = np.random.default_rng(1)
    n, m, d = 300, 45, 5
    x = rng.random((n, d))
    y = np.sin(3.0 * x).sum(1) + 0.1 * rng.standard_normal(n)
    xp = rng.random((m, d))
    hp = np.concatenate([[0.3] if p == "wn" else np.concatenate([[rng.uniform(0.8, 1.3)], rng.uniform(0.5, 1.5, d) / np.sqrt(d),
                                                                    [0.7] if p == "rq" else []]) for p in parts])
    gp = pg.Exact_GP(T(x), T(y), compose(parts))
    gp.set_params(T(hp))
    mean, var, dmean, dvar = gp.predict_grad(T(xp), var="diag")
    rdm, rdv = kr.predict_grads(parts, hp, x, y, xp)
    check("predict_grad %s dmean" % "+".join(parts), dmean, T(rdm), 1e-9)
    check("predict_grad %s dvar" % "+".join(parts), dvar, T(rdv), 1e-9)
    g_mu = rng.standard_normal(m)
    for var_kind in ("none", "diag", "full"):
        g_2 = rng.standard_normal((m, m) if var_kind == "full" else m)
        xq = T(xp).to("cuda").requires_grad_(True)
        out = gp.predict(xq, var=var_kind)
        loss = (dev(g_mu) * out[0]).sum() + ((dev(g_2) * out[1]).sum() if var_kind != "none" else 0.0)
        loss.backward()
        check("autograd %s %s" % ("+".join(parts), var_kind), xq.grad, T(kr.predict_vjp(parts, hp, x, y, xp, var_kind, g_mu, g_2)), 1e-9)


def test_predict_grad_batched_experts():
    parts = ["rq", "wn"]
    nc, n, m, d = 3, 200, 33, 3
    rng = np.random.default_rng(2)
    x = rng.random((nc, n, d))
    y = rng.standard_normal((nc, n))
    xp = rng.random((m, d))
    hps = np.concatenate([rng.uniform(0.8, 1.3, (nc, 1)), rng.uniform(0.5, 1.5, (nc, d)) / np.sqrt(d), rng.uniform(0.6, 2.0, (nc, 1)),
                          np.full((nc, 1), 0.3)], axis=1)
    gp = pg.Exact_GP(T(x), T(y), compose(parts))
    gp.set_params(T(hps))
    mean, var, dmean, dvar = gp.predict_grad(T(xp), var="diag")
    assert dmean.shape == (nc, m, d)
    for c in range(nc):
        rdm, rdv = kr.predict_grads(parts, hps[c], x[c], y[c], xp)
        check("predict_grad batched expert %d dmean" % c, dmean[c], T(rdm), 1e-9)
        check("predict_grad batched expert %d dvar" % c, dvar[c], T(rdv), 1e-9)


def test_append_equals_fresh_fit():
    """append of 10 points against a fresh fit: TOL64 = 1e-9 (ten times that on derivatives), tests/test_append_gpu.py::compare."""
    parts = ["rq", "wn"]
    d = 4
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.random((410, d)))
    y = torch.from_numpy(np.sin(3.0 * x.numpy()).sum(1) + 0.1 * rng.standard_normal(410))
    hp = T(np.concatenate([[1.1], rng.uniform(0.5, 1.5, d) / np.sqrt(d), [0.8], [0.3]]))
    gp = pg.Exact_GP(x[:400].clone(), y[:400].clone(), compose(parts))
    gp.set_params(hp)
    gp.update()
    gp.append(x[400:], y[400:])
    assert torch.equal(gp.x, x) and torch.equal(gp.y, y)
    ref = pg.Exact_GP(x.clone(), y.clone(), compose(parts))
    ref.set_params(hp)
    xp = torch.from_numpy(rng.random((60, d)))
    tol = 1e-9
    mu, var = gp.predict(xp, var="diag")
    mr_, vr_ = ref.predict(xp, var="diag")
    check("mean", mu, mr_, tol)
    check("diag variance", var, vr_, tol)
    check("full covariance", gp.predict(xp, var="full")[1], ref.predict(xp, var="full")[1], tol)
    g, gr = gp.predict_grad(xp), ref.predict_grad(xp)
    check("predict_grad d mean", g[2], gr[2], tol * 10)
    check("predict_grad d var", g[3], gr[3], tol * 10)
    la, ga = pg.MLE(gp).loss_and_grad(hp.numpy().copy())
    lr, grr = pg.MLE(ref).loss_and_grad(hp.numpy().copy())
    check("MLE loss", torch.tensor([float(la)]), torch.tensor([float(lr)]), tol)
    check("MLE grad", torch.from_numpy(ga), torch.from_numpy(grr), tol * 10)
    mu_ref, _ = kr.predict(parts, hp.numpy(), x.numpy(), y.numpy(), xp.numpy())
    np.testing.assert_allclose(N(mu), mu_ref, rtol=0, atol=1e-9)


def test_batched_experts_match_their_loop():
    """4 x 250, d = 4.  Bounds: test_matern_family_gpu.py::test_batched_experts_match_their_loop."""
    rng = np.random.default_rng(22)
    nc, n, m, d = 4, 250, 30, 4
    x = rng.random((nc, n, d))
    y = np.sin(-x.sum(-1)) + 0.1 * rng.standard_normal((nc, n))
    xp = rng.random((nc, m, d))
    parts = ["rq", "wn"]
    hp = np.concatenate([0.8 + 0.4 * rng.random((nc, 1)), 0.5 + rng.random((nc, d)), 0.6 + 2.0 * rng.random((nc, 1)), np.full((nc, 1), 0.1)],
                        axis=1)
    gp = pg.Exact_GP(T(x), T(y), compose(parts))
    gp.set_params(T(hp))
    mu, var = gp.predict(T(xp), var="diag")
    loss, grad = pg.MLE(pg.Exact_GP(T(x), T(y), compose(parts))).loss_and_grad(hp.copy())
    assert grad.shape == (nc, d + 3)
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
        mu_ref, var_ref = kr.predict(parts, hp[c], x[c], y[c], xp[c])
        np.testing.assert_allclose(N(mu1), mu_ref, rtol=0, atol=1e-10)
        np.testing.assert_allclose(N(var1).ravel(), var_ref, rtol=0, atol=1e-10)


def test_grbcm():
    """3 x 120 + 40.  Bounds: test_matern_family_gpu.py::test_grbcm_with_matern32."""
    rng = np.random.default_rng(33)
    nc, nsc, ng, m, d = 3, 120, 40, 25, 3
    xl, xg, xs = rng.random((nc, nsc, d)), rng.random((ng, d)), rng.random((m, d))
    yl, yg = np.sin(-xl.sum(-1)), np.sin(-xg.sum(-1))
    parts = ["rq", "wn"]
    hp_g = np.concatenate([[1.0], 0.6 + rng.random(d), [0.9], [0.1]])
    hp_l = np.concatenate([0.9 + 0.2 * rng.random((nc, 1)), 0.6 + rng.random((nc, d)), 0.6 + rng.random((nc, 1)), np.full((nc, 1), 0.1)], axis=1)
    model = pg.GRBCM(T(xl), T(yl), T(xg), T(yg), compose(parts))
    model.gpg.set_params(T(hp_g))
    model.gpl.set_params(T(hp_l))
    mu, var = model.predict(T(xs), var="diag")
    mu_ref, var_ref = kr.grbcm_predict(parts, hp_g, hp_l, xl, yl, xg, yg, xs)
    np.testing.assert_allclose(N(mu), mu_ref, rtol=0, atol=1e-9)
    np.testing.assert_allclose(N(var).ravel(), var_ref, rtol=1e-9, atol=1e-11)


def test_sk_wrap():
    rng = np.random.default_rng(44)
    n, m, d = 900, 40, 3
    x, y = orc.synth(n, d, seed=44)
    xp = rng.random((m, d))
    parts = ["rq", "wn"]
    hp = np.concatenate([[1.0], 0.5 + rng.random(d), [0.8], [0.1]])
    gp = pg.Exact_GP(T(x[:10]), T(y[:10]), compose(parts))
    gp.set_params(T(hp))
    sk = pg.SK_WRAP(gp).fit(T(x), T(y))
    np.testing.assert_allclose(N(sk.predict(T(xp))), kr.predict(parts, hp, x, y, xp)[0], rtol=0, atol=1e-10)


# --------------------------------------------------------------------------- 6. the SE limit
def test_se_limit_on_the_device(ops, monkeypatch):
    """alpha = 1e4 (a = 1e8): 0 <= K_RQ - K_SE <= K_SE (exp(sq^2 / (2 a)) - 1) around the library's OWN squared-exponential build, widened
    by the build tolerance (2e-14, test 1) on either side, in both body families."""
    rng = np.random.default_rng(5)
    n, d = 200, 5
    x = rng.random((n, d))
    hp_se = np.concatenate([[1.2], 0.4 + 0.8 * rng.random(d), [0.1]])
    hp = np.concatenate([hp_se[:-1], [1.0e4], [0.1]])
    sq = kr.sqdist(hp_se, x)
    for mode in ("2", "0"):
        monkeypatch.setenv("PG_KB_MFMA", mode)
        k, ks = ops.empty(256, 256), ops.empty(256, 256)
        ops.kernel_build(one_spec(["rq", "wn"], d), dev(hp), dev(x), None, k)
        ops.kernel_build(one_spec(["se", "wn"], d), dev(hp_se), dev(x), None, ks)
        diff, k_se = (host(k) - host(ks))[:n, :n], host(ks)[:n, :n] - 0.01 * np.eye(n)
        print("PG_KB_MFMA=%s: K_RQ - K_SE in [%.2e, %.2e], bound's largest entry %.2e" % (mode, diff.min(), diff.max(), (k_se * np.expm1(sq * sq / 2e8)).max()))
        assert (diff >= -2e-14).all()
        assert (diff <= k_se * np.expm1(sq * sq / 2.0e8) + 2e-14).all()


# --------------------------------------------------------------------------- 7. refusals
def test_refusals(ops):
    from pygpr_amd._ops import make_spec

    x = dev(np.random.default_rng(1).random((10, 2)))
    with pytest.raises(RuntimeError, match="unknown kernel kind 7"):
        ops.kernel_build(make_spec([7], [0], []), dev(np.ones(4)), x, None, ops.empty(64, 64))
    with pytest.raises(RuntimeError, match="unknown kernel kind 7"):
        ops.kernel_grad_build(make_spec([7], [0], []), dev(np.ones(4)), x, ops.empty(4, 10, 10))
    cov = compose(["rq", "wn"])
    with pytest.raises(AssertionError):
        cov.kernel(torch.ones(2 + 1 + 1, dtype=torch.float64), x.cpu())          # d + 1 values and the noise: one short of d + 2 + 1
    with pytest.raises(AssertionError):
        pg.MLE(pg.Exact_GP(x.cpu(), torch.zeros(10, dtype=torch.float64), cov)).loss_and_grad(np.ones(2 + 1 + 1))
