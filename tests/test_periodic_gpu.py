"""GPU tier of the periodic kernel: kind 8, whose block is 2 d + 1 wide and whose distance is not a function of the scaled squared
distance, through every covariance path (C ABI entry points, the dK stack with its period slabs, the fused gradient with its period
entries, Exact_GP / MLE / LOO / predict_grad / append / batched experts / GRBCM / SK_WRAP / sampler) against the direct-difference
restatement of tests/kernel_ref.py.

Shapes: n = 130 against m = 70 (two 64-tiles and a ragged edge: a diagonal tile, an interior tile, padding), d in {1, 3, 8, 17} (17 is past
the matrix-pipe bound of 16 and must take the same route as 8), data in [-3, 3]^d with periods from 0.7 to 7 (rint reduces by up to four
periods).  Tolerances on this data: K 1e-13 and dK 1e-12 absolute, NLML 1e-10 relative, its gradient 1e-8 of its largest entry, predictions
1e-10 absolute; fp32: 4e-6 on K and 3 x 3e-3 on the gradient, what tests/test_rq_gpu.py grants its own kind."""
import numpy as np
import pytest
import torch

import pygpr_amd as pg

import kernel_ref as kr
import loo_ref
from kind_tools import N, T, builds, check, compose, dev, grad_inputs, host, one_spec, ops  # noqa: F401  (ops: the fixture)

pytestmark = pytest.mark.gpu


def synth(n, d, seed, m=0):
    """Points in [-3, 3]^d, a smooth periodic signal plus noise, and m test points."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-3.0, 3.0, (n, d))
    y = np.sin(2.0 * np.pi * x[:, 0] / 1.3) + 0.5 * np.cos(x.sum(1)) + 0.1 * rng.standard_normal(n)
    return (x, y, rng.uniform(-3.0, 3.0, (m, d))) if m else (x, y)


def periods(rng, d):
    """Mixed sizes: 0.7 .. 2.5 (several periods inside the data's extent of 6), every third one 7 (longer than the extent)."""
    p = rng.uniform(0.7, 2.5, d)
    p[2::3] = 7.0
    return p


def block(part, d, rng, sigma=1.1):
    if part == "wn":
        return np.array([0.1])
    tail = periods(rng, d) if part == "per" else ([0.8] if part == "rq" else [])
    return np.concatenate([[sigma], (0.5 + rng.random(d)) / np.sqrt(d), tail])


def hp_of(parts, d, rng):
    return np.concatenate([block(p, d, rng) for p in parts])


# --------------------------------------------------------------------------- 1. entry points, symmetry, diagonal, routing
@pytest.mark.parametrize("d", [1, 3, 8, 17])
def test_entry_points_against_the_restatement(ops, monkeypatch, d):
    """Mirrored, lower-only and cross builds, the dK stack with its period slabs and the fused gradient with its period entries, fp64 /
    fp32.  K is bit-for-bit symmetric and its diagonal exactly sigma^2 + (jitter + sigma_n^2).  Routing, pinned by result: a lone Periodic
    never takes the matrix pipe, so PG_KB_MFMA = 2 / 0 and PG_GRAD_MFMA = 1 / 0 give the same BITS at every d, and d = 17 (past the
    matrix-pipe bound) meets the tolerances d = 8 meets."""
    from pygpr_amd._ops import pad_to

    rng = np.random.default_rng(10 * d + 3)
    n, m = 130, 70
    x, y, xp = synth(n, d, seed=d, m=m)
    parts = ["per", "wn"]
    hp = np.concatenate([[1.2], (0.4 + 0.8 * rng.random(d)) / np.sqrt(d), periods(rng, d), [0.1]])
    spec, npad = one_spec(parts, d), pad_to(n)
    ref = kr.kernel(parts, hp, x) + 1e-7 * np.eye(n)
    ref_x = kr.kernel(parts, hp, x, xp)
    for dtype, tol in ((torch.float64, 1e-13), (torch.float32, 4e-6)):
        out = {}
        for mode in ("2", "0"):
            monkeypatch.setenv("PG_KB_MFMA", mode)
            out[mode] = builds(ops, spec, hp, x, xp, dtype)
        monkeypatch.delenv("PG_KB_MFMA")
        full, low, cross = out["2"]
        print("d=%d %s: K err %.2e, cross err %.2e (bound %.0e)" % (d, dtype, np.abs(full[:n, :n] - ref).max(), np.abs(cross[:m, :n] - ref_x).max(), tol))
        for a, b in zip(out["2"], out["0"]):
            assert np.array_equal(a, b)                                               # no matrix-pipe body: the same kernel either way
        np.testing.assert_allclose(full[:n, :n], ref, atol=tol, rtol=0)
        np.testing.assert_allclose(cross[:m, :n], ref_x, atol=tol, rtol=0)
        assert np.array_equal(full[:n, :n], full[:n, :n].T)                           # exactly symmetric
        pad_ref = np.eye(npad)
        pad_ref[:n, :n] = full[:n, :n]
        assert np.array_equal(full, pad_ref)                                          # identity padding
        assert not cross[m:, :].any() and not cross[:, n:].any()                      # zero padding of a cross build
        tl = np.tril_indices(npad)
        assert np.array_equal(low[tl], full[tl])                                      # lower-only == mirrored on the lower triangle
        if dtype == torch.float64:
            dgv = 1.2 ** 2 + (1e-7 + 0.1 ** 2)
        else:
            dgv = np.float64(np.float32(1.2 ** 2) + np.float32(1e-7 + 0.1 ** 2))
        assert (np.diag(full)[:n] == dgv).all()                                       # exactly sigma^2 + (jitter + sigma_n^2)
    k_ref, dk_ref = kr.kernel_and_grad(parts, hp, x)
    k, dk = compose(parts).kernel_and_grad(T(hp), T(x))
    assert dk.shape == (2 * d + 2, n, n) and all(dk_ref[d + 1 + kk].any() for kk in range(d))
    print("d=%d: dK err %.2e (bound 1e-12), period slabs %.2e" % (d, np.abs(N(dk) - dk_ref).max(), np.abs(N(dk)[d + 1: 2 * d + 1] - dk_ref[d + 1: 2 * d + 1]).max()))
    np.testing.assert_allclose(N(k), k_ref, rtol=0, atol=1e-13)
    np.testing.assert_allclose(N(dk), dk_ref, rtol=0, atol=1e-12)
    _, grad_ref = kr.nlml_and_grad(parts, hp, x, y)
    scale = np.abs(grad_ref).max()
    assert grad_ref[d + 1: 2 * d + 1].all()
    for dtype, tol in ((torch.float64, 1e-8), (torch.float32, 3 * 3e-3)):
        hpd, xd, kinv, alpha_v = grad_inputs(ops, spec, hp, x, y, dtype)
        work = ops.empty(ops.nlml_grad_worksize(n, hp.size))
        got = {}
        for mode in ("1", "0"):
            monkeypatch.setenv("PG_GRAD_MFMA", mode)
            g = ops.zeros(hp.size)
            ops.nlml_grad(spec, hpd, xd, n, kinv, alpha_v, g, work)
            got[mode] = host(g)
        monkeypatch.delenv("PG_GRAD_MFMA")
        print("d=%d %s: gradient err / max %.2e, period entries %.2e (bound %.0e)" % (
            d, dtype, np.abs(got["1"] - grad_ref).max() / scale, np.abs(got["1"] - grad_ref)[d + 1: 2 * d + 1].max() / scale, tol))
        assert np.array_equal(got["1"], got["0"])                                     # the VALU contraction either way
        np.testing.assert_allclose(got["1"], grad_ref, rtol=tol, atol=tol * scale)


# --------------------------------------------------------------------------- 2. offset data
def test_offset_data_against_long_double():
    """Points in [-3, 3]^3 shifted by 1e4, periods around 1, five pairs down to 1e-9 apart.  K and the dK stack against a long-double
    evaluation of the same inputs; the allowance is four times the error the NumPy fp64 direct form shows on these inputs, measured here
    (the reference's own rounding plus a margin for a different but equally good polynomial).  The warped-point form, which takes the
    phase of the coordinate itself, is two to three orders of magnitude outside that allowance."""
    rng = np.random.default_rng(12)
    d = 3
    x = rng.uniform(-3.0, 3.0, (60, d))
    extra = []
    for s, i in zip((0.0, 1e-12, 1e-9, 1e-6, 1e-3), (3, 11, 19, 27, 35)):
        u = rng.standard_normal(d)
        extra.append(x[i] + s * u / np.linalg.norm(u))
    x = np.concatenate([x, np.array(extra)]) + 1.0e4
    n = x.shape[0]
    parts = ["per", "wn"]
    hp = np.concatenate([[1.2], [0.9, 1.3, 0.6], [0.7, 1.0, 1.6], [0.1]])
    k_ld, dk_ld = kr.kernel_and_grad(parts, hp, x, dtype=np.longdouble)
    k_np, dk_np = kr.kernel_and_grad(parts, hp, x)
    err_np = float(np.abs(k_np - k_ld).max())
    derr_np = float(np.abs(dk_np - dk_ld).max())
    k, dk = compose(parts).kernel_and_grad(T(hp), T(x))
    err = float(np.abs(N(k) - k_ld).max())
    derr = float(np.abs(N(dk) - dk_ld).max())
    print("offset data: K err %.2e (NumPy direct form %.2e, allowance %.2e); dK err %.2e (NumPy %.2e, allowance %.2e)" % (
        err, err_np, 4 * err_np, derr, derr_np, 4 * derr_np))
    assert np.isfinite(N(k)).all() and np.isfinite(N(dk)).all()
    assert np.array_equal(N(k), N(k).T) and (np.diag(N(k)) == 1.2 ** 2 + 0.1 ** 2).all()
    assert N(k)[3, 60] == 1.2 ** 2                                                    # an exact duplicate off the diagonal
    assert err <= 4 * err_np
    assert derr <= 4 * derr_np
    xs = x[::-1].copy()
    kx = N(compose(parts).kernel(T(hp), T(x), T(xs)))                                 # a cross build meets the same pairs
    errx = float(np.abs(kx - kr.kernel(parts, hp, x, xs, dtype=np.longdouble)).max())
    print("offset data: cross K err %.2e" % errx)
    assert errx <= 4 * err_np


# --------------------------------------------------------------------------- 3. dK stack, several components
@pytest.mark.parametrize("parts", [["per", "wn"], ["per", "se", "wn"], ["rq", "per", "wn"]], ids=lambda p: "+".join(p))
def test_dk_stack_and_compose(parts):
    """A lone child, one of the general body's cases beside the squared exponential, and a wide block in front of a wide block."""
    rng = np.random.default_rng(len(parts) + 7)
    n, m, d = 130, 70, 3
    x, y, xp = synth(n, d, seed=5, m=m)
    hp = hp_of(parts, d, rng)
    cov = compose(parts)
    np.testing.assert_allclose(N(cov.kernel(T(hp), T(x))), kr.kernel(parts, hp, x), rtol=0, atol=1e-13)
    np.testing.assert_allclose(N(cov.kernel(T(hp), T(x), T(xp))), kr.kernel(parts, hp, x, xp), rtol=0, atol=1e-13)
    k, dk = cov.kernel_and_grad(T(hp), T(x))
    k_ref, dk_ref = kr.kernel_and_grad(parts, hp, x)
    assert dk.shape == (kr.nhp_of(parts, d), n, n)
    assert np.array_equal(N(k), N(k).T)
    np.testing.assert_allclose(N(k), k_ref, rtol=0, atol=1e-13)
    np.testing.assert_allclose(N(dk), dk_ref, rtol=0, atol=1e-12)
    gp = pg.Exact_GP(T(x), T(y), cov)
    gp.set_params(T(hp))
    loss, grad = pg.MLE(gp).loss_and_grad(hp.copy())
    loss_ref, grad_ref = kr.nlml_and_grad(parts, hp, x, y)
    np.testing.assert_allclose(loss, loss_ref, rtol=1e-10)
    np.testing.assert_allclose(grad, grad_ref, rtol=1e-8, atol=1e-8 * np.abs(grad_ref).max())
    mu, var = gp.predict(T(xp), var="diag")                                           # K** reads every child's sigma by its offset
    mu_ref, var_ref = kr.predict(parts, hp, x, y, xp)
    np.testing.assert_allclose(N(mu), mu_ref, rtol=0, atol=1e-10)
    np.testing.assert_allclose(N(var), var_ref, rtol=0, atol=1e-10)


def test_compose_longer_than_one_pass():
    """Six stationary children (PG_MAX_COMP = 4): two passes, a periodic child in each, beside SE, Matern and RQ children and noise."""
    parts = ["per", "se", "m32", "rq", "wn", "per", "m12"]
    rng = np.random.default_rng(3)
    n, m, d = 130, 70, 3
    x, y, xp = synth(n, d, seed=6, m=m)
    hp = np.concatenate([block(p, d, rng, sigma=0.7) for p in parts])
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
def test_nan_coordinate_and_nan_period(ops):
    """A NaN coordinate reaches its point's row and column only.  A NaN period reaches every pair of real points (the phase of every
    difference, D = 0 included) and nothing else: the padding stays the identity."""
    rng = np.random.default_rng(4)
    n, d = 70, 3
    x = rng.uniform(-3.0, 3.0, (n, d))
    xn = x.copy()
    xn[23, 1] = np.nan
    hp = np.array([1.0, 0.7, 0.8, 0.9, 0.8, 1.3, 2.1, 0.1])
    hp_nan = hp.copy()
    hp_nan[d + 2] = np.nan
    pad = np.eye(128)[n:, :]
    for dt in (torch.float64, torch.float32):
        k = ops.empty(128, 128, dtype=dt)
        ops.kernel_build(one_spec(["per", "wn"], d), dev(hp), dev(xn, dt), None, k, jitter=1e-7)
        got = host(k)
        assert np.isnan(got[23, :n]).all() and np.isnan(got[:n, 23]).all()
        assert np.isfinite(np.delete(np.delete(got[:n, :n], 23, 0), 23, 1)).all()
        assert np.array_equal(got[n:, :], pad) and np.array_equal(got[:, n:], pad.T)
        ops.kernel_build(one_spec(["per", "wn"], d), dev(hp_nan), dev(x, dt), None, k, jitter=1e-7)
        got = host(k)
        assert np.isnan(got[:n, :n]).all()
        assert np.array_equal(got[n:, :], pad) and np.array_equal(got[:, n:], pad.T)
    # in a sum the other child's values do not rescue the pair, and do not suffer elsewhere
    hp2 = np.concatenate([hp[:-1], [0.9, 0.5, 0.6, 0.7], [0.1]])
    k = ops.empty(128, 128)
    ops.kernel_build(one_spec(["per", "se", "wn"], d), dev(hp2), dev(xn), None, k, jitter=1e-7)
    got = host(k)
    assert np.isnan(got[23, :n]).all() and np.isnan(got[:n, 23]).all()
    assert np.isfinite(np.delete(np.delete(got[:n, :n], 23, 0), 23, 1)).all()
    dk = N(compose(["per", "wn"]).kernel_and_grad(T(hp), T(xn))[1])
    assert np.isnan(dk[: 2 * d + 1, 23, :]).all() and np.isnan(dk[: 2 * d + 1, :, 23]).all()
    assert np.isfinite(np.delete(np.delete(dk, 23, 1), 23, 2)).all()


# --------------------------------------------------------------------------- 5. public surface
@pytest.mark.parametrize("n,d", [(1000, 5), (2049, 8)])
def test_exact_gp_and_mle(n, d):
    """n = 2049: an odd tile count, padded to 2304."""
    rng = np.random.default_rng(n)
    x, y, xp = synth(n, d, seed=9, m=60)
    parts = ["per", "wn"]
    hp = hp_of(parts, d, rng)
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
    """LOO(model).loss_and_grad against loo_ref's closed forms (R&W 5.10 - 5.13) on kernel_ref's kernel and slabs."""
    parts = ["per", "wn"]
    n, d = 130, 3
    x, y = synth(n, d, seed=21)
    hp = np.concatenate([[1.1], np.linspace(0.5, 0.9, d), [0.9, 1.7, 7.0], [0.3]])
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


@pytest.mark.parametrize("parts,d", [(["per", "wn"], 3), (["per", "wn"], 17), (["per", "m32", "wn"], 8)], ids=lambda p: "+".join(p) if isinstance(p, list) else str(p))
def test_predict_grad_and_autograd(parts, d):
    """predict_grad and autograd in xp against kernel_ref's x*-derivatives: 1e-9 relative to the largest entry, as tests/test_xgrad_gpu.py
    and tests/test_rq_gpu.py ask of the same quantities.  d = 17 takes the kernel that walks the coordinates in passes of sixteen."""
    rng = np.random.default_rng(1)
    n, m = 130, 70
    x, y, xp = synth(n, d, seed=1, m=m)
    hp = np.concatenate([[0.3] if p == "wn" else block(p, d, rng) for p in parts])
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


def test_batched_experts_match_their_loop():
    """3 x 130, d = 3: predictions, NLML and its gradient, predict_grad -- each expert against its own single model and the restatement."""
    rng = np.random.default_rng(22)
    nc, n, m, d = 3, 130, 33, 3
    parts = ["per", "wn"]
    x = rng.uniform(-3.0, 3.0, (nc, n, d))
    y = np.sin(2.0 * np.pi * x[..., 0] / 1.3) + 0.1 * rng.standard_normal((nc, n))
    xp = rng.uniform(-3.0, 3.0, (nc, m, d))
    hp = np.stack([hp_of(parts, d, rng) for _ in range(nc)])
    gp = pg.Exact_GP(T(x), T(y), compose(parts))
    gp.set_params(T(hp))
    mu, var = gp.predict(T(xp), var="diag")
    _, _, dmean, dvar = gp.predict_grad(T(xp), var="diag")
    loss, grad = pg.MLE(pg.Exact_GP(T(x), T(y), compose(parts))).loss_and_grad(hp.copy())
    assert grad.shape == (nc, 2 * d + 2) and dmean.shape == (nc, m, d)
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
        rdm, rdv = kr.predict_grads(parts, hp[c], x[c], y[c], xp[c])
        check("predict_grad batched expert %d dmean" % c, dmean[c], T(rdm), 1e-9)
        check("predict_grad batched expert %d dvar" % c, dvar[c], T(rdv), 1e-9)


def test_append_equals_fresh_fit():
    """append of 10 points against a fresh fit: 1e-9 (ten times that on derivatives), tests/test_append_gpu.py::compare."""
    parts = ["per", "wn"]
    d = 3
    rng = np.random.default_rng(0)
    xa, ya, xpa = synth(140, d, seed=2, m=60)
    x, y, xp = T(xa), T(ya), T(xpa)
    hp = T(np.concatenate([[1.1], rng.uniform(0.5, 1.5, d) / np.sqrt(d), periods(rng, d), [0.3]]))
    gp = pg.Exact_GP(x[:130].clone(), y[:130].clone(), compose(parts))
    gp.set_params(hp)
    gp.update()
    gp.append(x[130:], y[130:])
    assert torch.equal(gp.x, x) and torch.equal(gp.y, y)
    ref = pg.Exact_GP(x.clone(), y.clone(), compose(parts))
    ref.set_params(hp)
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
    mu_ref, _ = kr.predict(parts, hp.numpy(), xa, ya, xpa)
    np.testing.assert_allclose(N(mu), mu_ref, rtol=0, atol=1e-9)


def test_grbcm():
    """3 x 120 + 40.  Bounds: tests/test_rq_gpu.py::test_grbcm."""
    rng = np.random.default_rng(33)
    nc, nsc, ng, m, d = 3, 120, 40, 25, 3
    xl, xg, xs = rng.uniform(-3, 3, (nc, nsc, d)), rng.uniform(-3, 3, (ng, d)), rng.uniform(-3, 3, (m, d))
    yl, yg = np.sin(2.0 * np.pi * xl[..., 0] / 1.3), np.sin(2.0 * np.pi * xg[..., 0] / 1.3)
    parts = ["per", "wn"]
    hp_g = hp_of(parts, d, rng)
    hp_l = np.stack([hp_of(parts, d, rng) for _ in range(nc)])
    model = pg.GRBCM(T(xl), T(yl), T(xg), T(yg), compose(parts))
    model.gpg.set_params(T(hp_g))
    model.gpl.set_params(T(hp_l))
    mu, var = model.predict(T(xs), var="diag")
    mu_ref, var_ref = kr.grbcm_predict(parts, hp_g, hp_l, xl, yl, xg, yg, xs)
    np.testing.assert_allclose(N(mu), mu_ref, rtol=0, atol=1e-9)
    np.testing.assert_allclose(N(var).ravel(), var_ref, rtol=1e-9, atol=1e-11)


def test_sk_wrap():
    rng = np.random.default_rng(44)
    n, d = 300, 3
    x, y, xp = synth(n, d, seed=44, m=40)
    parts = ["per", "wn"]
    hp = hp_of(parts, d, rng)
    gp = pg.Exact_GP(T(x[:10]), T(y[:10]), compose(parts))
    gp.set_params(T(hp))
    sk = pg.SK_WRAP(gp).fit(T(x), T(y))
    np.testing.assert_allclose(N(sk.predict(T(xp))), kr.predict(parts, hp, x, y, xp)[0], rtol=0, atol=1e-10)


def test_sampler_mean_and_factor():
    """The sampler's mean is predict's, bit for bit; its factor reproduces predict's full covariance plus the jitter to the Cholesky
    backward-error bound tests/test_sample_gpu.py uses (1e-12 of the largest entry)."""
    rng = np.random.default_rng(55)
    n, m, d = 130, 70, 3
    x, y, xp = synth(n, d, seed=55, m=m)
    parts = ["per", "se", "wn"]
    hp = hp_of(parts, d, rng)
    gp = pg.Exact_GP(T(x), T(y), compose(parts))
    gp.set_params(T(hp))
    smp = gp.sampler(T(xp), noise=True, jitter=1e-7)
    pm, pc = gp.predict(T(xp), var="full")
    assert torch.equal(smp.mean, pm)
    L, c = smp.chol.double().numpy(), N(pc)
    err = np.abs(L @ L.T - (c + 1e-7 * np.eye(m))).max() / np.abs(c).max()
    print("sampler factor err %.2e (bound 1e-12)" % err)
    assert err <= 1e-12
    mu_ref, cov_ref = kr.predict(parts, hp, x, y, xp, var="full")
    np.testing.assert_allclose(N(pm), mu_ref, rtol=0, atol=1e-10)
    np.testing.assert_allclose(c, cov_ref, rtol=0, atol=1e-10)


# --------------------------------------------------------------------------- 6. refusals
def test_refusals(ops):
    """The periodic kind is a stationary kind of its own, never the stand-in PG_KIND_SQDIST is: where the scaled distance itself is refused (every
    entry point but pg_kernel_build) it is served, `Periodic.distance` -- the squared exponential's Euclidean distance, which goes
    through PG_KIND_SQDIST -- refuses, and the unassigned kinds stay refused."""
    from pygpr_amd import _lib
    from pygpr_amd._ops import make_spec

    d = 2
    x = dev(np.random.default_rng(1).random((10, d)))
    hp = dev(np.array([1.0, 0.8, 0.9, 1.3, 0.7]))
    ops.kernel_grad_build(make_spec([_lib.PG_KIND_PERIODIC], [0], []), hp, x, ops.empty(5, 10, 10))
    with pytest.raises(RuntimeError, match="unknown kernel kind 2"):
        ops.kernel_grad_build(make_spec([_lib.PG_KIND_SQDIST], [0], []), hp, x, ops.empty(5, 10, 10))
    with pytest.raises(TypeError):
        pg.Periodic().distance(x.cpu())
    for kind in (5, 7, 9):
        with pytest.raises(RuntimeError, match="unknown kernel kind %d" % kind):
            ops.kernel_build(make_spec([kind], [0], []), hp, x, None, ops.empty(64, 64))
        with pytest.raises(RuntimeError, match="unknown kernel kind %d" % kind):
            ops.kernel_grad_build(make_spec([kind], [0], []), hp, x, ops.empty(5, 10, 10))
    cov = compose(["per", "wn"])
    with pytest.raises(AssertionError):
        cov.kernel(torch.ones(d + 2 + 1, dtype=torch.float64), x.cpu())              # the rational quadratic's width: d - 1 short of 2 d + 1
    with pytest.raises(AssertionError):
        cov.kernel(torch.ones(2 * d + 1, dtype=torch.float64), x.cpu())              # the noise is missing
    with pytest.raises(AssertionError):
        pg.MLE(pg.Exact_GP(x.cpu(), torch.zeros(10, dtype=torch.float64), cov)).loss_and_grad(np.ones(d + 1 + 1))
