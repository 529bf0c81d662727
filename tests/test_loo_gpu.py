"""Exact_GP.loo_predict and the LOO loss on the GPU against tests/loo_ref.py (fp64 NumPy: closed forms and eq. 5.13).

Inputs are well conditioned throughout: oracle.synth data, sigma_n = 0.3, sigma and l in [0.5, 1.5].  The LOO gradient carries K^-1
twice, so its error is governed by cond(K)^2; with the default sigma_n = 1e-4 a comparison with a reference shows nothing, and that
regime is only asked to return finite numbers (test_default_noise_is_finite).

Bounds.  Each quantity's error is measured as max |got - ref| / max |ref| over all cases of this file on the MI355X; the bound is that
maximum times 10, rounded up to a power of ten (run-to-run reduction order, other boxes).  Every test prints its figure before it
asserts.  Measured maxima / bounds ("Leave-one-out cross-validation", has the same table):

    fp64   mean 1.6e-13 / 1e-11   var 8.6e-14 / 1e-12   loss 2.4e-14 / 1e-12   gradient 2.4e-14 / 1e-12
    fp32   mean 5.5e-5 / 1e-3     var 3.9e-5 / 1e-3     loss 4.8e-5 / 1e-3     gradient 7.4e-6 / 1e-4

(the fp64 figures sit under the sanity ceilings 1e-9 for mean / var / loss and 1e-7 for the gradient)."""
import functools

import numpy as np
import pytest
import torch

import loo_ref as lr
import pygpr_amd as pg
from oracle import pygpr_oracle as orc

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
BOUND = {
    (F64, "mean"): 1e-11, (F64, "var"): 1e-12, (F64, "loss"): 1e-12, (F64, "grad"): 1e-12,
    (F32, "mean"): 1e-3, (F32, "var"): 1e-3, (F32, "loss"): 1e-3, (F32, "grad"): 1e-4,
}
COV = {"se": pg.Squared_exponential, "m52": pg.Matern52, "m32": pg.Matern32, "m12": pg.Matern12, "wn": pg.White_noise}
KINDS = [["se", "wn"], ["m52", "wn"], ["m32", "wn"], ["m12", "wn"], ["se", "se", "wn"],
         ["se", "m52", "m32", "m12", "se", "m52", "wn"]]      # the last: six stationary children = two passes of PG_MAX_COMP
both = pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])


def hp_of(parts, d, seed=7):
    rng = np.random.default_rng(seed)
    return np.concatenate([[0.3] if p == "wn" else 0.5 + rng.random(d + 1) for p in parts])


@functools.lru_cache(maxsize=None)
def reference(parts, n, d, seed=11):
    """(x, y, hp, mean, var, loss, grad): computed once per case, shared, never modified (read-only arrays)."""
    parts = list(parts)
    x, y = orc.synth(n, d, seed=seed)
    hp = hp_of(parts, d)
    mu, var = lr.loo_predict(parts, hp, x, y)
    loss, grad = lr.loo_loss_and_grad(parts, hp, x, y)
    out = (x, y, hp, mu, var, np.float64(loss), grad)
    for a in out:
        a.setflags(write=False) if isinstance(a, np.ndarray) else None
    return out


def model(parts, x, y, hp, dtype):
    gp = pg.Exact_GP(torch.from_numpy(x.copy()).to(dtype), torch.from_numpy(y.copy()).to(dtype), pg.Compose([COV[p]() for p in parts]))
    gp.set_params(torch.from_numpy(hp.copy()))
    return gp


def err(got, ref, scale=0.0):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), scale, 1e-300))


def judge(dtype, what, got, ref, case, scale=0.0):
    """`scale`: for the mean, max |y| -- mu = y - alpha / c is a difference, and at n = 1 it is exactly 0."""
    e = err(got, ref, scale)
    print("loo_err %s %-4s %-40s measured %.3e bound %.0e" % ("f64" if dtype == F64 else "f32", what, case, e, BOUND[dtype, what]))
    assert np.all(np.isfinite(np.asarray(got, dtype=np.float64))) and e <= BOUND[dtype, what], (what, case, e)


def check_case(parts, n, d, dtype, predict=True):
    x, y, hp, mu_r, var_r, loss_r, grad_r = reference(tuple(parts), n, d)
    case = "%s n=%d d=%d" % ("+".join(parts), n, d)
    gp = model(parts, x, y, hp, dtype)
    if predict:
        mu, var = gp.loo_predict()
        assert mu.shape == (n,) and var.shape == (n,) and mu.dtype == dtype and var.dtype == dtype and mu.device == gp.x.device
        judge(dtype, "mean", mu.numpy(), mu_r, case, scale=float(np.abs(y).max()))
        judge(dtype, "var", var.numpy(), var_r, case)
    loss, grad = pg.LOO(gp).loss_and_grad(hp.copy())
    judge(dtype, "loss", loss, loss_r, case)
    judge(dtype, "grad", grad, grad_r, case)
    return loss, grad


@both
@pytest.mark.parametrize("n", [1, 2, 127, 128, 129, 255, 256, 257, 700])
def test_sizes(n, dtype):
    """One padded block with the 128-block edges inside it, the pad boundary, three 256-blocks with a ragged last chunk."""
    check_case(["se", "wn"], n, 3, dtype)


@both
@pytest.mark.parametrize("d", [1, 3, 17])
@pytest.mark.parametrize("parts", KINDS, ids=["+".join(k) for k in KINDS])
def test_kinds_and_dimensions(parts, d, dtype):
    """Every kind, a two-component sum, a Compose of two passes; d = 17 is above the matrix-pipe contraction's limit."""
    check_case(parts, 300, d, dtype)


def test_fp32_agrees_with_fp64_on_the_device():
    x, y, hp, *_ = reference(("se", "m32", "wn"), 257, 3)
    parts = ["se", "m32", "wn"]
    out = {}
    for dt in (F64, F32):
        gp = model(parts, x, y, hp, dt)
        mu, var = gp.loo_predict()
        loss, grad = pg.LOO(gp).loss_and_grad(hp.copy())
        out[dt] = (mu.numpy(), var.numpy(), loss, grad)
    for what, a, b in zip(("mean", "var", "loss", "grad"), out[F32], out[F64]):
        judge(F32, what, a, b, "fp32 against fp64 HIP, se+m32+wn n=257")


@both
@pytest.mark.parametrize("k", [5, 130])
def test_loo_predict_after_append_equals_fresh_fit(k, dtype):
    """5 points stay inside the padded size, 130 take two blocks and grow it."""
    parts, n, d = ["se", "wn"], 250, 3
    x, y = orc.synth(n + k, d, seed=3)
    hp = hp_of(parts, d)
    gp = model(parts, x[:n], y[:n], hp, dtype)
    gp.update()
    gp.append(torch.from_numpy(x[n:].copy()).to(dtype), torch.from_numpy(y[n:].copy()).to(dtype))
    mu, var = gp.loo_predict()
    fresh = model(parts, x, y, hp, dtype)
    mu_f, var_f = fresh.loo_predict()
    mu_r, var_r = lr.loo_predict(parts, hp, x, y)
    case = "append k=%d" % k
    for got_m, got_v, tag in ((mu, var, " appended"), (mu_f, var_f, " fresh")):
        judge(dtype, "mean", got_m.numpy(), mu_r, case + tag)
        judge(dtype, "var", got_v.numpy(), var_r, case + tag)
    judge(dtype, "mean", mu.numpy(), mu_f.numpy(), case + " appended against fresh")
    judge(dtype, "var", var.numpy(), var_f.numpy(), case + " appended against fresh")


def test_nan_in_y_propagates_and_the_next_call_is_clean():
    """alpha = K^-1 y is NaN everywhere once one y_i is: every mean and the loss are NaN, the variances (c alone) are untouched; the
    call returns, and the same objects are correct again on clean data."""
    parts, n, d = ["se", "wn"], 300, 3
    x, y, hp, mu_r, var_r, loss_r, grad_r = reference(tuple(parts), n, d)
    gp = model(parts, x, y, hp, F64)
    loo = pg.LOO(gp)
    bad = torch.from_numpy(y.copy())
    bad[17] = float("nan")
    gp.y = bad
    mu, var = gp.loo_predict()
    assert bool(torch.isnan(mu).all())
    judge(F64, "var", var.numpy(), var_r, "NaN in y[17]")
    loss, grad = loo.loss_and_grad(hp.copy())
    assert np.isnan(loss) and np.isnan(grad).all()
    gp.y = torch.from_numpy(y.copy())
    mu, var = gp.loo_predict()
    judge(F64, "mean", mu.numpy(), mu_r, "clean again")
    judge(F64, "var", var.numpy(), var_r, "clean again")
    loss, grad = loo.loss_and_grad(hp.copy())
    judge(F64, "loss", loss, loss_r, "clean again")
    judge(F64, "grad", grad, grad_r, "clean again")


def test_cg_on_the_loo_loss_decreases_it(tmp_path, monkeypatch):
    """CG(LOO(model)) from cov.init_params (sigma = l = 1, sigma_n = 1e-4), five iterations.  The points are spread over [0, 20]^2 so
    that K is well conditioned at those parameters (cond 1.2e3).  On unit-cube data it is not: the loss there is 9e7 with a gradient of
    1.6e11 in sigma_n, and scipy's CG line search gives up at iteration 0 even on the fp64 NumPy reference's own loss and gradient."""
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(5)
    x = 20.0 * rng.random((200, 2))
    y = np.sin(-0.3 * x.sum(1)) + 0.3 * rng.standard_normal(200)
    cov = pg.Compose([pg.Squared_exponential(), pg.White_noise()])
    gp = pg.Exact_GP(torch.from_numpy(x), torch.from_numpy(y), cov)
    loo = pg.LOO(gp)
    start = cov.init_params(gp.x).numpy().copy()
    assert np.array_equal(start, gp.params.numpy())
    l0 = float(loo.loss(start))
    opt = pg.CG(loo)
    opt.args.update(maxiter=5, disp=False)
    opt.minimize()
    end = gp.params.numpy().copy()
    l1 = float(loo.loss(end))
    print("loo CG: %.6f -> %.6f in %d iterations" % (l0, l1, opt.res.nit))
    assert np.isfinite(l1) and l1 < l0
    # start (sigma_n = 1e-4) and end (the optimiser's choice) are outside the cases the bounds were measured on: the sanity ceiling
    np.testing.assert_allclose(l0, lr.loo_loss(["se", "wn"], start, x, y), rtol=1e-9)
    np.testing.assert_allclose(l1, lr.loo_loss(["se", "wn"], end, x, y), rtol=1e-9)


def test_loss_then_grad_reuses_the_factor(monkeypatch):
    parts, n, d = ["se", "m52", "wn"], 257, 3
    x, y, hp, _, _, loss_r, grad_r = reference(tuple(parts), n, d)
    gp = model(parts, x, y, hp, F64)
    ops = pg._ops.get_ops()
    calls = []
    real = ops.build_factor
    monkeypatch.setattr(ops, "build_factor", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    loo = pg.LOO(gp)
    loss = loo.loss(hp.copy())
    grad = loo.grad(hp.copy())
    assert len(calls) == 1                                       # the gradient continued from the factor the loss left behind
    judge(F64, "loss", loss, loss_r, "loss then grad")
    judge(F64, "grad", grad, grad_r, "loss then grad")
    both_, = [pg.LOO(gp).loss_and_grad(hp.copy())]
    assert len(calls) == 2 and both_[0] == loss
    judge(F64, "grad", grad, both_[1], "loss then grad against loss_and_grad")


def test_n2048_loss_and_gradient():
    """Eight 256-blocks; the recursive split of the factorisation stays off at this size."""
    check_case(["se", "wn"], 2048, 2, F64, predict=False)


def test_default_noise_is_finite():
    """sigma_n = 1e-4 (the covariance classes' default): cond(K)^2 governs the gradient's error, nothing to compare -- finite only."""
    x, y = orc.synth(300, 3, seed=2)
    hp = np.concatenate([[1.0], np.ones(3), [1e-4]])
    gp = model(["se", "wn"], x, y, hp, F64)
    mu, var = gp.loo_predict()
    loss, grad = pg.LOO(gp).loss_and_grad(hp.copy())
    assert bool(torch.isfinite(mu).all()) and bool(torch.isfinite(var).all()) and np.isfinite(loss) and np.isfinite(grad).all()
