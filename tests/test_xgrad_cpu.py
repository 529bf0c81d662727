"""CPU tier of the derivatives in the test points: tests/xgrad_ref.py (the torch restatement whose autograd gradients are the GPU tier's
reference) against central finite differences of tests/kernel_ref.predict, for every kind, Compose, the diagonal variance and the full
covariance; the Matern-1/2 convention at r = 0; and the C ABI / Python surface of the new entry points (no GPU needed)."""
import numpy as np
import pytest
import torch

import kernel_ref as kr
import xgrad_ref as xr

KINDS = ["se", "m52", "m32", "m12"]


def _problem(parts, n=30, m=6, d=3, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.random((n, d))
    y = np.sin(3.0 * x).sum(1) + 0.1 * rng.standard_normal(n)
    xp = rng.random((m, d))
    hp = []
    for p in parts:
        hp += [0.2] if p == "wn" else [rng.uniform(0.8, 1.3)] + list(rng.uniform(0.8, 2.0, d))
    return x, y, xp, np.array(hp)


def _fd(fun, xp, h=1e-6):
    """Central differences of fun(xp) -> array, in every coordinate of every test point: [m, d, *fun.shape]."""
    out = []
    for p in range(xp.shape[0]):
        row = []
        for k in range(xp.shape[1]):
            a, b = xp.copy(), xp.copy()
            a[p, k] += h
            b[p, k] -= h
            row.append((fun(a) - fun(b)) / (2 * h))
        out.append(row)
    return np.array(out)


@pytest.mark.parametrize("parts", [["se", "wn"], ["m52", "wn"], ["m32", "wn"], ["m12", "wn"], ["se", "m12", "wn"]])
def test_reference_diag_against_finite_differences(parts):
    x, y, xp, hp = _problem(parts)
    T = torch.from_numpy
    mean, var, dmean, dvar = xr.predict_grads(parts, T(hp), T(x), T(y), T(xp))
    m0, v0 = kr.predict(parts, hp, x, y, xp, "diag")
    np.testing.assert_allclose(mean.numpy(), m0, rtol=1e-9, atol=1e-10)
    np.testing.assert_allclose(var.numpy(), v0, rtol=1e-7, atol=1e-9)
    fm = _fd(lambda a: kr.predict(parts, hp, x, y, a, "diag")[0], xp)      # [m, d, m]
    fv = _fd(lambda a: kr.predict(parts, hp, x, y, a, "diag")[1], xp)
    idx = np.arange(xp.shape[0])
    np.testing.assert_allclose(dmean.numpy(), fm[idx, :, idx], atol=1e-6 * max(1.0, np.abs(fm).max()))
    np.testing.assert_allclose(dvar.numpy(), fv[idx, :, idx], atol=1e-6 * max(1.0, np.abs(fv).max()))
    # each output depends on its own test point only
    off = fm.copy()
    off[idx, :, idx] = 0.0
    assert np.abs(off).max() < 1e-7


@pytest.mark.parametrize("parts", [["se", "wn"], ["m52", "m32", "wn"], ["m12", "wn"]])
def test_reference_full_vjp_against_finite_differences(parts):
    x, y, xp, hp = _problem(parts, seed=1)
    rng = np.random.default_rng(7)
    g_mu, g_cov = rng.standard_normal(xp.shape[0]), rng.standard_normal((xp.shape[0], xp.shape[0]))
    T = torch.from_numpy
    g = xr.vjp(parts, T(hp), T(x), T(y), T(xp), "full", T(g_mu), T(g_cov)).numpy()

    def loss(a):
        mean, cov = kr.predict(parts, hp, x, y, a, "full")
        return np.array(g_mu @ mean + np.sum(g_cov * cov))

    fd = _fd(loss, xp)
    np.testing.assert_allclose(g, fd, atol=1e-6 * max(1.0, np.abs(fd).max()))


def test_reference_contraction_is_the_weighted_kernel_derivative():
    """contraction() against the closed form dk/dx*_pk = 2 c base l_k^2 D_k of kernel_ref (COEF = 2 c), every kind."""
    rng = np.random.default_rng(3)
    d = 4
    xq, z = rng.random((5, d)), rng.random((9, d))
    u, b = rng.standard_normal(9), rng.standard_normal((5, 9))
    for part in KINDS:
        hpc = np.concatenate([[1.2], rng.uniform(0.5, 2.0, d)])
        sq = kr.sqdist(hpc, z, xq)
        base = kr.radial(part, hpc, sq)[1]
        dk = kr.COEF[part] * base[:, :, None] * hpc[1:] ** 2 * (xq[:, None, :] - z[None, :, :])     # [m, n, d]
        ou, ob = xr.contraction([part], torch.from_numpy(hpc), torch.from_numpy(xq), torch.from_numpy(z), torch.from_numpy(u),
                                torch.from_numpy(b))
        np.testing.assert_allclose(ou.numpy(), np.einsum("i,pik->pk", u, dk), rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(ob.numpy(), np.einsum("pi,pik->pk", b, dk), rtol=1e-12, atol=1e-14)


def test_reference_m12_convention_at_coincident_points():
    """A test point on a training point: Matern-1/2 has a cusp there; the pair contributes 0 (finite gradients), while the smooth kinds
    keep their true derivative (0 for that pair: D = 0)."""
    rng = np.random.default_rng(4)
    x = rng.random((12, 2))
    y = rng.standard_normal(12)
    xp = np.concatenate([x[:2], rng.random((2, 2))])
    for part in KINDS:
        parts = [part, "wn"]
        hp = torch.tensor([1.0, 1.5, 0.7, 0.3], dtype=torch.float64)
        _, _, dmean, dvar = xr.predict_grads(parts, hp, torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(xp))
        assert torch.isfinite(dmean).all() and torch.isfinite(dvar).all(), part
    ou, _ = xr.contraction(["m12"], torch.tensor([1.0, 1.5, 0.7], dtype=torch.float64), torch.from_numpy(x[:1]),
                           torch.from_numpy(x[:1]), u=torch.ones(1, dtype=torch.float64))
    assert float(ou.abs().max()) == 0.0


def test_c_abi_and_python_surface_declare_the_new_entry_points():
    from pygpr_amd import _lib
    from pygpr_amd._ops import HipOps
    from pygpr_amd.gpr import Exact_GP

    syms = _lib.header_symbols()
    for name in ("pg_kernel_xgrad", "pg_kernel_xgrad_worksize"):
        assert name in syms and name in _lib._SIGS
    assert hasattr(HipOps, "kernel_xgrad") and hasattr(HipOps, "kernel_xgrad_batched")
    assert callable(getattr(Exact_GP, "predict_grad", None))
