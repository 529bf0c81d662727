"""Sparse_GP on the host: the restatement (tests/sparse_ref.py) checked against itself -- two forms of the loss, the closed-form gradient
against central differences, the bound against the exact NLML -- and the Python class logic of pygpr_amd/sparse.py on a test double
of the device ops.  No GPU."""
import ast
import ctypes
import os

import numpy as np
import pytest
import torch

import kernel_ref as kr
import pygpr_amd as pg
import sparse_ref as sr
from oracle_ops import KindOracleOps, _np
from pygpr_amd import _lib, _ops
from pygpr_amd import sparse as sparse_mod

MODELS = {
    "se+wn": (["se", "wn"], lambda: pg.Compose([pg.Squared_exponential(), pg.White_noise()])),
    "m32+rq+wn": (["m32", "rq", "wn"], lambda: pg.Compose([pg.Matern32(), pg.Rational_quadratic(), pg.White_noise()])),
    "se*per+wn": ([("se", "per"), "wn"], lambda: pg.Compose([pg.Product([pg.Squared_exponential(), pg.Periodic()]), pg.White_noise()])),
}


problem, tol_of = sr.problem, sr.tol_of


# ------------------------------------------------------------------------------------------- the restatement against itself
@pytest.mark.parametrize("name", sorted(MODELS))
def test_dense_and_woodbury_forms_agree(name):
    terms = MODELS[name][0]
    hp, x, y, z = problem(terms)
    err = sr.self_error(terms, hp, x, y, z)
    print("self error", name, err, "cond(Kuu)", np.linalg.cond(sr.kuu_kuf(terms, hp, x, z)[0]))
    assert err < 1e-10
    mu_w, cov_w = sr.predict(terms, hp, x, y, z, x[:50] + 0.01, var="full")
    mu_d, cov_d = sr.predict_dense(terms, hp, x, y, z, x[:50] + 0.01)
    assert np.abs(mu_w - mu_d).max() < 1e-9 * np.abs(mu_d).max() and np.abs(cov_w - cov_d).max() < 1e-9 * np.abs(cov_d).max()
    assert np.allclose(np.diag(cov_w), sr.predict(terms, hp, x, y, z, x[:50] + 0.01, var="diag")[1], rtol=0, atol=1e-14)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_gradient_against_central_differences(name):
    terms = MODELS[name][0]
    hp, x, y, z = problem(terms, n=120, m=20)
    _, g = sr.loss_and_grad(terms, hp, x, y, z)
    fd = np.zeros_like(g)
    for i in range(hp.size):
        h = 1e-5 * max(1.0, abs(hp[i]))
        up, dn = hp.copy(), hp.copy()
        up[i] += h
        dn[i] -= h
        fd[i] = (sr.loss_dense(terms, up, x, y, z) - sr.loss_dense(terms, dn, x, y, z)) / (2 * h)
    # central differences of a loss known to 1e-12 relative at step 1e-5: 1e-12 |L| / 1e-5 of rounding, h^2 of truncation
    assert np.abs(g - fd).max() <= 1e-6 * np.abs(fd).max()


def test_cross_grad_terms_reduce_to_grad_terms_on_one_point_set():
    terms = [("se", "per"), "m12", "rq", "wn"]
    rng = np.random.default_rng(0)
    x = rng.random((23, 2))
    hp = 0.6 + rng.random(kr.nhp_of(terms, 2))
    sym = {i: s for i, s in kr.grad_terms(terms, hp, x)}
    cross = {i: s for i, s in sr.cross_grad_terms(terms, hp, x, x)}
    assert sorted(cross) == sorted(i for i in sym if i != hp.size - 1)
    for i, s in cross.items():
        np.testing.assert_allclose(s, sym[i], rtol=0, atol=1e-15)


def test_bound_lies_above_the_exact_nlml_and_tightens_with_m():
    terms = MODELS["se+wn"][0]
    hp, x, y, z = problem(terms, n=300, m=60)
    exact = kr.nlml(terms, hp, x, y)
    gaps = [sr.loss_woodbury(terms, hp, x, y, z[:m]) - exact for m in (10, 20, 40, 60)]       # nested inducing sets
    print("gaps", gaps)
    assert all(g > 0 for g in gaps) and all(b < a for a, b in zip(gaps, gaps[1:]))
    # every point an inducing point: Q = Kff up to the jitter on Kuu, the bound is the exact NLML
    assert abs(sr.loss_woodbury(terms, hp, x[:80], y[:80], x[:80]) - kr.nlml(terms, hp, x[:80], y[:80])) < 1e-3


# ------------------------------------------------------------------------------------------- the header
def test_sparse_header_parses_and_binds():
    text = open(_lib.HEADER_SPARSE).read()
    protos = _lib.parse_prototypes(text)
    assert sorted(protos) == ["pg_kernel_cross_grad", "pg_kernel_cross_grad_worksize"]
    assert _lib._SIGS_SPARSE == _lib.signatures(protos)
    others = set(_lib.header_symbols()) | set(_lib._SIGS_LOO) | set(_lib._SIGS_SAMPLE)
    assert not set(protos) & others and "#define PG_KIND" not in text
    vp, i, lg = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    assert _lib._SIGS_SPARSE["pg_kernel_cross_grad_worksize"] == (lg, [i, i, i])
    assert _lib._SIGS_SPARSE["pg_kernel_cross_grad"] == (i, [vp, i, ctypes.POINTER(_lib.CovSpec), vp, vp, lg, i, vp, lg, i, i, vp, lg, vp, i, vp, vp])
    lib = _lib.load(check_symbols=True)
    for name, (res, args) in _lib._SIGS_SPARSE.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    # host arithmetic: tile rows x strips of four column tiles x nhp
    assert lib.pg_kernel_cross_grad_worksize(70, 150, 5) == 2 * 1 * 5 and lib.pg_kernel_cross_grad_worksize(64, 64 * 5, 3) == 1 * 2 * 3
    assert lib.pg_kernel_cross_grad_worksize(0, 10, 3) == 0 and lib.pg_kernel_cross_grad_worksize(-1, 10, 3) == -1
    assert lib.pg_kernel_cross_grad(None, 0, None, None, None, 1, 1, None, 1, 1, 1, None, 1, None, 0, None, None) != 0      # null handle: refused
    import inspect

    assert "HEADER_SPARSE" in inspect.getsource(_lib.build_id)


def test_every_sparse_export_has_a_framed_case():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_sparse_gpu.py")
    used = {n.attr for n in ast.walk(ast.parse(open(path).read())) if isinstance(n, ast.Attribute) and n.attr.startswith("pg_")}
    assert sorted(set(_lib._SIGS_SPARSE) - used) == []


# ------------------------------------------------------------------------------------------- host logic on a test double
class SparseOracleOps(KindOracleOps):
    """KindOracleOps plus the raw product (NT / NN, lower tiles for tri) and the rectangular contraction, in NumPy."""

    def __init__(self):
        self.cross_calls = []

    def gemm_raw(self, variant, m, n, k, alpha, a, b, beta, c, tri=0, klo=0, khi=0):
        assert variant in (_lib.GEMM_NT, _lib.GEMM_NT_64, _lib.GEMM_NN) and klo == khi == 0 and m % 128 == n % 128 == 0 and k % 16 == 0
        tile = 64 if variant == _lib.GEMM_NT_64 else 128
        aa, bb = _np(a)[:m, :k], (_np(b)[:k, :n] if variant == _lib.GEMM_NN else _np(b)[:n, :k].T)
        out = alpha * (aa @ bb) + (beta * _np(c)[:m, :n] if beta != 0 else 0.0)
        if tri:                    # tiles on and below the diagonal; strictly above it inside the diagonal tiles: unspecified
            ti, tj = np.arange(m)[:, None] // tile, np.arange(n)[None, :] // tile
            keep = _np(c)[:m, :n].copy()
            out = np.where(tj <= ti, out, keep)
            out[(ti == tj) & (np.arange(n)[None, :] > np.arange(m)[:, None])] = np.nan
        _np(c)[:m, :n] = out

    def kernel_cross_grad_worksize(self, m, n, nhp):
        return ((m + 63) // 64) * ((((n + 63) // 64) + 3) // 4) * nhp

    def kernel_cross_grad(self, spec, hp, z, x, w, grad, accumulate=False, work=None):
        (sp,) = spec if isinstance(spec, (list, tuple)) else [spec]
        assert work is not None and work.numel() >= self.kernel_cross_grad_worksize(z.shape[0], x.shape[0], grad.numel())
        model, h, index = self._model(sp, _np(hp), z.shape[1])
        m, n = z.shape[0], x.shape[0]
        g = sr.cross_grad(model, h, _np(z), _np(x), _np(w)[:m, :n])
        self.cross_calls.append((m, n, bool(accumulate)))
        for j, p in enumerate(index[: len(index) - sp.nnoise]):      # (the noise entries sit behind the blocks and are nobody's here)
            grad[p] = (grad[p] if accumulate else 0.0) + float(g[j])
        return grad


@pytest.fixture
def sparse_ops(monkeypatch, tmp_path):
    ops = SparseOracleOps()
    monkeypatch.setattr(_ops, "_OPS", ops)
    monkeypatch.chdir(tmp_path)
    return ops


def model_of(name, n=300, m=40, **kw):
    terms, make = MODELS[name]
    hp, x, y, z = problem(terms, n=n, m=m, **kw)
    gp = pg.Sparse_GP(torch.from_numpy(x), torch.from_numpy(y), make(), torch.from_numpy(z))
    gp.set_params(torch.from_numpy(hp))
    return terms, hp, x, y, z, gp


@pytest.mark.parametrize("name", sorted(MODELS))
@pytest.mark.parametrize("chunk", [128, 32768])
def test_class_agrees_with_the_restatement(sparse_ops, monkeypatch, name, chunk):
    monkeypatch.setattr(sparse_mod, "_SPARSE_CHUNK", chunk)
    terms, hp, x, y, z, gp = model_of(name)
    tol = tol_of(sr.self_error(terms, hp, x, y, z))
    l_ref, g_ref = sr.loss_and_grad(terms, hp, x, y, z)
    vfe = pg.VFE(gp)
    loss, grad = vfe.loss_and_grad(hp.copy())
    assert abs(loss - l_ref) <= tol * abs(l_ref) and np.abs(grad - g_ref).max() <= tol * np.abs(g_ref).max()
    assert abs(pg.VFE(gp).loss(hp.copy()) - l_ref) <= tol * abs(l_ref)
    nch = -(-x.shape[0] // chunk)
    want = [(40, 40, False)] + [(40, min(chunk, 300 - s), True) for s in range(0, 300, chunk)]
    assert sparse_ops.cross_calls == want and len(want) == 1 + nch
    xp = np.random.default_rng(1).random((37, 3))
    mu_ref, cov_ref = sr.predict(terms, hp, x, y, z, xp, var="full")
    mu, var = gp.predict(torch.from_numpy(xp), var="diag")
    assert np.abs(mu.numpy() - mu_ref).max() <= tol * np.abs(mu_ref).max()
    assert np.abs(var.numpy() - np.diag(cov_ref)).max() <= tol * np.abs(cov_ref).max()
    mu2, cov = gp.predict(torch.from_numpy(xp), var="full")
    assert np.abs(cov.numpy() - cov_ref).max() <= tol * np.abs(cov_ref).max() and torch.equal(cov, cov.T)
    assert np.abs(mu2.numpy() - mu_ref).max() <= tol * np.abs(mu_ref).max()
    assert gp.predict(torch.from_numpy(xp), var="none")[1] is NotImplemented


def test_predict_chunks_the_test_points(sparse_ops, monkeypatch):
    terms, hp, x, y, z, gp = model_of("se+wn")
    xp = torch.from_numpy(np.random.default_rng(2).random((70, 3)))
    whole = gp.predict(xp, var="diag")
    monkeypatch.setattr(sparse_mod, "_CHUNK", 32)
    parts = gp.predict(xp, var="diag")
    assert torch.allclose(whole[0], parts[0], rtol=0, atol=1e-13) and torch.allclose(whole[1], parts[1], rtol=0, atol=1e-13)


def test_state_and_memo_follow_the_data(sparse_ops):
    terms, hp, x, y, z, gp = model_of("se+wn")
    assert gp.need_upd
    gp.update()
    assert not gp.need_upd
    vfe = pg.VFE(gp)
    l0 = float(vfe.loss(hp.copy()))
    gp.z = torch.from_numpy(z[:30].copy())                     # assigning z marks the model dirty and drops the loss's memo
    assert gp.need_upd
    l1 = float(vfe.loss(hp.copy()))
    assert abs(l1 - sr.loss_woodbury(terms, hp, x, y, z[:30])) <= 1e-9 * abs(l1) and l1 > l0
    gp.update()
    gp.y = torch.from_numpy(y + 1.0)
    assert gp.need_upd
    gp.update()
    gp.set_params(torch.from_numpy(hp * 1.1))
    assert gp.need_upd
    assert isinstance(vfe, pg.Loss) and "Sparse_GP" in pg.__all__ and "VFE" in pg.__all__


def test_training_lowers_the_bound(sparse_ops):
    terms, hp, x, y, z, gp = model_of("se+wn", n=150, m=20)
    gp.set_params(gp.cov.init_params(gp.x))
    vfe = pg.VFE(gp)
    start = float(vfe.loss(gp.params.numpy().copy()))
    opt = pg.CG(vfe)
    opt.args.update(maxiter=8, disp=False)
    opt.minimize()
    assert float(vfe.loss(gp.params.numpy().copy())) < start - 1.0


def test_failed_factorisation_raises_and_leaves_the_model_dirty(sparse_ops):
    terms, hp, x, y, z, gp = model_of("se+wn")
    zbad = z.copy()
    zbad[3, 1] = np.nan
    gp.z = torch.from_numpy(zbad)
    with pytest.raises(torch.linalg.LinAlgError):
        gp.update()
    assert gp.need_upd
    with pytest.raises(torch.linalg.LinAlgError):
        pg.VFE(gp).loss(hp.copy())
    gp.z = torch.from_numpy(z)
    gp.update()
    assert not gp.need_upd


def test_refusals(sparse_ops):
    rng = np.random.default_rng(0)
    x, y, z = torch.from_numpy(rng.random((50, 2))), torch.from_numpy(rng.random(50)), torch.from_numpy(rng.random((8, 2)))
    se_wn = lambda: pg.Compose([pg.Squared_exponential(), pg.White_noise()])      # noqa: E731
    with pytest.raises(ValueError, match="White_noise"):
        pg.Sparse_GP(x, y, pg.Squared_exponential(), z)
    long_sum = pg.Compose([pg.Squared_exponential() for _ in range(_lib.PG_MAX_COMP + 1)] + [pg.White_noise()])
    with pytest.raises(NotImplementedError, match="pass"):
        pg.Sparse_GP(x, y, long_sum, z)
    with pytest.raises(NotImplementedError, match="batched"):
        pg.Sparse_GP(x[None], y[None], se_wn(), z)
    with pytest.raises(TypeError, match="float64"):
        pg.Sparse_GP(x.float(), y.float(), se_wn(), z.float())
    with pytest.raises(TypeError, match="float64"):
        pg.Sparse_GP(x, y, se_wn(), z.float())
    gp = pg.Sparse_GP(x, y, se_wn(), z)
    gp.set_params(torch.stack([gp.params, gp.params]))
    with pytest.raises(NotImplementedError, match="batched"):
        gp.update()
    with pytest.raises(NotImplementedError, match="batched"):
        pg.VFE(gp).loss(np.stack([gp.params[0].numpy()] * 2))
    gp = pg.Sparse_GP(x, y, se_wn(), z)
    for call in (lambda: gp.append(x[:2], y[:2]), gp.loo_predict, lambda: gp.sampler(x[:3]), lambda: gp.sample(x[:3])):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(NotImplementedError, match="differentiable"):
        gp.predict(x[:3].clone().requires_grad_(True), var="diag")
    with pytest.raises(TypeError):
        pg.VFE(pg.Exact_GP(x, y, se_wn()))
