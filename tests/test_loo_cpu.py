"""Leave-one-out cross-validation without a GPU: the reference's own mathematics (tests/loo_ref.py), the second public header and its
bindings, the framed-coverage rule for that header, and the host logic of LOO / Exact_GP.loo_predict on a NumPy test double."""
import ast
import ctypes
import os

import numpy as np
import pytest
import torch

import loo_ref as lr
import pygpr_amd as pg
from oracle_ops import OracleOps, _np
from pygpr_amd import _lib, _ops

PARTS = ["se", "m32", "wn"]


def _problem(n=25, d=3, seed=0, parts=PARTS):
    rng = np.random.default_rng(seed)
    x = rng.random((n, d))
    y = np.sin(3 * x.sum(1)) + 0.3 * rng.standard_normal(n)
    hp = np.concatenate([np.concatenate([[0.5 + rng.random()], 0.5 + rng.random(d)]) if p != "wn" else [0.3] for p in parts])
    return x, y, hp


# ------------------------------------------------------------------------------------------- the reference itself
def test_closed_forms_match_n_refits():
    x, y, hp = _problem()
    mu, var = lr.loo_predict(PARTS, hp, x, y)
    bm, bv = lr.loo_bruteforce(PARTS, hp, x, y)
    np.testing.assert_allclose(mu, bm, rtol=0, atol=1e-12)
    np.testing.assert_allclose(var, bv, rtol=0, atol=1e-12)
    np.testing.assert_allclose(lr.loo_loss(PARTS, hp, x, y), lr.loss_from(bm, bv, y), rtol=0, atol=1e-12)
    np.testing.assert_allclose(lr.loo_loss_and_grad(PARTS, hp, x, y)[0], lr.loss_from(bm, bv, y), rtol=0, atol=1e-12)


def test_gradient_matches_central_differences():
    x, y, hp = _problem()
    _, g = lr.loo_loss_and_grad(PARTS, hp, x, y)
    h = 1e-6
    fd = np.array([(lr.loo_loss(PARTS, hp + h * e, x, y) - lr.loo_loss(PARTS, hp - h * e, x, y)) / (2 * h) for e in np.eye(hp.size)])
    np.testing.assert_allclose(g, fd, rtol=1e-5, atol=1e-5 * np.abs(fd).max())


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_weighted_matrix_form_equals_eq_5_13(seed):
    """1/2 sum G o dK with G = 2 K^-1 W K^-1 - b alpha^T - alpha b^T (what the library contracts, as S S^T + q q^T - p p^T) against
    eq. 5.13 evaluated per hyper-parameter, on random inputs."""
    x, y, hp = _problem(n=30, d=2, seed=seed, parts=["m52", "se", "wn"])
    g513 = lr.loo_loss_and_grad(["m52", "se", "wn"], hp, x, y)[1]
    gmat = lr.grad_gmatrix(["m52", "se", "wn"], hp, x, y)
    np.testing.assert_allclose(gmat, g513, rtol=0, atol=1e-10 * max(1.0, np.abs(g513).max()))
    # ... and the split the kernels use: S S^T + q q^T - p p^T is that G
    kinv, alpha, c = lr._solve(["m52", "se", "wn"], hp, x, y)
    w = 0.5 / c + 0.5 * alpha ** 2 / c ** 2
    b = kinv @ (alpha / c)
    s = kinv * np.sqrt(2 * w)
    p, q = (alpha + b) / np.sqrt(2), (alpha - b) / np.sqrt(2)
    np.testing.assert_allclose(s @ s.T + np.outer(q, q) - np.outer(p, p), lr.gmatrix(kinv, alpha), rtol=0, atol=1e-10 * np.abs(kinv).max() ** 2)


# ------------------------------------------------------------------------------------------- the second header
def test_loo_header_parses_and_binds():
    text = open(_lib.HEADER_LOO).read()
    protos = _lib.parse_prototypes(text)
    assert sorted(protos) == ["pg_loo_fold", "pg_loo_terms", "pg_loo_terms_worksize", "pg_loo_weights"]
    assert _lib._SIGS_LOO == _lib.signatures(protos)             # the closed vocabulary: signatures() raises on any other type
    assert not set(protos) & set(_lib.header_symbols()) and not set(_lib._SIGS_LOO) & set(_lib._SIGS)
    assert "#define PG_KIND" not in text
    vp, i, lg = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    assert _lib._SIGS_LOO["pg_loo_terms_worksize"] == (lg, [i])
    assert _lib._SIGS_LOO["pg_loo_terms"] == (i, [vp, i, i, i, vp, lg] + [vp] * 8)
    lib = _lib.load(check_symbols=True)
    for name, (res, args) in _lib._SIGS_LOO.items():
        fn = getattr(lib, name)                                  # a symbol of the built library ...
        assert isinstance(fn, ctypes._CFuncPtr) and fn.restype is res and list(fn.argtypes) == args
    # host arithmetic, no device: 256-row chunks of partial sums + the finishing launch's words; a bad size is refused
    assert lib.pg_loo_terms_worksize(512) == 2 * 512 + 2 + 2 and lib.pg_loo_terms_worksize(100) == -1
    assert lib.pg_loo_terms(None, 0, 1, 256, None, 256, None, None, None, None, None, None, None, None) != 0      # null handle: refused
    assert HEADER_IN_BUILD_ID()


def HEADER_IN_BUILD_ID():
    import inspect

    return "HEADER_LOO" in inspect.getsource(_lib.build_id)


NO_BUFFER = {"pg_loo_terms_worksize"}


def test_every_buffer_taking_loo_export_has_a_framed_case():
    """The rule of tests/test_framed_cpu.py, continued for include/pygpr_hip_loo.h: every export with a device buffer is called in
    tests/test_loo_framed_gpu.py, and the worksize export sizes a framed workspace there."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_loo_framed_gpu.py")
    tree = ast.parse(open(path).read())
    used = {n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute) and n.attr.startswith("pg_")}
    exports = set(_lib._SIGS_LOO)
    assert NO_BUFFER <= exports
    assert sorted(exports - NO_BUFFER - used) == [], "exports with a device buffer and no framed case"
    assert sorted(NO_BUFFER - used) == [], "worksize exports that no framed case sizes its workspace with"


# ------------------------------------------------------------------------------------------- host logic on a test double
class LooOracleOps(OracleOps):
    """OracleOps plus the leave-one-out ops and the raw product, in NumPy; counts factorisations."""

    def __init__(self):
        self.factorisations = 0
        self.terms_calls = 0

    def build_factor(self, *a, **k):
        self.factorisations += 1
        return super().build_factor(*a, **k)

    def loo_terms_worksize(self, n_pad):
        return (n_pad // 256) * n_pad + n_pad // 256 + 2

    def loo_terms(self, minv, alpha, y, n, c, mu, var, out, work):
        self.terms_calls += 1
        m = np.tril(_np(minv).astype(np.float64))[:n, :n]
        cc = (m * m).sum(0)
        a, yy = _np(alpha).astype(np.float64)[:n], _np(y).astype(np.float64)[:n]
        c[:n] = torch.from_numpy(cc)
        mu[:n] = torch.from_numpy(yy - a / cc)
        var[:n] = torch.from_numpy(1.0 / cc)
        out[0] = float(np.sum(-0.5 * np.log(cc) + 0.5 * a * a / cc) + 0.5 * n * np.log(2 * np.pi))

    def loo_weights(self, c, alpha, kinv, n, p, q):
        cc, a = _np(c).astype(np.float64)[:n], _np(alpha).astype(np.float64)[:n]
        k = _np(kinv)
        b = k[:n, :n].astype(np.float64) @ (a / cc)
        k[:n, :n] *= np.sqrt(cc + a * a) / cc
        p[:n] = torch.from_numpy((a + b) / np.sqrt(2))
        q[:n] = torch.from_numpy((a - b) / np.sqrt(2))

    def loo_fold(self, m, q, n):
        qq = _np(q).astype(np.float64)[:n]
        _np(m)[:n, :n] += np.tril(np.outer(qq, qq))

    def gemm_raw(self, variant, m, n, k, alpha, a, b, beta, c, tri=0, klo=0, khi=0):
        assert variant == _lib.GEMM_NT and beta == 0.0
        c.copy_(torch.from_numpy(np.tril(alpha * _np(a).astype(np.float64) @ _np(b).astype(np.float64).T)))


@pytest.fixture
def fake_ops(monkeypatch, tmp_path):
    ops = LooOracleOps()
    monkeypatch.setattr(_ops, "_OPS", ops)
    monkeypatch.chdir(tmp_path)
    return ops


def _model(n=40, d=2, seed=5):
    rng = np.random.default_rng(seed)
    x = rng.random((n, d))
    y = np.sin(3 * x.sum(1)) + 0.3 * rng.standard_normal(n)
    hp = np.array([1.1, 0.8, 1.3, 0.9, 0.6, 1.2, 0.3])
    cov = pg.Compose([pg.Squared_exponential(), pg.Matern52(), pg.White_noise()])
    gp = pg.Exact_GP(torch.from_numpy(x.copy()), torch.from_numpy(y.copy()), cov)
    gp.set_params(torch.from_numpy(hp.copy()))
    return gp, x, y, hp, ["se", "m52", "wn"]


def test_loo_loss_and_grad_host_path(fake_ops):
    gp, x, y, hp, parts = _model()
    l_ref, g_ref = lr.loo_loss_and_grad(parts, hp, x, y)
    loo = pg.LOO(gp)
    assert isinstance(loo, pg.Loss) and "LOO" in pg.__all__
    loss, grad = loo.loss_and_grad(hp.copy())
    np.testing.assert_allclose(loss, l_ref, rtol=1e-10)
    np.testing.assert_allclose(grad, g_ref, rtol=0, atol=1e-8 * np.abs(g_ref).max())
    assert fake_ops.factorisations == 1
    # memo, level one: the same question again costs nothing; a loss after a gradient neither
    loo.loss_and_grad(hp.copy())
    loo.loss(hp.copy())
    assert fake_ops.factorisations == 1 and np.array_equal(loo.grad(hp.copy()), grad)


def test_loo_loss_then_grad_reuses_the_factor(fake_ops):
    gp, x, y, hp, parts = _model()
    loo = pg.LOO(gp)
    loss = loo.loss(hp.copy())
    np.testing.assert_allclose(loss, lr.loo_loss(parts, hp, x, y), rtol=1e-10)
    assert fake_ops.factorisations == 1
    grad = loo.grad(hp.copy())                                   # level two: the factor is still in the work buffers
    assert fake_ops.factorisations == 1
    fresh = pg.LOO(gp).loss_and_grad(hp.copy())[1]
    np.testing.assert_allclose(grad, fresh, rtol=1e-12, atol=0)
    loo.grad(hp * 1.01)                                          # other parameters: a new factorisation
    assert fake_ops.factorisations == 3
    loo.memoize = False
    loo.loss(hp.copy()), loo.loss(hp.copy())
    assert fake_ops.factorisations == 5


def test_loo_sees_changed_data_and_bad_pivots(fake_ops):
    gp, x, y, hp, parts = _model()
    loo = pg.LOO(gp)
    l0 = loo.loss(hp.copy())
    gp.y.mul_(2.0)                                               # an in-place edit bumps the version: part of the memo key
    l1 = loo.loss(hp.copy())
    np.testing.assert_allclose(l1, lr.loo_loss(parts, hp, x, 2 * y), rtol=1e-10)
    assert l0 != l1 and fake_ops.factorisations == 2
    bad = hp.copy()
    bad[0] = np.nan
    with pytest.raises(torch.linalg.LinAlgError):
        loo.loss_and_grad(bad)
    np.testing.assert_allclose(loo.loss(hp.copy()), l1, rtol=1e-12)


def test_loo_refuses_batched_models(fake_ops):
    gp, x, y, hp, parts = _model()
    with pytest.raises(NotImplementedError, match="batched"):
        pg.LOO(gp).loss(np.stack([hp, hp]))
    xb = torch.from_numpy(np.stack([x, x[::-1].copy()]))
    yb = torch.from_numpy(np.stack([y, y[::-1].copy()]))
    gb = pg.Exact_GP(xb, yb, gp.cov)
    with pytest.raises(NotImplementedError, match="batched"):
        pg.LOO(gb).loss_and_grad(hp.copy())
    with pytest.raises(NotImplementedError, match="batched models \\(more than one expert\\) are not supported"):
        gb.loo_predict()
    assert pg.GRBCM.loo_predict is pg.GPR.loo_predict              # the committee keeps the base class's refusal
    with pytest.raises(NotImplementedError, match="GPR has no leave-one-out prediction"):
        pg.GPR.loo_predict(pg.GPR(xb, yb, gp.cov))


def test_loo_predict_host_path(fake_ops):
    gp, x, y, hp, parts = _model()
    assert gp.need_upd
    mu, var = gp.loo_predict()                                   # a dirty model is fitted first
    assert not gp.need_upd and mu.shape == var.shape == (40,) and mu.dtype == torch.float64
    mr_, vr_ = lr.loo_predict(parts, hp, x, y)
    np.testing.assert_allclose(mu.numpy(), mr_, rtol=0, atol=1e-10)
    np.testing.assert_allclose(var.numpy(), vr_, rtol=0, atol=1e-10)
    minv = gp._experts[0].minv
    gp.loo_predict()
    assert gp._experts[0].minv is minv and fake_ops.terms_calls == 2 and fake_ops.factorisations == 1      # L^-1 is kept, nothing refitted
    gp.set_params(torch.from_numpy(hp * 1.1))                    # dirty again: refit, new inverse
    mu2, _ = gp.loo_predict()
    np.testing.assert_allclose(mu2.numpy(), lr.loo_predict(parts, hp * 1.1, x, y)[0], rtol=0, atol=1e-10)
    assert fake_ops.factorisations == 2
    gp.y = torch.from_numpy(y + 1.0)                             # assigning data marks the model dirty as well
    mu3, _ = gp.loo_predict()
    np.testing.assert_allclose(mu3.numpy(), lr.loo_predict(parts, hp * 1.1, x, y + 1.0)[0], rtol=0, atol=1e-10)
