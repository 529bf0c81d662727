"""The derivative's matrix-free product on the host: the restatement (tests/dmatmul_ref.py) against central differences of the product
it differentiates and against the torch contraction, the new header, and the two public features -- FunctionSamples.grad and
Iterative_GP.predict_grad -- on oracle ops.  No GPU.

The oracle ops are tests/oracle_ops.KindOracleOps with the matrix-free products this model calls restated in NumPy (kernel_matmul,
kernel_matmul_dx, feature_matmul, kernel_xgrad's vector and B forms): the host logic -- shapes, blocks of test points and of coordinates, the
shared solve, the refusals -- runs where there is no device."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import dmatmul_ref as dr
import feature_ref as fr
import kernel_ref as kr
import matmul_ref as mr
import pygpr_amd as pg
import xgrad_ref as xr
from kind_tools import cov_of
from oracle_ops import KindOracleOps, _np
from pygpr_amd import _lib, _ops
from pygpr_amd import iterative as it_mod
from pygpr_amd.covar import spec_of
from pygpr_amd.pathwise import FunctionSamples
from pygpr_amd.sparse import _stationary

MODELS = {"se+wn": ["se", "wn"], "m12": ["m12"], "m32+m52": ["m32", "m52"], "rq": ["rq"], "per": ["per"], "se*per": [("se", "per")],
          "rq*m12*per+se": [("rq", "m12", "per"), "se"]}


def _hp(terms, d, rng):
    hp = []
    for part in kr.flat(terms):
        if part == "wn":
            hp += [0.3]
            continue
        hp += [0.8 + 0.4 * rng.random()] + list((0.8 + 0.8 * rng.random(d)) / np.sqrt(d))
        hp += [1.3] if part == "rq" else (list(0.6 + 0.5 * rng.random(d)) if part == "per" else [])
    return np.array(hp)


# ------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", sorted(MODELS))
def test_the_restatement_is_the_derivative_of_the_product(name):
    """Central differences of matmul_ref.matmul in np.longdouble, tests/test_xgrad_cpu.py's practice: step 1e-6, allowance 1e-6 of
    max(1, the largest difference quotient)."""
    terms, d = MODELS[name], 3
    rng = np.random.default_rng(5)
    hp = _hp(terms, d, rng)
    xrow, xcol, v = rng.random((6, d)), rng.random((11, d)), rng.standard_normal((11, 4))
    out, scale = dr.matmul_dx(terms, hp, xrow, xcol, v, np.longdouble)
    assert out.shape == scale.shape == (6, d, 4) and out.dtype == np.longdouble
    h = np.longdouble(1e-6)
    fd = np.zeros((6, d, 4), np.longdouble)
    for k in range(d):
        a, b = np.asarray(xrow, np.longdouble).copy(), np.asarray(xrow, np.longdouble).copy()
        a[:, k] += h                      # (row i of the product depends on row point i alone: every row steps at once)
        b[:, k] -= h
        fd[:, k, :] = (mr.matmul(terms, hp, a, xcol, v, dtype=np.longdouble)[0] - mr.matmul(terms, hp, b, xcol, v, dtype=np.longdouble)[0]) / (2 * h)
    err = float(np.max(np.abs(out - fd)))
    print("%-16s restatement vs central differences %.2e" % (name, err))
    assert err <= 1e-6 * max(1.0, float(np.abs(fd).max()))
    o64, s64 = dr.matmul_dx(terms, hp, xrow, xcol, v)
    assert o64.dtype == np.float64 and float(np.max(np.abs(o64 - out) / scale)) <= 16 * dr.own_dk(terms, hp, xrow, xcol) + 13 * 2.0 ** -53
    vec, svec = dr.matmul_dx(terms, hp, xrow, xcol, v[:, 1])
    one, sone = dr.matmul_dx(terms, hp, xrow, xcol, v[:, 1:2])      # a vector counts as one column
    assert vec.shape == (6, d) and np.array_equal(vec, one[:, :, 0]) and np.array_equal(svec, sone[:, :, 0])
    np.testing.assert_allclose(vec, o64[:, :, 1], rtol=0, atol=11 * 2.0 ** -52 * float(s64[:, :, 1].max()))


@pytest.mark.parametrize("parts", [["se"], ["m52", "wn"], ["m32", "se"], ["m12"]])
def test_the_restatement_is_the_contraction_column_by_column(parts):
    rng = np.random.default_rng(6)
    d = 4
    hp = _hp(parts, d, rng)
    xq, z, v = rng.random((5, d)), rng.random((9, d)), rng.standard_normal((9, 3))
    out, _ = dr.matmul_dx(parts, hp, xq, z, v)
    T = torch.from_numpy
    for c in range(3):
        ou, _ = xr.contraction(parts, T(hp), T(xq), T(z), u=T(np.ascontiguousarray(v[:, c])))
        np.testing.assert_allclose(out[:, :, c], ou.numpy(), rtol=1e-12, atol=1e-14)


def test_the_restatements_conventions():
    """Matern-1/2 at r = 0 contributes 0; own_dk is taken against the row's largest entry and floored."""
    hp = np.array([1.0, 1.5, 0.7])
    x = np.random.default_rng(4).random((7, 2))
    dk = dr.dkernel(["m12"], hp, x, x)
    assert dk.shape == (2, 7, 7) and np.all(dk[:, np.arange(7), np.arange(7)] == 0.0) and np.isfinite(dk).all()
    assert dr.own_dk(["se"], hp, x, x) >= 2.0 ** -53 and dr.own_dk(["se"], hp, x[:0], x[:0]) == 2.0 ** -53
    # a periodic derivative next to its zero crossing: tiny entries, whose error relative to themselves is not what the product sees
    hpp = np.array([1.0, 1.5, 0.7, 0.9, 1.1])
    assert dr.own_dk(["per"], hpp, x, x + np.array([0.45, 0.55])) < 1e-13


# ------------------------------------------------------------------------------------------- the header
def test_dmatmul_header_parses_binds_and_is_exported():
    text = open(_lib.HEADER_DMATMUL).read()
    protos = _lib.parse_prototypes(text)
    assert sorted(protos) == ["pg_kernel_matmul_dx", "pg_kernel_matmul_dx_worksize"]
    assert _lib._SIGS_DMATMUL == _lib.signatures(protos)
    others = (set(_lib.header_symbols()) | set(_lib._SIGS_LOO) | set(_lib._SIGS_SAMPLE) | set(_lib._SIGS_SPARSE) | set(_lib._SIGS_SELECT)
              | set(_lib._SIGS_MATMUL) | set(_lib._SIGS_LOWRANK) | set(_lib._SIGS_FEATURE))
    assert not set(protos) & others and "#define PG_KIND" not in text
    # the conventions text is the matmul header's, word for word
    conv = lambda t: t[t.index(" * Conventions:"): t.index("#ifndef")]      # noqa: E731
    assert conv(text) == conv(open(_lib.HEADER_MATMUL).read())
    vp, i, lg = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    assert _lib._SIGS_DMATMUL["pg_kernel_matmul_dx_worksize"] == (lg, [i, i, i, i])
    assert _lib._SIGS_DMATMUL["pg_kernel_matmul_dx"] == (i, [vp, i, ctypes.POINTER(_lib.CovSpec), vp, vp, lg, i, vp, lg, i, i, vp, lg, i, vp, lg, lg,
                                                             vp, vp])
    lib = _lib.load(check_symbols=True)
    for name, (res, args) in _lib._SIGS_DMATMUL.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    # host arithmetic: pg_kernel_matmul's segments, one 64 x (chunks x 8, or 4 at d <= 4) x 32 partial tile per row tile and segment
    ws = lib.pg_kernel_matmul_dx_worksize
    assert ws(65536, 65536, 8, 16) == 0 and ws(1, 300, 3, 3) == 0 and ws(0, 0, 0, 0) == 0
    assert ws(5, 5000, 3, 2) == 16 * 64 * 4 * 32 and ws(5, 5000, 8, 2) == 16 * 64 * 8 * 32 and ws(5, 5000, 17, 33) == 16 * 64 * 24 * 64
    assert ws(5, 5000, 3, 2) == 4 * lib.pg_kernel_matmul_worksize(5, 5000, 2)
    assert ws(-1, 0, 1, 0) == -1 and ws(5, -1, 1, 1) == -1 and ws(5, 5, -1, 1) == -1 and ws(5, 5, 1, -1) == -1
    assert lib.pg_kernel_matmul_dx(None, 0, None, None, None, 1, 1, None, 1, 1, 1, None, 1, 1, None, 1, 1, None, None) != 0      # null handle: refused
    assert b"pg_kernel_matmul_dx" in lib.pg_last_error()
    assert "HEADER_DMATMUL" in inspect.getsource(_lib.build_id) and "_SIGS_DMATMUL" in inspect.getsource(_lib.load)
    assert hasattr(_ops.HipOps, "kernel_matmul_dx") and hasattr(_ops.HipOps, "kernel_matmul_dx_worksize")
    assert callable(getattr(pg.Iterative_GP, "predict_grad", None)) and callable(getattr(FunctionSamples, "grad", None))


# ------------------------------------------------------------------------------------------- the public features on oracle ops
class DxOracleOps(KindOracleOps):
    """KindOracleOps with the matrix-free products of Iterative_GP and FunctionSamples restated in NumPy."""

    def kernel_matmul_worksize(self, nr, nc, nrhs):
        return 0

    def kernel_matmul_dx_worksize(self, nr, nc, d, nrhs):
        return 0

    def kernel_matmul(self, spec, hp, xr, xc, v, out=None, jitter=0.0, work=None):
        x = _np(xr)
        model, h, _ = self._model(spec, _np(hp), x.shape[1])
        res, _ = mr.matmul(model, h, x, None if xc is None else _np(xc), _np(v), jitter)
        res = torch.from_numpy(np.ascontiguousarray(res))
        return res if out is None else out.copy_(res)

    def kernel_matmul_dx(self, spec, hp, xr, xc, v, out=None, work=None):
        x = _np(xr)
        model, h, _ = self._model(spec, _np(hp), x.shape[1])
        res, _ = dr.matmul_dx(model, h, x, _np(xc), _np(v))
        res = torch.from_numpy(np.ascontiguousarray(res))
        return res if out is None else out.copy_(res)

    def feature_matmul(self, x, nu, u, w, out=None, work=None):
        res = torch.from_numpy(np.ascontiguousarray(fr.matmul(_np(x), _np(nu), _np(u), _np(w))[0]))
        return res if out is None else out.copy_(res)

    def kernel_xgrad(self, spec, hp, xq, z, u=None, b=None, out_u=None, out_b=None, trans_b=False, accumulate=False):
        assert (u is None) != (b is None) and not accumulate
        q = _np(xq)
        model, h, _ = self._model(spec, _np(hp), q.shape[1])
        dk = dr.dkernel(model, h, q, _np(z))                               # [d, m, n]
        if u is not None:                                                  # the vector form: one weight per training point
            res = torch.from_numpy(np.einsum("kpi,i->pk", dk, _np(u)[: dk.shape[2]]))
            return (res if out_u is None else out_u.copy_(res)), None
        w = _np(b).T[: q.shape[0]] if trans_b else _np(b)                  # [m, >= n]
        res = torch.from_numpy(np.einsum("kpi,pi->pk", dk, w[:, : dk.shape[2]]))
        return None, (res if out_b is None else out_b.copy_(res))


@pytest.fixture
def dx_ops(monkeypatch):
    ops = DxOracleOps()
    monkeypatch.setattr(_ops, "_OPS", ops)
    return ops


def _problem(parts, n=60, m=23, d=3, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.random((n, d))
    y = np.sin(3.0 * x).sum(1) + 0.1 * rng.standard_normal(n)
    hp = []
    for p in parts:
        hp += [0.2] if p == "wn" else [rng.uniform(0.8, 1.3)] + list(rng.uniform(0.8, 2.0, d))
    return x, y, rng.random((m, d)), np.array(hp)


@pytest.mark.parametrize("parts", [["se", "wn"], ["m52", "m12", "wn"]])
def test_predict_grad_on_oracle_ops(dx_ops, monkeypatch, parts):
    """Against tests/xgrad_ref.predict_grads on the dense factor: 2 cond(A) tol of the largest reference entry (the solves stop at
    tol) plus 1e-9 of it, the dense yardstick of tests/test_xgrad_gpu.py.  _RHS_BLOCK = 8: three blocks of test points, the last of 7."""
    monkeypatch.setattr(it_mod, "_RHS_BLOCK", 8)
    x, y, xp, hp = _problem(parts)
    T = torch.from_numpy
    tol = 1e-11
    model = pg.Iterative_GP(T(x), T(y), cov_of(parts), rank=0, tol=tol)
    model.set_params(T(hp))
    mean, var, dmean, dvar = model.predict_grad(T(xp), var="diag")
    m0, v0 = model.predict(T(xp), var="diag")
    assert torch.equal(mean, m0) and torch.equal(var, v0)
    assert dmean.shape == dvar.shape == xp.shape and dmean.dtype == torch.float64
    rm, rv, rdm, rdv = xr.predict_grads(parts, T(hp), T(x), T(y), T(xp))
    cond = float(np.linalg.cond(kr.kernel(parts, hp, x) + kr.JITTER * np.eye(x.shape[0])))
    for label, got, ref in (("dmean", dmean, rdm), ("dvar", dvar, rdv)):
        scale = float(ref.abs().max())
        err = float((got - ref).abs().max())
        print("%s %s: err %.2e (bound %.2e, cond %.2e)" % ("+".join(parts), label, err, (2 * cond * tol + 1e-9) * scale, cond))
        assert err <= (2 * cond * tol + 1e-9) * scale
    calls = []
    solve = model._solve
    monkeypatch.setattr(model, "_solve", lambda *a, **k: calls.append(1) or solve(*a, **k))
    mean1, dmean1 = model.predict_grad(T(xp), var="none")
    assert calls == [] and torch.equal(mean1, mean) and torch.equal(dmean1, dmean)
    model.predict_grad(T(xp), var="diag")
    assert len(calls) == 3
    with pytest.raises(ValueError, match="'diag' or 'none'"):
        model.predict_grad(T(xp), var="full")
    with pytest.raises(NotImplementedError, match="no batches"):
        model.predict_grad(T(xp)[None])
    with pytest.raises(TypeError, match="float64 only"):
        model.predict_grad(T(xp).float())
    with pytest.raises(NotImplementedError, match="use an Exact_GP for derivatives in the test points"):
        model.predict(T(xp).requires_grad_(True))


@pytest.mark.parametrize("prior", [False, True])
def test_function_samples_grad_on_oracle_ops(dx_ops, monkeypatch, prior):
    """A snapshot built from given arrays: grad against the exact restatement of the sample from frequencies, phases, weights and
    data_weights in np.longdouble (the oracle ops round in float64: 1e-12 of the largest entry), and against central differences of
    the snapshot's own values.  Five coordinates at two per feature product: blocks of 2, 2 and 1."""
    from pygpr_amd import pathwise

    terms, d, n, S, nf = ["se", "m32", "wn"], 5, 17, 3, 12
    monkeypatch.setattr(pathwise, "_GRAD_COLUMNS", 2 * S)
    rng = np.random.default_rng(8)
    hp = _hp(terms, d, rng)
    (sp,), _ = spec_of(cov_of(terms), d)
    T = torch.from_numpy
    x, xp = rng.random((n, d)), rng.random((9, d))
    nu, w, v = rng.standard_normal((nf, d)), rng.standard_normal((nf, S)), rng.standard_normal((n, S))
    u = np.where(np.arange(nf) % 2 == 1, -0.25, 0.0)
    fs = FunctionSamples(None if prior else _stationary(sp), None if prior else T(hp), None if prior else T(x), T(nu), T(u), T(w),
                         None if prior else T(v), nf // 2, 0, None)
    if prior:
        assert fs.data_weights is None
    else:
        assert np.array_equal(fs.data_weights, v) and fs.data_weights is not v
    got = fs.grad(T(xp))
    assert got.shape == (S, 9, d) and got.dtype == torch.float64
    two_pi = 8 * np.arctan(np.longdouble(1))
    wk = (two_pi * np.asarray(fs.frequencies, np.longdouble)[:, :, None] * np.asarray(fs.weights, np.longdouble)[:, None, :]).reshape(nf, d * S)
    ref = fr.matmul(xp, fs.frequencies, fs.phases + 0.25, wk, np.longdouble)[0].reshape(9, d, S)
    if not prior:
        ref = ref + dr.matmul_dx(["se", "m32"], hp[: 2 * (d + 1)], xp, x, fs.data_weights, np.longdouble)[0]
    ref = np.transpose(ref, (2, 0, 1))
    err = float(np.max(np.abs(got.numpy() - ref)))
    print("grad (prior %s): err %.2e of %.2e" % (prior, err, float(np.abs(ref).max())))
    assert err <= 1e-12 * float(np.abs(ref).max())
    h = 1e-6
    for k in range(d):
        e = np.zeros(d)
        e[k] = h
        fd = (fs(T(xp + e)) - fs(T(xp - e))).numpy() / (2 * h)
        assert float(np.max(np.abs(fd - got.numpy()[:, :, k]))) <= 1e-6 * max(1.0, float(np.abs(ref).max()))
    with pytest.raises(NotImplementedError, match="no batches"):
        fs.grad(T(xp)[None])
    with pytest.raises(TypeError, match="float64 only"):
        fs.grad(T(xp).float())
