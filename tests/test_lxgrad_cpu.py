"""The low-rank training-input gradient on the host: the new header, the worksize arithmetic and the restatement (tests/lxgrad_ref.py)
against tests/kernel_ref.kernel_xgrad contracted with the formed weight.  No GPU."""
import ctypes
import inspect

import numpy as np
import pytest

import kernel_ref as kr
import lxgrad_ref as lx
import pygpr_amd as pg
from pygpr_amd import _lib, _ops

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


def test_lxgrad_header_parses_binds_and_is_exported():
    text = open(_lib.HEADER_LXGRAD).read()
    protos = _lib.parse_prototypes(text)
    assert sorted(protos) == ["pg_kernel_lowrank_xgrad", "pg_kernel_lowrank_xgrad_worksize"]
    assert _lib._SIGS_LXGRAD == _lib.signatures(protos)
    others = (set(_lib.header_symbols()) | set(_lib._SIGS_LOO) | set(_lib._SIGS_SAMPLE) | set(_lib._SIGS_SPARSE) | set(_lib._SIGS_SELECT)
              | set(_lib._SIGS_MATMUL) | set(_lib._SIGS_LOWRANK) | set(_lib._SIGS_FEATURE) | set(_lib._SIGS_DMATMUL) | set(_lib._SIGS_ROWSQ))
    assert not set(protos) & others and "#define PG_KIND" not in text
    # the conventions text is the low-rank header's, word for word
    conv = lambda t: t[t.index(" * Conventions:"): t.index("#ifndef")]      # noqa: E731
    assert conv(text) == conv(open(_lib.HEADER_LOWRANK).read())
    vp, i, lg = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    assert _lib._SIGS_LXGRAD["pg_kernel_lowrank_xgrad_worksize"] == (lg, [i, i, i, i])
    assert _lib._SIGS_LXGRAD["pg_kernel_lowrank_xgrad"] == (i, [vp, i, ctypes.POINTER(_lib.CovSpec), vp, vp, lg, i, vp, lg, i, i, vp, lg, vp, lg, i,
                                                                vp, lg, i, vp, vp])
    lib = _lib.load(check_symbols=True)
    for name, (res, args) in _lib._SIGS_LXGRAD.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert lib.pg_kernel_lowrank_xgrad(None, 0, None, None, None, 1, 1, None, 1, 1, 1, None, 1, None, 1, 1, None, 1, 0, None, None) != 0   # null handle
    assert b"pg_kernel_lowrank_xgrad" in lib.pg_last_error()
    assert "HEADER_LXGRAD" in inspect.getsource(_lib.build_id) and "_SIGS_LXGRAD" in inspect.getsource(_lib.load)
    assert hasattr(_ops.HipOps, "kernel_lowrank_xgrad") and hasattr(_ops.HipOps, "kernel_lowrank_xgrad_worksize")
    assert callable(getattr(pg.Stochastic_MLE, "grad_x", None)) and callable(getattr(pg.MLE, "grad_x", None))
    assert "nlml_of_inputs" in pg.__all__


def test_worksize_arithmetic():
    """pg_kernel_matmul's segments at one right-hand side times the passes of 32 factor columns: one slab of 64-row tiles by chunks of
    coordinates (8, or 4 at d <= 4) for each, none when there is one slab."""
    ws = _lib.load().pg_kernel_lowrank_xgrad_worksize
    assert ws(65536, 65536, 8, 16) == 0 and ws(1, 300, 3, 3) == 0 and ws(0, 0, 0, 0) == 0 and ws(70, 150, 3, 0) == 0 and ws(70, 0, 3, 4) == 0
    assert ws(5, 5000, 3, 2) == 16 * 64 * 4 and ws(5, 5000, 8, 2) == 16 * 64 * 8 and ws(5, 5000, 17, 33) == 2 * 16 * 64 * 24
    assert ws(70, 150, 3, 32) == 0 and ws(70, 150, 3, 33) == 2 * 128 * 4 and ws(70, 150, 33, 64) == 2 * 128 * 40
    assert ws(5, 5000, 3, 2) == 4 * _lib.load().pg_kernel_rowsq_worksize(5, 5000)
    for nr in (0, 1, 64, 65, 5000, 40000):
        for nc in (0, 1, 511, 512, 513, 5000):
            for d, r in ((1, 1), (4, 32), (5, 33), (64, 64)):
                assert ws(nr, nc, d, r) == lx.worksize(nr, nc, d, r), (nr, nc, d, r)
    assert ws(-1, 0, 1, 0) == -1 and ws(5, -1, 1, 1) == -1 and ws(5, 5, -1, 1) == -1 and ws(5, 5, 1, -1) == -1


@pytest.mark.parametrize("name", sorted(MODELS))
def test_the_restatement_is_kernel_xgrad_against_the_formed_weight(name):
    terms, d, nr, nc, r = MODELS[name], 3, 7, 11, 5
    rng = np.random.default_rng(5)
    hp = _hp(terms, d, rng)
    xr, xc = rng.random((nr, d)), rng.random((nc, d))
    u, v, vs = rng.standard_normal((nr, r)), rng.standard_normal((nc, r)), rng.standard_normal((nr, r))
    for sym in (False, True):
        vv, cols = (vs, xr) if sym else (v, xc)
        out, scale = lx.lowrank_xgrad(terms, hp, xr, None if sym else xc, u, vv)
        dk = kr.kernel_xgrad(terms, hp, cols, xr)                  # [d, nr, nc]: dk(xr_i, cols_j)/dxr_ik
        w = u @ vv.T
        w = w + w.T if sym else w
        want = np.stack([np.sum(w * dk[k], axis=1) for k in range(d)], 1)
        assert out.shape == scale.shape == (nr, d) and out.dtype == np.float64
        assert np.all(np.abs(out - want) <= 8 * 2.0 ** -52 * scale) and np.all(scale >= np.abs(out))
        old, _ = lx.lowrank_xgrad(terms, hp, xr, None if sym else xc, u, vv, np.longdouble)
        assert old.dtype == np.longdouble and np.all(np.abs(old - out) <= 1e-13 * scale)
    # the symmetric form is the gradient of sum_ij (U V^T)_ij k(x_i, x_j) in x: central differences in longdouble
    out, _ = lx.lowrank_xgrad(terms, hp, xr, None, u, vs, np.longdouble)
    w = np.asarray(u, np.longdouble) @ np.asarray(vs, np.longdouble).T
    f = lambda x: np.sum(w * kr.kernel(terms, hp, x, x, dtype=np.longdouble))      # noqa: E731  (cross form: no noise on the diagonal)
    h = np.longdouble(1e-6)
    fd = np.zeros((nr, d), np.longdouble)
    for i in range(nr):
        for k in range(d):
            a, b = np.asarray(xr, np.longdouble).copy(), np.asarray(xr, np.longdouble).copy()
            a[i, k] += h
            b[i, k] -= h
            fd[i, k] = (f(a) - f(b)) / (2 * h)
    err = float(np.max(np.abs(out - fd)))
    print("%-16s symmetric restatement vs central differences %.2e" % (name, err))
    # (the diagonal k(x_i, x_i) does not move with x_i: the convention that a pair at r = 0 contributes 0 is exact, Matern-1/2 included)
    assert err <= 1e-6 * max(1.0, float(np.abs(fd).max()))
