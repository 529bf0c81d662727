"""pg_kernel_lowrank_grad on the host: the seventh header, its binding, the worksize arithmetic and the restatement
(tests/lowrank_ref.py) against the contraction it restates.  No GPU."""
import ast
import ctypes
import inspect
import os

import numpy as np
import pytest

import kernel_ref as kr
import lowrank_ref as lr
import sparse_ref as sr
from pygpr_amd import _lib


def test_lowrank_header_parses_binds_and_is_exported():
    text = open(_lib.HEADER_LOWRANK).read()
    protos = _lib.parse_prototypes(text)
    assert sorted(protos) == ["pg_kernel_lowrank_grad", "pg_kernel_lowrank_grad_worksize"]
    assert _lib._SIGS_LOWRANK == _lib.signatures(protos)
    others = (set(_lib.header_symbols()) | set(_lib._SIGS_LOO) | set(_lib._SIGS_SAMPLE) | set(_lib._SIGS_SPARSE) | set(_lib._SIGS_SELECT)
              | set(_lib._SIGS_MATMUL))
    assert not set(protos) & others and "#define PG_KIND" not in text
    vp, i, lg = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    assert _lib._SIGS_LOWRANK["pg_kernel_lowrank_grad_worksize"] == (lg, [i, i, i, i])
    assert _lib._SIGS_LOWRANK["pg_kernel_lowrank_grad"] == (i, [vp, i, ctypes.POINTER(_lib.CovSpec), vp, vp, lg, i, vp, lg, i, i, vp, lg, vp, lg,
                                                               i, vp, i, vp, vp])
    lib = _lib.load(check_symbols=True)
    for name, (res, args) in _lib._SIGS_LOWRANK.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert "HEADER_LOWRANK" in inspect.getsource(_lib.build_id) and "_SIGS_LOWRANK" in inspect.getsource(_lib.load)
    assert lib.pg_kernel_lowrank_grad(None, 0, None, None, None, 1, 1, None, 1, 1, 1, None, 1, None, 1, 1, None, 0, None, None) != 0      # null handle
    assert b"pg_kernel_lowrank_grad" in lib.pg_last_error()


def test_worksize_arithmetic():
    """One slot row of nhp doubles per column tile, segment of row tiles and pass of 32 factor columns; segments hold at least four row
    tiles and grow so that a pass has at most 32768 workgroups."""
    ws = _lib.load().pg_kernel_lowrank_grad_worksize
    assert ws(70, 150, 1, 5) == 1 * 3 * 1 * 5                      # two row tiles: one segment; three column tiles
    assert ws(130, 70, 33, 9) == 1 * 2 * 2 * 9                     # 33 factor columns: two passes
    assert ws(257, 257, 17, 7) == 2 * 5 * 1 * 7                    # five row tiles: segments of four
    assert ws(65536, 65536, 16, 10) == 32 * 1024 * 10              # 1024 x 1024 tiles: segments of 32 row tiles
    assert ws(262144, 262144, 16, 10) == 8 * 4096 * 10             # segments of 512
    assert ws(5, 2000, 2, 4) == 32 * 4 and ws(1, 1, 64, 3) == 2 * 3
    for shape in [(0, 150, 4, 5), (70, 0, 4, 5), (70, 150, 0, 5), (0, 0, 0, 0), (70, 150, 4, 0)]:
        assert ws(*shape) == 0
    for shape in [(-1, 1, 1, 1), (1, -1, 1, 1), (1, 1, -1, 1), (1, 1, 1, -1)]:
        assert ws(*shape) == -1
    rng = np.random.default_rng(0)
    for _ in range(200):
        nr, nc, r, nhp = int(rng.integers(0, 400000)), int(rng.integers(0, 400000)), int(rng.integers(0, 65)), int(rng.integers(0, 20))
        assert ws(nr, nc, r, nhp) == lr.worksize(nr, nc, r, nhp)


def test_every_lowrank_export_has_a_framed_case():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_lowrank_grad_gpu.py")
    tree = ast.parse(open(path).read())
    case = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "case_lowrank_grad")
    used = {n.attr for n in ast.walk(case) if isinstance(n, ast.Attribute) and n.attr.startswith("pg_")}
    assert sorted(set(_lib._SIGS_LOWRANK) - used) == []


@pytest.mark.parametrize("name,terms", [("se+wn", ["se", "wn"]), ("rq+m12", ["rq", "m12"]), ("se*per", [("se", "per")])])
def test_restatement_is_cross_grad_on_the_formed_weight(name, terms):
    """The restatement against sparse_ref.cross_grad on W = U V^T, the symmetric form against the cross form on the one point set and
    against kernel_ref.grad_terms, and U <-> V against the transposed weight."""
    rng = np.random.default_rng(4)
    d, nr, nc, r = 3, 37, 53, 5
    hp = np.concatenate([[0.9 if p != "wn" else 0.3] + ([] if p == "wn" else list(0.8 + rng.random(d)) + ([1.3] if p == "rq" else [])
                                                       + (list(0.6 + rng.random(d)) if p == "per" else [])) for p in kr.flat(terms)])
    xr, xc, u, v = rng.random((nr, d)), rng.random((nc, d)), rng.standard_normal((nr, r)), rng.standard_normal((nc, r))
    mine = lr.mine(terms, d)
    got = lr.lowrank_grad(terms, hp, xr, xc, u, v)
    want = sr.cross_grad(terms, hp, xr, xc, u @ v.T)
    s = lr.scale(terms, hp, xr, xc, u, v)
    err = float(np.max(np.abs(got - want)[mine] / s[mine]))
    print("%s: restatement against cross_grad on the formed weight: %.2e of S_p" % (name, err))
    assert err <= 4 * 2.0 ** -52 and not got[~mine].any()
    ld = lr.lowrank_grad(terms, hp, xr, xc, u, v, np.longdouble)
    assert ld.dtype == np.longdouble and float(np.max(np.abs(ld - got)[mine] / s[mine])) <= 64 * 2.0 ** -53
    v2 = rng.standard_normal((nr, r))
    sym = lr.lowrank_grad(terms, hp, xr, None, u, v2)
    assert np.array_equal(sym, lr.lowrank_grad(terms, hp, xr, xr, u, v2))
    w = u @ v2.T
    s2 = lr.scale(terms, hp, xr, None, u, v2)
    for i, slab in kr.grad_terms(terms, hp, xr):
        if mine[i]:
            assert abs(np.sum(w * slab) - sym[i]) <= 8 * 2.0 ** -52 * s2[i]
    swapped = lr.lowrank_grad(terms, hp, xr, None, v2, u)
    assert np.max(np.abs(swapped - sym)[mine] / s2[mine]) <= 8 * 2.0 ** -52
