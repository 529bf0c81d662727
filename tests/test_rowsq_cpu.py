"""pg_kernel_rowsq on the host: the new header parses, binds and is exported by the built library, the worksize arithmetic, the
refusals that need no device, and the restatement (tests/rowsq_ref.py) in float64 against np.longdouble inside the kernel's own
bound.  No GPU."""
import ctypes
import inspect

import numpy as np
import pytest

import matmul_ref as mr
import rowsq_ref as rr
from pygpr_amd import _lib

MODELS = {"se+wn": ["se", "wn"], "m12": ["m12"], "rq": ["rq"], "per": ["per"], "se+m52": ["se", "m52"], "se*per": [("se", "per")]}


def _hp(terms, d, rng):
    import kernel_ref as kr

    hp = []
    for part in kr.flat(terms):
        if part == "wn":
            hp += [0.3]
            continue
        hp += [0.8 + 0.4 * rng.random()] + list((0.8 + 0.8 * rng.random(d)) / np.sqrt(d))
        hp += [1.3] if part == "rq" else (list(0.6 + 0.5 * rng.random(d)) if part == "per" else [])
    return np.array(hp)


def test_rowsq_header_parses_binds_and_is_exported():
    text = open(_lib.HEADER_ROWSQ).read()
    protos = _lib.parse_prototypes(text)
    assert sorted(protos) == ["pg_kernel_rowsq", "pg_kernel_rowsq_worksize"]
    assert _lib._SIGS_ROWSQ == _lib.signatures(protos)
    others = (set(_lib.header_symbols()) | set(_lib._SIGS_LOO) | set(_lib._SIGS_SAMPLE) | set(_lib._SIGS_SPARSE) | set(_lib._SIGS_SELECT)
              | set(_lib._SIGS_MATMUL) | set(_lib._SIGS_LOWRANK) | set(_lib._SIGS_FEATURE) | set(_lib._SIGS_DMATMUL))
    assert not set(protos) & others and "#define PG_KIND" not in text
    # the conventions text is the matmul header's, word for word
    conv = lambda t: t[t.index(" * Conventions:"): t.index("#ifndef")]      # noqa: E731
    assert conv(text) == conv(open(_lib.HEADER_MATMUL).read())
    vp, i, lg = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    assert _lib._SIGS_ROWSQ["pg_kernel_rowsq_worksize"] == (lg, [i, i])
    assert _lib._SIGS_ROWSQ["pg_kernel_rowsq"] == (i, [vp, i, ctypes.POINTER(_lib.CovSpec), vp, vp, lg, i, vp, lg, i, i, vp, lg, vp, vp])
    lib = _lib.load(check_symbols=True)
    for name, (res, args) in _lib._SIGS_ROWSQ.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert "HEADER_ROWSQ" in inspect.getsource(_lib.build_id) and "_SIGS_ROWSQ" in inspect.getsource(_lib.load)


def test_worksize_is_the_plan_of_one_right_hand_side():
    """pg_kernel_matmul's segments at one column, one double a row and segment instead of a 64 x 32 partial tile."""
    lib = _lib.load()
    assert lib.pg_kernel_rowsq_worksize(65536, 65536) == 0 and lib.pg_kernel_rowsq_worksize(1, 300) == 0
    assert lib.pg_kernel_rowsq_worksize(5, 5000) == 16 * 64                    # 79 column tiles: 16 segments of five
    assert lib.pg_kernel_rowsq_worksize(8192, 32768) == 4 * 128 * 64          # 128 row tiles: four segments fill 512 workgroups
    assert lib.pg_kernel_rowsq_worksize(0, 0) == 0 and lib.pg_kernel_rowsq_worksize(70, 0) == 0
    assert lib.pg_kernel_rowsq_worksize(-1, 0) == -1 and lib.pg_kernel_rowsq_worksize(5, -1) == -1
    for nr, nc in ((5, 5000), (8192, 32768), (257, 17), (100, 2000)):         # the same segments as the product's
        assert lib.pg_kernel_rowsq_worksize(nr, nc) * 32 == lib.pg_kernel_matmul_worksize(nr, nc, 1)


def test_a_null_handle_is_refused_with_a_text():
    lib = _lib.load()
    assert lib.pg_kernel_rowsq(None, 0, None, None, None, 1, 1, None, 1, 1, 1, None, 1, None, None) != 0
    assert b"pg_kernel_rowsq" in lib.pg_last_error()


@pytest.mark.parametrize("name", sorted(MODELS))
@pytest.mark.parametrize("d", [1, 3, 17])
@pytest.mark.parametrize("nr,nc", [(70, 150), (5, 5000), (257, 17), (64, 64)])
def test_the_float64_restatement_is_inside_the_kernels_bound(name, d, nr, nc):
    terms = MODELS[name]
    rng = np.random.default_rng(1000 * nr + 10 * nc + d)
    hp = _hp(terms, d, rng)
    xr, xc = rng.random((nr, d)), rng.random((nc, d))
    ref = rr.rowsq(terms, hp, xr, xc, np.longdouble)
    assert ref.dtype == np.longdouble and ref.shape == (nr,)
    got = rr.rowsq(terms, hp, xr, xc)
    own = mr.own_k(terms, hp, xr, xc)
    bound = rr.bound_of(own, nc)
    fig = float(np.max(np.abs(got - ref) / ref))
    print("%-8s %4dx%-4d d=%-2d float64 restatement %.2e  own_K %.2e  (bound %.2e)" % (name, nr, nc, d, fig, own, bound))
    assert np.all(np.abs(got - ref) <= bound * ref)
    # the definition, pair by pair, on a corner of the case
    k = mr.stationary_kernel(terms, hp, xr[:3], xc[:7])
    assert np.allclose(rr.rowsq(terms, hp, xr[:3], xc[:7]), [sum(v * v for v in row) for row in k], rtol=1e-14, atol=0)


def test_an_empty_column_range_gives_zeros():
    out = rr.rowsq(["se", "wn"], np.array([1.0, 1.0, 1.0, 0.3]), np.zeros((4, 2)), np.zeros((0, 2)))
    assert out.shape == (4,) and not out.any()
