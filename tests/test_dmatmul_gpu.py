"""pg_kernel_matmul_dx on the MI355X: OUT[i][k][c] = sum_j dk(Xr_i, Xc_j)/dXr_ik V[j][c] against the NumPy restatement
(tests/dmatmul_ref.py), for reproducibility, the NaN rules, empty shapes, points far from the origin and refusals.

Tolerance, per entry and derived, never fitted: with S_ikc = sum_j |dK_ijk V_jc| the device may miss the np.longdouble product by
(16 own_dK + (nc + 2) 2^-53) S_ikc.  own_dK is the restatement's own float64-vs-longdouble error in dK, relative to the largest entry of
a row and coordinate and floored at 2^-53 (dmatmul_ref.own_dk says why not per entry); the second term is the any-order bound of a sum
of nc products.  A dropped or doubled column tile, a coordinate chunk written to the wrong place or a panel taken twice misses it by
orders of magnitude.  Every case prints what it measured."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import dmatmul_ref as dr
from kind_tools import dev, ops  # noqa: F401  (ops: the module's fixture)
from test_framed_gpu import F64
from test_kmatmul_gpu import CROSS
from test_sparse_gpu import DEEP_D, DEEP_MODELS, KMODELS, _hp, spec_for

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def dcase(name, nr, nc, nrhs, d, same=False):
    """Inputs, the longdouble product, its scale, the float64 restatement and its own dK error, computed once per case.  same: Xc is
    Xr's buffer (nc == nr)."""
    terms = KMODELS[name]
    rng = np.random.default_rng(100000 * nrhs + 1000 * nr + 10 * nc + d)
    hp = _hp(terms, d, rng)
    xr = rng.random((nr, d))
    xc = xr if same else rng.random((nc, d))
    v = rng.standard_normal((nc, nrhs))
    ref, scale = dr.matmul_dx(terms, hp, xr, xc, v, np.longdouble)
    assert ref.dtype == np.longdouble
    ref64, _ = dr.matmul_dx(terms, hp, xr, xc, v)
    return terms, hp, xr, xc, v, ref, np.asarray(scale, np.float64), ref64, dr.own_dk(terms, hp, xr, xc)


def bound_of(own, nc):
    return 16 * own + (nc + 2) * 2.0 ** -53


def judge(label, got, ref, scale, ref64, own, nc):
    bound = bound_of(own, nc)
    err = np.asarray(np.abs(got - ref), np.float64)
    safe = np.where(scale > 0, scale, 1.0)
    fig = float(np.max(err / safe))
    mine = float(np.max(np.abs(ref64 - ref) / safe))
    print("%-44s device %.2e  float64 restatement %.2e  own_dK %.2e  (bound %.2e)" % (label, fig, mine, own, bound))
    assert np.isfinite(got).all()
    assert np.all(err <= bound * scale), (label, fig, bound)


def call(ops, terms, hp, xr, xc, v, same=False):
    d = xr.shape[1]
    xrd = dev(xr)
    out = ops.kernel_matmul_dx(spec_for(terms, d), dev(hp), xrd, xrd if same else dev(xc), dev(v))
    torch.cuda.synchronize()
    return out.cpu().numpy()


# every model and shape at d = 1, 3, 17 (one chunk of four coordinates; three chunks of eight in DMAX 32), then d = 5, 9, 33 (DMAX 8, 16
# and 64: one, two and five chunks, the last with its opt-in LDS size) at one ragged two-by-three-tile shape with two panels
GRID = [s + (d, name) for name in sorted(KMODELS) for d in (1, 3, 17) for s in CROSS]
GRID += [(70, 150, 20, d, name) for d in DEEP_D for name in DEEP_MODELS]


@pytest.mark.parametrize("nr,nc,nrhs,d,name", GRID, ids=["-".join(str(v) for v in c) for c in GRID])
def test_against_the_restatement(ops, nr, nc, nrhs, d, name):
    terms, hp, xr, xc, v, ref, scale, ref64, own = dcase(name, nr, nc, nrhs, d)
    got = call(ops, terms, hp, xr, xc, v)
    assert got.shape == (nr, d, nrhs)
    judge("%s %dx%d nrhs=%d d=%d" % (name, nr, nc, nrhs, d), got, ref, scale, ref64, own, nc)


@pytest.mark.parametrize("name", ["m12", "se+m52", "se*per"])
def test_the_column_points_may_be_the_row_points(ops, name):
    """Xc the same buffer as Xr: every row meets itself at r = 0, where the smooth kinds' derivative is 0 and Matern-1/2's pair
    contributes 0 by convention (the restatement's)."""
    terms, hp, xr, xc, v, ref, scale, ref64, own = dcase(name, 130, 130, 5, 3, same=True)
    got = call(ops, terms, hp, xr, xc, v, same=True)
    judge("%s 130 points against themselves" % name, got, ref, scale, ref64, own, 130)


def test_points_far_from_the_origin_lose_nothing(ops):
    """Points c + m 2^-10 with c = 2^20: exactly representable, so every difference is exact and the output must meet the SAME bound
    against the reference of the unshifted points -- what direct differences buy (an expanded form would lose 2^20 / 2^-10 ulps)."""
    name, nr, nc, nrhs, d = "se+m52", 70, 150, 5, 3
    terms = KMODELS[name]
    rng = np.random.default_rng(77)
    hp = _hp(terms, d, rng)
    xr = rng.integers(0, 1024, (nr, d)) * 2.0 ** -10
    xc = rng.integers(0, 1024, (nc, d)) * 2.0 ** -10
    v = rng.standard_normal((nc, nrhs))
    ref, scale = dr.matmul_dx(terms, hp, xr, xc, v, np.longdouble)
    ref64, _ = dr.matmul_dx(terms, hp, xr, xc, v)
    own = dr.own_dk(terms, hp, xr, xc)
    c = 2.0 ** 20
    assert np.array_equal((xr + c) - c, xr) and np.array_equal((xc + c) - c, xc)
    got = call(ops, terms, hp, xr + c, xc + c, v)
    judge("%s shifted by 2^20" % name, got, ref, np.asarray(scale, np.float64), ref64, own, nc)


def test_the_long_row_case_is_split_into_column_segments(ops):
    assert ops.kernel_matmul_dx_worksize(5, 5000, 3, 2) > 0 and ops.kernel_matmul_dx_worksize(300, 1, 3, 5) == 0
    for bad in ((-1, 5, 3, 2), (5, -1, 3, 2), (5, 5, -3, 2), (5, 5, 3, -2)):
        assert ops.kernel_matmul_dx_worksize(*bad) == -1


def test_a_vector_counts_as_one_column(ops):
    terms, hp, xr, xc, v, *_ = dcase("se+wn", 70, 150, 1, 3)
    got = call(ops, terms, hp, xr, xc, v[:, 0])
    assert got.shape == (70, 3)
    assert got.tobytes() == call(ops, terms, hp, xr, xc, v)[:, :, 0].tobytes()


@pytest.mark.parametrize("nr,nc,nrhs,d", [(130, 70, 33, 3), (5, 5000, 2, 3), (70, 150, 1, 17)])
def test_two_calls_are_bit_equal_and_a_nan_reaches_what_it_enters(ops, nr, nc, nrhs, d):
    terms, hp, xr, xc, v, *_ = dcase("se+m52", nr, nc, nrhs, d)
    a, b = (call(ops, terms, hp, xr, xc, v) for _ in range(2))
    assert a.tobytes() == b.tobytes()
    col = min(1, nrhs - 1)
    vn = v.copy()
    vn[nc // 2, col] = np.nan                             # one entry of V: its column of every row and coordinate, and no other
    got = call(ops, terms, hp, xr, xc, vn)
    assert np.isnan(got[:, :, col]).all() and np.array_equal(np.delete(got, col, axis=2), np.delete(a, col, axis=2))
    xn = xr.copy()
    xn[nr - 1, 0] = np.nan                                # one row point: its row, every coordinate and column
    got = call(ops, terms, hp, xn, xc, v)
    assert np.isnan(got[nr - 1]).all() and np.array_equal(got[:nr - 1], a[:nr - 1])


def test_empty_shapes(ops):
    terms, hp, xr, xc, v, *_ = dcase("se+wn", 70, 150, 1, 3)
    spec, hpd = spec_for(terms, 3), dev(hp)
    empty = lambda *s: torch.empty(*s, dtype=F64, device="cuda")      # noqa: E731
    out = ops.kernel_matmul_dx(spec, hpd, dev(xr), empty(0, 3), empty(0, 4), out=torch.full((70, 3, 4), 7.25, dtype=F64, device="cuda"))
    assert bool((out == 0).all())                                      # an empty sum writes zeros
    assert ops.kernel_matmul_dx(spec, hpd, empty(0, 3), dev(xc), dev(v)).shape == (0, 3, 1)
    assert ops.kernel_matmul_dx(spec, hpd, dev(xr), dev(xc), empty(150, 0)).shape == (70, 3, 0)
    torch.cuda.synchronize()


def test_refusals_carry_a_text_and_enqueue_nothing(ops):
    terms, hp, xr, xc, v, *_ = dcase("se+wn", 70, 150, 1, 3)
    lib, d = ops.lib, 3
    out = torch.full((70, 3, 1), 7.25, dtype=F64, device="cuda")
    hpd, xrd, xcd, vd = dev(hp), dev(xr), dev(xc), dev(v)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    q = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    good = spec_for(terms, d)

    def rc(spec=good, dtype=0, d_=d, nr=70, xc_=q(xcd), ldv=1, ldo=3, ldk=1):
        return lib.pg_kernel_matmul_dx(ops.h, dtype, C.byref(spec), q(hpd), q(xrd), d, nr, xc_, d, 150, d_, q(vd), ldv, 1, q(out), ldo, ldk,
                                       C.c_void_p(0), st)

    sqdist = spec_for(terms, d)
    sqdist.kind[0] = 2                                                 # PG_KIND_SQDIST
    assert rc(dtype=1) != 0 and b"float64 only" in lib.pg_last_error()
    assert rc(spec=sqdist) != 0 and b"unknown kernel kind 2" in lib.pg_last_error()
    assert rc(xc_=C.c_void_p(0)) == -1 and b"cross form only" in lib.pg_last_error()
    assert rc(d_=0) != 0 and b"PG_MAX_DIM" in lib.pg_last_error()
    assert rc(d_=65) != 0 and rc(nr=-1) != 0 and rc(ldv=0) != 0 and rc(ldk=0) != 0
    assert rc(ldo=2) != 0 and b"ldo >= d * ldk" in lib.pg_last_error()
    work_needed = lib.pg_kernel_matmul_dx(ops.h, 0, C.byref(good), q(hpd), q(xrd), d, 5, q(dev(np.zeros((5000, 3)))), d, 5000, d,
                                          q(dev(np.zeros((5000, 1)))), 1, 1, q(out), 3, 1, C.c_void_p(0), st)
    assert work_needed != 0 and b"workspace" in lib.pg_last_error()
    with pytest.raises(ValueError, match="cross form only"):
        ops.kernel_matmul_dx(good, hpd, xrd, None, vd)
    torch.cuda.synchronize()
    assert bool((out == 7.25).all())
    assert rc() == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.25).any())
