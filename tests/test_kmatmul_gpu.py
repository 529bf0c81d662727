"""pg_kernel_matmul on the MI355X: OUT = k(Xr, Xc) V (and the symmetric operator with its shift) against the NumPy restatement
(tests/matmul_ref.py), on framed operands, for reproducibility, empty shapes and refusals.

Tolerance, per entry and derived, never fitted: with S_ic = sum_j |K_ij V_jc| (+ |shift V_ic|) the device may miss the
np.longdouble product by (16 own_K + (nc + 2) 2^-53) S_ic.  own_K is the largest relative float64-vs-longdouble difference of the
restatement's K entries in that case, floored at 2^-53 (the project's 16 x kernel yardstick); the second term is the any-order bound of
a sum of nc products (plus the shift's product and sum).  A dropped or doubled column tile misses it by orders of magnitude.  Every
case prints what it measured."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import matmul_ref as mr
from kind_tools import dev, ops  # noqa: F401  (ops: the module's fixture)
from test_framed_gpu import F64, ok, p, run
from test_sparse_gpu import DEEP_D, DEEP_MODELS, KMODELS, _hp, spec_for

pytestmark = pytest.mark.gpu

CROSS = [(70, 150, 1), (64, 64, 16), (1, 300, 3), (300, 1, 5), (130, 70, 33), (5, 5000, 2)]
SYMMETRIC = [(150, 4), (257, 17)]
JITTER = 1e-6


@functools.lru_cache(maxsize=None)
def mcase(name, nr, nc, nrhs, d, symmetric=False):
    """Inputs, the longdouble product, its scale and the restatement's own K error, computed once per case."""
    terms = KMODELS[name] if not symmetric or "wn" in KMODELS[name] else KMODELS[name] + ["wn"]      # symmetric: sigma_n = 0.3 in every model
    rng = np.random.default_rng(100000 * nrhs + 1000 * nr + 10 * nc + d)
    hp = _hp(terms, d, rng)
    xr = rng.random((nr, d))
    xc = None if symmetric else rng.random((nc, d))
    v = rng.standard_normal((nr if symmetric else nc, nrhs))
    jit = JITTER if symmetric else 0.0
    ref, scale = mr.matmul(terms, hp, xr, xc, v, jit, np.longdouble)
    assert ref.dtype == np.longdouble
    ref64, _ = mr.matmul(terms, hp, xr, xc, v, jit)
    own = mr.own_k(terms, hp, xr, xr if symmetric else xc)
    return terms, hp, xr, xc, v, jit, ref, np.asarray(scale, np.float64), ref64, own


def judge(label, got, ref, scale, ref64, own, nc):
    bound = 16 * own + (nc + 2) * 2.0 ** -53
    err = np.asarray(np.abs(got - ref), np.float64)
    fig = float(np.max(err / scale))
    mine = float(np.max(np.abs(ref64 - ref) / scale))
    print("%-44s device %.2e  float64 restatement %.2e  own_K %.2e  (bound %.2e)" % (label, fig, mine, own, bound))
    assert np.isfinite(got).all()
    assert np.all(err <= bound * scale), (label, fig, bound)


def call(ops, terms, hp, xr, xc, v, jitter):
    d = xr.shape[1]
    out = ops.kernel_matmul(spec_for(terms, d), dev(hp), dev(xr), dev(xc) if xc is not None else None, dev(v), jitter=jitter)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# every model and shape at d = 1, 3, 17 (the kernel's DMAX 4 and 32), then d = 5, 9, 33 (DMAX 8, 16 and 64, the last with its opt-in LDS
# size) at one ragged two-by-three-tile shape with two panels of right-hand sides, for a plain, a periodic and a product model
CROSS_GRID = [s + (d, name) for name in sorted(KMODELS) for d in (1, 3, 17) for s in CROSS]
CROSS_GRID += [(70, 150, 20, d, name) for d in DEEP_D for name in DEEP_MODELS]


@pytest.mark.parametrize("nr,nc,nrhs,d,name", CROSS_GRID, ids=["-".join(str(v) for v in c) for c in CROSS_GRID])
def test_cross_form_against_the_restatement(ops, nr, nc, nrhs, d, name):
    terms, hp, xr, xc, v, jit, ref, scale, ref64, own = mcase(name, nr, nc, nrhs, d)
    got = call(ops, terms, hp, xr, xc, v, jit)
    assert got.shape == (nr, nrhs)
    judge("%s %dx%d nrhs=%d d=%d" % (name, nr, nc, nrhs, d), got, ref, scale, ref64, own, nc)


def test_the_long_row_case_is_split_into_column_segments(ops):
    assert ops.kernel_matmul_worksize(5, 5000, 2) > 0 and ops.kernel_matmul_worksize(300, 1, 5) == 0
    assert ops.kernel_matmul_worksize(-1, 5, 2) == -1 and ops.kernel_matmul_worksize(5, -1, 2) == -1 and ops.kernel_matmul_worksize(5, 5, -2) == -1


@pytest.mark.parametrize("name", sorted(KMODELS))
@pytest.mark.parametrize("d", [1, 3, 17])
@pytest.mark.parametrize("n,nrhs", SYMMETRIC)
def test_symmetric_form_against_the_restatement(ops, n, nrhs, d, name):
    terms, hp, xr, xc, v, jit, ref, scale, ref64, own = mcase(name, n, n, nrhs, d, symmetric=True)
    got = call(ops, terms, hp, xr, None, v, jit)
    judge("%s sym n=%d nrhs=%d d=%d" % (name, n, nrhs, d), got, ref, scale, ref64, own, n)


def test_the_symmetric_form_is_the_matrix_the_symmetric_build_writes(ops):
    """The same operator as pg_kernel_build's symmetric matrix (noise and jitter on the diagonal), to the bound above."""
    from pygpr_amd._ops import pad_to

    terms, hp, xr, xc, v, jit, ref, scale, ref64, own = mcase("se+wn", 150, 150, 4, 3, symmetric=True)
    n, npad = 150, pad_to(150)
    k = ops.empty(npad, npad)
    ops.kernel_build(spec_for(terms, 3), dev(hp), dev(xr), None, k, jitter=jit)
    dense = k[:n, :n].cpu().numpy() @ v
    got = call(ops, terms, hp, xr, None, v, jit)
    assert np.all(np.abs(got - dense) <= 2 * (16 * own + (n + 2) * 2.0 ** -53) * scale)


def test_a_vector_counts_as_one_column(ops):
    terms, hp, xr, xc, v, jit, ref, scale, ref64, own = mcase("se+wn", 70, 150, 1, 3)
    got = call(ops, terms, hp, xr, xc, v[:, 0], jit)
    assert got.shape == (70,)
    assert got.tobytes() == call(ops, terms, hp, xr, xc, v, jit)[:, 0].tobytes()


@pytest.mark.parametrize("nr,nc,nrhs", [(130, 70, 33), (5, 5000, 2)])
def test_two_calls_are_bit_equal_and_a_nan_reaches_what_it_enters(ops, nr, nc, nrhs):
    terms, hp, xr, xc, v, jit, *_ = mcase("se+m52", nr, nc, nrhs, 3)
    a, b = (call(ops, terms, hp, xr, xc, v, jit) for _ in range(2))
    assert a.tobytes() == b.tobytes()
    vn = v.copy()
    vn[nc // 2, 1] = np.nan                               # one entry of V: its column of OUT, and no other
    got = call(ops, terms, hp, xr, xc, vn, jit)
    assert np.isnan(got[:, 1]).all() and np.array_equal(np.delete(got, 1, axis=1), np.delete(a, 1, axis=1))
    xn = xr.copy()
    xn[nr - 1, 0] = np.nan                                # one row point: its row
    got = call(ops, terms, hp, xn, xc, v, jit)
    assert np.isnan(got[nr - 1]).all() and np.array_equal(got[:nr - 1], a[:nr - 1])
    xn = xc.copy()
    xn[nc - 1, 2] = np.nan                                # one column point: every entry sums over it
    assert np.isnan(call(ops, terms, hp, xr, xn, v, jit)).all()


def test_empty_shapes(ops):
    terms, hp, xr, xc, v, jit, *_ = mcase("se+wn", 70, 150, 1, 3)
    spec, hpd = spec_for(terms, 3), dev(hp)
    empty = lambda *s: torch.empty(*s, dtype=F64, device="cuda")      # noqa: E731
    out = ops.kernel_matmul(spec, hpd, dev(xr), empty(0, 3), empty(0, 4), out=torch.full((70, 4), 7.25, dtype=F64, device="cuda"))
    assert bool((out == 0).all())                                      # an empty sum writes zeros
    assert ops.kernel_matmul(spec, hpd, empty(0, 3), dev(xc), dev(v)).shape == (0, 1)
    assert ops.kernel_matmul(spec, hpd, dev(xr), dev(xc), empty(150, 0)).shape == (70, 0)
    assert ops.kernel_matmul(spec, hpd, empty(0, 3), None, empty(0, 2)).shape == (0, 2)
    torch.cuda.synchronize()


def test_refusals_carry_a_text_and_enqueue_nothing(ops):
    terms, hp, xr, xc, v, jit, *_ = mcase("se+wn", 70, 150, 1, 3)
    lib, d = ops.lib, 3
    out = torch.full((70, 1), 7.25, dtype=F64, device="cuda")
    hpd, xrd, xcd, vd = dev(hp), dev(xr), dev(xc), dev(v)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    q = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    good = spec_for(terms, d)

    def rc(spec=good, dtype=0, d_=d, nr=70, ldv=1, ldo=1):
        return lib.pg_kernel_matmul(ops.h, dtype, C.byref(spec), q(hpd), q(xrd), d, nr, q(xcd), d, 150, d_, q(vd), ldv, 1, 0.0, q(out), ldo,
                                    C.c_void_p(0), st)

    sqdist = spec_for(terms, d)
    sqdist.kind[0] = 2                                                 # PG_KIND_SQDIST
    assert rc(dtype=1) != 0 and b"float64 only" in lib.pg_last_error()
    assert rc(spec=sqdist) != 0 and b"unknown kernel kind 2" in lib.pg_last_error()
    assert rc(d_=0) != 0 and b"PG_MAX_DIM" in lib.pg_last_error()
    assert rc(d_=65) != 0 and rc(nr=-1) != 0 and rc(ldv=0) != 0 and rc(ldo=0) != 0
    work_needed = lib.pg_kernel_matmul(ops.h, 0, C.byref(good), q(hpd), q(xrd), d, 5, q(dev(np.zeros((5000, 3)))), d, 5000, d,
                                       q(dev(np.zeros((5000, 1)))), 1, 1, 0.0, q(out), 1, C.c_void_p(0), st)
    assert work_needed != 0 and b"workspace" in lib.pg_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.25).all())
    assert rc() == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.25).any())


# ------------------------------------------------------------------------------------------- framed operands
def case_matmul(bed, name, nr, nc, nrhs, d, symmetric):
    terms, hp, xr, xc, v, jit, ref, scale, ref64, own = mcase(name, nr, nc, nrhs, d, symmetric=symmetric)
    xrf = bed.put("Xr", xr)
    xcf = None if symmetric else bed.put("Xc", xc)
    vf = bed.put("V", v)
    hf = bed.put("hp", hp, dtype=F64)
    of = bed.put("OUT", shape=(nr, nrhs), role="out")
    lw = int(bed.lib.pg_kernel_matmul_worksize(nr, nc, nrhs))
    work = bed.put("work", shape=(lw,), dtype=F64, role="out", written=np.zeros(lw, bool), scratch=np.ones(lw, bool)) if lw else None
    spec = spec_for(terms, d)
    ok(bed, bed.lib.pg_kernel_matmul(bed.h, bed.code, C.byref(spec), p(hf), p(xrf), xrf.ld, nr, p(xcf), xcf.ld if xcf is not None else 0,
                                     0 if symmetric else nc, d, p(vf), vf.ld, nrhs, float(jit), p(of), of.ld, p(work), bed.st()))
    tol = (16 * own + (nc + 2) * 2.0 ** -53) * float(scale.max())
    return [("OUT", np.asarray(ref, np.float64), None, tol + 2.0 ** -53 * float(np.abs(ref64).max()), 0.0)]


@pytest.mark.parametrize("gapset", ["odd", "mixed"])
@pytest.mark.parametrize("name,nr,nc,nrhs,d,symmetric", [("se*per", 3, 600, 5, 3, False), ("se+wn", 257, 257, 17, 3, True)],
                         ids=["cross-segments", "symmetric"])
def test_matmul_framed(ops, gapset, name, nr, nc, nrhs, d, symmetric):
    """Odd gaps on Xr, Xc, V and OUT: everything outside [0, nr) x [0, nrhs) keeps its sentinel, the inputs keep their bits, the
    workspace is used inside its stated size, and the framed call gives the packed call's bits."""
    if not symmetric:
        assert ops.kernel_matmul_worksize(nr, nc, nrhs) > 0      # the framed cross case takes the segment path
    run(ops, case_matmul, F64, gapset, name=name, nr=nr, nc=nc, nrhs=nrhs, d=d, symmetric=symmetric)
