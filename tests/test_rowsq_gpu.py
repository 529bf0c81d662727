"""pg_kernel_rowsq on the MI355X: OUT[i] = sum_j k(Xr_i, Xc_j)^2 against the np.longdouble restatement (tests/rowsq_ref.py), for
reproducibility, the empty sum, how a NaN travels, on framed operands and for its refusals.

Tolerance, per entry and derived, never fitted (tests/rowsq_ref.py): with S_i = sum_j k_ij^2 the device may miss the longdouble figure
by (32 own_K + (nc + 2) 2^-53) S_i -- tests/test_kmatmul_gpu.py's bound with the value's error doubled by the square.  own_K is the
largest relative float64-vs-longdouble difference of the restatement's K entries in that case, floored at 2^-53.  A dropped or doubled
column tile, or a lost g group of a row, misses it by orders of magnitude.  Every case prints what it measured.

Shapes: (70, 150) two row tiles against three column tiles, both ragged; (5, 5000) the segmented path and its fold; (257, 17) five row
tiles, one short column tile; (64, 64) exactly one tile.  d = 1, 3, 17: the kernel's DMAX 4 and 32."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import matmul_ref as mr
import rowsq_ref as rr
from kind_tools import dev, ops  # noqa: F401  (ops: the module's fixture)
from test_framed_gpu import F64, ok, p, run
from test_sparse_gpu import KMODELS, _hp, spec_for

pytestmark = pytest.mark.gpu

SHAPES = [(70, 150), (5, 5000), (257, 17), (64, 64)]
SENT = 7.25


@functools.lru_cache(maxsize=None)
def rcase(name, nr, nc, d):
    """Inputs, the longdouble figure, the float64 restatement's and the restatement's own K error, computed once per case."""
    terms = KMODELS[name]
    rng = np.random.default_rng(1000 * nr + 10 * nc + d)
    hp = _hp(terms, d, rng)
    xr, xc = rng.random((nr, d)), rng.random((nc, d))
    ref = rr.rowsq(terms, hp, xr, xc, np.longdouble)
    assert ref.dtype == np.longdouble
    return terms, hp, xr, xc, ref, rr.rowsq(terms, hp, xr, xc), mr.own_k(terms, hp, xr, xc)


def call(ops, terms, hp, xr, xc, out=None):
    d = xr.shape[1]
    xcd = dev(xc) if xc.shape[0] else torch.empty((0, d), dtype=F64, device="cuda")
    out = ops.kernel_rowsq(spec_for(terms, d), dev(hp), dev(xr), xcd, out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


GRID = [s + (d, name) for name in sorted(KMODELS) for d in (1, 3, 17) for s in SHAPES]


@pytest.mark.parametrize("nr,nc,d,name", GRID, ids=["-".join(str(v) for v in c) for c in GRID])
def test_against_the_restatement(ops, nr, nc, d, name):
    terms, hp, xr, xc, ref, ref64, own = rcase(name, nr, nc, d)
    got = call(ops, terms, hp, xr, xc)
    assert got.shape == (nr,)
    bound = rr.bound_of(own, nc)
    err = np.asarray(np.abs(got - ref), np.float64)
    scale = np.asarray(ref, np.float64)
    print("%-8s %4dx%-4d d=%-2d device %.2e  float64 restatement %.2e  own_K %.2e  (bound %.2e)"
          % (name, nr, nc, d, float(np.max(err / scale)), float(np.max(np.abs(ref64 - ref) / ref)), own, bound))
    assert np.isfinite(got).all()
    assert np.all(err <= bound * scale)


def test_the_long_row_case_is_split_into_column_segments(ops):
    assert ops.kernel_rowsq_worksize(5, 5000) > 0 and ops.kernel_rowsq_worksize(257, 17) == 0
    assert ops.kernel_rowsq_worksize(-1, 5) == -1 and ops.kernel_rowsq_worksize(5, -1) == -1


@pytest.mark.parametrize("nr,nc", [(70, 150), (5, 5000)])
def test_two_calls_are_bit_equal_and_a_nan_reaches_what_it_enters(ops, nr, nc):
    terms, hp, xr, xc, *_ = rcase("se+m52", nr, nc, 3)
    a, b = (call(ops, terms, hp, xr, xc) for _ in range(2))
    assert a.tobytes() == b.tobytes()
    xn = xr.copy()
    xn[nr - 1, 0] = np.nan                                # one row point: its entry, and no other
    got = call(ops, terms, hp, xn, xc)
    assert np.isnan(got[nr - 1]) and got[:nr - 1].tobytes() == a[:nr - 1].tobytes()
    xn = xc.copy()
    xn[nc - 1, 2] = np.nan                                # one column point: every row sums over it
    assert np.isnan(call(ops, terms, hp, xr, xn)).all()


def test_an_empty_sum_writes_zeros(ops):
    terms, hp, xr, xc, *_ = rcase("se+wn", 70, 150, 3)
    out = torch.full((70,), SENT, dtype=F64, device="cuda")
    got = call(ops, terms, hp, xr, xc[:0], out=out)
    assert got.shape == (70,) and not got.any()
    xn = xr.copy()
    xn[3, 1] = np.nan                                     # no pair exists: a NaN row point enters nothing
    assert not call(ops, terms, hp, xn, xc[:0]).any()
    assert ops.kernel_rowsq(spec_for(terms, 3), dev(hp), torch.empty((0, 3), dtype=F64, device="cuda"), dev(xc)).shape == (0,)
    torch.cuda.synchronize()


def test_a_strided_out_is_written_at_its_stride(ops):
    terms, hp, xr, xc, *_ = rcase("se+wn", 70, 150, 3)
    buf = torch.full((70, 3), SENT, dtype=F64, device="cuda")
    got = call(ops, terms, hp, xr, xc, out=buf[:, 1])
    assert got.tobytes() == call(ops, terms, hp, xr, xc).tobytes()
    assert bool((buf[:, 0] == SENT).all()) and bool((buf[:, 2] == SENT).all())


def test_refusals_carry_a_text_and_enqueue_nothing(ops):
    terms, hp, xr, xc, *_ = rcase("se+wn", 70, 150, 3)
    lib, d = ops.lib, 3
    out = torch.full((70,), SENT, dtype=F64, device="cuda")
    hpd, xrd, xcd = dev(hp), dev(xr), dev(xc)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    q = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    good = spec_for(terms, d)

    def rc(spec=good, dtype=0, d_=d, nr=70, ldo=1, xc_=q(xcd)):
        return lib.pg_kernel_rowsq(ops.h, dtype, C.byref(spec), q(hpd), q(xrd), d, nr, xc_, d, 150, d_, q(out), ldo, C.c_void_p(0), st)

    sqdist = spec_for(terms, d)
    sqdist.kind[0] = 2                                                 # PG_KIND_SQDIST
    assert rc(dtype=1) < 0 and b"float64 only" in lib.pg_last_error()              # PG_F32
    assert rc(spec=sqdist) < 0 and b"unknown kernel kind 2" in lib.pg_last_error()
    assert rc(d_=0) < 0 and b"PG_MAX_DIM" in lib.pg_last_error()
    assert rc(d_=65) < 0 and b"PG_MAX_DIM" in lib.pg_last_error()
    assert rc(nr=-1) < 0 and rc(ldo=0) < 0
    assert rc(xc_=C.c_void_p(0)) < 0 and b"cross form only" in lib.pg_last_error()
    big = dev(np.zeros((5000, 3)))
    work_needed = lib.pg_kernel_rowsq(ops.h, 0, C.byref(good), q(hpd), q(xrd), d, 5, q(big), d, 5000, d, q(out), 1, C.c_void_p(0), st)
    assert work_needed < 0 and b"workspace" in lib.pg_last_error()
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
    assert rc() == 0
    torch.cuda.synchronize()
    assert not bool((out == SENT).any())


# ------------------------------------------------------------------------------------------- framed operands
def case_rowsq(bed, name, nr, nc, d):
    terms, hp, xr, xc, ref, ref64, own = rcase(name, nr, nc, d)
    xrf, xcf = bed.put("Xr", xr), bed.put("Xc", xc)
    hf = bed.put("hp", hp, dtype=F64)
    of = bed.put("OUT", shape=(nr, 1), role="out")                    # one column at ld = 1 + gap: the gap keeps its sentinel
    lw = int(bed.lib.pg_kernel_rowsq_worksize(nr, nc))
    work = bed.put("work", shape=(lw,), dtype=F64, role="out", written=np.zeros(lw, bool), scratch=np.ones(lw, bool)) if lw else None
    assert not bed.framed or (of.ld > 1 and xrf.ld > d and xcf.ld > d)
    spec = spec_for(terms, d)
    ok(bed, bed.lib.pg_kernel_rowsq(bed.h, bed.code, C.byref(spec), p(hf), p(xrf), xrf.ld, nr, p(xcf), xcf.ld, nc, d, p(of), of.ld, p(work),
                                    bed.st()))
    tol = (rr.bound_of(own, nc) + 2.0 ** -53) * float(np.max(ref))    # (the reference, rounded to float64)
    return [("OUT", np.asarray(ref, np.float64)[:, None], None, tol, 0.0)]


@pytest.mark.parametrize("gapset", ["odd", "mixed"])
@pytest.mark.parametrize("name,nr,nc,d", [("se*per", 3, 600, 3), ("se+wn", 257, 70, 3)], ids=["segments", "plain"])
def test_rowsq_framed(ops, gapset, name, nr, nc, d):
    """Odd gaps on Xr, Xc and OUT: everything outside the nr entries keeps its sentinel, the inputs keep their bits, the workspace is
    used inside its stated size, and the framed call gives the packed call's bits."""
    assert (ops.kernel_rowsq_worksize(nr, nc) > 0) == (nr == 3)       # the first case takes the segment path
    run(ops, case_rowsq, F64, gapset, name=name, nr=nr, nc=nc, d=d)
