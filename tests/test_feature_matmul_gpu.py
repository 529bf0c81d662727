"""pg_feature_matmul on the MI355X: OUT = Phi(X) W for random Fourier features against the NumPy restatement (tests/feature_ref.py),
on framed operands, for reproducibility, NaN propagation, empty shapes and refusals.

Tolerance, per entry and derived, never fitted: with S_ic = sum_f |W_fc| the device may miss the np.longdouble product by
(16 own + (nf + 2) 2^-53) S_ic.  own is the largest ABSOLUTE float64-vs-longdouble difference of the restatement's Phi entries in that
case, floored at 2^-53 (the project's 16 x kernel yardstick; the errors of a cosine are absolute -- the argument's rounding moves it by
that much whatever its value -- so the scale is not |Phi W|); the second term is the any-order bound of a sum of nf products.  A
dropped or doubled feature tile misses it by orders of magnitude.  Every case prints what it measured."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import feature_ref as fr
from kind_tools import dev, ops  # noqa: F401  (ops: the module's fixture)
from test_framed_gpu import F64, ok, p, run

pytestmark = pytest.mark.gpu

# one panel, a full panel, two panels, two blocks of 32; segments and the fold; more than one row tile with few features; the least
SHAPES = [(70, 150, 1), (70, 150, 16), (70, 150, 17), (70, 150, 33), (5, 5000, 2), (257, 17, 4), (1, 1, 1)]
DIMS = [1, 3, 17, 33]            # the register ladder: DMAX 4, 4, 32, 64
MORE = [(70, 150, 17, 7), (5, 5000, 2, 7), (70, 150, 17, 12), (5, 5000, 2, 12)]      # ... and its steps DMAX 8 and 16
MORE += [(70, 150, 17, 5), (70, 150, 17, 9)]      # d = 5, 9 as the covariance kernels' tests have them (d = 33 at this shape: DIMS)


@functools.lru_cache(maxsize=None)
def fcase(nr, nf, nrhs, d):
    """Inputs, the longdouble product, its scale and the restatement's own Phi error, computed once per case."""
    rng = np.random.default_rng(100000 * nrhs + 1000 * nr + 10 * nf + d)
    x = 4.0 * rng.random((nr, d)) - 2.0
    nu = 0.6 * rng.standard_normal((nf, d))
    u = rng.random(nf) - 0.5
    w = rng.standard_normal((nf, nrhs))
    ref, scale = fr.matmul(x, nu, u, w, np.longdouble)
    assert ref.dtype == np.longdouble
    ref64, _ = fr.matmul(x, nu, u, w)
    return x, nu, u, w, ref, np.asarray(scale, np.float64), ref64, fr.own_phi(x, nu, u)


def judge(label, got, ref, scale, ref64, own, nf):
    bound = 16 * own + (nf + 2) * 2.0 ** -53
    err = np.asarray(np.abs(got - ref), np.float64)
    fig = float(np.max(err / scale))
    mine = float(np.max(np.abs(ref64 - ref) / scale))
    print("%-34s device %.2e  float64 restatement %.2e  own %.2e  (bound %.2e)" % (label, fig, mine, own, bound))
    assert np.isfinite(got).all()
    assert np.all(err <= bound * scale), (label, fig, bound)


def call(ops, x, nu, u, w):
    out = ops.feature_matmul(dev(x), dev(nu), dev(u), dev(w))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("nr,nf,nrhs,d", [s + (d,) for d in DIMS for s in SHAPES] + MORE)
def test_against_the_restatement(ops, nr, nf, nrhs, d):
    x, nu, u, w, ref, scale, ref64, own = fcase(nr, nf, nrhs, d)
    got = call(ops, x, nu, u, w)
    assert got.shape == (nr, nrhs)
    judge("%dx%d nrhs=%d d=%d" % (nr, nf, nrhs, d), got, ref, scale, ref64, own, nf)


def test_the_few_rows_case_is_split_into_feature_segments(ops):
    assert ops.feature_matmul_worksize(5, 5000, 2) > 0 and ops.feature_matmul_worksize(300, 1, 5) == 0
    assert ops.feature_matmul_worksize(-1, 5, 2) == -1 and ops.feature_matmul_worksize(5, -1, 2) == -1 and ops.feature_matmul_worksize(5, 5, -2) == -1


def test_a_vector_counts_as_one_column(ops):
    x, nu, u, w, *_ = fcase(70, 150, 1, 3)
    got = call(ops, x, nu, u, w[:, 0])
    assert got.shape == (70,)
    assert got.tobytes() == call(ops, x, nu, u, w)[:, 0].tobytes()


@pytest.mark.parametrize("nr,nf,nrhs", [(70, 150, 33), (5, 5000, 2)])
def test_two_calls_are_bit_equal_and_a_nan_reaches_what_it_enters(ops, nr, nf, nrhs):
    x, nu, u, w, *_ = fcase(nr, nf, nrhs, 3)
    a, b = (call(ops, x, nu, u, w) for _ in range(2))
    assert a.tobytes() == b.tobytes()
    wn = w.copy()
    wn[nf // 2, 1] = np.nan                               # one entry of W: its column of OUT, and no other
    got = call(ops, x, nu, u, wn)
    assert np.isnan(got[:, 1]).all() and np.array_equal(np.delete(got, 1, axis=1), np.delete(a, 1, axis=1))
    xn = x.copy()
    xn[nr - 1, 0] = np.nan                                # one row point: its row
    got = call(ops, xn, nu, u, w)
    assert np.isnan(got[nr - 1]).all() and np.array_equal(got[:nr - 1], a[:nr - 1])
    nn = nu.copy()
    nn[nf - 1, 2] = np.nan                                # one frequency: every entry sums over it
    assert np.isnan(call(ops, x, nn, u, w)).all()
    un = u.copy()
    un[0] = np.nan                                        # one phase: likewise
    assert np.isnan(call(ops, x, nu, un, w)).all()


def test_phases_zero_and_minus_a_quarter_are_cosine_and_sine(ops):
    """W = I picks the features themselves: phase 0 gives cos(2 pi x . nu), phase -1/4 sin(2 pi x . nu), each to the bound of one term."""
    rng = np.random.default_rng(5)
    nr, d, nf = 70, 3, 16
    x = 4.0 * rng.random((nr, d)) - 2.0
    nu = np.repeat(0.6 * rng.standard_normal((nf // 2, d)), 2, axis=0)
    u = np.tile([0.0, -0.25], nf // 2)
    got = call(ops, x, nu, u, np.eye(nf))
    arg = 2 * np.pi * (np.asarray(x, np.longdouble) @ np.asarray(nu[0::2], np.longdouble).T)
    own = fr.own_phi(x, nu, u)
    bound = 16 * own + (nf + 2) * 2.0 ** -53
    ec = float(np.max(np.abs(got[:, 0::2] - np.cos(arg))))
    es = float(np.max(np.abs(got[:, 1::2] - np.sin(arg))))
    print("cos %.2e  sin %.2e  own %.2e  (bound %.2e)" % (ec, es, own, bound))
    assert ec <= bound and es <= bound
    assert float(np.max(np.abs(got[:, 0::2] ** 2 + got[:, 1::2] ** 2 - 1.0))) <= 4 * bound


def test_empty_shapes(ops):
    x, nu, u, w, *_ = fcase(70, 150, 1, 3)
    empty = lambda *s: torch.empty(*s, dtype=F64, device="cuda")      # noqa: E731
    out = ops.feature_matmul(dev(x), empty(0, 3), empty(0), empty(0, 4), out=torch.full((70, 4), 7.25, dtype=F64, device="cuda"))
    assert bool((out == 0).all())                                      # an empty sum writes zeros
    assert ops.feature_matmul(empty(0, 3), dev(nu), dev(u), dev(w)).shape == (0, 1)
    assert ops.feature_matmul(dev(x), dev(nu), dev(u), empty(150, 0)).shape == (70, 0)
    torch.cuda.synchronize()


def test_refusals_carry_a_text_and_enqueue_nothing(ops):
    x, nu, u, w, *_ = fcase(70, 150, 1, 3)
    lib, d = ops.lib, 3
    out = torch.full((70, 1), 7.25, dtype=F64, device="cuda")
    xd, nd, ud, wd = dev(x), dev(nu), dev(u), dev(w)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    q = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731

    def rc(dtype=0, d_=d, nr=70, nf=150, nrhs=1, ldx=d, ldn=d, ldw=1, ldo=1):
        return lib.pg_feature_matmul(ops.h, dtype, q(xd), ldx, nr, q(nd), ldn, nf, d_, q(ud), q(wd), ldw, nrhs, q(out), ldo, C.c_void_p(0), st)

    assert rc(dtype=1) != 0 and b"float64 only" in lib.pg_last_error()
    assert rc(d_=0) != 0 and b"PG_MAX_DIM" in lib.pg_last_error()
    assert rc(d_=65) != 0 and b"PG_MAX_DIM" in lib.pg_last_error()
    assert rc(nr=-1) != 0 and rc(nf=-1) != 0 and rc(nrhs=-1) != 0 and rc(ldx=2) != 0 and rc(ldn=2) != 0 and rc(ldw=0) != 0 and rc(ldo=0) != 0
    big_nu, big_u, big_w = dev(np.zeros((5000, 3))), dev(np.zeros(5000)), dev(np.zeros((5000, 1)))
    work_needed = lib.pg_feature_matmul(ops.h, 0, q(xd), d, 5, q(big_nu), d, 5000, d, q(big_u), q(big_w), 1, 1, q(out), 1, C.c_void_p(0), st)
    assert work_needed != 0 and b"workspace" in lib.pg_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.25).all())
    assert rc() == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.25).any())


# ------------------------------------------------------------------------------------------- framed operands
def case_feature(bed, nr, nf, nrhs, d):
    x, nu, u, w, ref, scale, ref64, own = fcase(nr, nf, nrhs, d)
    xf, nf_, uf, wf = bed.put("X", x), bed.put("NU", nu), bed.put("U", u, dtype=F64), bed.put("W", w)
    of = bed.put("OUT", shape=(nr, nrhs), role="out")
    lw = int(bed.lib.pg_feature_matmul_worksize(nr, nf, nrhs))
    work = bed.put("work", shape=(lw,), dtype=F64, role="out", written=np.zeros(lw, bool), scratch=np.ones(lw, bool)) if lw else None
    ok(bed, bed.lib.pg_feature_matmul(bed.h, bed.code, p(xf), xf.ld, nr, p(nf_), nf_.ld, nf, d, p(uf), p(wf), wf.ld, nrhs, p(of), of.ld,
                                      p(work), bed.st()))
    tol = (16 * own + (nf + 2) * 2.0 ** -53) * float(scale.max())
    return [("OUT", np.asarray(ref, np.float64), None, tol + 2.0 ** -53 * float(np.abs(ref64).max()), 0.0)]


@pytest.mark.parametrize("gapset", ["odd", "mixed"])
@pytest.mark.parametrize("nr,nf,nrhs,d", [(3, 600, 5, 3), (257, 150, 17, 5)], ids=["segments", "two-panels"])
def test_feature_matmul_framed(ops, gapset, nr, nf, nrhs, d):
    """Odd gaps on X, NU, W and OUT: everything outside [0, nr) x [0, nrhs) keeps its sentinel, the inputs keep their bits, the
    workspace is used inside its stated size, and the framed call gives the packed call's bits."""
    if nr == 3:
        assert ops.feature_matmul_worksize(nr, nf, nrhs) > 0      # the first case takes the segment path
    run(ops, case_feature, F64, gapset, nr=nr, nf=nf, nrhs=nrhs, d=d)
