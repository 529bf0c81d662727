"""pg_kernel_lowrank_xgrad on the MI355X: OUT[i][k] (+)= sum_j (U V^T [+ V U^T])_ij dk(Xr_i, Xc_j)/dXr_ik with neither the weight nor dk
formed, in the cross and the symmetric form, against the NumPy restatement (tests/lxgrad_ref.py) in np.longdouble.

Tolerance, per entry and derived, never fitted: tests/test_dmatmul_gpu.py's bound with the rank added to the length of the sum.  With
S_ik = sum_j (sum_t |U_it V_jt| [+ |V_it U_jt|]) |dK_ijk| the device may miss the longdouble contraction by
    (16 own_dK + (nc + R + 2) 2^-53) S_ik,      R = r (cross form), 2 r (symmetric form: two chains of matrix instructions make one weight)
own_dK is the restatement's own float64-vs-longdouble error in dK (dmatmul_ref.own_dk); the second term is the any-order bound of a sum of
nc products whose weights are themselves sums of R products.  An accumulating call also rounds OUT + sum once: half an ulp of the
result.  A dropped or doubled column tile, a chunk written to the wrong place, a pass taken twice or a weight block met by the wrong
pairs misses the bound by orders of magnitude.  Every case prints what it measured."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import dmatmul_ref as dr
import lxgrad_ref as lx
from kind_tools import dev, ops  # noqa: F401  (ops: the module's fixture)
from test_framed_gpu import F64, gaps_odd, ok, p, run
from test_sparse_gpu import DEEP_D, DEEP_MODELS, KMODELS, SENT, _hp, spec_for

pytestmark = pytest.mark.gpu

CROSS = [(70, 150, 1), (64, 64, 16), (1, 300, 3), (130, 70, 33), (70, 150, 64), (70, 150, 0), (5, 5000, 2)]
SYM = [(150, 4), (257, 17), (64, 16), (1, 1)]
EPS = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def xcase(name, nr, nc, r, d, sym=False):
    """Inputs, the longdouble reference, its scale, the float64 restatement and own_dK, computed once per case."""
    terms = KMODELS[name]
    rng = np.random.default_rng(100000 * r + 1000 * nr + 10 * nc + d + (7 if sym else 0))
    hp = _hp(terms, d, rng)
    xr = rng.random((nr, d))
    xc = None if sym else rng.random((nc, d))
    u = rng.standard_normal((nr, r))
    v = rng.standard_normal((nr if sym else nc, r))
    ref, scale = lx.lowrank_xgrad(terms, hp, xr, xc, u, v, np.longdouble)
    assert ref.dtype == np.longdouble
    ref64, _ = lx.lowrank_xgrad(terms, hp, xr, xc, u, v)
    return terms, hp, xr, xc, u, v, ref, np.asarray(scale, np.float64), ref64, dr.own_dk(terms, hp, xr, xr if sym else xc)


def bound_of(own, nc, r, sym):
    return 16 * own + (nc + (2 * r if sym else r) + 2) * EPS


def call(ops, terms, hp, xr, xc, u, v, start=None):
    d = xr.shape[1]
    out = None if start is None else dev(start)
    out = ops.kernel_lowrank_xgrad(spec_for(terms, d), dev(hp), dev(xr), None if xc is None else dev(xc), dev(u), dev(v), out,
                                   accumulate=start is not None)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def judge(label, got, ref, scale, ref64, own, nc, r, sym, start=None):
    bound = bound_of(own, nc, r, sym)
    want = ref if start is None else ref + start
    err = np.asarray(np.abs(got - want), np.float64)
    allowed = bound * scale + (0.0 if start is None else EPS * np.abs(np.asarray(want, np.float64)))
    safe = np.where(scale > 0, scale, 1.0)
    fig = float(np.max(err / safe)) if err.size else 0.0
    mine = float(np.max(np.abs(ref64 - ref) / safe)) if err.size else 0.0
    print("%-48s device %.2e  float64 restatement %.2e  own_dK %.2e  (bound %.2e)" % (label, fig, mine, own, bound))
    assert got.shape == ref.shape and np.isfinite(got).all()
    assert np.all(err <= allowed), (label, fig, bound)


def grid(shapes, deep):
    """Every model and shape at d = 1, 3, 17 (one chunk of four coordinates; three chunks of eight in DMAX 32), then d = 5, 9, 33 (DMAX 8,
    16 and 64: one, two and five chunks, the last with its opt-in LDS size) at the one shape `deep`."""
    g = [s + (d, name) for name in sorted(KMODELS) for d in (1, 3, 17) for s in shapes]
    g += [deep + (d, name) for d in DEEP_D for name in DEEP_MODELS]
    return g, ["-".join(str(v) for v in c) for c in g]


CROSS_GRID, CROSS_IDS = grid(CROSS, (70, 150, 5))
SYM_GRID, SYM_IDS = grid(SYM, (150, 5))


@pytest.mark.parametrize("nr,nc,r,d,name", CROSS_GRID, ids=CROSS_IDS)
def test_cross_form_against_the_restatement(ops, nr, nc, r, d, name):
    terms, hp, xr, xc, u, v, ref, scale, ref64, own = xcase(name, nr, nc, r, d)
    got = call(ops, terms, hp, xr, xc, u, v)
    judge("%s %dx%d r=%d d=%d" % (name, nr, nc, r, d), got, ref, scale, ref64, own, nc, r, False)


@pytest.mark.parametrize("n,r,d,name", SYM_GRID, ids=SYM_IDS)
def test_symmetric_form_against_the_restatement(ops, n, r, d, name):
    terms, hp, xr, _, u, v, ref, scale, ref64, own = xcase(name, n, n, r, d, sym=True)
    got = call(ops, terms, hp, xr, None, u, v)
    judge("%s sym n=%d r=%d d=%d" % (name, n, r, d), got, ref, scale, ref64, own, n, r, True)


@pytest.mark.parametrize("shape", CROSS + SYM, ids=["-".join(str(v) for v in s) for s in CROSS + SYM])
def test_accumulation_adds_to_a_filled_out(ops, shape):
    sym = len(shape) == 2
    nr, nc, r = (shape[0], shape[0], shape[1]) if sym else shape
    name, d = ("se*per", 3) if sym else ("se+m52", 9)
    terms, hp, xr, xc, u, v, ref, scale, ref64, own = xcase(name, nr, nc, r, d, sym=sym)
    start = SENT + np.arange(nr * d, dtype=np.float64).reshape(nr, d) / 16
    got = call(ops, terms, hp, xr, xc, u, v, start)
    judge("%s %s acc d=%d" % (name, shape, d), got, ref, scale, ref64, own, nc, r, sym, start)


def test_the_long_row_case_is_split_into_column_segments(ops):
    ws = ops.kernel_lowrank_xgrad_worksize
    assert ws(5, 5000, 3, 2) > 0 and ws(300, 1, 3, 5) == 0 and ws(70, 150, 3, 33) > 0
    for nr, nc, d, r in [(5, 5000, 3, 2), (70, 150, 17, 64), (257, 257, 9, 17), (5, 5000, 33, 40)]:
        assert ws(nr, nc, d, r) == lx.worksize(nr, nc, d, r)
    for bad in ((-1, 5, 3, 2), (5, -1, 3, 2), (5, 5, -3, 2), (5, 5, 3, -2)):
        assert ws(*bad) == -1


@pytest.mark.parametrize("name", sorted(KMODELS))
@pytest.mark.parametrize("n,r", [(150, 4), (257, 17)])
def test_the_forms_agree(ops, n, r, name):
    """The symmetric form against the cross form called with [U | V], [V | U] and Xc = Xr: the same weight from one chain of 2 r steps
    where the symmetric form has two of r.  Each meets the derived bound, so they differ by at most twice it; not compared bitwise."""
    d = 3
    terms, hp, xr, _, u, v, ref, scale, ref64, own = xcase(name, n, n, r, d, sym=True)
    sym = call(ops, terms, hp, xr, None, u, v)
    cross = call(ops, terms, hp, xr, xr, np.concatenate([u, v], 1), np.concatenate([v, u], 1))
    judge("%s n=%d r=%d cross form on [U|V], [V|U]" % (name, n, r), cross, ref, scale, ref64, own, n, r, True)
    diff = np.abs(sym - cross)
    print("%-8s n=%d r=%d symmetric - cross form %.2e of S" % (name, n, r, float(np.max(diff / np.where(scale > 0, scale, 1.0)))))
    assert np.all(diff <= 2 * bound_of(own, n, r, True) * scale)


def test_points_far_from_the_origin_lose_nothing(ops):
    """Points c + m 2^-10 with c = 2^20: exactly representable, so every difference is exact and the output must meet the SAME bound
    against the reference of the unshifted points."""
    name, nr, nc, r, d = "se+m52", 70, 150, 5, 3
    terms = KMODELS[name]
    rng = np.random.default_rng(77)
    hp = _hp(terms, d, rng)
    xr = rng.integers(0, 1024, (nr, d)) * 2.0 ** -10
    xc = rng.integers(0, 1024, (nc, d)) * 2.0 ** -10
    u, v = rng.standard_normal((nr, r)), rng.standard_normal((nc, r))
    c = 2.0 ** 20
    assert np.array_equal((xr + c) - c, xr) and np.array_equal((xc + c) - c, xc)
    for sym in (False, True):
        vv = rng.standard_normal((nr, r)) if sym else v
        ref, scale = lx.lowrank_xgrad(terms, hp, xr, None if sym else xc, u, vv, np.longdouble)
        ref64, _ = lx.lowrank_xgrad(terms, hp, xr, None if sym else xc, u, vv)
        own = dr.own_dk(terms, hp, xr, xr if sym else xc)
        got = call(ops, terms, hp, xr + c, None if sym else xc + c, u, vv)
        judge("%s shifted by 2^20 %s" % (name, "sym" if sym else "cross"), got, ref, np.asarray(scale, np.float64), ref64, own,
              nr if sym else nc, r, sym)


@pytest.mark.parametrize("nr,nc,r,d,sym", [(130, 70, 33, 3, False), (5, 5000, 2, 3, False), (70, 150, 1, 17, False), (257, 257, 17, 3, True)])
def test_two_calls_are_bit_equal(ops, nr, nc, r, d, sym):
    terms, hp, xr, xc, u, v, *_ = xcase("se+m52", nr, nc, r, d, sym=sym)
    a, b = (call(ops, terms, hp, xr, xc, u, v) for _ in range(2))
    assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("nr,nc,r,d", [(130, 70, 33, 3), (5, 5000, 2, 3), (70, 150, 1, 17)])
def test_a_nan_reaches_what_it_enters(ops, nr, nc, r, d):
    """The cross form, as the header states it: a row point or U[i] its row and no other (the others bit-equal to the clean run), V[j] or a
    column point every row."""
    terms, hp, xr, xc, u, v, *_ = xcase("se+m52", nr, nc, r, d)
    clean = call(ops, terms, hp, xr, xc, u, v)
    row = nr - 1
    for what in ("row point", "U"):
        xn, un = xr.copy(), u.copy()
        if what == "row point":
            xn[row, 0] = np.nan
        else:
            un[row, r - 1] = np.nan
        got = call(ops, terms, hp, xn, xc, un, v)
        assert np.isnan(got[row]).all(), what
        assert np.delete(got, row, axis=0).tobytes() == np.delete(clean, row, axis=0).tobytes(), what
    for what in ("column point", "V"):
        xn, vn = xc.copy(), v.copy()
        if what == "column point":
            xn[nc // 2, d - 1] = np.nan
        else:
            vn[nc - 1, 0] = np.nan
        got = call(ops, terms, hp, xr, xn, u, vn)
        assert np.isnan(got).all(), what


def test_a_nan_in_the_symmetric_form_reaches_every_row(ops):
    terms, hp, xr, _, u, v, *_ = xcase("se+m52", 150, 150, 4, 3, sym=True)
    for what in ("point", "U", "V"):
        xn, un, vn = xr.copy(), u.copy(), v.copy()
        {"point": xn, "U": un, "V": vn}[what][77, 1] = np.nan
        assert np.isnan(call(ops, terms, hp, xn, None, un, vn)).all(), what


def test_empty_shapes(ops):
    terms = KMODELS["se+wn"]
    d = 3
    hp = _hp(terms, d, np.random.default_rng(0))
    rng = np.random.default_rng(1)
    for nr, nc, r, sym in [(70, 0, 4, False), (70, 150, 0, False), (70, 70, 0, True), (0, 150, 4, False), (0, 0, 4, True)]:
        assert ops.kernel_lowrank_xgrad_worksize(nr, nc, d, r) == 0
        xr, xc, u, v = rng.random((nr, d)), rng.random((nc, d)), rng.random((nr, r)), rng.random((nc, r))
        start = np.full((nr, d), SENT)
        got = call(ops, terms, hp, xr, None if sym else xc, u, v)
        assert got.shape == (nr, d) and np.array_equal(got, np.zeros((nr, d))), (nr, nc, r, sym)      # the empty sum writes zeros
        got = call(ops, terms, hp, xr, None if sym else xc, u, v, start)
        assert np.array_equal(got, start), (nr, nc, r, sym)                                         # ... and added, leaves OUT alone


def test_refusals_before_anything_is_enqueued(ops):
    terms, hp, xr, xc, u, v, *_ = xcase("se+wn", 70, 150, 64, 3)
    lib, d = ops.lib, 3
    out = torch.full((70, 3), SENT, dtype=F64, device="cuda")
    xrd, xcd, hpd = dev(xr), dev(xc), dev(hp)
    ud, vd = dev(np.concatenate([u, u[:, :1]], 1)), dev(np.concatenate([v, v[:, :1]], 1))      # 65 columns: r = 65 addresses memory that exists
    work = torch.zeros(ops.kernel_lowrank_xgrad_worksize(70, 150, 3, 64), dtype=F64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    q = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    good = spec_for(terms, d)

    def rc(spec=good, dtype=0, r=64, wk=q(work), ldu=65, nr=70, d_=d, xc_=q(xcd), v_=q(vd), ldo=3):
        return lib.pg_kernel_lowrank_xgrad(ops.h, dtype, C.byref(spec), q(hpd), q(xrd), d, nr, xc_, d, 150, d_, q(ud), ldu, v_, 65, r, q(out),
                                           ldo, 0, wk, st)

    sq = spec_for(terms, d)
    sq.kind[0] = 2                                           # PG_KIND_SQDIST
    assert rc(r=65) == -1 and b"r <= 64" in lib.pg_last_error()
    assert rc(d_=0) == -1 and b"PG_MAX_DIM" in lib.pg_last_error()
    assert rc(dtype=1) == -1 and b"float64 only" in lib.pg_last_error()
    assert rc(spec=sq) == -1 and b"pg_kernel_lowrank_xgrad" in lib.pg_last_error()
    assert rc(xc_=C.c_void_p(0), v_=C.c_void_p(0)) == -1 and b"symmetric form needs V" in lib.pg_last_error()
    assert rc(ldo=2) == -1 and b"ldo >= d" in lib.pg_last_error()
    assert rc(r=-1) == -1 and rc(nr=-1) == -1 and rc(d_=65) == -1 and rc(ldu=63) == -1
    assert rc(wk=C.c_void_p(0)) == -1 and b"workspace" in lib.pg_last_error()
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
    assert rc() == 0
    torch.cuda.synchronize()
    assert not bool((out == SENT).any())


# ------------------------------------------------------------------------------------------- framed operands
def case_lowrank_xgrad(bed, name, nr, nc, r, d, accumulate, sym):
    terms, hp, xr, xc, u, v, ref, scale, ref64, own = xcase(name, nr, nc, r, d, sym=sym)
    start = SENT + np.arange(nr * d, dtype=np.float64).reshape(nr, d) / 16
    xrf, uf, vf = bed.put("Xr", xr), bed.put("U", u), bed.put("V", v)
    xcf = None if sym else bed.put("Xc", xc)
    hf = bed.put("hp", hp, dtype=F64)
    of = bed.put("OUT", start, dtype=F64, role="inout") if accumulate else bed.put("OUT", shape=(nr, d), dtype=F64, role="out")
    lw = int(bed.lib.pg_kernel_lowrank_xgrad_worksize(nr, nc, d, r))
    assert lw == lx.worksize(nr, nc, d, r)
    work = bed.put("work", shape=(lw,), dtype=F64, role="out", written=np.zeros(lw, bool), scratch=np.ones(lw, bool)) if lw else None
    spec = spec_for(terms, d)
    ok(bed, bed.lib.pg_kernel_lowrank_xgrad(bed.h, bed.code, C.byref(spec), p(hf), p(xrf), xrf.ld, nr, p(xcf), 0 if sym else xcf.ld, nc, d,
                                            p(uf), uf.ld, p(vf), vf.ld, r, p(of), of.ld, int(accumulate), p(work), bed.st()))
    want = np.asarray(ref, np.float64) + (start if accumulate else 0.0)
    tol = float(np.max(bound_of(own, nc, r, sym) * scale + (EPS * np.abs(want) if accumulate else 0.0)))
    return [("OUT", want, None, tol, 0.0)]


@gaps_odd
@pytest.mark.parametrize("name,nr,nc,r,d,accumulate,sym", [("se+wn", 5, 5000, 2, 3, False, False), ("rq", 257, 257, 17, 17, False, True),
                                                           ("se*per", 130, 70, 33, 3, True, False)])
def test_lowrank_xgrad_framed(ops, gapset, name, nr, nc, r, d, accumulate, sym):
    """Strided Xr, Xc, U, V and OUT inside guard bands whose every word, the gaps of the rows included, is a quiet NaN: the guards stay
    intact, the inputs unchanged, OUT has the packed call's bits and no NaN."""
    run(ops, case_lowrank_xgrad, F64, gapset, name=name, nr=nr, nc=nc, r=r, d=d, accumulate=accumulate, sym=sym)
