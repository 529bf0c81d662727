"""pg_kernel_lowrank_grad on the MI355X: the contraction against a weight U V^T that is never formed, in the cross and the symmetric
form, against the NumPy restatement (tests/lowrank_ref.py) in np.longdouble.

Bound (every test prints what it measured).  Per entry, relative to S_p = sum_ij (sum_t |U_it| |V_jt|) |dk_ij/dtheta_p|:
  16 x own + (r + 2) 2^-53          cross form
  16 x own + (2 r + 2) 2^-53        symmetric form (two chains of matrix instructions make one weight)
own: the float64 restatement's difference from the longdouble one on the same scale, floored at 2^-53.  The second term is the weight:
the restatement rounds W once from an r-term sum of its own order, the device sums r (2 r) products in the matrix pipe's order.  An
accumulating call also rounds grad[p] + sum once (test_sparse_gpu.judge's half-ulp)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import lowrank_ref as lr
from kind_tools import dev, ops  # noqa: F401  (ops: the module's fixture)
from test_framed_gpu import F64, gaps_odd, ok, p, run
from test_sparse_gpu import DEEP_D, DEEP_MODELS, KMODELS, SENT, _hp, spec_for

pytestmark = pytest.mark.gpu

CROSS = [(70, 150, 1), (64, 64, 16), (1, 300, 3), (130, 70, 33), (5, 2000, 2), (70, 150, 64), (70, 150, 0)]
SYM = [(150, 4), (257, 17), (64, 16), (1, 1)]
EPS = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def lcase(name, nr, nc, r, d, sym=False):
    """Inputs, the longdouble reference, the scale S_p and the float64 restatement's own error, computed once per case."""
    terms = KMODELS[name]
    rng = np.random.default_rng(100000 * r + 1000 * nr + 10 * nc + d + (7 if sym else 0))
    hp = _hp(terms, d, rng)
    xr = rng.random((nr, d))
    xc = None if sym else rng.random((nc, d))
    u = rng.standard_normal((nr, r))
    v = rng.standard_normal((nr if sym else nc, r))
    ref = lr.lowrank_grad(terms, hp, xr, xc, u, v, np.longdouble)
    f64 = lr.lowrank_grad(terms, hp, xr, xc, u, v, np.float64)
    scale = lr.scale(terms, hp, xr, xc, u, v)
    mine = lr.mine(terms, d)
    safe = np.where(scale > 0, scale, 1.0)
    own = max(float(np.max((np.abs(f64 - ref) / safe)[mine])), EPS) if mine.any() else EPS
    return terms, hp, xr, xc, u, v, np.asarray(ref, np.float64), ref, scale, mine, own


def call(ops, terms, hp, xr, xc, u, v, accumulate, start):
    d = xr.shape[1]
    grad = dev(start)
    out = ops.kernel_lowrank_grad(spec_for(terms, d), dev(hp), dev(xr), None if xc is None else dev(xc), dev(u), dev(v), grad,
                                  accumulate=accumulate)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def allowed_of(own, r, sym, scale, want=None):
    a = (16 * own + ((2 * r + 2) if sym else (r + 2)) * EPS) * scale
    return a + (EPS * np.abs(want) if want is not None else 0.0)


def judge(label, got, start, accumulate, ref_ld, scale, mine, own, r, sym):
    want = ref_ld + (start if accumulate else 0.0)
    err = np.abs(np.asarray(got, np.longdouble) - want).astype(np.float64)
    allowed = allowed_of(own, r, sym, scale, np.asarray(want, np.float64) if accumulate else None)
    rel = err[mine] / np.where(scale[mine] > 0, scale[mine], 1.0)
    print("%-44s device %.2e  restatement %.2e  (bound %.2e)" % (label, float(rel.max()) if rel.size else 0.0, own,
                                                                 16 * own + ((2 * r + 2) if sym else (r + 2)) * EPS))
    assert np.array_equal(got[~mine], start[~mine]), "entries outside the spec's stationary blocks were touched"
    assert np.all(err[mine] <= allowed[mine]), (label, float(rel.max()), own)


def grid(shapes, deep):
    """Every model, shape and mode at d = 1, 3, 17 (DMAX 4 and 32), then d = 5, 9, 33 (DMAX 8 and 16: the column point held in registers,
    pairs unrolled by two and by one; DMAX 64: the opt-in LDS size) at the one shape `deep` for a plain, a periodic and a product model."""
    g = [s + (d, name, acc) for acc in (False, True) for name in sorted(KMODELS) for d in (1, 3, 17) for s in shapes]
    g += [deep + (d, name, False) for d in DEEP_D for name in DEEP_MODELS]
    return g, ["-".join(str(v) for v in c[:-1]) + ("-acc" if c[-1] else "-set") for c in g]


CROSS_GRID, CROSS_IDS = grid(CROSS, (70, 150, 5))
SYM_GRID, SYM_IDS = grid(SYM, (150, 5))


@pytest.mark.parametrize("nr,nc,r,d,name,accumulate", CROSS_GRID, ids=CROSS_IDS)
def test_cross_form_against_the_restatement(ops, nr, nc, r, d, name, accumulate):
    terms, hp, xr, xc, u, v, ref, ref_ld, scale, mine, own = lcase(name, nr, nc, r, d)
    start = np.full(hp.size, SENT) + np.arange(hp.size)
    got = call(ops, terms, hp, xr, xc, u, v, accumulate, start)
    judge("%s %dx%d r=%d d=%d %s" % (name, nr, nc, r, d, "acc" if accumulate else "set"), got, start, accumulate, ref_ld, scale, mine, own, r,
          False)


@pytest.mark.parametrize("n,r,d,name,accumulate", SYM_GRID, ids=SYM_IDS)
def test_symmetric_form_against_the_restatement(ops, n, r, d, name, accumulate):
    terms, hp, xr, _, u, v, ref, ref_ld, scale, mine, own = lcase(name, n, n, r, d, sym=True)
    start = np.full(hp.size, SENT) + np.arange(hp.size)
    got = call(ops, terms, hp, xr, None, u, v, accumulate, start)
    judge("%s sym n=%d r=%d d=%d %s" % (name, n, r, d, "acc" if accumulate else "set"), got, start, accumulate, ref_ld, scale, mine, own, r,
          True)


@pytest.mark.parametrize("name", sorted(KMODELS))
@pytest.mark.parametrize("n,r", [(150, 4), (257, 17)])
def test_the_forms_agree(ops, n, r, name):
    """The symmetric form against the cross form on Xc = Xr, against pg_kernel_cross_grad on the materialised W, and against itself
    with U and V exchanged: each within twice the bound."""
    d = 3
    terms, hp, xr, _, u, v, ref, ref_ld, scale, mine, own = lcase(name, n, n, r, d, sym=True)
    start = np.full(hp.size, SENT)
    sym = call(ops, terms, hp, xr, None, u, v, False, start)
    cross = call(ops, terms, hp, xr, xr, u, v, False, start)
    swapped = call(ops, terms, hp, xr, None, v, u, False, start)
    grad = dev(start)
    ops.kernel_cross_grad(spec_for(terms, d), dev(hp), dev(xr), dev(xr), dev(u @ v.T), grad)
    torch.cuda.synchronize()
    dense = grad.cpu().numpy()
    bound = 2 * allowed_of(own, r, True, scale)
    for label, other in (("cross form", cross), ("cross_grad on W", dense), ("U and V exchanged", swapped)):
        diff = np.abs(sym - other)
        print("%-8s n=%d r=%d symmetric form - %-18s %.2e of S_p (bound %.2e)" % (name, n, r, label, float(np.max(diff[mine] / scale[mine])),
                                                                                  2 * (16 * own + (2 * r + 2) * EPS)))
        assert np.all(diff[mine] <= bound[mine]) and np.array_equal(other[~mine], start[~mine])


def test_two_calls_are_bit_equal(ops):
    for sym in (False, True):
        terms, hp, xr, xc, u, v, *_ = lcase("se+m52", 130, 130 if sym else 70, 33, 3, sym=sym)
        start = np.full(hp.size, SENT)
        a, b = (call(ops, terms, hp, xr, xc, u, v, False, start) for _ in range(2))
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("sym", [False, True], ids=["cross", "sym"])
def test_a_nan_reaches_the_entries_it_enters(ops, sym):
    terms, hp, xr, xc, u, v, ref, ref_ld, scale, mine, own = lcase("se+m52", 130, 130 if sym else 70, 33, 3, sym=sym)
    start = np.full(hp.size, SENT)
    ncol = xr.shape[0] if sym else xc.shape[0]
    for what in ("row point", "column point", "U", "V"):
        a = {"xr": xr.copy(), "xc": None if sym else xc.copy(), "u": u.copy(), "v": v.copy()}
        if what == "row point":
            a["xr"][67, 1] = np.nan
        elif what == "column point":
            (a["xr"] if sym else a["xc"])[ncol - 1, 2] = np.nan
        elif what == "U":
            a["u"][129, 32] = np.nan
        else:
            a["v"][ncol - 3, 0] = np.nan
        got = call(ops, terms, hp, a["xr"], a["xc"], a["u"], a["v"], False, start)
        print("NaN in a %-12s -> %d of %d entries NaN" % (what, int(np.isnan(got[mine]).sum()), int(mine.sum())))
        assert np.isnan(got[mine]).all() and np.array_equal(got[~mine], start[~mine])
    # a NaN in one component's parameter: the other component's entries stay finite (and right)
    masks = lr.component_masks(terms, 3)
    hpn = hp.copy()
    hpn[np.flatnonzero(masks[1])[1]] = np.nan             # a length scale of the Matern component
    got = call(ops, terms, hpn, xr, xc, u, v, False, start)
    assert np.isnan(got[masks[1]]).all() and np.isfinite(got[masks[0]]).all()
    assert np.all(np.abs(got - ref)[masks[0]] <= allowed_of(own, 33, sym, scale)[masks[0]])


def test_empty_shapes(ops):
    terms = KMODELS["se+wn"]
    d = 3
    hp = _hp(terms, d, np.random.default_rng(0))
    mine = lr.mine(terms, d)
    start = np.full(hp.size, SENT)
    rng = np.random.default_rng(1)
    for nr, nc, r, sym in [(0, 150, 4, False), (70, 0, 4, False), (0, 0, 4, False), (70, 150, 0, False), (0, 0, 4, True), (70, 70, 0, True)]:
        assert ops.kernel_lowrank_grad_worksize(nr, nc, r, hp.size) == 0
        xr, xc, u, v = rng.random((nr, d)), rng.random((nc, d)), rng.random((nr, r)), rng.random((nc, r))
        for accumulate in (False, True):
            got = call(ops, terms, hp, xr, None if sym else xc, u, v, accumulate, start)
            assert np.array_equal(got[mine], start[mine] if accumulate else np.zeros(int(mine.sum()))), (nr, nc, r, sym, accumulate)
            assert np.array_equal(got[~mine], start[~mine])


def test_refusals_before_anything_is_enqueued(ops):
    terms, hp, xr, xc, u, v, *_ = lcase("se+wn", 70, 150, 64, 3)
    lib, d = ops.lib, 3
    grad = dev(np.full(hp.size, SENT))
    xrd, xcd, hpd = dev(xr), dev(xc), dev(hp)
    ud, vd = dev(np.concatenate([u, u[:, :1]], 1)), dev(np.concatenate([v, v[:, :1]], 1))      # 65 columns: r = 65 addresses memory that exists
    work = torch.zeros(ops.kernel_lowrank_grad_worksize(70, 150, 64, hp.size), dtype=F64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    q = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    good = spec_for(terms, d)

    def rc(spec=good, dtype=0, r=64, wk=q(work), ldu=65, nr=70, d_=d):
        return lib.pg_kernel_lowrank_grad(ops.h, dtype, C.byref(spec), q(hpd), q(xrd), d, nr, q(xcd), d, 150, d_, q(ud), ldu, q(vd), 65, r,
                                          q(grad), 0, wk, st)

    sq = spec_for(terms, d)
    sq.kind[0] = 2                                           # PG_KIND_SQDIST
    assert rc(dtype=1) == -1 and b"float64 only" in lib.pg_last_error()
    assert rc(spec=sq) == -1 and b"pg_kernel_lowrank_grad" in lib.pg_last_error()
    assert rc(r=65) == -1 and b"r <= 64" in lib.pg_last_error()
    assert rc(r=-1) == -1 and rc(nr=-1) == -2 and rc(d_=65) == -2 and rc(ldu=63) == -1
    assert rc(wk=C.c_void_p(0)) == -1 and b"workspace" in lib.pg_last_error()
    torch.cuda.synchronize()
    assert bool((grad == SENT).all())
    assert rc() == 0
    torch.cuda.synchronize()
    assert not bool((grad[:4] == SENT).any()) and float(grad[4]) == SENT


# ------------------------------------------------------------------------------------------- framed operands
def case_lowrank_grad(bed, name, nr, nc, r, d, accumulate, sym):
    terms, hp, xr, xc, u, v, ref, ref_ld, scale, mine, own = lcase(name, nr, nc, r, d, sym=sym)
    start = np.full(hp.size, SENT) + np.arange(hp.size)
    xrf, uf, vf = bed.put("Xr", xr), bed.put("U", u), bed.put("V", v)
    xcf = None if sym else bed.put("Xc", xc)
    hf = bed.put("hp", hp, dtype=F64)
    gf = bed.put("grad", start, dtype=F64, role="inout", written=mine)
    lw = int(bed.lib.pg_kernel_lowrank_grad_worksize(nr, nc, r, hp.size))
    assert lw == lr.worksize(nr, nc, r, hp.size) and lw > 0
    work = bed.put("work", shape=(lw,), dtype=F64, role="out", written=np.zeros(lw, bool), scratch=np.ones(lw, bool))
    spec = spec_for(terms, d)
    ok(bed, bed.lib.pg_kernel_lowrank_grad(bed.h, bed.code, C.byref(spec), p(hf), p(xrf), xrf.ld, nr, p(xcf), 0 if sym else xcf.ld, nc, d,
                                           p(uf), uf.ld, p(vf), vf.ld, r, p(gf), int(accumulate), p(work), bed.st()))
    want = ref + (start if accumulate else 0.0)
    tol = float(np.max(allowed_of(own, r, sym, scale, want if accumulate else None)[mine]))
    return [("grad", np.where(mine, want, start), None, tol, 0.0)]


@gaps_odd
@pytest.mark.parametrize("name,nr,nc,r,d,accumulate,sym", [("se+wn", 70, 150, 1, 3, False, False), ("se*per", 130, 70, 33, 3, True, False),
                                                           ("rq", 257, 257, 17, 17, False, True), ("se+m52", 150, 150, 4, 1, True, True)])
def test_lowrank_grad_framed(ops, gapset, name, nr, nc, r, d, accumulate, sym):
    run(ops, case_lowrank_grad, F64, gapset, name=name, nr=nr, nc=nc, r=r, d=d, accumulate=accumulate, sym=sym)
