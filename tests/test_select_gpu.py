"""Greedy inducing-point selection on the MI355X: pg_greedy_select through the C ABI (via _ops and on framed operands) and the Python
surface (select_inducing, Sparse_GP.greedy, Sparse_GP.select_inducing) against the NumPy restatement (tests/select_ref.py).

Pivot sequences are NOT compared for equality: the restatement's own float64 and long-double runs disagree on the product model
(two residuals tie exactly at some steps), and on the squared exponential the top two come within 1e-10 kdiag of each other.  The
device's sequence is REPLAYED in the long-double restatement instead, and every choice is judged against the residuals the replay
holds at that step.  Tolerances (none is a guess; every test prints what it measured next to its bound):

  own    the largest difference between the float64 and the long-double replay of the restatement's own pivots on that input, over
         every step's residuals, relative to kdiag
  s      16 max(own, m_max 2^-53) kdiag: the floor term is one rounding per update at magnitude <= kdiag
  a chosen p_j must hold  r_ref[p_j] >= max_i r_ref - s  and  r_ref[p_j] > floor - s;  a stop before m_max needs  max_i r_ref <= floor + s;
  |trace_dev[j] - trace_ref[j]| <= n s;  |resid_dev - resid_ref| <= s entrywise;  step 0 takes index 0;  no index twice.

The model-level tolerance is tests/test_sparse_gpu.py's: 50 x the disagreement of the restatement's dense and Woodbury forms, floored at
1e-10."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import kernel_ref as kr
import pygpr_amd as pg
import select_ref as sel
import sparse_ref as sr
from kind_tools import cov_of, dev, one_spec, ops  # noqa: F401  (ops: the module's fixture)
from pygpr_amd import _lib
from pygpr_amd._ops import JITTER
from test_framed_gpu import F64, GAPSETS, Bed, p
from test_select_cpu import duplicates_case
from test_sparse_gpu import KMODELS, hold

pytestmark = pytest.mark.gpu

SENT = 7.25       # what trace / resid entries the call must not touch hold before it
ISENT = -77       # ... and piv / count


def spec_for(terms, d):
    return one_spec(terms, d, product=any(isinstance(t, tuple) for t in terms))


def _hp(terms, d, rng):
    """sparse_ref.problem's hyper-parameters, the inverse length scales shrunk with the dimension above 3."""
    shrink = np.sqrt(3.0 / d) if d > 3 else 1.0
    hp = []
    for part in kr.flat(terms):
        if part == "wn":
            hp += [0.3]
            continue
        hp += [0.9 + 0.2 * rng.random()] + list((2.5 + 0.6 * rng.random(d)) * shrink)
        hp += [1.5] if part == "rq" else (list(0.7 + 0.3 * rng.random(d)) if part == "per" else [])
    return np.array(hp)


CASE_MODELS = dict(KMODELS, se=["se"])


@functools.lru_cache(maxsize=None)
def case(name, n, m_max, d, special=None):
    """Inputs, the restatement's own pivots and its own error, computed once per case."""
    terms = CASE_MODELS[name]
    rng = np.random.default_rng(100000 * d + 100 * n + m_max)
    if special == "stop":                                  # tests/test_select_cpu.py's early stop
        rng = np.random.default_rng(5)
        x = rng.random((n, d))
        hp = np.array([1.0, 2.5 + 0.6 * rng.random()])
    elif special == "dup":
        hp, x = duplicates_case()
    elif special == "full":
        x, hp = rng.random((n, d)), np.array([1.1, 6.0, 7.0])
    else:
        x = rng.random((n, d))
        hp = _hp(terms, d, rng)
        if special == "nan":
            x[41, 1] = np.nan
    assert x.shape == (n, d) and hp.size == kr.nhp_of(terms, d)
    run = sel.greedy(terms, hp, x, m_max, JITTER)
    own = sel.own_error(terms, hp, x, run.piv)
    return terms, hp, x, run, own


def device_run(ops, terms, hp, x, m_max, floor=JITTER, extra=3):
    """One call through _ops on sentinel-filled outputs `extra` longer than needed: (piv, count, trace, resid, tails untouched)."""
    n, d = x.shape
    piv = torch.full((m_max + extra,), ISENT, dtype=torch.int32, device="cuda")
    count = torch.full((1 + extra,), ISENT, dtype=torch.int32, device="cuda")
    trace = torch.full((m_max + extra,), SENT, dtype=torch.float64, device="cuda")
    resid = torch.full((n + extra,), SENT, dtype=torch.float64, device="cuda")
    xd = dev(x) if n else torch.empty((0, d), dtype=torch.float64, device="cuda")
    ops.greedy_select(spec_for(terms, d), dev(hp), xd, m_max, floor, out=(piv, count, trace, resid))
    torch.cuda.synchronize()
    piv, count, trace, resid = (t.cpu().numpy() for t in (piv, count, trace, resid))
    c = int(count[0])
    assert 0 <= c <= m_max
    clean = bool((piv[c:] == ISENT).all() and (count[1:] == ISENT).all() and (trace[c:] == SENT).all() and (resid[n:] == SENT).all())
    return piv[:c].astype(np.int64), c, trace[:c], resid[:n], clean


def judge(label, terms, hp, x, m_max, floor, own, piv, c, trace, resid, nan_point=None):
    n = x.shape[0]
    rep = sel.replay(terms, hp, x, piv, np.longdouble)
    kd = float(rep.kdiag)
    s = 16 * max(own, m_max * 2.0 ** -53) * kd
    with np.errstate(invalid="ignore"):
        top = np.array([np.nanmax(rep.hist[j]) for j in range(c + 1)], dtype=np.longdouble)
    took = np.array([rep.hist[j][piv[j]] for j in range(c)], dtype=np.longdouble)
    gap = float(np.max(top[:c] - took)) if c else 0.0
    keep = np.ones(n, bool)
    if nan_point is not None:
        keep[nan_point] = False
    e_res = float(np.max(np.abs(resid[keep] - rep.resid[keep]))) if n else 0.0
    e_tr = float(np.max(np.abs(trace - rep.trace))) if (c and nan_point is None) else 0.0
    print("%-34s count %3d/%3d  max - chosen %.2e  resid %.2e (s %.2e)  trace %.2e (n s %.2e)  own %.2e  left %.2e (floor %.1e)" %
          (label, c, m_max, gap, e_res, s, e_tr, n * s, own, float(top[c]), floor))
    assert len(set(piv.tolist())) == c and (c == 0 or piv[0] == 0)
    assert np.all(took >= top[:c] - s) and np.all(took > floor - s), (label, gap)
    if c < m_max:
        assert top[c] <= floor + s, (label, float(top[c]))
    assert e_res <= s and e_tr <= n * s, (label, e_res, e_tr)
    if nan_point is None:
        assert np.isfinite(trace).all() and np.isfinite(resid).all()
    return rep


SHAPES = [(name, 300, 40, 3, None) for name in sorted(KMODELS)] + [
    ("se", 333, 64, 1, "stop"),             # early stop: entries past count keep their sentinel
    ("m12", 257, 257, 2, "full"),           # full rank; a one-point tail past a workgroup pair, an odd n (the last lane's padding)
    ("se", 130, 130, 2, "dup"),             # exact duplicates, stop at the floor
    ("se+m52", 2100, 16, 2, None),          # seventeen workgroups of partials
    ("rq", 700, 90, 17, None),              # d above 16; more than 64 columns: every wave's unrolled body and its tail
    ("se", 1, 1, 1, None),                  # a single point
    ("se*per", 129, 37, 2, None),           # one point past a workgroup, a column count that is no multiple of the unroll
]


@pytest.mark.parametrize("name,n,m_max,d,special", SHAPES)
def test_selection_replays_in_the_restatement(ops, name, n, m_max, d, special):
    terms, hp, x, run, own = case(name, n, m_max, d, special)
    piv, c, trace, resid, clean = device_run(ops, terms, hp, x, m_max)
    judge("%s n=%d m=%d d=%d" % (name if special is None else special, n, m_max, d), terms, hp, x, m_max, JITTER, own, piv, c, trace, resid)
    assert clean, "entries behind count (or behind the outputs) were touched"
    if special == "stop":
        assert c == len(run.piv) == 13
    if special == "full":
        assert c == 257 and np.all(np.abs(resid) <= 2.0 ** -53) and abs(trace[-1]) <= 257 * 2.0 ** -53      # rounding noise squared
    if special == "dup":
        chosen = x[piv]
        assert c < 100 and len(np.unique(chosen, axis=0)) == c       # never a duplicate of a selected point; the floor ended it
    if special is None:
        assert c == m_max


def test_a_higher_floor_stops_sooner(ops):
    terms, hp, x, run, own = case("se+wn", 300, 40, 3, None)
    kd = float(run.kdiag)
    piv, c, trace, resid, clean = device_run(ops, terms, hp, x, 40, floor=0.5 * kd)
    judge("se+wn floor kdiag / 2", terms, hp, x, 40, 0.5 * kd, own, piv, c, trace, resid)
    assert clean and 1 <= c < 40 and c == len(sel.greedy(terms, hp, x, 40, 0.5 * kd).piv)


def test_empty_problems_write_count_alone(ops):
    terms, hp, x, *_ = case("se+wn", 300, 40, 3, None)
    piv, c, trace, resid, clean = device_run(ops, terms, hp, x, 0)
    assert c == 0 and clean and (resid == SENT).all()                  # m_max = 0: not even the residuals
    piv, c, trace, resid, clean = device_run(ops, terms, hp, np.zeros((0, 3)), 0)
    assert c == 0 and clean
    assert ops.greedy_select_worksize(0, 0) == 9 and ops.greedy_select_worksize(3, 4) == -1
    with pytest.raises(ValueError, match="m_max"):
        ops.greedy_select(spec_for(terms, 3), dev(hp), dev(x), 301, JITTER)


def test_two_calls_agree_bitwise(ops):
    terms, hp, x, run, own = case("se*per", 300, 40, 3, None)
    a, b = (device_run(ops, terms, hp, x, 40) for _ in range(2))
    assert a[1] == b[1] and all(u.tobytes() == v.tobytes() for u, v in zip((a[0], a[2], a[3]), (b[0], b[2], b[3])))


def test_a_nan_coordinate_is_never_selected(ops):
    terms, hp, x, run, own = case("se+wn", 300, 40, 3, "nan")
    piv, c, trace, resid, clean = device_run(ops, terms, hp, x, 40)
    assert clean and c == 40 and 41 not in piv
    assert np.isnan(trace).all() and np.isnan(resid[41]) and np.isfinite(np.delete(resid, 41)).all()      # the first trace is the first NaN one
    judge("se+wn, NaN in point 41", terms, hp, x, 40, JITTER, own, piv, c, trace, resid, nan_point=41)


def test_refusals_come_before_anything_is_enqueued(ops):
    terms, hp, x, *_ = case("se+wn", 300, 40, 3, None)
    lib, n, d, m = ops.lib, 300, 3, 40
    piv, count = (torch.full((k,), ISENT, dtype=torch.int32, device="cuda") for k in (m, 1))
    trace, resid = (torch.full((k,), SENT, dtype=torch.float64, device="cuda") for k in (m, n))
    xd, hpd = dev(x), dev(hp)
    work = torch.zeros(ops.greedy_select_worksize(n, m), dtype=torch.float64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    q = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    good = spec_for(terms, d)

    def rc(h=ops.h, dtype=0, spec=good, n_=n, d_=d, m_=m, ldx=d, cnt=None):
        return lib.pg_greedy_select(h, dtype, C.byref(spec) if spec is not None else None, q(hpd), q(xd), ldx, n_, d_, m_, JITTER, q(piv),
                                    q(count) if cnt is None else cnt, q(trace), q(resid), q(work), st)

    sqdist = spec_for(terms, d)
    sqdist.kind[0] = _lib.PG_KIND_SQDIST
    empty = spec_for(terms, d)
    empty.ncomp = 0
    assert rc(dtype=_lib.PG_F32) < 0 and b"float64" in lib.pg_last_error()
    assert rc(d_=0) < 0 and b"PG_MAX_DIM" in lib.pg_last_error()
    assert rc(d_=_lib.PG_MAX_DIM + 1) < 0 and rc(m_=n + 1) < 0 and rc(n_=-1, m_=0) < 0 and rc(m_=-1) < 0
    assert rc(spec=sqdist) < 0 and b"unknown kernel kind" in lib.pg_last_error()
    assert rc(spec=empty) < 0 and b"no stationary component" in lib.pg_last_error()
    assert rc(spec=None) < 0 and rc(h=None) < 0 and rc(ldx=d - 1) < 0 and rc(cnt=C.c_void_p(0)) < 0
    torch.cuda.synchronize()
    assert bool((piv == ISENT).all() and (count == ISENT).all() and (trace == SENT).all() and (resid == SENT).all())
    assert rc() == 0
    torch.cuda.synchronize()
    assert int(count[0]) == 40 and not bool((trace == SENT).any())


def test_a_workspace_at_an_odd_word_gives_the_same_bits(ops):
    """The factor's columns are read 16 bytes at a time: a workspace that starts 8 bytes off a 16-byte boundary is shifted by the one
    word the worksize holds for that, inside the stated size (the word behind it keeps its sentinel)."""
    terms, hp, x, run, own = case("se+m52", 300, 40, 3, None)
    n, d, m = 300, 3, 40
    size = ops.greedy_select_worksize(n, m)
    xd, hpd, spec = dev(x), dev(hp), spec_for(terms, d)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    got = []
    for shift in (0, 1):
        buf = torch.full((size + 4,), SENT, dtype=torch.float64, device="cuda")
        assert buf.data_ptr() % 16 == 0
        piv, count = (torch.full((k,), ISENT, dtype=torch.int32, device="cuda") for k in (m, 1))
        trace, resid = (torch.full((k,), SENT, dtype=torch.float64, device="cuda") for k in (m, n))
        rc = ops.lib.pg_greedy_select(ops.h, 0, C.byref(spec), C.c_void_p(hpd.data_ptr()), C.c_void_p(xd.data_ptr()), d, n, d, m, JITTER,
                                      C.c_void_p(piv.data_ptr()), C.c_void_p(count.data_ptr()), C.c_void_p(trace.data_ptr()),
                                      C.c_void_p(resid.data_ptr()), C.c_void_p(buf.data_ptr() + 8 * shift), st)
        assert rc == 0, ops.lib.pg_last_error().decode()
        torch.cuda.synchronize()
        assert bool((buf[shift + size:] == SENT).all()) and (shift == 0 or float(buf[0]) == SENT)
        got.append(b"".join(t.cpu().numpy().tobytes() for t in (piv, count, trace, resid)))
    assert got[0] == got[1] and int(count[0]) == 40


# ------------------------------------------------------------------------------------------- framed operands
def framed_call(bed, terms, hp, x, m_max, count_ref):
    n, d = x.shape
    xf = bed.put("X", x)
    hf = bed.put("hp", hp, dtype=F64)
    head = np.arange(m_max) < count_ref
    pf = bed.put("piv", shape=(m_max,), dtype=torch.int32, role="out", written=head)
    cf = bed.put("count", shape=(1,), dtype=torch.int32, role="out")
    tf = bed.put("trace", shape=(m_max,), dtype=F64, role="out", written=head)
    rf = bed.put("resid", shape=(n,), dtype=F64, role="out")
    lw = int(bed.lib.pg_greedy_select_worksize(n, m_max))
    assert lw == 1 + m_max * ((n + 1) // 2 * 2) + n + 3 * ((n + 127) // 128) + m_max + 8
    work = bed.put("work", shape=(lw,), dtype=F64, role="out", written=np.zeros(lw, bool), scratch=np.ones(lw, bool))
    spec = spec_for(terms, d)
    rc = bed.lib.pg_greedy_select(bed.h, 0, C.byref(spec), p(hf), p(xf), xf.ld, n, d, m_max, JITTER, p(pf), p(cf), p(tf), p(rf), p(work), bed.st())
    assert rc == 0, bed.lib.pg_last_error().decode()
    return xf.ld


@pytest.mark.parametrize("gapset", GAPSETS + ["odd"])
@pytest.mark.parametrize("name,n,m_max,d,special", [("se", 333, 64, 1, "stop"), ("se*per", 300, 40, 3, None)])
def test_greedy_select_framed(ops, gapset, name, n, m_max, d, special):
    """ldx > d, guard bands around X, hp, piv, count, trace, resid and a workspace of exactly the stated size: inputs unchanged, bands
    intact, the tails past count untouched, the same bits as on packed operands, and the sequence replays."""
    terms, hp, x, run, own = case(name, n, m_max, d, special)
    beds = {}
    for gs in (None, gapset):
        bed = Bed(ops, F64, gs)
        ldx = framed_call(bed, terms, hp, x, m_max, len(run.piv))
        bed.check()                                       # synchronises; the frame checks of every operand
        beds[gs] = bed
        assert gs is None or ldx > d
    out = {}
    for nm in ("piv", "count", "trace", "resid"):
        f, g = beds[gapset].items[nm][0], beds[None].items[nm][0]
        a, b = f.bits(), g.wview.cpu().numpy()
        assert np.array_equal(a, b), "%s: framed and packed calls differ" % nm
        out[nm] = f.view.cpu().numpy()
    c = int(out["count"][0])
    assert c == len(run.piv)
    judge("framed %s %s" % (name if special is None else special, gapset), terms, hp, x, m_max, JITTER, own, out["piv"][:c].astype(np.int64), c,
          out["trace"][:c], out["resid"])


# ------------------------------------------------------------------------------------------- the Python surface and the model
def test_select_inducing_returns_the_c_abis_selection(ops):
    terms, hp, x, run, own = case("se+m52", 2100, 16, 2, None)
    piv, c, trace, resid, _ = device_run(ops, terms, hp, x, 16)
    xt = torch.from_numpy(x)
    res = pg.select_inducing(xt, cov_of(terms), torch.from_numpy(hp), 16)
    assert isinstance(res, pg.Selection) and res.index.dtype == torch.int64 and res.index.device == xt.device
    assert res.index.tolist() == piv.tolist() and res.trace.numpy().tobytes() == trace.tobytes() and res.residual.numpy().tobytes() == resid.tobytes()
    on_dev = pg.select_inducing(xt.cuda(), cov_of(terms), hp, 16, tol=0.5)       # results sit where x sits; tol 0.5: the floor is kdiag / 2
    assert on_dev.index.is_cuda and on_dev.trace.is_cuda and on_dev.residual.is_cuda
    want = sel.greedy(terms, hp, x, 16, 0.5 * float(run.kdiag))
    assert len(on_dev.index) == len(want.piv) < 16 and float(on_dev.residual.max()) <= 0.5 * float(run.kdiag)


@functools.lru_cache(maxsize=None)
def model_case():
    terms = ["se", "wn"]
    hp, x, y, _ = sr.problem(terms, n=700, m=90)
    xp = np.random.default_rng(9).random((130, 3))
    return terms, hp, x, y, xp


def model_refs(terms, hp, x, y, z, xp):
    """tests/test_sparse_gpu.py's mcase at a given z: the restatement's answers and its own error per quantity."""
    loss, grad = sr.loss_and_grad(terms, hp, x, y, z)
    mu, cov = sr.predict(terms, hp, x, y, z, xp, var="full")
    mu_d, cov_d = sr.predict_dense(terms, hp, x, y, z, xp)
    own = {"loss": sr.self_error(terms, hp, x, y, z), "mean": float(np.abs(mu - mu_d).max() / np.abs(mu_d).max()),
           "cov": float(np.abs(cov - cov_d).max() / np.abs(cov_d).max())}
    print("restatement's own error", own, "cond(Kuu) %.2e" % np.linalg.cond(sr.kuu_kuf(terms, hp, x, z)[0]))
    return loss, grad, mu, cov, own


def test_greedy_model_against_the_restatement(ops):
    terms, hp, x, y, xp = model_case()
    xt, yt = torch.from_numpy(x), torch.from_numpy(y)
    gp = pg.Sparse_GP.greedy(xt, yt, cov_of(terms), 90, params=torch.from_numpy(hp))
    assert gp.z.shape == (90, 3) and gp.need_upd and torch.equal(gp.params, torch.from_numpy(hp))
    index = pg.select_inducing(xt, cov_of(terms), hp, 90).index
    assert torch.equal(gp.z, xt[index]) and len(set(index.tolist())) == 90
    z = x[index.numpy()]
    loss, grad, mu, cov, own = model_refs(terms, hp, x, y, z, xp)
    got_l, got_g = pg.VFE(gp).loss_and_grad(hp.copy())
    hold("greedy z: loss", got_l, loss, own["loss"])
    hold("greedy z: gradient", got_g, grad, own["loss"])
    m1, vd = gp.predict(torch.from_numpy(xp), var="diag")
    hold("greedy z: mean", m1.numpy(), mu, own["mean"])
    hold("greedy z: variance", vd.numpy(), np.diag(cov), own["cov"])
    _, _, _, z_helper = sr.problem(terms, n=700, m=90)
    print("bound at the greedy z %.4f, at problem's own z %.4f" % (float(got_l), sr.loss_woodbury(terms, hp, x, y, z_helper)))


def test_reselecting_marks_a_fitted_model_dirty(ops):
    terms, hp, x, y, xp = model_case()
    xt = torch.from_numpy(x)
    gp = pg.Sparse_GP.greedy(xt, torch.from_numpy(y), cov_of(terms), 90, params=torch.from_numpy(hp))
    vfe = pg.VFE(gp)
    l90 = float(vfe.loss(hp.copy()))
    gp.update()
    assert not gp.need_upd
    res = gp.select_inducing(m=60)
    assert gp.need_upd and gp.z.shape == (60, 3) and torch.equal(gp.z, xt[res.index])
    z = x[res.index.numpy()]
    loss, grad, mu, cov, own = model_refs(terms, hp, x, y, z, xp)
    m1, vd = gp.predict(torch.from_numpy(xp), var="diag")                      # the next predict refits on the new z
    assert not gp.need_upd
    hold("reselected z: mean", m1.numpy(), mu, own["mean"])
    hold("reselected z: variance", vd.numpy(), np.diag(cov), own["cov"])
    l60 = float(vfe.loss(hp.copy()))                                           # the memo of the same params was dropped with the old z
    hold("reselected z: loss", l60, loss, own["loss"])
    assert l60 > l90
