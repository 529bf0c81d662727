"""The three buffer-taking exports of include/pygpr_hip_vecchia.h through ctypes on FRAMED operands (tests/framed.py, the harness of
tests/test_framed_gpu.py unchanged): strided views in sentinel memory (ld = width + gap, the int32 tables included), workspaces of
exactly the stated worksize -- inputs unchanged, gaps and guards untouched, every output entry written, the packed call's bits, values
-- and once each under the stream harness of tests/streamed.py (StreamBed: the inputs are revealed late on a busy side stream, the
outputs are consumed directly behind the call).  tests/test_vecchia_cpu.py checks this file against the header's stream-taking names.

Values: pg_knn integer for integer on grid coordinates (tests/test_vecchia_gpu.py); the block kernels by that file's rule, four times
the distance of the float64 restatement from the np.longdouble one with a floor of 64 eps of the value's scale."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import kernel_ref as kr
import streamed
import test_framed_gpu as fg
import vecchia_ref as vr
from streamed import StreamBed
from test_framed_gpu import F64, ok, ops, p, run  # noqa: F401  (ops: the fixture)
from test_rowsq_cpu import MODELS, _hp

import kind_tools as kt

pytestmark = pytest.mark.gpu
I32 = torch.int32
EPS = 2.0 ** -52
N, D, M, Q, FIRST, COUNT = 130, 3, 5, 70, 37, 41
NAME = "se*per"


def _allow(f64, ld, scale=None):
    ld = np.asarray(ld, np.longdouble)
    scale = float(np.max(np.abs(ld))) if scale is None else float(scale)
    return max(4.0 * float(np.max(np.abs(np.asarray(f64, np.longdouble) - ld))), 64.0 * EPS * scale)


@functools.lru_cache(maxsize=None)
def knn_case(causal):
    rng = np.random.default_rng(41 + causal)
    x = rng.integers(0, 8, (N, D)) / 64.0
    xq = x if causal else rng.integers(0, 8, (Q, D)) / 64.0
    s = 2.0 ** rng.integers(-2, 3, D)
    return x, xq, s, vr.knn(xq, x, s, M, bool(causal))


def case_knn(bed, causal):
    x, xq, s, ref = knn_case(causal)
    q = xq.shape[0]
    xf = bed.put("Xc", x)
    qf = xf if causal else bed.put("Xq", xq)
    sf = bed.put("s", s, dtype=F64)
    nf = bed.put("nbr", shape=(q, M), dtype=I32, role="out")
    assert not bed.framed or (xf.ld > D and nf.ld > M)
    ok(bed, bed.lib.pg_knn(bed.h, 0, p(qf), qf.ld, q, p(xf), xf.ld, N, D, p(sf), M, causal, p(nf), nf.ld, bed.st()))
    return [("nbr", ref.astype(np.float64), None, 0.0, 0.0)]


@functools.lru_cache(maxsize=None)
def block_case():
    terms = MODELS[NAME]
    rng = np.random.default_rng(43)
    x = rng.random((N, D))
    y = np.sin(3.0 * x.sum(1)) + 0.1 * rng.standard_normal(N)
    hp = _hp(terms, D, rng)
    nbr = vr.knn(x, x, None, M, True)
    nbr[rng.random(nbr.shape) < 0.2] = -1
    nb = nbr[FIRST: FIRST + COUNT]
    tr = [vr.nlml_and_grad(terms, hp, x, y, nb, kr.JITTER, dt, first=FIRST) for dt in (np.float64, np.longdouble)]
    xq = rng.random((Q, D))
    nq = vr.knn(xq, x, None, M, False)
    nq[rng.random(nq.shape) < 0.2] = -1
    pr = [vr.predict(terms, hp, x, y, xq, nq, kr.JITTER, dt) for dt in (np.float64, np.longdouble)]
    return terms, hp, x, y, nb, tr, xq, nq, pr


def _spec(terms):
    return kt.one_spec(terms, D, product=any(isinstance(t, tuple) for t in terms))


def case_nlml(bed):
    terms, hp, x, y, nb, (f64, ld), _, _, _ = block_case()
    nhp = hp.size
    xf, yf, hf = bed.put("X", x), bed.put("Y", y), bed.put("hp", hp, dtype=F64)
    nf = bed.put("nbr", nb, dtype=I32)
    cm, cv = bed.put("cmean", shape=(COUNT,), role="out"), bed.put("cvar", shape=(COUNT,), role="out")
    out, grad = bed.put("out", shape=(1,), dtype=F64, role="out"), bed.put("grad", shape=(nhp,), dtype=F64, role="out")
    info = bed.put("info", shape=(1,), dtype=I32, role="out")
    lw = int(bed.lib.pg_vecchia_nlml_grad_worksize(COUNT, D, nhp))
    assert lw == ((COUNT + 3) // 4) * (nhp + 2)      # d = 3, nhp = 11: four wavefronts a workgroup, one row each
    work = bed.put("work", shape=(lw,), dtype=F64, role="out", written=np.zeros(lw, bool), scratch=np.ones(lw, bool))
    spec = _spec(terms)
    ok(bed, bed.lib.pg_vecchia_nlml_grad(bed.h, 0, C.byref(spec), p(hf), nhp, p(xf), xf.ld, N, D, p(yf), p(nf), nf.ld, M, FIRST, COUNT, kr.JITTER, 1,
                                         p(cm), p(cv), p(out), p(grad), p(info), p(work), bed.st()))
    yt = y[FIRST: FIRST + COUNT]
    lscale = float(np.sum(np.abs(0.5 * (np.log(ld[3]) + (yt - ld[2]) ** 2 / ld[3] + np.log(2 * np.pi)))))
    f = lambda a: np.asarray(a, np.float64)      # noqa: E731
    return [("out", f(ld[0]), None, _allow(f64[0], ld[0], lscale), 0.0), ("grad", f(ld[1]), None, _allow(f64[1], ld[1]), 0.0),
            ("cmean", f(ld[2]), None, _allow(f64[2], ld[2], np.max(np.abs(y))), 0.0), ("cvar", f(ld[3]), None, _allow(f64[3], ld[3]), 0.0),
            ("info", 0.0, None, 0.0, 0.0)]


def case_predict(bed):
    terms, hp, x, y, _, _, xq, nq, (f64, ld) = block_case()
    xf, yf, hf, qf = bed.put("X", x), bed.put("Y", y), bed.put("hp", hp, dtype=F64), bed.put("Xq", xq)
    nf = bed.put("nbr", nq, dtype=I32)
    mean, var = bed.put("mean", shape=(Q,), role="out"), bed.put("var", shape=(Q,), role="out")
    info = bed.put("info", shape=(1,), dtype=I32, role="out")
    lw = int(bed.lib.pg_vecchia_predict_worksize(Q, D))
    assert lw == ((Q + 3) // 4) * 2                  # d = 3 without hp slots: four wavefronts a workgroup
    work = bed.put("work", shape=(lw,), dtype=F64, role="out", written=np.zeros(lw, bool), scratch=np.ones(lw, bool))
    spec = _spec(terms)
    ok(bed, bed.lib.pg_vecchia_predict(bed.h, 0, C.byref(spec), p(hf), p(xf), xf.ld, N, D, p(yf), p(qf), qf.ld, Q, p(nf), nf.ld, M, kr.JITTER,
                                       p(mean), p(var), p(info), p(work), bed.st()))
    f = lambda a: np.asarray(a, np.float64)      # noqa: E731
    return [("mean", f(ld[0]), None, _allow(f64[0], ld[0], np.max(np.abs(y))), 0.0), ("var", f(ld[1]), None, _allow(f64[1], ld[1]), 0.0),
            ("info", 0.0, None, 0.0, 0.0)]


@pytest.mark.parametrize("gapset", ["odd", "mixed"])
@pytest.mark.parametrize("causal", [1, 0])
def test_knn_framed(ops, gapset, causal):
    run(ops, case_knn, F64, gapset, causal=causal)


@pytest.mark.parametrize("gapset", ["odd", "mixed"])
def test_nlml_grad_framed(ops, gapset):
    run(ops, case_nlml, F64, gapset)


@pytest.mark.parametrize("gapset", ["odd", "mixed"])
def test_predict_framed(ops, gapset):
    run(ops, case_predict, F64, gapset)


# ---- the stream contract ---------------------------------------------------------------------------------------------------------------------
def _streamed(ops, monkeypatch, export, case, **kw):
    """run() with tests/streamed.py's bed in its framed half.  Where two streams do not run side by side the checks are blind, not
    wrong (tests/streamed.py): the case still runs and says so."""
    print("streams run side by side: %s" % streamed.probe_concurrent_streams())
    monkeypatch.setattr(fg, "FRAMED_BED", StreamBed)
    del StreamBed.log[:]
    try:
        run(ops, case, F64, "mixed", **kw)
    finally:
        streamed.close_all()
        torch.cuda.synchronize()
    assert export in StreamBed.log


def test_knn_streamed(ops, monkeypatch):
    _streamed(ops, monkeypatch, "pg_knn", case_knn, causal=1)


def test_nlml_grad_streamed(ops, monkeypatch):
    _streamed(ops, monkeypatch, "pg_vecchia_nlml_grad", case_nlml)


def test_predict_streamed(ops, monkeypatch):
    _streamed(ops, monkeypatch, "pg_vecchia_predict", case_predict)
