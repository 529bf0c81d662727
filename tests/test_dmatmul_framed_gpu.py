"""pg_kernel_matmul_dx on FRAMED operands (tests/framed.py, the harness of tests/test_framed_gpu.py unchanged): strided views in sentinel
memory with odd gaps, ldo > d ldk > d nrhs, a workspace of exactly pg_kernel_matmul_dx_worksize -- frame checks, the packed call's bits,
values -- for every model of tests/test_framed_kinds_gpu.py that is one pg_covspec pass (the entry point takes one spec).

OUT is framed as the matrix [nr][d * ldk] it is in memory, ldk = nrhs + 3: the call writes columns k * ldk + c, c < nrhs, and the rest
of a row -- the gap between two coordinates' columns as well as the gap behind the row -- must keep its sentinel.  The shape takes the
segment path (3 rows against 600 column points: partial tiles in the workspace, folded by the second launch).

Reference: tests/dmatmul_ref.py in np.longdouble; allowance: test_dmatmul_gpu.py's derived bound at the largest scale of the case."""
import ctypes as C
import functools

import numpy as np
import pytest

import dmatmul_ref as dr
from test_dmatmul_gpu import bound_of
from test_framed_gpu import F64, ok, ops, p, run  # noqa: F401  (ops: the fixture)
from test_framed_kinds_gpu import MODELS, hp_of, passes_of

pytestmark = pytest.mark.gpu

ONE_PASS = [mid for mid in MODELS if len(passes_of(mid)) == 1]
NR, NC, NRHS, KGAP = 3, 600, 5, 3


@functools.lru_cache(maxsize=None)
def fcase(mid):
    model, d = MODELS[mid]
    rng = np.random.default_rng(sum(map(ord, mid)))
    hp = hp_of(model, d, rng)
    xr, xc, v = rng.random((NR, d)), rng.random((NC, d)), rng.standard_normal((NC, NRHS))
    ref, scale = dr.matmul_dx(model, hp, xr, xc, v, np.longdouble)
    return hp, xr, xc, v, np.asarray(ref, np.float64), np.asarray(scale, np.float64), dr.own_dk(model, hp, xr, xc)


def case_dmatmul(bed, mid):
    model, d = MODELS[mid]
    hp, xr, xc, v, ref, scale, own = fcase(mid)
    ldk = NRHS + KGAP
    written = np.tile(np.arange(ldk) < NRHS, d)[None, :]                       # [1, d * ldk]: the columns the call writes
    xrf, xcf, vf = bed.put("Xr", xr), bed.put("Xc", xc), bed.put("V", v)
    hf = bed.put("hp", hp, dtype=F64)
    of = bed.put("OUT", shape=(NR, d * ldk), role="out", written=written)
    lw = int(bed.lib.pg_kernel_matmul_dx_worksize(NR, NC, d, NRHS))
    assert lw > 0
    work = bed.put("work", shape=(lw,), dtype=F64, role="out", written=np.zeros(lw, bool), scratch=np.ones(lw, bool))
    spec = passes_of(mid)[0][0]
    assert of.ld >= d * ldk > d * NRHS and (not bed.framed or of.ld > d * ldk)
    ok(bed, bed.lib.pg_kernel_matmul_dx(bed.h, bed.code, C.byref(spec), p(hf), p(xrf), xrf.ld, NR, p(xcf), xcf.ld, NC, d, p(vf), vf.ld, NRHS,
                                        p(of), of.ld, ldk, p(work), bed.st()))
    want = np.zeros((NR, d, ldk))
    want[:, :, :NRHS] = ref
    tol = bound_of(own, NC) * float(scale.max()) + 2.0 ** -53 * float(np.abs(ref).max())      # (the reference, rounded to float64)
    print("%s d=%d: own_dK %.2e, allowance %.2e of max|ref| %.2e" % (mid, d, own, tol, np.abs(ref).max()))
    return [("OUT", want.reshape(NR, d * ldk), written, tol, 0.0)]


@pytest.mark.parametrize("gapset", ["odd", "mixed"])
@pytest.mark.parametrize("mid", ONE_PASS)
def test_matmul_dx_framed(ops, gapset, mid):
    run(ops, case_dmatmul, F64, gapset, mid=mid)
