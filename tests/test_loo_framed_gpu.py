"""Every buffer-taking export of include/pygpr_hip_loo.h through ctypes on FRAMED operands (tests/framed.py; the harness of
tests/test_framed_gpu.py: packed call, framed call, same bits, guards, values); tests/test_loo_cpu.py checks this list against the
header.  Operands are strided views (ld = width + gap, base 16- but not 256-byte aligned) in sentinel memory, the workspace is
exactly pg_loo_terms_worksize doubles, and what the header says is not read (L^-1 above its diagonal 128-blocks) holds NaN.

Values are compared with NumPy in fp64 on the inputs AS ROUNDED to the dtype, so that only the kernels' own arithmetic is judged:
the kernels accumulate in fp64 for both dtypes and round an output once to the dtype, so the bound is the worst case of an n-term
fp64 sum plus that rounding, doubled: tol(dtype, n) = 2 (n 2^-53 + eps(dtype)), relative to the sum of the magnitudes that are added."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_framed_gpu import F32, F64, both, gaps, gaps_odd, ok, ops, p, run, state  # noqa: F401  (ops: the module's fixture)

pytestmark = pytest.mark.gpu

EPS = {F64: 2.0 ** -53, F32: 2.0 ** -24}


def tol(dtype, n):
    return 2.0 * (n * 2.0 ** -53 + EPS[dtype])


CASES = [(300, 512), (129, 256), (512, 512)]      # two chunks with padding, one chunk with a one-row second block, no padding


def _rounded(a, dtype):
    return np.asarray(a, dtype=np.float32 if dtype == F32 else np.float64).astype(np.float64)


def case_terms(bed, n, n_pad, nan_at=None):
    s = state(n, n_pad)
    dt = bed.dtype
    alpha, y = s["alpha"].copy(), s["y"].copy()
    if nan_at is not None:
        y[nan_at] = np.nan
    minv = bed.put("Minv", s["M"], poison=s["unread"] if bed.framed else None)
    al = bed.put("alpha", alpha)
    yy = bed.put("y", y)
    c = bed.put("c", shape=(n,), role="out")
    mu = bed.put("mu", shape=(n,), role="out")
    var = bed.put("var", shape=(n,), role="out")
    out = bed.put("out", shape=(1,), dtype=F64, role="out")
    lw = int(bed.lib.pg_loo_terms_worksize(n_pad))
    assert lw == (n_pad // 256) * n_pad + n_pad // 256 + 2
    work = bed.put("work", shape=(lw,), dtype=F64, role="out", written=np.zeros(lw, bool), scratch=np.ones(lw, bool))
    ok(bed, bed.lib.pg_loo_terms(bed.h, bed.code, n, n_pad, p(minv), minv.ld, p(al), p(yy), p(c), p(mu), p(var), p(out), p(work), bed.st()))
    m = np.tril(_rounded(s["M"], dt))[:n, :n]
    a, yr = _rounded(alpha, dt)[:n], _rounded(y, dt)[:n]
    cr = (m * m).sum(0)
    e = tol(dt, n)
    fin = np.isfinite(yr)
    loss = float(np.sum(-0.5 * np.log(cr) + 0.5 * a * a / cr) + 0.5 * n * np.log(2 * np.pi)) if fin.all() else np.nan
    lscale = float(np.sum(np.abs(0.5 * np.log(cr)) + 0.5 * a * a / cr)) + 0.5 * n * np.log(2 * np.pi)
    return [("c", cr, None, 0.0, e), ("var", 1.0 / cr, None, 0.0, e),
            ("mu", yr - a / cr, None, e * float(np.max(np.abs(np.nan_to_num(yr)) + np.abs(a / cr))), e),
            ("out", loss, None, tol(F64, n) * lscale, 0.0)]


@both
@gaps
@pytest.mark.parametrize("n,n_pad", CASES)
def test_loo_terms(ops, dtype, gapset, n, n_pad):
    run(ops, case_terms, dtype, gapset, n=n, n_pad=n_pad)


@both
def test_loo_terms_nan_in_y_stays_in_its_point(ops, dtype):
    """NaN in y[i]: NaN in mu[i] and in the loss, nowhere else (assert_allclose treats NaN == NaN as equal, and only there)."""
    run(ops, case_terms, dtype, "mixed", n=300, n_pad=512, nan_at=137)


@both
def test_loo_terms_refuses_misaligned_rows(ops, dtype):
    n_pad = 256
    lib = ops.lib
    item = 8 if dtype == F64 else 4
    buf = torch.zeros(n_pad * (n_pad + 1) + 8, dtype=dtype, device="cuda")
    vec = torch.ones(6, n_pad, dtype=dtype, device="cuda")
    out = torch.full((1,), 7.0, dtype=F64, device="cuda")
    work = torch.zeros(int(lib.pg_loo_terms_worksize(n_pad)), dtype=F64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    v = [C.c_void_p(vec[i].data_ptr()) for i in range(5)]
    code = 0 if dtype == F64 else 1
    for ptr, ld in ((buf.data_ptr(), n_pad + 1), (buf.data_ptr() + item, n_pad)):      # rows, then base, off the 16-byte grid
        rc = lib.pg_loo_terms(ops.h, code, 200, n_pad, C.c_void_p(ptr), ld, v[0], v[1], v[2], v[3], v[4], C.c_void_p(out.data_ptr()),
                              C.c_void_p(work.data_ptr()), st)
        assert rc != 0 and b"16-byte" in lib.pg_last_error()
    torch.cuda.synchronize()
    assert float(out[0]) == 7.0 and bool((vec == 1).all())      # nothing was enqueued


def _fitted(n, n_pad):
    s = state(n, n_pad)
    m = np.tril(s["M"])
    kinv = m.T @ m                                                # identity in the padding
    return s, kinv


def case_weights(bed, n, n_pad):
    s, kinv = _fitted(n, n_pad)
    dt = bed.dtype
    c0 = np.diag(kinv)[:n].copy()
    real = np.zeros((n_pad, n_pad), bool)
    real[:n, :n] = True
    kf = bed.put("Kinv", kinv, role="inout", written=real)
    cc = bed.put("c", c0)
    al = bed.put("alpha", s["alpha"][:n])
    pp = bed.put("p", shape=(n,), role="out")
    qq = bed.put("q", shape=(n,), role="out")
    ok(bed, bed.lib.pg_loo_weights(bed.h, bed.code, n, p(cc), p(al), p(kf), kf.ld, p(pp), p(qq), bed.st()))
    k, c, a = _rounded(kinv, dt)[:n, :n], _rounded(c0, dt), _rounded(s["alpha"][:n], dt)
    b = k @ (a / c)
    babs = np.abs(k) @ np.abs(a / c)
    e = tol(dt, n)
    sref = np.array(_rounded(kinv, dt))
    sref[:n, :n] = k * (np.sqrt(c + a * a) / c)
    ptol = e * float(np.max(np.abs(a) + babs))
    return [("Kinv", sref, None, 0.0, e), ("p", (a + b) / np.sqrt(2), None, ptol, 0.0), ("q", (a - b) / np.sqrt(2), None, ptol, 0.0)]


@both
@gaps
@pytest.mark.parametrize("n,n_pad", CASES)
def test_loo_weights(ops, dtype, gapset, n, n_pad):
    run(ops, case_weights, dtype, gapset, n=n, n_pad=n_pad)


def case_fold(bed, n, n_pad):
    rng = np.random.default_rng(n)
    dt = bed.dtype
    m0 = rng.standard_normal((n_pad, n_pad))
    q0 = rng.standard_normal(n)
    low = np.zeros((n_pad, n_pad), bool)
    low[:n, :n] = np.tril(np.ones((n, n), bool))
    mf = bed.put("M", m0, role="inout", written=low)
    qf = bed.put("q", q0)
    ok(bed, bed.lib.pg_loo_fold(bed.h, bed.code, n, p(mf), mf.ld, p(qf), bed.st()))
    m, q = _rounded(m0, dt), _rounded(q0, dt)
    ref = m.copy()
    ref[:n, :n] += np.tril(np.outer(q, q))
    return [("M", ref, None, tol(dt, 1) * float(np.max(np.abs(m)) + np.max(np.abs(q)) ** 2), 0.0)]


@both
@gaps_odd
@pytest.mark.parametrize("n,n_pad", [(300, 512), (65, 256)])
def test_loo_fold(ops, dtype, gapset, n, n_pad):
    run(ops, case_fold, dtype, gapset, n=n, n_pad=n_pad)
