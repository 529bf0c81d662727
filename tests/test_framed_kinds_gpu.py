"""The kinds that came after tests/test_framed_gpu.py -- rational quadratic (block d + 2), periodic (block 2 d + 1), products
(PG_SPEC_PRODUCT, several widths in one spec) and a sum that needs two passes -- through every export of include/pygpr_hip.h that takes a
`const pg_covspec*`, on FRAMED operands.  The harness is that of tests/test_framed_gpu.py, unchanged: a packed call, then the framed
call (strided views in sentinel memory, ld = width + gap, expert strides larger than minimal, workspaces of exactly pg_*_worksize),
frame checks, same bits as the packed call (no exemption), values, and NaN wherever the header says nothing is read.  The sentinel
is a quiet NaN, so an over-read of hp, X, u or B that reaches the arithmetic fails the value check.  tests/test_framed_cpu.py checks the
list of entry points against the header and the model table against the kinds of pygpr_amd/_lib.py.

Reference: tests/kernel_ref.py in fp64, never another GPU call.  Specs come from pygpr_amd.covar.spec_of, so the block offsets are
the library's own layout.  Data in [0, 1)^d; sigma 1.2, inverse length scales 0.4 .. 1.2, periods 0.7 .. 2.5 (a difference of up to
1 against a period of 0.7: the phase is reduced by a period), alpha 0.8, noise 0.05 .. 0.15 (0.3 where a matrix is factored).

Allowances are those of the packed tests of the same entry point and kind (cited at each case): K 1e-13 / 4e-6, dK 1e-12 /
5e-6 max(1, |dK|), NLML gradient 1e-8 / 3 x 3e-3 of max|g|, pg_kernel_xgrad 1e-12 / 1e-4 of max|ref|, the factor of a built K
1e-10 / 2e-5 cond(L); the fp32 build of a product of three or more factors takes the relative rule of
test_product_gpu.py::test_entry_points_against_the_restatement (F x 4e-6 / 1.44 of max|K|).  Every element-wise allowance goes through
test_product_gpu.allowance: kernel_ref's own fp64 error against its long-double evaluation, on at most 64 points (32 test points) of
the case's inputs, is printed beside it, and the allowance would be four times that error if a quarter of it did not cover the error."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import append_ref as ar
import kernel_ref as kr
from framed import min_gap
from kind_tools import cov_of
from pygpr_amd import _lib
from test_framed_gpu import F32, F64, Bed, _ftol, _inv_tol, both, gaps, gaps_odd, kstate, ok, ops, p, ptr_at, run, tiles_low  # noqa: F401  (ops: the fixture)
from test_product_gpu import allowance

pytestmark = pytest.mark.gpu

KIND_OF = {"se": _lib.PG_KIND_RBF, "m52": _lib.PG_KIND_MATERN52, "m32": _lib.PG_KIND_MATERN32, "m12": _lib.PG_KIND_MATERN12,
           "rq": _lib.PG_KIND_RQ, "per": _lib.PG_KIND_PERIODIC}
# id -> (terms, d); a term is a part name or a tuple of factors (tests/kernel_ref.py).  The route each takes:
MODELS = {
    "R1": (["rq", "wn"], 13),                      # matrix-pipe build and gradient bodies (kmfma.hip); block d + 2
    "R2": (["rq", "se", "wn"], 31),                # VALU bodies; the component after a d + 2 block
    "P1": (["per", "wn"], 5),                      # PER bodies; block 2 d + 1
    "P2": (["se", "per", "rq", "wn"], 4),          # PER instantiation carrying three widths in one sum
    "X1": ([("se", "per"), "wn"], 3),              # PROD, the locally periodic kernel
    "X2": ([("rq", "m12", "per"), "wn"], 17),      # PROD past the d <= 16 instantiations
    "C1": (["m32", ("se", "per"), "wn"], 3),       # two passes: the plain child with the noise, then the product with accumulate = 1
    "S1": (["se", "m52", "wn"], 5),                # the older kinds: pg_kernel_xgrad batched, transposed and accumulating
}
SEVEN = ["R1", "R2", "P1", "P2", "X1", "X2", "C1"]
NE = 3


@functools.lru_cache(maxsize=None)
def passes_of(mid):
    """[(pg_covspec, terms, idx)] of a model, in the order the library runs them: the spec of the pass, the terms it evaluates and the
    indices of their parameters in hp (kernel_ref evaluates `terms` on hp[idx]).  One entry unless the sum holds a product beside a
    plain child (covar.spec_of: the plain children and the noise first, then one product pass per Product, without noise)."""
    from pygpr_amd.covar import spec_of

    model, d = MODELS[mid]
    specs, nhp = spec_of(cov_of(model), d)
    assert nhp == kr.nhp_of(model, d)
    blocks, o = [], 0
    for t in model:
        w = sum(kr.width(q, d) for q in kr.factors(t))
        blocks.append((t, np.arange(o, o + w)))
        o += w
    if len(specs) == 1:
        out = [(specs[0], list(model), np.arange(nhp))]
    else:
        plain = [b for b in blocks if not isinstance(b[0], tuple)]
        prods = [b for b in blocks if isinstance(b[0], tuple)]
        assert len(specs) == 1 + len(prods)
        out = [(specs[0], [t for t, _ in plain], np.concatenate([i for _, i in plain]))] + [(sp, [t], i) for sp, (t, i) in zip(specs[1:], prods)]
    for sp, terms, idx in out:      # the spec's offsets are the starts of the blocks this pass owns
        nc = sp.ncomp & ~_lib.PG_SPEC_PRODUCT
        starts, o = [], 0
        for q in kr.flat(terms):
            starts.append(int(idx[o]))
            o += kr.width(q, d)
        assert sorted(list(sp.off[:nc]) + list(sp.noise_off[:sp.nnoise])) == sorted(starts), (mid, terms)
        assert bool(sp.ncomp & _lib.PG_SPEC_PRODUCT) == any(isinstance(t, tuple) for t in terms)
    return out


def one_spec(mid):
    ps = passes_of(mid)
    assert len(ps) == 1
    return ps[0][0]


def hp_of(model, d, rng, noise=None):
    out = []
    for q in kr.flat(model):
        if q == "wn":
            out.append([0.05 + 0.1 * rng.random() if noise is None else noise])
            continue
        out += [[1.2], 0.4 + 0.8 * rng.random(d)]
        if q == "per":
            out.append(rng.uniform(0.7, 2.5, d))
        if q == "rq":
            out.append([0.8])
    return np.concatenate(out)


def others(nhp, idx):
    """Boolean mask of the parameters a pass does not own (poisoned in the framed call: a pass reads its own blocks only)."""
    m = np.ones(nhp, bool)
    m[idx] = False
    return m


def put_hp(bed, mid, hp, i):
    """hp as the operand of pass i: with more than one pass the other passes' blocks hold NaN in the framed call."""
    ps = passes_of(mid)
    return bed.put("hp%d" % i, hp, dtype=F64, poison=others(hp.size, ps[i][2]) if len(ps) > 1 else None)


def k_tol(mid, dtype, ref, hp, x, xp=None):
    """K: 1e-13 (test_rq_gpu / test_periodic_gpu / test_product_gpu) and 4e-6 in fp32; a product of F >= 3 factors in fp32: F x 4e-6 / 1.44
    of max|K| (test_entry_points_against_the_restatement).  A sum evaluated in two passes rounds each pass to fp32 once and then adds
    them: one fp32 allowance per pass, the rule test_framed_gpu.test_kernel_build_cross_and_accumulate applies to its second pass."""
    model, d = MODELS[mid]
    nf = max(len(kr.factors(t)) for t in model)
    if dtype == F64:
        tol = 1e-13
    else:
        tol = (nf * (4e-6 / 1.44) * float(np.abs(ref).max()) if nf >= 3 else 4e-6) * len(passes_of(mid))
    s, sp = x[:64], (None if xp is None else xp[:32])
    tol, err = allowance(tol, kr.kernel(model, hp, s, sp), kr.kernel(model, hp, s, sp, dtype=np.longdouble))
    print("%s %s K: allowance %.2e, kernel_ref's own error %.2e" % (mid, "f64" if dtype == F64 else "f32", tol, err))
    return tol


def sized(shapes, small="mixed"):
    """(shape, gapset) pairs: every gap set at the shapes that hold 300 points, `mixed` alone at the small ones."""
    return [(s, g) for s in shapes for g in (["min", "wide", "mixed"] if 300 in np.atleast_1d(s) else [small])]


# ------------------------------------------------------------------------------------------- 1. pg_kernel_build, symmetric
@functools.lru_cache(maxsize=None)
def sym_inputs(mid, n):
    model, d = MODELS[mid]
    rng = np.random.default_rng(1000 * n + d)
    x, hp = rng.random((n + 3, d)), hp_of(model, d, rng)
    ref = np.eye(512)
    ref[:n, :n] = kr.kernel(model, hp, x[:n]) + 1e-7 * np.eye(n)
    return x, hp, ref


def sym_case(mid, n, dtype, seen=None):
    model, d = MODELS[mid]
    x, hp, ref = sym_inputs(mid, n)
    tol = k_tol(mid, dtype, ref, hp, x[:n])
    pois = np.zeros((n + 3, d), bool)
    pois[n:] = True
    npad = 512

    def case(bed, lower_only):
        xd = bed.put("x", x, poison=pois)
        k = bed.put("k", shape=(npad, npad), role="out", written=tiles_low(npad, npad, 64) if lower_only else None)
        for i, (sp, _, _) in enumerate(passes_of(mid)):      # (C1: its passes in order on the one output)
            hpd = put_hp(bed, mid, hp, i)
            ok(bed, bed.lib.pg_kernel_build(bed.h, bed.code, C.byref(sp), p(hpd), p(xd), xd.ld, n, None, 0, 0, d, lower_only, int(i > 0),
                                            1e-7 if i == 0 else 0.0, p(k), k.ld, npad, npad, bed.st()))
        if seen is not None:
            seen.append(k)
        return [("k", ref, np.tril(np.ones((npad, npad), bool)) if lower_only else None, tol, 0)]

    return case


@both
@pytest.mark.parametrize("n,gapset", sized([1, 37, 300]))
@pytest.mark.parametrize("mid", SEVEN)
def test_kernel_build_symmetric(ops, mid, n, gapset, dtype):
    """Mirrored and lower-only builds on rows_pad = 512: K[:n, :n] and the identity padding (the whole matrix is compared); lower_only
    leaves the 64-tiles above the diagonal untouched.  X has ldx > d and three trailing NaN rows that are never read."""
    case = sym_case(mid, n, dtype)
    run(ops, case, dtype, gapset, lower_only=0)
    run(ops, case, dtype, gapset, lower_only=1)


# ------------------------------------------------------------------------------------------- 2. pg_kernel_build, cross + accumulate
@functools.lru_cache(maxsize=None)
def cross_inputs(mid, nr, nc):
    model, d = MODELS[mid]
    rng = np.random.default_rng(100 * nr + nc + d)
    xr, xc, hp = rng.random((nr, d)), rng.random((nc, d)), hp_of(model, d, rng)
    return xr, xc, hp, kr.kernel(model, hp, xc, xr)


def cross_case(mid, nr, nc, dtype, seen=None):
    model, d = MODELS[mid]
    xr, xc, hp, kx = cross_inputs(mid, nr, nc)
    rp, cp = (512 if nr > 256 else 256), (512 if nc > 256 else 256)
    ref = np.zeros((rp, cp))
    ref[:nr, :nc] = kx
    real = np.zeros((rp, cp), bool)
    real[:nr, :nc] = True
    tol = k_tol(mid, dtype, kx, hp, xc, xr)

    def case(bed, acc):
        a, b = bed.put("xr", xr), bed.put("xc", xc)
        k = bed.put("k", ref if acc else None, shape=(rp, cp), role="inout" if acc else "out", written=real if acc else None)
        for i, (sp, _, _) in enumerate(passes_of(mid)):
            hpd = put_hp(bed, mid, hp, i)
            ok(bed, bed.lib.pg_kernel_build(bed.h, bed.code, C.byref(sp), p(hpd), p(a), a.ld, nr, p(b), b.ld, nc, d, 0, int(acc or i > 0), 0.0, p(k),
                                            k.ld, rp, cp, bed.st()))
        if seen is not None:
            seen.append(k)
        return [("k", (2.0 if acc else 1.0) * ref, None, tol * (2 if acc else 1), 0)]      # (K += k: both terms carry the allowance)

    return case


@both
@pytest.mark.parametrize("shape,gapset", sized([(37, 300), (300, 1), (1, 37)]))
@pytest.mark.parametrize("mid", SEVEN)
def test_kernel_build_cross_and_accumulate(ops, mid, shape, gapset, dtype):
    """Cross build (zero padding, rows_pad 256 / 512 x cols_pad 512 / 256), then accumulate passes of the same model onto the result:
    K += k with the padding bitwise unchanged.  C1: every pass reads hp with the OTHER pass's blocks poisoned."""
    case = cross_case(mid, shape[0], shape[1], dtype)
    run(ops, case, dtype, gapset, acc=0)
    run(ops, case, dtype, gapset, acc=1)


@both
@pytest.mark.parametrize("mid", ["R1", "P1", "X1"])
def test_kernel_build_routing(ops, monkeypatch, mid, dtype):
    """The bodies of the model table are reached, pinned by result (test_product_gpu): with PG_KB_MFMA = 0 and with the default both
    meet the allowance; the periodic and the product spec never take the matrix pipe, so their BITS agree; the rational quadratic at
    d = 13 does take it by default, so its bits differ from the VALU body's (an expansion against direct differences)."""
    bits = {}
    for mode in ("0", None):
        if mode is None:
            monkeypatch.delenv("PG_KB_MFMA", raising=False)
        else:
            monkeypatch.setenv("PG_KB_MFMA", mode)
        seen = []
        run(ops, sym_case(mid, 300, dtype, seen), dtype, "mixed", lower_only=0)
        run(ops, cross_case(mid, 37, 300, dtype, seen), dtype, "mixed", acc=0)
        bits[mode] = [seen[1].bits(), seen[3].bits()]      # (the framed call of each run)
    same = all(np.array_equal(a, b) for a, b in zip(bits["0"], bits[None]))
    assert same == (mid != "R1")


# ------------------------------------------------------------------------------------------- 3. pg_kernel_build_batched
@both
@gaps
@pytest.mark.parametrize("mid", ["R1", "P1", "X1"])
def test_kernel_build_batched(ops, mid, dtype, gapset):
    """Three experts in one launch, each with its own points and hyper-parameters (hp batch gap 4, k_stride larger than rows_pad * ldk):
    a symmetric build and a cross build with shared row points (xr_stride = 0).  Allowances of pg_kernel_build."""
    model, d = MODELS[mid]
    n, m = 300, 37
    rng = np.random.default_rng(5 + d)
    xs, xq = rng.random((NE, n, d)), rng.random((m, d))
    hps = np.stack([hp_of(model, d, rng) for _ in range(NE)])
    spec = one_spec(mid)
    rs, rc = np.stack([np.eye(512)] * NE), np.zeros((NE, 256, 512))
    for e in range(NE):
        rs[e, :n, :n] = kr.kernel(model, hps[e], xs[e]) + 1e-7 * np.eye(n)
        rc[e, :m, :n] = kr.kernel(model, hps[e], xs[e], xq)
    tol = max(k_tol(mid, dtype, rs[0, :n, :n], hps[0], xs[0]), k_tol(mid, dtype, rc[0, :m, :n], hps[0], xs[0], xq))

    def case(bed, sym):
        x, hpd = bed.put("x", xs), bed.put("hp", hps, dtype=F64, batch_gap=4)
        if sym:
            k = bed.put("k", shape=(NE, 512, 512), role="out")
            ok(bed, bed.lib.pg_kernel_build_batched(bed.h, bed.code, C.byref(spec), p(hpd), hpd.ld, p(x), x.ld, x.estride, n, None, 0, 0, 0, d, 0,
                                                    1e-7, p(k), k.ld, k.estride, 512, 512, NE, bed.st()))
            return [("k", rs, None, tol, 0)]
        q = bed.put("xq", xq)
        k = bed.put("k", shape=(NE, 256, 512), role="out")
        ok(bed, bed.lib.pg_kernel_build_batched(bed.h, bed.code, C.byref(spec), p(hpd), hpd.ld, p(q), q.ld, 0, m, p(x), x.ld, x.estride, n, d, 0, 0.0,
                                                p(k), k.ld, k.estride, 256, 512, NE, bed.st()))
        return [("k", rc, None, tol, 0)]

    run(ops, case, dtype, gapset, sym=1)
    run(ops, case, dtype, gapset, sym=0)


@both
@pytest.mark.parametrize("mid", ["P1", "X1"])
def test_kernel_build_empty_operands(ops, mid, dtype):
    """The modes of test_framed_gpu.test_kernel_build_empty_operands on the PER and PROD configurations: nr == 0 or nc == 0 gives
    padding only (identity / zeros; lower 64-tiles with lower_only) and the empty point set -- one row of NaN -- is never touched."""
    model, d = MODELS[mid]
    hp, spec = hp_of(model, d, np.random.default_rng(1)), one_spec(mid)
    full = np.random.default_rng(2).random((40, d))

    def case(bed, mode, batched):
        empty, pts, hpd = bed.put("x", np.full((1, d), np.nan)), bed.put("pts", full), bed.put("hp", hp, dtype=F64)
        ne = 2 if batched else 1
        sym = mode in ("sym", "low")
        rp, cp = (256, 256) if sym else (512, 256)
        wr = tiles_low(rp, cp, 64) if mode == "low" else None
        k = bed.put("k", shape=(ne, rp, cp) if batched else (rp, cp), role="out", written=wr)
        xr, nr, xc, nc = {"sym": (empty, 0, None, 0), "low": (empty, 0, None, 0), "cross00": (empty, 0, empty, 0), "cross0n": (empty, 0, pts, 40),
                          "crossn0": (pts, 40, empty, 0)}[mode]
        if batched:
            ok(bed, bed.lib.pg_kernel_build_batched(bed.h, bed.code, C.byref(spec), p(hpd), 0, p(xr), xr.ld, 0, nr, p(xc), xc.ld if xc else 0, 0, nc, d,
                                                    int(mode == "low"), 1e-7, p(k), k.ld, k.estride, rp, cp, ne, bed.st()))
        else:
            ok(bed, bed.lib.pg_kernel_build(bed.h, bed.code, C.byref(spec), p(hpd), p(xr), xr.ld, nr, p(xc), xc.ld if xc else 0, nc, d,
                                            int(mode == "low"), 0, 1e-7, p(k), k.ld, rp, cp, bed.st()))
        return [("k", np.eye(rp) if sym else np.zeros((rp, cp)), wr, 0, 0)]

    for mode in ("sym", "low", "cross00", "cross0n", "crossn0"):
        for batched in (0, 1):
            run(ops, case, dtype, "mixed", mode=mode, batched=batched)


# ------------------------------------------------------------------------------------------- 4. pg_kernel_grad_build
@functools.lru_cache(maxsize=None)
def dk_inputs(mid, n=70):
    model, d = MODELS[mid]
    rng = np.random.default_rng(12 + d)
    x, hp = rng.random((n, d)), hp_of(model, d, rng)
    dk = kr.kernel_and_grad(model, hp, x)[1]
    own = (kr.kernel_and_grad(model, hp, x[:64])[1], kr.kernel_and_grad(model, hp, x[:64], dtype=np.longdouble)[1])
    return x, hp, dk, own


@both
@gaps_odd
@pytest.mark.parametrize("mid", ["R2", "P2", "X1", "X2"])
def test_kernel_grad_build(ops, mid, dtype, gapset):
    """The whole dK stack (contiguous by contract: only X is strided, odd ldx included) against kernel_ref.kernel_and_grad.
    Allowances: 1e-12 (test_rq_gpu / test_periodic_gpu / test_product_gpu); fp32 5e-6 max(1, |dK|) (test_product_gpu)."""
    model, d = MODELS[mid]
    n = 70
    x, hp, dk, own = dk_inputs(mid)
    spec, nhp = one_spec(mid), hp.size
    tol, err = allowance(1e-12 if dtype == F64 else 5e-6 * max(1.0, float(np.abs(dk).max())), *own)
    print("%s %s dK: allowance %.2e, kernel_ref's own error %.2e" % (mid, "f64" if dtype == F64 else "f32", tol, err))

    def case(bed):
        xd, hpd = bed.put("x", x), bed.put("hp", hp, dtype=F64)
        out = bed.put("dk", shape=(nhp * n * n,), role="out")
        ok(bed, bed.lib.pg_kernel_grad_build(bed.h, bed.code, C.byref(spec), p(hpd), p(xd), xd.ld, n, d, p(out), bed.st()))
        return [("dk", dk.reshape(-1), None, tol, 0)]

    run(ops, case, dtype, gapset)


# ------------------------------------------------------------------------------------------- 5 / 6. pg_nlml_grad, pg_nlml_grad_batched
@functools.lru_cache(maxsize=None)
def gradient_inputs(mid, n=333, seed=0):
    """x, hp, K^-1, alpha, the gradient 1/2 sum (K^-1 - a a^T) o dK_k from kernel_ref's slabs (test_framed_gpu.grad_case), and the
    reference's own error in that contraction on the first 64 points, relative to max|g| like the check."""
    model, d = MODELS[mid]
    rng = np.random.default_rng(7 * n + d + seed)
    x, hp = rng.random((n, d)), hp_of(model, d, rng)
    kinv = np.linalg.inv(kr.kernel(model, hp, x) + 1e-7 * np.eye(n))
    kinv = 0.5 * (kinv + kinv.T)
    alpha = kinv @ rng.standard_normal(n)
    w = kinv - np.outer(alpha, alpha)
    g = np.zeros(hp.size)
    for k, slab in kr.grad_terms(model, hp, x):
        g[k] += 0.5 * (w * slab).sum()
    ws = w[:64, :64]
    g64 = 0.5 * np.einsum("ij,pij->p", ws, kr.kernel_and_grad(model, hp, x[:64])[1])
    gld = 0.5 * np.einsum("ij,pij->p", ws.astype(np.longdouble), kr.kernel_and_grad(model, hp, x[:64], dtype=np.longdouble)[1])
    return x, hp, kinv, alpha, g, float(np.abs(g64 - gld).max() / np.abs(g64).max())


def g_tol(mid, dtype, err):
    """test_product_gpu: 1e-8 of max|g| (or four times the reference's own error), fp32 3 x 3e-3; rtol = tol, atol = tol max|g|."""
    tol = max(1e-8, 4.0 * err) if dtype == F64 else 3 * 3e-3
    print("%s %s gradient: allowance %.2e of max|g|, kernel_ref's own error %.2e" % (mid, "f64" if dtype == F64 else "f32", tol, err))
    return tol


def grad_case(mid, dtype, i, seen=None):
    """Pass i of the model's gradient: it writes the entries of its own children and leaves the others' bits alone."""
    model, d = MODELS[mid]
    n, n_pad = 333, 512
    x, hp, kinv, alpha, g, err = gradient_inputs(mid)
    kp, ap = np.eye(n_pad), np.zeros(n_pad)
    kp[:n, :n], ap[:n] = kinv, alpha
    sp, _, idx = passes_of(mid)[i]
    mine = ~others(hp.size, idx)
    tol, nhp = g_tol(mid, dtype, err), hp.size

    def case(bed):
        xd, hpd, k, al = bed.put("x", x), put_hp(bed, mid, hp, i), bed.put("kinv", kp), bed.put("alpha", ap)
        gr = bed.put("grad", shape=(nhp,), dtype=F64, role="out", written=mine)
        lw = int(bed.lib.pg_nlml_grad_worksize(n, nhp))
        w = bed.put("work", shape=(lw,), dtype=F64, role="out", written=np.zeros(lw, bool), scratch=np.ones(lw, bool))
        ok(bed, bed.lib.pg_nlml_grad(bed.h, bed.code, C.byref(sp), p(hpd), p(xd), xd.ld, n, d, p(k), k.ld, p(al), p(gr), nhp, p(w), lw, bed.st()))
        if seen is not None:
            seen.append(gr)
        return [("grad", g, mine, tol * np.abs(g).max(), tol)]

    return case


@both
@gaps
@pytest.mark.parametrize("mid", ["R1", "P1", "X1", "X2", "C1"])
def test_nlml_grad(ops, mid, dtype, gapset):
    """n = 333 inside n_pad = 512 (identity-padded K^-1, zero-padded alpha), ldx > d, workspace exactly pg_nlml_grad_worksize.  C1 pass by
    pass: each writes its own entries only (the rest of grad keeps the sentinel) and reads hp with the other pass's blocks poisoned."""
    for i in range(len(passes_of(mid))):
        run(ops, grad_case(mid, dtype, i), dtype, gapset)


@both
@pytest.mark.parametrize("mid", ["R1", "P1", "X1"])
def test_nlml_grad_routing(ops, monkeypatch, mid, dtype):
    """PG_GRAD_MFMA = 0 and the default both meet the allowance; the periodic and the product spec take the VALU contraction either way
    (same bits), the rational quadratic at d = 13 the matrix pipe by default (other bits)."""
    bits = {}
    for mode in ("0", None):
        if mode is None:
            monkeypatch.delenv("PG_GRAD_MFMA", raising=False)
        else:
            monkeypatch.setenv("PG_GRAD_MFMA", mode)
        seen = []
        run(ops, grad_case(mid, dtype, 0, seen), dtype, "mixed")
        bits[mode] = seen[1].bits()
    assert np.array_equal(bits["0"], bits[None]) == (mid != "R1")


@both
@gaps
@pytest.mark.parametrize("mid", ["P1", "X1"])
def test_nlml_grad_batched(ops, mid, dtype, gapset):
    """Three experts into columns 1: of an [nexp, 1 + nhp] block (column 0 keeps its bits), hp / alpha / outs at batch gaps, workspace
    exactly nexp * pg_nlml_grad_worksize (test_framed_gpu.test_nlml_grad_batched_values)."""
    model, d = MODELS[mid]
    n, n_pad = 333, 512
    cs = [gradient_inputs(mid, n, e) for e in range(NE)]
    spec, nhp = one_spec(mid), cs[0][1].size
    kp, ap = np.stack([np.eye(n_pad)] * NE), np.zeros((NE, n_pad))
    for e, c in enumerate(cs):
        kp[e, :n, :n], ap[e, :n] = c[2], c[3]
    gref = np.stack([np.concatenate([[0.0], c[4]]) for c in cs])
    cols = np.zeros((NE, 1 + nhp), bool)
    cols[:, 1:] = True
    tol = g_tol(mid, dtype, max(c[5] for c in cs))
    scale = np.abs(gref).max(axis=1).min()      # (the smallest of the experts' max|g|: one absolute allowance for the block)

    def case(bed):
        xd, hpd = bed.put("x", np.stack([c[0] for c in cs])), bed.put("hp", np.stack([c[1] for c in cs]), dtype=F64, batch_gap=1)
        k, al = bed.put("kinv", kp), bed.put("alpha", ap, batch_gap=2 * min_gap(dtype))
        outs = bed.put("outs", shape=(NE, 1 + nhp), dtype=F64, role="out", written=cols, batch_gap=5)
        lw = NE * int(bed.lib.pg_nlml_grad_worksize(n, nhp))
        w = bed.put("work", shape=(lw,), dtype=F64, role="out", written=np.zeros(lw, bool), scratch=np.ones(lw, bool))
        ok(bed, bed.lib.pg_nlml_grad_batched(bed.h, bed.code, C.byref(spec), p(hpd), hpd.ld, p(xd), xd.ld, xd.estride, n, d, p(k), k.ld, k.estride,
                                             p(al), al.ld, ptr_at(outs, 1), outs.ld, nhp, p(w), lw, NE, bed.st()))
        return [("outs", gref, cols, tol * scale, tol)]

    run(ops, case, dtype, gapset)


# ------------------------------------------------------------------------------------------- 7. pg_build_potrf_trtri, _checked, _batched
@functools.lru_cache(maxsize=None)
def fit_state(mid, n, n_pad, seed=0):
    """test_framed_gpu.kstate on a model of the table: noise 0.3, K = kernel_ref.kernel + 1e-7 I, its padded fit (append_ref.padded_fit)."""
    model, d = MODELS[mid]
    rng = np.random.default_rng(50 + seed + n + d)
    x, hp = rng.random((n, d)), hp_of(model, d, rng, noise=0.3)
    K = kr.kernel(model, hp, x) + 1e-7 * np.eye(n)
    L, invd, M, u, alpha = ar.padded_fit(K, rng.standard_normal(n), n_pad, garbage=np.nan)
    return dict(x=x, hp=hp, L=np.nan_to_num(L), M=np.nan_to_num(M), invd=invd, condL=float(np.sqrt(np.linalg.cond(K))))


@both
@pytest.mark.parametrize("entry", ["build", "checked", "batched"])
@pytest.mark.parametrize("mid", ["R1", "P1", "X1"])
def test_build_and_factor(ops, mid, entry, dtype):
    """K built inside the factorisation from framed X and hp (gap set `mixed`): n = 200 / 256 single and checked; three experts at
    n = 300 / 512 with hp_stride, x_stride, a_stride, inv_stride, m_stride all larger than minimal.  Allowances of
    test_framed_gpu.test_factor_schedules / test_factor_batched: the factor of a built K 1e-10 / 2e-5 cond(L), L^-1 and its diagonal
    blocks 1e-8 / 1e-9 and the forward-error bound in fp32."""
    model, d = MODELS[mid]
    spec = one_spec(mid)
    ne = NE if entry == "batched" else 1
    n, n_pad = (300, 512) if entry == "batched" else (200, 256)
    ss = [fit_state(mid, n, n_pad, e) for e in range(ne)]
    low, up = np.tril(np.ones((n_pad, n_pad), bool)), np.triu(np.ones((n_pad, n_pad), bool), 1)
    worst = max(ss, key=lambda q: q["condL"])

    def single(bed):
        s = ss[0]
        ws = int(bed.lib.pg_potrf_worksize(bed.code, n_pad))
        wmask = np.arange(ws) < n_pad * 128
        invd = bed.put("invd", shape=(ws,), role="out", written=wmask, scratch=~wmask)
        info = bed.put("info", shape=(1,), dtype=torch.int32, role="out")
        x, hpd = bed.put("x", s["x"]), bed.put("hp", s["hp"], dtype=F64)
        a = bed.put("a", shape=(n_pad, n_pad), role="out", written=low, scratch=up)
        m = bed.put("minv", shape=(n_pad, n_pad), role="out", written=low, scratch=up)
        args = (bed.h, bed.code, C.byref(spec), p(hpd), p(x), x.ld, n, d, 1e-7, p(a), a.ld, n_pad, p(invd), p(info), p(m), m.ld, bed.st())
        if entry == "checked":
            ih = C.c_int(-7)
            ok(bed, bed.lib.pg_build_potrf_trtri_checked(*args, C.byref(ih)))
            assert ih.value == 0
        else:
            ok(bed, bed.lib.pg_build_potrf_trtri(*args))
        return [("info", 0, None, 0, 0), ("a", s["L"], low, _ftol(dtype, 1e-10, 2e-5 * s["condL"]), 0),
                ("invd", np.concatenate([s["invd"].reshape(-1), np.zeros(ws - n_pad * 128)]), wmask, _inv_tol(dtype, s, 128, 1e-9), 0),
                ("minv", s["M"], low, _inv_tol(dtype, s, n_pad, 1e-8), 0)]

    def batched(bed):
        ws = int(bed.lib.pg_potrf_worksize(bed.code, n_pad))
        wmask = np.broadcast_to(np.arange(ws) < n_pad * 128, (ne, ws))
        invd = bed.put("invd", shape=(ne, ws), role="out", written=wmask, scratch=~wmask, batch_gap=2 * min_gap(dtype))
        info = bed.put("info", shape=(ne,), dtype=torch.int32, role="out")
        m = bed.put("minv", shape=(ne, n_pad, n_pad), role="out", written=low, scratch=up)
        x, hpd = bed.put("x", np.stack([s["x"] for s in ss])), bed.put("hp", np.stack([s["hp"] for s in ss]), dtype=F64, batch_gap=3)
        a = bed.put("a", shape=(ne, n_pad, n_pad), role="out", written=low, scratch=up)
        ok(bed, bed.lib.pg_build_potrf_trtri_batched(bed.h, bed.code, C.byref(spec), p(hpd), hpd.ld, p(x), x.ld, x.estride, n, d, 1e-7, p(a), a.ld,
                                                     a.estride, n_pad, p(invd), invd.ld, p(info), p(m), m.ld, m.estride, ne, bed.st()))
        return [("info", 0, None, 0, 0), ("a", np.stack([s["L"] for s in ss]), low, _ftol(dtype, 1e-10, 2e-5 * worst["condL"]), 0),
                ("minv", np.stack([s["M"] for s in ss]), low, _inv_tol(dtype, worst, n_pad, 1e-8), 0)]

    run(ops, batched if entry == "batched" else single, dtype, "mixed")


# ------------------------------------------------------------------------------------------- 8. pg_kernel_xgrad
@functools.lru_cache(maxsize=None)
def xg_inputs(mid, m=37, n=70):
    model, d = MODELS[mid]
    rng = np.random.default_rng(31 + d)
    xq, zs = rng.random((m, d)), rng.random((NE, n, d))
    hps = np.stack([hp_of(model, d, rng) for _ in range(NE)])
    us, bs = rng.standard_normal((NE, n)), rng.standard_normal((NE, m, n))
    ref_u, ref_b = np.zeros((NE, m, d)), np.zeros((NE, m, d))
    for e in range(NE):
        dks = kr.kernel_xgrad(model, hps[e], zs[e], xq)                       # [d, m, n]
        ref_u[e], ref_b[e] = np.einsum("kpi,i->pk", dks, us[e]), np.einsum("kpi,pi->pk", dks, bs[e])
    # the reference's own error in the contraction on 64 x 32 of expert 0's pairs, relative to the largest entry like the check
    b0 = bs[0][:32, :64]
    s64 = np.einsum("kpi,pi->pk", kr.kernel_xgrad(model, hps[0], zs[0][:64], xq[:32]), b0)
    sld = np.einsum("kpi,pi->pk", kr.kernel_xgrad(model, hps[0], zs[0][:64], xq[:32], dtype=np.longdouble), b0.astype(np.longdouble))
    return xq, zs, hps, us, bs, ref_u, ref_b, float(np.abs(s64 - sld).max() / np.abs(s64).max())


@both
@gaps_odd
@pytest.mark.parametrize("trans_b", [0, 1])
@pytest.mark.parametrize("mid", ["P1", "X1", "R2", "S1"])
def test_kernel_xgrad_batched(ops, mid, trans_b, dtype, gapset):
    """Three experts, each with its own hp, Z, u, B and outputs, at one shared Xq (xq_stride = 0); u and B in one call, B row-major and
    stored transposed; the call again with accumulate = 1 doubles both outputs.  u carries five entries beyond n and B three rows beyond
    what is indexed (beyond m; stored transposed: beyond n), all NaN in the framed call -- the header says they are never read.  The
    workspace is exactly pg_kernel_xgrad_worksize(h, m, n, d, 3).  Allowances: 1e-12 / 1e-4 of max|ref| (test_xgrad_gpu, test_product_gpu)."""
    model, d = MODELS[mid]
    m, n = 37, 70
    xq, zs, hps, us, bs, ref_u, ref_b, err = xg_inputs(mid)
    spec = one_spec(mid)
    tol = max(1e-12, 4.0 * err) if dtype == F64 else 1e-4
    print("%s %s xgrad: allowance %.2e of max|ref|, kernel_ref's own error %.2e" % (mid, "f64" if dtype == F64 else "f32", tol, err))
    upad, umask = np.zeros((NE, n + 5)), np.zeros((NE, n + 5), bool)
    upad[:, :n], umask[:, n:] = us, True
    stored = bs.transpose(0, 2, 1) if trans_b else bs
    bpad = np.zeros((NE, stored.shape[1] + 3, stored.shape[2]))
    bmask = np.zeros(bpad.shape, bool)
    bpad[:, :stored.shape[1]], bmask[:, stored.shape[1]:] = stored, True

    def case(bed, calls):
        q, z, hpd = bed.put("xq", xq), bed.put("z", zs), bed.put("hp", hps, dtype=F64, batch_gap=3)
        ud, bd = bed.put("u", upad, poison=umask, batch_gap=2 * min_gap(dtype) + 1), bed.put("B", bpad, poison=bmask)
        ou, ob = bed.put("out_u", shape=(NE, m, d), role="out"), bed.put("out_b", shape=(NE, m, d), role="out")
        lw = int(bed.lib.pg_kernel_xgrad_worksize(bed.h, m, n, d, NE))
        assert lw > 0
        w = bed.put("work", shape=(lw,), dtype=F64, role="out", written=np.zeros(lw, bool), scratch=np.ones(lw, bool))
        for acc in range(calls):
            ok(bed, bed.lib.pg_kernel_xgrad(bed.h, bed.code, C.byref(spec), p(hpd), hpd.ld, p(q), q.ld, 0, m, p(z), z.ld, z.estride, n, d, p(ud), ud.ld,
                                            p(ou), ou.ld, ou.estride, p(bd), bd.ld, bd.estride, trans_b, p(ob), ob.ld, ob.estride, acc, p(w), lw, NE,
                                            bed.st()))
        return [("out_u", calls * ref_u, None, tol * calls * np.abs(ref_u).max(), 0), ("out_b", calls * ref_b, None, tol * calls * np.abs(ref_b).max(), 0)]

    run(ops, case, dtype, gapset, calls=1)
    run(ops, case, dtype, gapset, calls=2)


# ------------------------------------------------------------------------------------------- 9. pg_predict_mean_q_kt_batched
@both
@gaps
@pytest.mark.parametrize("mid", ["P2", "X1"])
def test_predict_batched_prior_variance(ops, mid, dtype, gapset):
    """The one other export that takes a spec: it forms kss_e, the constant diagonal of K**, on the device from hp + e * hp_stride --
    the sum of sigma_c^2 of a sum spec, their PRODUCT of a product spec, plus the noise -- through off[] of blocks of three widths.
    Kt, Minv and alpha as in test_framed_gpu.test_prediction_entry_points (any fitted state serves: only kss depends on the spec);
    allowances as there: 1e-10, fp32 5e-4 of max(1, max|ref|)."""
    model, d = MODELS[mid]
    n, n_pad, m, m_pad = 300, 512, 37, 256
    ss = [kstate(n, n_pad, e) for e in range(NE)]
    rng = np.random.default_rng(m + d)
    hps = np.stack([hp_of(model, d, rng) for _ in range(NE)])
    kss = np.array([kr.kernel(model, hps[e], np.zeros((1, d)))[0, 0] for e in range(NE)])      # one point against itself: the prior variance
    blk = tiles_low(n_pad, n_pad)
    kts = np.zeros((NE, m_pad, n_pad))
    kts[:, :m, :n] = rng.standard_normal((NE, m, n))
    Ms, als = np.stack([s["M"] for s in ss]), np.stack([s["alpha"] for s in ss])
    vts = np.einsum("emk,enk->emn", kts, Ms)
    ref = np.concatenate([np.einsum("emn,en->em", kts, als), kss[:, None] - (vts ** 2).sum(2)], axis=1)
    spec, nw, vg = one_spec(mid), (n_pad // 64) * m_pad, 2 * min_gap(dtype)

    def case(bed):
        mm, al = bed.put("minv", Ms, poison=np.broadcast_to(~blk, Ms.shape)), bed.put("alpha", als, batch_gap=vg)
        kt, hpd = bed.put("kt", kts), bed.put("hp", hps, dtype=F64, batch_gap=1)
        mv = bed.put("meanvar", shape=(NE, 2 * m_pad), role="out", batch_gap=vg)
        w = bed.put("work", shape=(NE, nw), role="out", written=np.zeros((NE, nw), bool), scratch=np.ones((NE, nw), bool), batch_gap=vg)
        ok(bed, bed.lib.pg_predict_mean_q_kt_batched(bed.h, bed.code, n_pad, m_pad, p(kt), kt.ld, kt.estride, p(mm), mm.ld, mm.estride, p(al), al.ld,
                                                     p(mv), mv.ld, ptr_at(mv, m_pad), mv.ld, C.byref(spec), p(hpd), hpd.ld, p(w), w.ld, NE, bed.st()))
        return [("meanvar", ref, None, _ftol(dtype, 1e-10, 5e-4 * max(1.0, np.abs(ref).max())), 0)]

    run(ops, case, dtype, gapset)
