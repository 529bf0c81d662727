"""Every C-ABI entry point that takes a device buffer, called through ctypes on FRAMED operands (tests/test_framed_cpu.py checks
the list against include/pygpr_hip.h).  Framed operands (tests/framed.py) are strided views
(ld = width + gap, expert strides larger than minimal, base 16- but not 256-byte aligned) inside sentinel memory, workspaces of
exactly pg_*_worksize elements.  Per case and dtype:

  value      the logical region against NumPy / tests/kernel_ref.py / tests/append_ref.py in fp64 (never another GPU call), at
             the tolerance of the existing test of that entry point (cited at each case)
  same bits  as the same call on packed, freshly allocated operands (tiling is by index, not by address)
  guards     every word outside the views still holds the sentinel; inputs bitwise unchanged (gaps included); outputs carry no
             sentinel where the header says the call writes, and keep their bits everywhere else
  unread     parts the header says are not read hold NaN in the framed call only -- the bits still agree

Exemptions from "same bits": none.  Gaps: the smallest legal one (2 fp64 / 4 fp32 elements), 132 (wider than a tile, not a
multiple of one), and "mixed" (a different gap per operand, so that a swapped ld cannot cancel).  The scalar entry points also run
with odd gaps (1, 3).  An overrun lands in guard rows the test owns (framed.ROW_GUARD = the tallest tile), so it is detected, not
faulted on.

The kinds of this file's tables are the squared exponential, the Matern family and PG_KIND_SQDIST, whose blocks are all d + 1 wide
(make_spec below).  The kinds added since -- rational quadratic (d + 2), periodic (2 d + 1), product specs and a sum in two passes --
are framed in tests/test_framed_kinds_gpu.py (370 tests on this file's harness, by import), through every export that takes a
covariance spec; tests/test_framed_cpu.py holds that file to the header and to the kinds of pygpr_amd/_lib.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import append_ref as ar
import kernel_ref as kr
from framed import SENTINEL32, SENTINEL64, frame, min_gap

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
DTYPES = [F64, F32]
KIND = {"se": 0, "m52": 1, "sqdist": 2, "m32": 3, "m12": 4}


@pytest.fixture(scope="module")
def ops():
    from pygpr_amd._ops import get_ops

    return get_ops()


class Packed:
    """The packed stand-in of a Frame: a fresh contiguous allocation, sentinel-filled, same interface."""

    def __init__(self, shape, dtype, name):
        self.name, self.dtype = name, dtype
        self.view = torch.empty(tuple(shape), dtype=dtype, device="cuda")
        self.item = self.view.element_size()
        self.wview = self.view.view(torch.int64 if self.item == 8 else torch.int32)
        self.wview.fill_(SENTINEL64 if self.item == 8 else SENTINEL32)
        self.cols = shape[-1]
        self.rows = shape[-2] if len(shape) >= 2 else 1
        self.ld, self.estride = self.cols, self.rows * self.cols

    def fill(self, data):
        self.view.copy_(torch.as_tensor(np.array(data)).reshape(self.view.shape).to("cuda", self.dtype))
        return self

    @property
    def ptr(self):
        return self.view.data_ptr()


class Bed:
    """Allocates the operands of one call, framed or packed, and afterwards runs the frame checks on all of them."""

    def __init__(self, ops, dtype, gapset):
        self.ops, self.lib, self.h, self.dtype, self.gapset = ops, ops.lib, ops.h, dtype, gapset
        self.code = 0 if dtype == F64 else 1
        self.framed = gapset is not None
        self.items, self.k = {}, 0

    def st(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def _gap(self, dtype, ndim):
        if ndim < 2:
            return 0
        g = min_gap(dtype)
        seq = {"min": [g], "wide": [132], "mixed": [g, 132, 3 * g, 132 + g], "odd": [1, 3]}[self.gapset]
        self.k += 1
        return seq[(self.k - 1) % len(seq)]

    def put(self, name, data=None, shape=None, dtype=None, role="in", written=None, scratch=None, poison=None, batch_gap=None):
        """role: in (never written) / out (sentinel before the call) / inout (data before the call).  written: boolean mask of what
        the call must write (None with role out/inout: everything); scratch: what it may write; poison: what it must not read."""
        dtype = dtype or self.dtype
        shape = tuple(np.shape(data)) if shape is None else tuple(shape)
        if self.framed:
            item = 8 if dtype == F64 else 4
            bg = (3 * 16 // item if batch_gap is None else batch_gap) if len(shape) == 3 or (len(shape) == 2 and batch_gap is not None) else 0
            if len(shape) == 2 and batch_gap is not None:       # stacked vectors [nexp, n]: the expert stride is the row stride
                f = frame(shape, dtype, "cuda", gap=bg, name=name)
            else:
                f = frame(shape, dtype, "cuda", gap=self._gap(dtype, len(shape)), batch_gap=bg, name=name)
            assert f.ptr % 16 == 0 and f.ptr % 256 != 0
        else:
            f = Packed(shape, dtype, name)
        if data is not None:
            f.fill(data)
        if self.framed:
            if poison is not None:
                f.poison(poison)
            f.snapshot()
        self.items[name] = (f, role, written, scratch)
        return f

    def check(self):
        torch.cuda.synchronize()
        if not self.framed:
            return
        for name, (f, role, written, scratch) in self.items.items():
            f.check_guards()
            if role == "in":
                f.check_unchanged()
                continue
            w = np.ones(f.view.shape, bool) if written is None else np.broadcast_to(written, f.view.shape)
            f.check_written(w)
            f.check_unchanged(except_mask=w if scratch is None else (w | np.broadcast_to(scratch, f.view.shape)))


def p(f):
    return C.c_void_p(f.ptr) if f is not None else C.c_void_p(0)


def ok(bed, rc):
    assert rc == 0, bed.lib.pg_last_error().decode()


def make_spec(parts, d):
    from pygpr_amd._ops import make_spec as ms

    kinds, offs, noise, o = [], [], [], 0
    for q in parts:
        if q == "wn":
            noise.append(o)
            o += 1
        else:
            kinds.append(KIND[q])
            offs.append(o)
            o += d + 1
    return ms(kinds, offs, noise)


FRAMED_BED = Bed      # the bed of run()'s framed half: tests/test_streamed_gpu.py puts tests/streamed.py's StreamBed here


def run(ops, case, dtype, gapset, **kw):
    """The case on packed operands, then on framed ones: frame checks, same bits, values."""
    beds = {}
    for gs in (None, gapset):
        bed = (Bed if gs is None else FRAMED_BED)(ops, dtype, gs)
        checks = case(bed, **kw)
        bed.check()
        beds[gs] = (bed, checks)
    bed, checks = beds[gapset]
    pbed = beds[None][0]
    for name, (f, role, written, scratch) in bed.items.items():
        if role == "in":
            continue
        w = np.ones(f.view.shape, bool) if written is None else np.broadcast_to(written, f.view.shape)
        got, want = f.bits(), pbed.items[name][0].wview.cpu().numpy()
        bad = (got != want) & w
        assert not bad.any(), "%s: %d words differ from the packed call, first at %s" % (name, bad.sum(), tuple(np.argwhere(bad)[0]))
    for name, ref, mask, atol, rtol in checks:
        got = bed.items[name][0].view.double().cpu().numpy()
        m = np.ones(got.shape, bool) if mask is None else np.broadcast_to(mask, got.shape)
        np.testing.assert_allclose(got[m], np.broadcast_to(ref, got.shape)[m], atol=atol, rtol=rtol, err_msg=name)


GAPSETS = ["min", "wide", "mixed"]
both = pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
gaps = pytest.mark.parametrize("gapset", GAPSETS)
gaps_odd = pytest.mark.parametrize("gapset", GAPSETS + ["odd"])      # scalar kernels: any ld >= width


def tiles_low(m, n, bs=128):
    mask = np.ones((m, n), bool)
    for i in range(0, n, bs):
        mask[i:i + bs, i + bs:] = False
    return mask


@functools.lru_cache(maxsize=None)
def state(n, n_pad, seed=0):
    """A fitted, padded model in NumPy: K (identity pad), L, inv_diag blocks, Minv, y, u, alpha; L and Minv carry NaN above their
    diagonal 128-blocks (append_ref.padded_fit: the part the library never reads)."""
    rng = np.random.default_rng(seed + n)
    x = rng.random((n, 3))
    K = ar.se_kernel(x, x) + 0.05 * np.eye(n)
    y = rng.standard_normal(n)
    L, invd, M, u, alpha = ar.padded_fit(K, y, n_pad, garbage=np.nan)
    Kp = np.eye(n_pad)
    Kp[:n, :n] = K
    yp = np.zeros(n_pad)
    yp[:n] = y
    blk = tiles_low(n_pad, n_pad)            # what is read: on and below the diagonal 128-blocks
    return dict(condL=float(np.sqrt(np.linalg.cond(K))), K=Kp, L=np.nan_to_num(L), M=np.nan_to_num(M), invd=invd, y=yp, u=u, alpha=alpha, unread=~blk, n=n, n_pad=n_pad)


# ------------------------------------------------------------------------------------------- GEMM core
@both
@gaps
@pytest.mark.parametrize("variant", ["NT", "NN", "TN", "TT"])
def test_gemm_variants(ops, variant, dtype, gapset):
    """tolerance: test_hip_kernels.test_gemm_variants (1e-12 k / 2e-4 k)"""
    from pygpr_amd import _lib

    m, n, k = 256, 384, 208
    rng = np.random.default_rng(0)
    opa, opb, c0 = rng.standard_normal((m, k)), rng.standard_normal((k, n)), rng.standard_normal((m, n))
    code = {"NT": _lib.GEMM_NT, "NN": _lib.GEMM_NN, "TN": _lib.GEMM_TN, "TT": _lib.GEMM_TT}[variant]

    def case(bed):
        a = bed.put("a", opa.T if variant[0] == "T" else opa)
        b = bed.put("b", opb.T if variant[1] == "T" else opb)
        c = bed.put("c", c0, role="inout")
        ok(bed, bed.lib.pg_gemm_raw(bed.h, bed.code, code, m, n, k, -0.5, p(a), a.ld, p(b), b.ld, 2.0, p(c), c.ld, 0, 0, 0, bed.st()))
        return [("c", -0.5 * opa @ opb + 2.0 * c0, None, (1e-12 if dtype == F64 else 2e-4) * k, 0)]

    run(ops, case, dtype, gapset)


@both
@pytest.mark.parametrize("variant_name,tm,tn,gapset", [(v, a, b, g) for v, a, b in (("GEMM_NT", 5, 3), ("GEMM_NT_64", 5, 3), ("GEMM_NT", 4, 4)) for g in GAPSETS]
                         + [("GEMM_NT", 24, 24, "mixed"), ("GEMM_NT", 33, 33, "mixed")])
def test_gemm_tri_trapezoid_and_mixed_launch(ops, variant_name, tm, tn, dtype, gapset):
    """tri = 1 on a square (lower tiles), on a trapezoid (N < M: test_gemm_trapezoid_tiles' 5 x 3) and at the tile counts whose
    launch ends in quarter tiles (test_gemm_mixed_launch_is_bit_identical: t = 24 full, t = 33 triangular).  Tiles above the diagonal
    keep their bits.  tolerance: those tests' 1e-11 (fp64); fp32: test_gemm_skinny_chain_variants' 2e-3."""
    from pygpr_amd import _lib

    m, n, k = 128 * tm, 128 * tn, 256
    tri = 0 if tm == 24 else 1
    rng = np.random.default_rng(100 * tm + tn)
    a0, c0 = rng.standard_normal((m, k)), rng.standard_normal((m, n))
    bs = 64 if variant_name == "GEMM_NT_64" else 128
    mask = tiles_low(m, n, bs) if tri else None

    def case(bed):
        a = bed.put("a", a0)
        c = bed.put("c", c0, role="inout", written=mask)
        ok(bed, bed.lib.pg_gemm_raw(bed.h, bed.code, getattr(_lib, variant_name), m, n, k, -1.0, p(a), a.ld, p(a), a.ld, 1.0, p(c), c.ld, tri,
                                    0, 0, bed.st()))
        low = np.tril(np.ones((m, n), bool)) if tri else None
        return [("c", c0 - a0 @ a0[:n].T, low, 1e-11 if dtype == F64 else 2e-3, 0)]

    run(ops, case, dtype, gapset)


@both
@gaps
@pytest.mark.parametrize("which", ["khi1", "klo2", "klo1_tri"])
def test_gemm_k_ranges(ops, which, dtype, gapset):
    """klo / khi from a triangular operand (test_gemm_triangular_k_ranges, atol 1e-11; fp32 at test_gemm_variants' 2e-4 k).  The
    strictly upper part of the triangular operand holds NaN in the framed call: the range skips it."""
    from pygpr_amd import _lib

    n = 512
    rng = np.random.default_rng(2)
    low, dense = np.tril(rng.standard_normal((n, n))), rng.standard_normal((n, n))
    up = tiles_low(n, n) == 0                # whole tiles above the diagonal are never loaded

    def case(bed):
        lo = bed.put("low", low, poison=up)
        de = bed.put("dense", dense)
        tol = 1e-11 if dtype == F64 else 2e-4 * n
        if which == "khi1":
            c = bed.put("c", shape=(n, n), role="out")
            ok(bed, bed.lib.pg_gemm_raw(bed.h, bed.code, _lib.GEMM_NN, n, n, n, 1.0, p(lo), lo.ld, p(de), de.ld, 0.0, p(c), c.ld, 0, 0, 1, bed.st()))
            return [("c", low @ dense, None, tol, 0)]
        if which == "klo2":
            c = bed.put("c", shape=(n, n), role="out")
            ok(bed, bed.lib.pg_gemm_raw(bed.h, bed.code, _lib.GEMM_NN, n, n, n, 1.0, p(de), de.ld, p(lo), lo.ld, 0.0, p(c), c.ld, 0, 2, 0, bed.st()))
            return [("c", dense @ low, None, tol, 0)]
        c = bed.put("c", shape=(n, n), role="out", written=tiles_low(n, n))
        ok(bed, bed.lib.pg_gemm_raw(bed.h, bed.code, _lib.GEMM_TN, n, n, n, 1.0, p(lo), lo.ld, p(lo), lo.ld, 0.0, p(c), c.ld, 1, 1, 0, bed.st()))
        return [("c", low.T @ low, np.tril(np.ones((n, n), bool)), tol, 0)]

    run(ops, case, dtype, gapset)


# ------------------------------------------------------------------------------------------- covariance
def _hp(parts, d, rng):
    return np.concatenate([[0.05 + 0.1 * rng.random()] if q == "wn" else np.concatenate([[1.2], 0.4 + 0.8 * rng.random(d)]) for q in parts])


def _ktol(parts, d, dtype):
    """fp64: 1e-14 on the VALU bodies (test_kernel_build), 2e-14 on the matrix pipe (test_matrix_pipe_bodies_...), 1e-13 for the
    Matern-1/2 and -3/2 kinds (test_matern_family_gpu); fp32: 5e-6 (test_kernel_build_fp32) / 4e-6 (matrix pipe)."""
    pipe = sum(q != "wn" for q in parts) == 1 and d <= 16
    if dtype == F32:
        return 4e-6 if pipe else 5e-6
    if "m12" in parts or "m32" in parts:
        return 1e-13
    return 2e-14 if pipe else 1e-14


BUILDS = [(["se", "se", "wn"], 31), (["se", "wn"], 2), (["m52", "wn"], 13), (["m32", "wn"], 16), (["m12", "wn"], 5), (["m32", "m12", "wn"], 4)]


@both
@gaps
@pytest.mark.parametrize("parts,d", BUILDS, ids=lambda v: "+".join(v) if isinstance(v, list) else str(v))
@pytest.mark.parametrize("n", [1, 37, 300])
def test_kernel_build_symmetric(ops, parts, d, n, dtype, gapset):
    """Mirrored and lower-only symmetric builds: K[:n, :n] + identity padding on rows_pad = 512; lower_only leaves the tiles above the
    diagonal alone.  X is framed with ldx > d; its rows from n on (3 padding rows) hold NaN and are never read."""
    rng = np.random.default_rng(n + d)
    x, hp = rng.random((n + 3, d)), _hp(parts, d, rng)
    npad, tol = 512, _ktol(parts, d, dtype)
    ref = np.eye(npad)
    ref[:n, :n] = kr.kernel(parts, hp, x[:n]) + 1e-7 * np.eye(n)
    spec = make_spec(parts, d)
    pois = np.zeros((n + 3, d), bool)
    pois[n:] = True

    def case(bed, lower_only):
        xd, hpd = bed.put("x", x, poison=pois), bed.put("hp", hp, dtype=F64)
        k = bed.put("k", shape=(npad, npad), role="out", written=tiles_low(npad, npad, 64) if lower_only else None)
        ok(bed, bed.lib.pg_kernel_build(bed.h, bed.code, C.byref(spec), p(hpd), p(xd), xd.ld, n, None, 0, 0, d, lower_only, 0, 1e-7, p(k), k.ld,
                                        npad, npad, bed.st()))
        return [("k", ref, np.tril(np.ones((npad, npad), bool)) if lower_only else None, tol, tol)]

    run(ops, case, dtype, gapset, lower_only=0)
    run(ops, case, dtype, gapset, lower_only=1)


@both
@gaps
@pytest.mark.parametrize("parts,d", BUILDS, ids=lambda v: "+".join(v) if isinstance(v, list) else str(v))
@pytest.mark.parametrize("nr,nc", [(37, 300), (300, 1), (1, 37)])
def test_kernel_build_cross_and_accumulate(ops, parts, d, nr, nc, dtype, gapset):
    """Cross build (zero padding, rows_pad 256 / 512 x cols_pad 512 / 256), then an accumulate pass of the same spec onto it: K += k,
    the padding left alone (bitwise)."""
    rng = np.random.default_rng(nr + nc + d)
    xr, xc, hp = rng.random((nr, d)), rng.random((nc, d)), _hp(parts, d, rng)
    rp, cp = (512 if nr > 256 else 256), (512 if nc > 256 else 256)
    tol, spec = _ktol(parts, d, dtype), make_spec(parts, d)
    ref = np.zeros((rp, cp))
    ref[:nr, :nc] = kr.kernel(parts, hp, xc, xr)
    real = np.zeros((rp, cp), bool)
    real[:nr, :nc] = True

    def case(bed, acc):
        a, b, hpd = bed.put("xr", xr), bed.put("xc", xc), bed.put("hp", hp, dtype=F64)
        k = bed.put("k", ref if acc else None, shape=(rp, cp), role="inout" if acc else "out", written=real if acc else None)
        ok(bed, bed.lib.pg_kernel_build(bed.h, bed.code, C.byref(spec), p(hpd), p(a), a.ld, nr, p(b), b.ld, nc, d, 0, acc, 0.0, p(k), k.ld, rp, cp,
                                        bed.st()))
        atol = _ktol(["se", "se", "wn"], 31, dtype) if acc else tol      # (accumulate passes run the VALU bodies)
        return [("k", (2.0 if acc else 1.0) * ref, None, max(atol, tol) * (2 if acc else 1), max(atol, tol))]

    run(ops, case, dtype, gapset, acc=0)
    run(ops, case, dtype, gapset, acc=1)


@both
def test_kernel_build_empty_operands(ops, dtype):
    """nr == 0 or nc == 0 (which the argument checks admit): the whole output is padding -- identity (symmetric; lower 64-tiles only
    with lower_only) / zeros (cross, also with only one of nr, nc zero) -- and an empty point set is not touched (it is a valid
    one-row operand full of NaN here).  Both the VALU (d = 31) and the matrix-pipe (d = 13) configurations, single and batched,
    rows_pad 512 x cols_pad 256 for the cross builds."""
    for parts, d in ((["se", "se", "wn"], 31), (["m52", "wn"], 13)):
        hp, spec = _hp(parts, d, np.random.default_rng(1)), make_spec(parts, d)
        full = np.random.default_rng(2).random((40, d))

        def case(bed, mode, batched):
            empty = bed.put("x", np.full((1, d), np.nan))
            pts = bed.put("pts", full)
            hpd = bed.put("hp", hp, dtype=F64)
            ne = 2 if batched else 1
            sym = mode in ("sym", "low")
            rp, cp = (256, 256) if sym else (512, 256)
            wr = tiles_low(rp, cp, 64) if mode == "low" else None
            k = bed.put("k", shape=(ne, rp, cp) if batched else (rp, cp), role="out", written=wr)
            xr, nr, xc, nc = {"sym": (empty, 0, None, 0), "low": (empty, 0, None, 0), "cross00": (empty, 0, empty, 0),
                              "cross0n": (empty, 0, pts, 40), "crossn0": (pts, 40, empty, 0)}[mode]
            if batched:
                ok(bed, bed.lib.pg_kernel_build_batched(bed.h, bed.code, C.byref(spec), p(hpd), 0, p(xr), xr.ld, 0, nr, p(xc), xc.ld if xc else 0, 0,
                                                        nc, d, int(mode == "low"), 1e-7, p(k), k.ld, k.estride, rp, cp, ne, bed.st()))
            else:
                ok(bed, bed.lib.pg_kernel_build(bed.h, bed.code, C.byref(spec), p(hpd), p(xr), xr.ld, nr, p(xc), xc.ld if xc else 0, nc, d,
                                                int(mode == "low"), 0, 1e-7, p(k), k.ld, rp, cp, bed.st()))
            return [("k", np.eye(rp) if sym else np.zeros((rp, cp)), wr, 0, 0)]

        for mode in ("sym", "low", "cross00", "cross0n", "crossn0"):
            for batched in (0, 1):
                run(ops, case, dtype, "mixed", mode=mode, batched=batched)


@both
@gaps
@pytest.mark.parametrize("parts,d", [(["m52", "wn"], 13), (["se", "m32", "wn"], 31), (["se", "wn"], 2)], ids=["pipe52-13", "valu-31", "pipe-se-2"])
def test_kernel_build_batched(ops, parts, d, dtype, gapset):
    """Three experts in one launch: symmetric with per-expert points and hyper-parameters, cross with shared row points (xr_stride 0);
    k_stride larger than rows_pad * ldk.  Per expert the numbers of pg_kernel_build (same tolerances)."""
    n, m, ne = 300, 37, 3
    rng = np.random.default_rng(5)
    xs, xq = rng.random((ne, n, d)), rng.random((m, d))
    hps = np.stack([_hp(parts, d, rng) for _ in range(ne)])
    spec, tol = make_spec(parts, d), _ktol(parts, d, dtype)

    def case(bed, sym):
        x, hpd = bed.put("x", xs), bed.put("hp", hps, dtype=F64, batch_gap=4)
        if sym:
            ref = np.stack([np.eye(512)] * ne)
            for e in range(ne):
                ref[e, :n, :n] = kr.kernel(parts, hps[e], xs[e]) + 1e-7 * np.eye(n)
            k = bed.put("k", shape=(ne, 512, 512), role="out")
            ok(bed, bed.lib.pg_kernel_build_batched(bed.h, bed.code, C.byref(spec), p(hpd), hpd.ld, p(x), x.ld, x.estride, n, None, 0, 0, 0, d, 0,
                                                    1e-7, p(k), k.ld, k.estride, 512, 512, ne, bed.st()))
        else:
            q = bed.put("xq", xq)
            ref = np.zeros((ne, 256, 512))
            for e in range(ne):
                ref[e, :m, :n] = kr.kernel(parts, hps[e], xs[e], xq)
            k = bed.put("k", shape=(ne, 256, 512), role="out")
            ok(bed, bed.lib.pg_kernel_build_batched(bed.h, bed.code, C.byref(spec), p(hpd), hpd.ld, p(q), q.ld, 0, m, p(x), x.ld, x.estride, n, d, 0,
                                                    0.0, p(k), k.ld, k.estride, 256, 512, ne, bed.st()))
        return [("k", ref, None, tol, tol)]

    run(ops, case, dtype, gapset, sym=1)
    run(ops, case, dtype, gapset, sym=0)


# ------------------------------------------------------------------------------------------- factor and solves
def _ftol(dtype, f64, f32):
    return f64 if dtype == F64 else f32


@both
@gaps
@pytest.mark.parametrize("n,n_pad", [(200, 256), (1100, 1280)])
@pytest.mark.parametrize("fused", [0, 1])
def test_potrf_and_potrf_trtri(ops, n, n_pad, fused, dtype, gapset):
    """A: lower triangle in, factor out in place; its strictly upper triangle holds NaN and is never read
    (test_factor_ignores_the_upper_triangle).  inv_diag is exactly pg_potrf_worksize: the first n * 128 elements are written, the rest
    is scratch.  tolerances: 1e-11 (test_coupled_chain_factor_matches_lapack), 1e-9 on L^-1 (test_coupled_chain_fused_inverse);
    fp32 2e-5 / 2e-4 (test_potrf_fp32).  The diagonal-block inverses: fp64 1e-10 (test_coupled_chain_factor_matches_lapack); no fp32 test
    of them exists, so the bound is the forward error of a 128 x 128 triangular inverse computed from an fp32 factor:
    128 eps32 cond(L) max|inv| (about 5e-3 here); the same bound with n_pad for 128 holds the whole fp32 L^-1 (test_potrf_fp32's
    2e-4 is for K^-1 of a better conditioned matrix and does not carry over)."""
    s = state(n, n_pad)
    low, up = np.tril(np.ones((n_pad, n_pad), bool)), np.triu(np.ones((n_pad, n_pad), bool), 1)

    def case(bed):
        ws = int(bed.lib.pg_potrf_worksize(bed.code, n_pad))
        a = bed.put("a", s["K"], role="inout", written=low, scratch=up, poison=up)
        wmask = np.arange(ws) < n_pad * 128
        invd = bed.put("invd", shape=(ws,), role="out", written=wmask, scratch=~wmask)
        info = bed.put("info", shape=(1,), dtype=torch.int32, role="out")
        checks = [("a", s["L"], low, _ftol(dtype, 1e-11, 2e-5), 0), ("info", 0, None, 0, 0),
                  ("invd", s["invd"].reshape(-1), None, _ftol(dtype, 1e-10, 128 * 2.0 ** -24 * s["condL"] * np.abs(s["invd"]).max()), 0)]
        if fused:
            m = bed.put("minv", shape=(n_pad, n_pad), role="out", written=low, scratch=up)
            ok(bed, bed.lib.pg_potrf_trtri(bed.h, bed.code, n_pad, p(a), a.ld, p(invd), p(info), p(m), m.ld, bed.st()))
            checks.append(("minv", s["M"], low, _ftol(dtype, 1e-9, n_pad * 2.0 ** -24 * s["condL"] * np.abs(s["M"]).max()), 0))
        else:
            ok(bed, bed.lib.pg_potrf(bed.h, bed.code, n_pad, p(a), a.ld, p(invd), p(info), bed.st()))
        checks[2] = ("invd", np.concatenate([s["invd"].reshape(-1), np.zeros(ws - n_pad * 128)]), wmask, checks[2][3], 0)
        return checks

    run(ops, case, dtype, gapset)


@both
@gaps
@pytest.mark.parametrize("n,n_pad", [(700, 768), (2200, 2304)])
def test_solves_from_the_factor(ops, n, n_pad, dtype, gapset):
    """pg_potrs_vec (workspace exactly pg_potrs_vec_worksize: both layouts, below and above 2048), pg_trtri, pg_lauum, pg_potri (its
    n x n work receives L^-1 with ld = n), pg_trmv both ways, pg_logdet, pg_nlml_value, pg_tril, pg_symmetrize.  L and Minv hold NaN
    above their diagonal 128-blocks.  tolerances: test_potrf_solves_inverse / test_potrs_vec_blocked_sweeps / test_potri_and_logdet
    (fp64), test_potrf_fp32 / test_potrs_vec_blocked_sweeps (fp32)."""
    s = state(n, n_pad)
    low, blk = np.tril(np.ones((n_pad, n_pad), bool)), ~s["unread"]
    kinv = s["M"].T @ s["M"]
    xref = kinv @ s["y"]
    rng = np.random.default_rng(9)
    v = rng.standard_normal(n_pad)

    def potrs_vec(bed):
        l, invd, y = bed.put("l", s["L"], poison=s["unread"]), bed.put("invd", s["invd"].reshape(-1)), bed.put("y", s["y"])
        x = bed.put("x", shape=(n_pad,), role="out")
        ws = int(bed.lib.pg_potrs_vec_worksize(bed.code, n_pad))
        w = bed.put("work", shape=(ws,), role="out", written=np.zeros(ws, bool), scratch=np.ones(ws, bool))
        ok(bed, bed.lib.pg_potrs_vec(bed.h, bed.code, n_pad, p(l), l.ld, p(invd), p(y), p(x), p(w), bed.st()))
        return [("x", xref, None, _ftol(dtype, 1e-11, 5e-4) * np.abs(xref).max(), 0)]

    def trtri(bed):
        l, invd = bed.put("l", s["L"], poison=s["unread"]), bed.put("invd", s["invd"].reshape(-1))
        m = bed.put("minv", shape=(n_pad, n_pad), role="out", written=low, scratch=~low)
        ok(bed, bed.lib.pg_trtri(bed.h, bed.code, n_pad, p(l), l.ld, p(invd), p(m), m.ld, bed.st()))
        return [("minv", s["M"], low, _ftol(dtype, 1e-11, 2e-4), 0)]

    def lauum(bed):
        m = bed.put("minv", s["M"], poison=s["unread"])
        k = bed.put("kinv", shape=(n_pad, n_pad), role="out", written=low, scratch=blk & ~low)
        ok(bed, bed.lib.pg_lauum(bed.h, bed.code, n_pad, p(m), m.ld, p(k), k.ld, bed.st()))
        return [("kinv", kinv, low, _ftol(dtype, 1e-10, 2e-4) * max(1.0, np.abs(kinv).max()), 0)]

    def potri(bed):
        l, invd = bed.put("l", s["L"], poison=s["unread"]), bed.put("invd", s["invd"].reshape(-1))
        k = bed.put("kinv", shape=(n_pad, n_pad), role="out", written=low, scratch=blk & ~low)
        w = bed.put("work", shape=(n_pad * n_pad,), role="out", written=low.reshape(-1), scratch=~low.reshape(-1))
        ok(bed, bed.lib.pg_potri(bed.h, bed.code, n_pad, p(l), l.ld, p(invd), p(k), k.ld, p(w), bed.st()))
        return [("kinv", kinv, low, _ftol(dtype, 1e-11, 2e-4) * max(1.0, np.abs(kinv).max()), 0),
                ("work", s["M"].reshape(-1), low.reshape(-1), _ftol(dtype, 1e-11, 2e-4), 0)]

    def trmv(bed, trans):
        m, x = bed.put("minv", s["M"], poison=s["unread"]), bed.put("x", v)
        y = bed.put("y", shape=(n_pad,), role="out")
        nw = (n_pad // 256) * n_pad
        w = bed.put("work", shape=(nw,), role="out", written=np.zeros(nw, bool), scratch=np.ones(nw, bool))
        ok(bed, bed.lib.pg_trmv(bed.h, bed.code, n_pad, p(m), m.ld, trans, p(x), p(y), p(w), bed.st()))
        ref = (s["M"].T if trans else s["M"]) @ v
        return [("y", ref, None, _ftol(dtype, 1e-11, 5e-4) * np.abs(ref).max(), 0)]

    for case, kw in ((potrs_vec, {}), (trtri, {}), (lauum, {}), (potri, {}), (trmv, dict(trans=0)), (trmv, dict(trans=1))):
        run(ops, case, dtype, gapset, **kw)


@both
@gaps_odd
def test_scalar_entry_points_take_any_ld(ops, dtype, gapset):
    """pg_tril, pg_symmetrize, pg_logdet, pg_nlml_value: scalar kernels, so odd leading dimensions (gaps 1 and 3) are legal.
    tolerances: test_potri_and_logdet (rtol 1e-12), test_nlml_value_and_grad (rtol 1e-11); fp32 1e-5 (the 1e-3 class of the module
    docstring of test_hip_kernels.py is for O(n^3) results; these are sums of n fp32 terms accumulated in fp64)."""
    n, n_pad = 300, 512
    s = state(n, n_pad)
    rng = np.random.default_rng(3)
    a0 = rng.standard_normal((n_pad, n_pad))
    up = np.triu(np.ones((n_pad, n_pad), bool), 1)
    up[n:, :] = False
    up[:, n:] = False
    diag = np.diag(s["L"])[:n]
    a0r = a0 if dtype == F64 else a0.astype(np.float32).astype(np.float64)      # what the device holds

    def tril(bed):
        a = bed.put("a", a0, role="inout", written=up)
        ok(bed, bed.lib.pg_tril(bed.h, bed.code, n, p(a), a.ld, bed.st()))
        return [("a", np.where(up, 0.0, a0r), None, 0, 0)]

    def symmetrize(bed):
        a = bed.put("a", a0, role="inout", written=up)
        ok(bed, bed.lib.pg_symmetrize(bed.h, bed.code, n, p(a), a.ld, bed.st()))
        return [("a", np.where(up, a0r.T, a0r), None, 0, 0)]

    def logdet(bed):
        l = bed.put("l", s["L"], poison=s["unread"])
        out = bed.put("out", shape=(1,), dtype=F64, role="out")
        ok(bed, bed.lib.pg_logdet(bed.h, bed.code, n, p(l), l.ld, p(out), bed.st()))
        return [("out", 2.0 * np.log(diag).sum(), None, 0, _ftol(dtype, 1e-12, 1e-5))]

    def nlml_value(bed):
        l, y, al = bed.put("l", s["L"], poison=s["unread"]), bed.put("y", s["y"]), bed.put("alpha", s["alpha"])
        out = bed.put("out", shape=(1,), dtype=F64, role="out")
        ok(bed, bed.lib.pg_nlml_value(bed.h, bed.code, n, p(l), l.ld, p(y), p(al), p(out), bed.st()))
        ref = 0.5 * s["y"] @ s["alpha"] + np.log(diag).sum() + 0.5 * n * np.log(2.0 * np.pi)
        return [("out", ref, None, 0, _ftol(dtype, 1e-11, 1e-5))]

    for case in (tril, symmetrize, logdet, nlml_value):
        run(ops, case, dtype, gapset)


@both
@gaps
@pytest.mark.parametrize("nrhs", [128, 384])
def test_potrs_and_trsm_matrix_rhs(ops, nrhs, dtype, gapset):
    """pg_potrs / pg_trsm_lower with Minv given and with L (Minv formed in `work`, which is exactly pg_potrs_worksize: n * n for
    L^-1 then n * nrhs).  tolerances: test_potrs_matrix_rhs_and_trsm (1e-10 / 1e-11 of max|ref|); fp32: 5e-4 of max|ref|
    (test_potrs_vec_blocked_sweeps)."""
    n, n_pad = 700, 768
    s = state(n, n_pad)
    rng = np.random.default_rng(nrhs)
    b0 = rng.standard_normal((n_pad, nrhs))
    vref = s["M"] @ b0
    xref = s["M"].T @ vref

    def case(bed, both_, have_minv):
        b = bed.put("b", b0)
        l = m = invd = None
        if have_minv:
            m = bed.put("minv", s["M"], poison=s["unread"])
        else:
            l, invd = bed.put("l", s["L"], poison=s["unread"]), bed.put("invd", s["invd"].reshape(-1))
        x = bed.put("x", shape=(n_pad, nrhs), role="out")
        ws = int(bed.lib.pg_potrs_worksize(bed.code, n_pad, nrhs, have_minv))
        w = bed.put("work", shape=(ws,), role="out", written=np.zeros(ws, bool), scratch=np.ones(ws, bool))
        fn = bed.lib.pg_potrs if both_ else bed.lib.pg_trsm_lower
        ok(bed, fn(bed.h, bed.code, n_pad, nrhs, p(l), l.ld if l else 0, p(invd), p(m), m.ld if m else 0, p(b), b.ld, p(x), x.ld, p(w), bed.st()))
        ref = xref if both_ else vref
        return [("x", ref, None, _ftol(dtype, 1e-10 if both_ else 1e-11, 5e-4) * np.abs(ref).max(), 0)]

    for both_ in (1, 0):
        for have_minv in (1, 0):
            run(ops, case, dtype, gapset, both_=both_, have_minv=have_minv)


# ------------------------------------------------------------------------------------------- gradient: NaN coordinates
@pytest.mark.parametrize("kind", ["se", "m52", "m32", "m12"])
def test_nlml_grad_propagates_a_nan_coordinate(ops, kind):
    """One NaN coordinate (inputs as in test_kernel_build_propagates_nan): the gradient is a contraction over all pairs, so the
    signal variance and every length scale of the component come out NaN -- in fp64 and fp32 alike, with the point in an interior
    tile (row 23 of 300) and in the ragged edge tile (row 290).  The fp32 interior Matern body used to clamp the squared distance
    with a max, which turned the NaN into 0 and gave a finite gradient."""
    parts, d, n, n_pad = [kind, "wn"], 3, 300, 512
    rng = np.random.default_rng(4)
    hp, spec = np.array([1.0, 0.7, 0.8, 0.9, 0.1]), make_spec([kind, "wn"], 3)
    kinv, alpha = np.eye(n_pad) + 0.01, rng.standard_normal(n_pad)
    seen = {}
    for dtype in DTYPES:
        for row in (23, 290):
            x = rng.random((n, d))
            x[row, 1] = np.nan
            bed = Bed(ops, dtype, "min")
            xd, hpd, k, al = bed.put("x", x), bed.put("hp", hp, dtype=F64), bed.put("kinv", kinv), bed.put("alpha", alpha)
            g = bed.put("grad", shape=(5,), dtype=F64, role="out", written=np.arange(5) < 5)
            lw = int(bed.lib.pg_nlml_grad_worksize(n, 5))
            w = bed.put("work", shape=(lw,), dtype=F64, role="out", written=np.zeros(lw, bool), scratch=np.ones(lw, bool))
            ok(bed, bed.lib.pg_nlml_grad(bed.h, bed.code, C.byref(spec), p(hpd), p(xd), xd.ld, n, d, p(k), k.ld, p(al), p(g), 5, p(w), lw, bed.st()))
            bed.check()
            seen[(dtype, row)] = np.isnan(g.view.cpu().numpy())
    want = np.array([True, True, True, True, False])          # sigma and l_1..l_3 of the component; the noise term has no pair
    for key, got in seen.items():
        assert np.array_equal(got, want), (key, got)


# ------------------------------------------------------------------------------------------- refusals (host only: nothing is launched)
def test_misaligned_operands_are_refused_on_the_host(ops):
    """Entry points whose kernels move 16-byte words at base + r * ld + c refuse an ld, a base or an expert stride that breaks
    16-byte alignment: a negative status and, after EACH call, the alignment text from pg_last_error naming the operand; nothing is
    enqueued (every buffer keeps its sentinel).  Also the new ld >= width checks."""
    lib, h, st = ops.lib, ops.h, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n, nexp = 256, 2
    spec = make_spec(GPARTS, GD)
    for dtype in DTYPES:
        code, item = (0, 8) if dtype == F64 else (1, 4)
        g = min_gap(dtype)
        odd = frame((n, n), dtype, "cuda", gap=1, name="odd")                          # odd ld
        off = frame((n, n), dtype, "cuda", gap=g, lead=16 // item + 1, name="off")     # base one element off
        good, good2 = frame((n, n), dtype, "cuda", gap=g, name="good"), frame((n, n), dtype, "cuda", gap=g, name="good2")
        invd = frame((int(lib.pg_potrf_worksize(code, n)),), dtype, "cuda", name="invd")
        info = frame((nexp,), torch.int32, "cuda", name="info")
        vec, vec2, vec3 = (frame((4 * n,), dtype, "cuda", name="vec%d" % i) for i in range(3))
        voff = frame((n,), dtype, "cuda", lead=16 // item + 1, name="voff")
        hp = frame((5,), F64, "cuda", name="hp")
        x = frame((n, GD), dtype, "cuda", name="x")
        grad = frame((5,), F64, "cuda", name="grad")
        every = [odd, off, good, good2, invd, info, vec, vec2, vec3, voff, hp, x, grad]
        G, G2, V = (p(good), good.ld), (p(good2), good2.ld), p(vec)
        bs = n * good.ld + 1                                                           # an expert stride that is not a multiple of 16 bytes
        for bad in (odd, off):
            B = (p(bad), bad.ld)
            calls = {
                "gemm A": lambda: lib.pg_gemm_raw(h, code, 0, n, n, n, 1.0, *B, *G, 0.0, *G2, 0, 0, 0, st),
                "gemm B": lambda: lib.pg_gemm_raw(h, code, 0, n, n, n, 1.0, *G, *B, 0.0, *G2, 0, 0, 0, st),
                "gemm C": lambda: lib.pg_gemm_raw(h, code, 0, n, n, n, 1.0, *G, *G, 0.0, *B, 0, 0, 0, st),
                "kernel_build K": lambda: lib.pg_kernel_build(h, code, C.byref(spec), p(hp), p(x), x.ld, n, None, 0, 0, GD, 0, 0, 0.0, *B, n, n, st),
                "potrf A": lambda: lib.pg_potrf(h, code, n, *B, p(invd), p(info), st),
                "potrf_trtri Minv": lambda: lib.pg_potrf_trtri(h, code, n, *G, p(invd), p(info), *B, st),
                "build A": lambda: lib.pg_build_potrf_trtri(h, code, C.byref(spec), p(hp), p(x), x.ld, n, GD, 0.0, *B, n, p(invd), p(info), *G, st),
                "build Minv": lambda: lib.pg_build_potrf_trtri(h, code, C.byref(spec), p(hp), p(x), x.ld, n, GD, 0.0, *G, n, p(invd), p(info), *B, st),
                "trtri L": lambda: lib.pg_trtri(h, code, n, *B, p(invd), *G, st),
                "trtri Minv": lambda: lib.pg_trtri(h, code, n, *G, p(invd), *B, st),
                "lauum Kinv": lambda: lib.pg_lauum(h, code, n, *G, *B, st),
                "lauum_batched Minv": lambda: lib.pg_lauum_batched(h, code, n, *B, 0, *G, 0, 1, st),
                "potri L": lambda: lib.pg_potri(h, code, n, *B, p(invd), *G, p(good2), st),
                "potrs_vec L": lambda: lib.pg_potrs_vec(h, code, n, *B, p(invd), V, p(vec2), p(vec3), st),
                "potrs B": lambda: lib.pg_potrs(h, code, n, n, None, 0, None, *G, *B, *G2, V, st),
                "potrs X": lambda: lib.pg_potrs(h, code, n, n, None, 0, None, *G, *G2, *B, V, st),
                "trsm Minv": lambda: lib.pg_trsm_lower(h, code, n, n, None, 0, None, *B, *G, *G2, V, st),
                "trmv Minv": lambda: lib.pg_trmv(h, code, n, *B, 1, V, p(vec2), p(vec3), st),
                "alpha_batched Minv": lambda: lib.pg_alpha_batched(h, code, n, *B, 0, V, 0, p(vec2), 0, p(vec3), 0, p(invd), 0, 1, st),
                "alpha_nlml_async Minv": lambda: lib.pg_alpha_nlml_async(h, code, n, n, *G, *B, V, p(vec2), p(vec3), p(invd), p(grad), st),
                "nlml_grad Kinv": lambda: lib.pg_nlml_grad(h, code, C.byref(spec), p(hp), p(x), x.ld, n, GD, *B, V, p(grad), 5, p(invd), 1 << 20, st),
                "predict_mean_q Ks": lambda: lib.pg_predict_mean_q(h, code, n, n, *B, *G, V, p(vec2), p(vec3), 1.0, p(invd), st),
                "predict_mean_q_kt Minv": lambda: lib.pg_predict_mean_q_kt(h, code, n, n, *G, *B, V, p(vec2), p(vec3), 1.0, p(invd), st),
                "trmm_lower Ks": lambda: lib.pg_trmm_lower(h, code, n, n, *G, *B, *G2, st),
                "trmm_lower_kt Vt": lambda: lib.pg_trmm_lower_kt_batched(h, code, n, n, *G, 0, *G2, 0, *B, 0, 1, st),
                "syrk_tn C": lambda: lib.pg_syrk_tn_sub(h, code, n, n, *G, *B, 1, st),
                "syrk_nt Vt": lambda: lib.pg_syrk_nt_sub_batched(h, code, n, n, *B, 0, *G, 0, 1, 1, st),
            }
            for what, call in calls.items():
                assert call() < 0, what
                assert b"16-byte aligned" in lib.pg_last_error(), (what, lib.pg_last_error())
        strides = {      # expert strides and vector bases
            "kernel_build_batched k_stride": lambda: lib.pg_kernel_build_batched(h, code, C.byref(spec), p(hp), 0, p(x), x.ld, 0, n, None, 0, 0, 0, GD, 0,
                                                                                 0.0, *G, bs, n, n, nexp, st),
            "factor_batched a_stride": lambda: lib.pg_build_potrf_trtri_batched(h, code, None, None, 0, None, 0, 0, n, 0, 0.0, *G, bs, n, p(invd),
                                                                                invd.cols, p(info), None, 0, 0, nexp, st),
            "lauum_batched k_stride": lambda: lib.pg_lauum_batched(h, code, n, *G, n * good.ld, *G2, bs, nexp, st),
            "alpha_batched y_stride": lambda: lib.pg_alpha_batched(h, code, n, *G, 0, V, n + 1, p(vec2), n, p(vec3), n, p(invd), n, nexp, st),
            "alpha_nlml_batched u_stride": lambda: lib.pg_alpha_nlml_batched(h, code, n, n, *G, 0, V, n, p(vec2), n + 1, p(vec3), n, p(invd), n, p(grad),
                                                                             1, nexp, st),
            "nlml_grad_batched k_stride": lambda: lib.pg_nlml_grad_batched(h, code, C.byref(spec), p(hp), 0, p(x), x.ld, 0, n, GD, *G, bs, V, n, p(grad),
                                                                           0, 5, p(invd), 1 << 20, nexp, st),
            "predict_batched kt_stride": lambda: lib.pg_predict_mean_q_kt_batched(h, code, n, n, *G, bs, None, 0, 0, V, n, p(vec2), n, None, 0, None, None,
                                                                                  0, p(invd), 0, nexp, st),
            "syrk_nt c_stride": lambda: lib.pg_syrk_nt_sub_batched(h, code, n, n, *G, n * good.ld, *G2, bs, nexp, 1, st),
            "trmv x": lambda: lib.pg_trmv(h, code, n, *G, 0, p(voff), V, None, st),
            "potrs_vec y": lambda: lib.pg_potrs_vec(h, code, n, *G, p(invd), p(voff), V, p(vec2), st),
        }
        for what, call in strides.items():
            assert call() < 0, what
            assert b"16-byte aligned" in lib.pg_last_error(), (what, lib.pg_last_error())
        small = {        # ld < width where no check existed
            "trtri ldl": lambda: lib.pg_trtri(h, code, 2 * n, *G, p(invd), *G2, st),
            "lauum ldm": lambda: lib.pg_lauum(h, code, 2 * n, *G, *G2, st),
            "trmv ldm": lambda: lib.pg_trmv(h, code, 2 * n, *G, 0, V, p(vec2), None, st),
            "potrs_vec ldl": lambda: lib.pg_potrs_vec(h, code, 2 * n, *G, p(invd), V, p(vec2), p(vec3), st),
            "nlml_grad ldk": lambda: lib.pg_nlml_grad(h, code, C.byref(spec), p(hp), p(x), x.ld, 2 * n, GD, *G, V, p(grad), 5, p(invd), 1 << 20, st),
            "nlml_grad ldx": lambda: lib.pg_nlml_grad(h, code, C.byref(spec), p(hp), p(x), GD - 1, n, GD, *G, V, p(grad), 5, p(invd), 1 << 20, st),
            "trmm_lower ldv": lambda: lib.pg_trmm_lower(h, code, n, 2 * n, *G, *G2, *G, st),
            "syrk_tn ldc": lambda: lib.pg_syrk_tn_sub(h, code, 2 * n, n, *G, *G2, 1, st),
            "predict_mean_q ldks": lambda: lib.pg_predict_mean_q(h, code, n, 2 * n, *G, *G2, V, p(vec2), p(vec3), 1.0, p(invd), st),
        }
        for what, call in small.items():
            assert call() < 0, what
            assert b"leading dimension" in lib.pg_last_error() or b"ld" in lib.pg_last_error(), (what, lib.pg_last_error())
        torch.cuda.synchronize()
        for f in every:
            f.check_guards()
            assert bool((f.wview == (SENTINEL64 if f.item == 8 else SENTINEL32)).all()), f.name     # nothing ran


# =========================================================================================== second table: everything else
def ptr_at(f, elems):
    """base + elems elements (what `outs[:, 1:]` or `work + n * n` is to a C caller)."""
    return C.c_void_p(f.ptr + elems * f.item)


GPARTS, GD = ["se", "wn"], 3


@functools.lru_cache(maxsize=None)
def kstate(n, n_pad, seed=0):
    """A model whose K comes from the covariance itself (Compose([SE, WN]), d = 3, jitter 1e-7): x, hp, y and the padded fit."""
    rng = np.random.default_rng(50 + seed + n)
    x = rng.random((n, GD))
    hp = np.array([1.1 + 0.1 * seed, 0.9, 1.2, 0.7, 0.3])
    K = kr.kernel(GPARTS, hp, x) + 1e-7 * np.eye(n)
    y = rng.standard_normal(n)
    L, invd, M, u, alpha = ar.padded_fit(K, y, n_pad, garbage=np.nan)
    yp = np.zeros(n_pad)
    yp[:n] = y
    nlml = 0.5 * y @ alpha[:n] + np.log(np.diag(L)[:n]).sum() + 0.5 * n * np.log(2.0 * np.pi)
    return dict(x=x, hp=hp, L=np.nan_to_num(L), M=np.nan_to_num(M), invd=invd, y=yp, u=u, alpha=alpha, nlml=nlml, unread=~tiles_low(n_pad, n_pad),
                condL=float(np.sqrt(np.linalg.cond(K))), n=n, n_pad=n_pad)


def _inv_tol(dtype, s, width, f64):
    """fp32 bound of an inverse computed from an fp32 factor: width eps32 cond(L) max|ref| (see test_potrf_and_potrf_trtri)."""
    return f64 if dtype == F64 else width * 2.0 ** -24 * s["condL"] * max(np.abs(s["M"]).max(), 1.0)


@both
@pytest.mark.parametrize("n,n_pad,mode,gapset", [(200, 256, "plain", g) for g in GAPSETS] + [(900, 1024, "plain", "mixed"), (900, 1024, "split", "mixed"),
                                                  (3000, 3072, "coupled", "mixed"), (3000, 3072, "classic", "mixed")])
@pytest.mark.parametrize("entry", ["potrf", "build", "checked"])
def test_factor_schedules(ops, entry, n, n_pad, mode, gapset, dtype):
    """pg_potrf / pg_build_potrf_trtri / _checked (with Minv) on framed A, inv_diag (exactly pg_potrf_worksize), info and Minv: the
    flag-coupled chain on (n_pad = 3072: six outer panels) and off (pg_set_coupled_chain), the recursive split lowered to 512
    (pg_set_recursive_split, n_pad = 1024).  tolerances as test_potrf_and_potrf_trtri (test_build_folded_into_the_factorisation:
    1e-10 on the factor of a built K)."""
    s = kstate(n, n_pad)
    low, up = np.tril(np.ones((n_pad, n_pad), bool)), np.triu(np.ones((n_pad, n_pad), bool), 1)
    spec = make_spec(GPARTS, GD)
    Kp = np.eye(n_pad)
    Kp[:n, :n] = kr.kernel(GPARTS, s["hp"], s["x"]) + 1e-7 * np.eye(n)

    def case(bed):
        ws = int(bed.lib.pg_potrf_worksize(bed.code, n_pad))
        wmask = np.arange(ws) < n_pad * 128
        invd = bed.put("invd", shape=(ws,), role="out", written=wmask, scratch=~wmask)
        info = bed.put("info", shape=(1,), dtype=torch.int32, role="out")
        checks = [("info", 0, None, 0, 0), ("invd", np.concatenate([s["invd"].reshape(-1), np.zeros(ws - n_pad * 128)]), wmask,
                                            _inv_tol(dtype, s, 128, 1e-9), 0)]
        if entry == "potrf":
            a = bed.put("a", Kp, role="inout", written=low, scratch=up, poison=up)
            ok(bed, bed.lib.pg_potrf(bed.h, bed.code, n_pad, p(a), a.ld, p(invd), p(info), bed.st()))
        else:
            x, hpd = bed.put("x", s["x"]), bed.put("hp", s["hp"], dtype=F64)
            a = bed.put("a", shape=(n_pad, n_pad), role="out", written=low, scratch=up)
            m = bed.put("minv", shape=(n_pad, n_pad), role="out", written=low, scratch=up)
            args = (bed.h, bed.code, C.byref(spec), p(hpd), p(x), x.ld, n, GD, 1e-7, p(a), a.ld, n_pad, p(invd), p(info), p(m), m.ld, bed.st())
            if entry == "checked":
                ih = C.c_int(-7)
                ok(bed, bed.lib.pg_build_potrf_trtri_checked(*args, C.byref(ih)))
                assert ih.value == 0
            else:
                ok(bed, bed.lib.pg_build_potrf_trtri(*args))
            checks.append(("minv", s["M"], low, _inv_tol(dtype, s, n_pad, 1e-8), 0))
        checks.append(("a", s["L"], low, _ftol(dtype, 1e-10, 2e-5 * s["condL"]), 0))
        return checks

    lib, h = ops.lib, ops.h
    try:
        if mode == "split":
            assert lib.pg_set_recursive_split(h, 512) == 0
        if mode == "classic":
            assert lib.pg_set_coupled_chain(h, 0) == 0
        run(ops, case, dtype, gapset)
        if mode == "coupled" and lib.pg_coupled_chain(h) == 1:
            assert lib.pg_last_coupled_panels(h) > 0
        if mode == "classic":
            assert lib.pg_last_coupled_panels(h) == 0
    finally:
        lib.pg_set_recursive_split(h, 16384)
        lib.pg_set_coupled_chain(h, 1)


@both
@gaps
@pytest.mark.parametrize("with_x", [1, 0])
def test_factor_batched(ops, with_x, dtype, gapset):
    """pg_build_potrf_trtri_batched, three experts, X given (per-expert points and hyper-parameters) and X == NULL (A holds the
    matrices); a_stride, inv_stride, m_stride larger than minimal.  tolerances: test_batched_factorisation (1e-11 / 1e-9; 1e-10 with the
    folded build); fp32 as test_potrf_and_potrf_trtri."""
    n, n_pad, ne = 300, 512, 3
    ss = [kstate(n, n_pad, e) for e in range(ne)]
    low, up = np.tril(np.ones((n_pad, n_pad), bool)), np.triu(np.ones((n_pad, n_pad), bool), 1)
    spec = make_spec(GPARTS, GD)
    Ks = np.stack([np.eye(n_pad)] * ne)
    for e, s in enumerate(ss):
        Ks[e, :n, :n] = kr.kernel(GPARTS, s["hp"], s["x"]) + 1e-7 * np.eye(n)

    def case(bed):
        ws = int(bed.lib.pg_potrf_worksize(bed.code, n_pad))
        wmask = np.broadcast_to(np.arange(ws) < n_pad * 128, (ne, ws))
        invd = bed.put("invd", shape=(ne, ws), role="out", written=wmask, scratch=~wmask, batch_gap=2 * min_gap(dtype))
        info = bed.put("info", shape=(ne,), dtype=torch.int32, role="out")
        m = bed.put("minv", shape=(ne, n_pad, n_pad), role="out", written=low, scratch=up)
        if with_x:
            x, hpd = bed.put("x", np.stack([s["x"] for s in ss])), bed.put("hp", np.stack([s["hp"] for s in ss]), dtype=F64, batch_gap=3)
            a = bed.put("a", shape=(ne, n_pad, n_pad), role="out", written=low, scratch=up)
            ok(bed, bed.lib.pg_build_potrf_trtri_batched(bed.h, bed.code, C.byref(spec), p(hpd), hpd.ld, p(x), x.ld, x.estride, n, GD, 1e-7, p(a),
                                                         a.ld, a.estride, n_pad, p(invd), invd.ld, p(info), p(m), m.ld, m.estride, ne, bed.st()))
        else:
            a = bed.put("a", Ks, role="inout", written=low, scratch=up, poison=np.broadcast_to(up, Ks.shape))
            ok(bed, bed.lib.pg_build_potrf_trtri_batched(bed.h, bed.code, None, None, 0, None, 0, 0, n_pad, 0, 0.0, p(a), a.ld, a.estride, n_pad,
                                                         p(invd), invd.ld, p(info), p(m), m.ld, m.estride, ne, bed.st()))
        s0 = ss[0]
        return [("info", 0, None, 0, 0), ("a", np.stack([s["L"] for s in ss]), low, _ftol(dtype, 1e-10, 2e-5 * s0["condL"]), 0),
                ("minv", np.stack([s["M"] for s in ss]), low, _inv_tol(dtype, max(ss, key=lambda q: q["condL"]), n_pad, 1e-8), 0)]

    run(ops, case, dtype, gapset)


@both
@gaps
def test_alpha_nlml_and_lauum_batched(ops, dtype, gapset):
    """pg_alpha_batched, pg_alpha_nlml_batched (three experts, every operand at a stride larger than minimal, out with a stride),
    pg_alpha_nlml_async and pg_lauum_batched.  Minv holds NaN above its diagonal 128-blocks.  tolerances: alpha as
    test_potrs_vec_blocked_sweeps (1e-11 / 5e-4 of max|ref|), NLML rtol 1e-10 (test_batched_gradient_path_...; fp32 1e-5 as
    test_scalar_entry_points_take_any_ld), K^-1 as test_solves_from_the_factor."""
    n, n_pad, ne = 300, 512, 3
    ss = [kstate(n, n_pad, e) for e in range(ne)]
    low, blk = np.tril(np.ones((n_pad, n_pad), bool)), tiles_low(n_pad, n_pad)
    Ms, ys = np.stack([s["M"] for s in ss]), np.stack([s["y"] for s in ss])
    us, als = np.stack([s["u"] for s in ss]), np.stack([s["alpha"] for s in ss])
    nw = (n_pad // 256) * n_pad
    vg = 2 * min_gap(dtype)
    atol = _ftol(dtype, 1e-11, 5e-4)

    def batched(bed, with_nlml):
        m = bed.put("minv", Ms, poison=np.broadcast_to(~blk, Ms.shape))
        y = bed.put("y", ys, batch_gap=vg)
        u = bed.put("u", shape=(ne, n_pad), role="out", batch_gap=vg)
        al = bed.put("alpha", shape=(ne, n_pad), role="out", batch_gap=2 * vg)
        w = bed.put("work", shape=(ne, nw), role="out", written=np.zeros((ne, nw), bool), scratch=np.ones((ne, nw), bool), batch_gap=vg)
        checks = [("u", us, None, atol * np.abs(us).max(), 0), ("alpha", als, None, atol * np.abs(als).max(), 0)]
        if with_nlml:
            col0 = np.zeros((ne, 3), bool)
            col0[:, 0] = True
            out = bed.put("out", shape=(ne, 3), dtype=F64, role="out", written=col0, batch_gap=0)
            ok(bed, bed.lib.pg_alpha_nlml_batched(bed.h, bed.code, n, n_pad, p(m), m.ld, m.estride, p(y), y.ld, p(u), u.ld, p(al), al.ld, p(w), w.ld,
                                                  p(out), out.ld, ne, bed.st()))
            checks.append(("out", np.array([[s["nlml"]] * 3 for s in ss]), col0, 0, _ftol(dtype, 1e-10, 1e-5)))
        else:
            ok(bed, bed.lib.pg_alpha_batched(bed.h, bed.code, n_pad, p(m), m.ld, m.estride, p(y), y.ld, p(u), u.ld, p(al), al.ld, p(w), w.ld, ne,
                                             bed.st()))
        return checks

    def asynch(bed):
        s = ss[0]
        l, m, y = bed.put("l", s["L"], poison=~blk), bed.put("minv", s["M"], poison=~blk), bed.put("y", s["y"])
        u, al = bed.put("u", shape=(n_pad,), role="out"), bed.put("alpha", shape=(n_pad,), role="out")
        w = bed.put("work", shape=(nw,), role="out", written=np.zeros(nw, bool), scratch=np.ones(nw, bool))
        out = bed.put("out", shape=(2,), dtype=F64, role="out")
        ok(bed, bed.lib.pg_alpha_nlml_async(bed.h, bed.code, n, n_pad, p(l), l.ld, p(m), m.ld, p(y), p(u), p(al), p(w), p(out), bed.st()))
        return [("u", s["u"], None, atol * np.abs(s["u"]).max(), 0), ("alpha", s["alpha"], None, atol * np.abs(s["alpha"]).max(), 0),
                ("out", np.array([s["nlml"], 2.0 * np.log(np.diag(s["L"])).sum()]), None, 0, _ftol(dtype, 1e-10, 1e-5))]

    def lauum(bed):
        m = bed.put("minv", Ms, poison=np.broadcast_to(~blk, Ms.shape))
        k = bed.put("kinv", shape=(ne, n_pad, n_pad), role="out", written=low, scratch=blk & ~low)
        ok(bed, bed.lib.pg_lauum_batched(bed.h, bed.code, n_pad, p(m), m.ld, m.estride, p(k), k.ld, k.estride, ne, bed.st()))
        ref = np.stack([q.T @ q for q in Ms])
        return [("kinv", ref, low, _ftol(dtype, 1e-10, 2e-4) * max(1.0, np.abs(ref).max()), 0)]

    run(ops, batched, dtype, gapset, with_nlml=0)
    run(ops, batched, dtype, gapset, with_nlml=1)
    run(ops, asynch, dtype, gapset)
    run(ops, lauum, dtype, gapset)


# ------------------------------------------------------------------------------------------- gradient values
GRADS = [(["se", "m52", "wn"], 5), (["se", "wn"], 5), (["m52", "wn"], 13), (["m32", "wn"], 2)]      # VALU, fast, matrix pipe x 2


@functools.lru_cache(maxsize=None)
def grad_case(pi, n, seed=0):
    parts, d = GRADS[pi]
    rng = np.random.default_rng(7 * n + pi + seed)
    x, hp = rng.random((n, d)), _hp(parts, d, rng)
    K = kr.kernel(parts, hp, x) + 1e-7 * np.eye(n)
    kinv = np.linalg.inv(K)
    kinv = 0.5 * (kinv + kinv.T)
    alpha = kinv @ rng.standard_normal(n)
    w = kinv - np.outer(alpha, alpha)
    g = np.zeros(hp.size)
    for k, slab in kr.grad_terms(parts, hp, x):
        g[k] += 0.5 * (w * slab).sum()
    return x, hp, kinv, alpha, g


def _gtol(dtype):
    """test_nlml_value_and_grad: rtol 1e-8, atol 1e-9 max|g|; fp32: test_matrix_pipe_bodies_...'s 3 x 3e-3 of max|g|."""
    return (1e-9, 1e-8) if dtype == F64 else (9e-3, 9e-3)


@both
@gaps
@pytest.mark.parametrize("pi", range(len(GRADS)), ids=["valu", "fast", "pipe52", "pipe32"])
@pytest.mark.parametrize("n", [333, 1500])
def test_nlml_grad_values(ops, n, pi, dtype, gapset):
    """pg_nlml_grad on framed X (ldx > d), Kinv (n_pad rows, identity padding), alpha, grad and a workspace of exactly
    pg_nlml_grad_worksize: against 1/2 sum (Kinv - alpha alpha^T) o dK_k in NumPy."""
    parts, d = GRADS[pi]
    x, hp, kinv, alpha, g = grad_case(pi, n)
    n_pad = -(-n // 256) * 256
    kp, ap = np.eye(n_pad), np.zeros(n_pad)
    kp[:n, :n], ap[:n] = kinv, alpha
    spec, nhp = make_spec(parts, d), hp.size
    at, rt = _gtol(dtype)

    def case(bed):
        xd, hpd, k, al = bed.put("x", x), bed.put("hp", hp, dtype=F64), bed.put("kinv", kp), bed.put("alpha", ap)
        gr = bed.put("grad", shape=(nhp,), dtype=F64, role="out")
        lw = int(bed.lib.pg_nlml_grad_worksize(n, nhp))
        w = bed.put("work", shape=(lw,), dtype=F64, role="out", written=np.zeros(lw, bool), scratch=np.ones(lw, bool))
        ok(bed, bed.lib.pg_nlml_grad(bed.h, bed.code, C.byref(spec), p(hpd), p(xd), xd.ld, n, d, p(k), k.ld, p(al), p(gr), nhp, p(w), lw, bed.st()))
        return [("grad", g, None, at * np.abs(g).max(), rt)]

    run(ops, case, dtype, gapset)


@both
@gaps
@pytest.mark.parametrize("pi", [0, 2], ids=["valu", "pipe52"])
def test_nlml_grad_batched_values(ops, pi, dtype, gapset):
    """pg_nlml_grad_batched, three experts, grad = outs[:, 1:] of an [nexp, 1 + nhp] block (column 0 keeps its bits); workspace exactly
    nexp * pg_nlml_grad_worksize."""
    parts, d = GRADS[pi]
    n, n_pad, ne = 333, 512, 3
    cs = [grad_case(pi, n, e) for e in range(ne)]
    spec, nhp = make_spec(parts, d), cs[0][1].size
    kp, ap = np.stack([np.eye(n_pad)] * ne), np.zeros((ne, n_pad))
    for e, c in enumerate(cs):
        kp[e, :n, :n], ap[e, :n] = c[2], c[3]
    gref = np.stack([np.concatenate([[0.0], c[4]]) for c in cs])
    cols = np.zeros((ne, 1 + nhp), bool)
    cols[:, 1:] = True
    at, rt = _gtol(dtype)

    def case(bed):
        xd, hpd = bed.put("x", np.stack([c[0] for c in cs])), bed.put("hp", np.stack([c[1] for c in cs]), dtype=F64, batch_gap=1)
        k, al = bed.put("kinv", kp), bed.put("alpha", ap, batch_gap=2 * min_gap(dtype))
        outs = bed.put("outs", shape=(ne, 1 + nhp), dtype=F64, role="out", written=cols, batch_gap=5)
        lw = ne * int(bed.lib.pg_nlml_grad_worksize(n, nhp))
        w = bed.put("work", shape=(lw,), dtype=F64, role="out", written=np.zeros(lw, bool), scratch=np.ones(lw, bool))
        ok(bed, bed.lib.pg_nlml_grad_batched(bed.h, bed.code, C.byref(spec), p(hpd), hpd.ld, p(xd), xd.ld, xd.estride, n, d, p(k), k.ld, k.estride,
                                             p(al), al.ld, ptr_at(outs, 1), outs.ld, nhp, p(w), lw, ne, bed.st()))
        return [("outs", gref, cols, at * np.abs(gref).max(), rt)]

    run(ops, case, dtype, gapset)


# ------------------------------------------------------------------------------------------- prediction / committee
@both
@gaps
@pytest.mark.parametrize("m", [37, 300])
def test_prediction_entry_points(ops, m, dtype, gapset):
    """pg_predict_mean_q, _kt, _kt_batched, pg_trmm_lower, pg_trmm_lower_kt_batched, pg_syrk_tn_sub, pg_syrk_nt_sub_batched with m test
    points inside m_pad.  tolerances: test_predict_mean_q (mean 1e-10, variance and covariance 1e-11, V 1e-12 -> 1e-11 against NumPy);
    fp32: 5e-4 of max|ref| (test_potrs_vec_blocked_sweeps' class for products against L^-1)."""
    n, n_pad, ne = 300, 512, 3
    m_pad = -(-m // 256) * 256
    ss = [kstate(n, n_pad, e) for e in range(ne)]
    rng = np.random.default_rng(m)
    blk = tiles_low(n_pad, n_pad)
    kts = np.zeros((ne, m_pad, n_pad))
    kts[:, :m, :n] = rng.standard_normal((ne, m, n))
    Ms, als = np.stack([s["M"] for s in ss]), np.stack([s["alpha"] for s in ss])
    hps = np.stack([s["hp"] for s in ss])
    kss = hps[:, 0] ** 2 + hps[:, 4] ** 2
    vts = np.einsum("emk,enk->emn", kts, Ms)                       # Kt Minv^T
    means, vars_ = np.einsum("emn,en->em", kts, als), kss[:, None] - (vts ** 2).sum(2)
    c0 = rng.standard_normal((ne, m_pad, m_pad))
    nw = (n_pad // 64) * m_pad
    spec = make_spec(GPARTS, GD)
    tol = lambda f64, ref: _ftol(dtype, f64, 5e-4 * max(1.0, np.abs(ref).max()))      # noqa: E731
    lowm = tiles_low(m_pad, m_pad)
    vg = 2 * min_gap(dtype)

    def single(bed, kt_form):
        mm, al = bed.put("minv", Ms[0], poison=~blk), bed.put("alpha", als[0])
        ks = bed.put("ks", kts[0] if kt_form else kts[0].T.copy())
        mean, var = bed.put("mean", shape=(m_pad,), role="out"), bed.put("var", shape=(m_pad,), role="out")
        w = bed.put("work", shape=(nw,), role="out", written=np.zeros(nw, bool), scratch=np.ones(nw, bool))
        fn = bed.lib.pg_predict_mean_q_kt if kt_form else bed.lib.pg_predict_mean_q
        ok(bed, fn(bed.h, bed.code, n_pad, m_pad, p(ks), ks.ld, p(mm), mm.ld, p(al), p(mean), p(var), float(kss[0]), p(w), bed.st()))
        return [("mean", means[0], None, tol(1e-10, means[0]), 0), ("var", vars_[0], None, tol(1e-11, vars_[0]), 0)]

    def batched(bed):
        mm, al = bed.put("minv", Ms, poison=np.broadcast_to(~blk, Ms.shape)), bed.put("alpha", als, batch_gap=vg)
        kt, hpd = bed.put("kt", kts), bed.put("hp", hps, dtype=F64, batch_gap=1)
        mv = bed.put("meanvar", shape=(ne, 2 * m_pad), role="out", batch_gap=vg)      # means and variances as halves of one row
        w = bed.put("work", shape=(ne, nw), role="out", written=np.zeros((ne, nw), bool), scratch=np.ones((ne, nw), bool), batch_gap=vg)
        ok(bed, bed.lib.pg_predict_mean_q_kt_batched(bed.h, bed.code, n_pad, m_pad, p(kt), kt.ld, kt.estride, p(mm), mm.ld, mm.estride, p(al), al.ld,
                                                     p(mv), mv.ld, ptr_at(mv, m_pad), mv.ld, C.byref(spec), p(hpd), hpd.ld, p(w), w.ld, ne, bed.st()))
        ref = np.concatenate([means, vars_], axis=1)
        return [("meanvar", ref, None, tol(1e-10, ref), 0)]

    def trmm(bed):
        mm, ks = bed.put("minv", Ms[0], poison=~blk), bed.put("ks", kts[0].T.copy())
        v = bed.put("v", shape=(n_pad, m_pad), role="out")
        ok(bed, bed.lib.pg_trmm_lower(bed.h, bed.code, n_pad, m_pad, p(mm), mm.ld, p(ks), ks.ld, p(v), v.ld, bed.st()))
        return [("v", vts[0].T, None, tol(1e-11, vts[0]), 0)]

    def trmm_kt(bed):
        mm, kt = bed.put("minv", Ms, poison=np.broadcast_to(~blk, Ms.shape)), bed.put("kt", kts)
        vt = bed.put("vt", shape=(ne, m_pad, n_pad), role="out")
        ok(bed, bed.lib.pg_trmm_lower_kt_batched(bed.h, bed.code, n_pad, m_pad, p(mm), mm.ld, mm.estride, p(kt), kt.ld, kt.estride, p(vt), vt.ld,
                                                 vt.estride, ne, bed.st()))
        return [("vt", vts, None, tol(1e-11, vts), 0)]

    def syrk_tn(bed, lower_only):
        v = bed.put("v", vts[0].T.copy())
        c = bed.put("c", c0[0], role="inout", written=tiles_low(m_pad, m_pad, 64) if lower_only else None,
                    scratch=None)
        ok(bed, bed.lib.pg_syrk_tn_sub(bed.h, bed.code, m_pad, n_pad, p(v), v.ld, p(c), c.ld, lower_only, bed.st()))
        ref = c0[0] - vts[0] @ vts[0].T
        return [("c", ref, np.tril(np.ones((m_pad, m_pad), bool)) if lower_only else None, tol(1e-11, ref), 0)]

    def syrk_nt(bed, lower_only):
        vt = bed.put("vt", vts)
        c = bed.put("c", c0, role="inout", written=tiles_low(m_pad, m_pad, 64) if lower_only else None)
        ok(bed, bed.lib.pg_syrk_nt_sub_batched(bed.h, bed.code, m_pad, n_pad, p(vt), vt.ld, vt.estride, p(c), c.ld, c.estride, ne, lower_only,
                                               bed.st()))
        ref = c0 - np.einsum("emk,enk->emn", vts, vts)
        return [("c", ref, np.tril(np.ones((m_pad, m_pad), bool)) if lower_only else None, tol(1e-11, ref), 0)]

    for case, kw in ((single, dict(kt_form=0)), (single, dict(kt_form=1)), (batched, {}), (trmm, {}), (trmm_kt, {}), (syrk_tn, dict(lower_only=0)),
                     (syrk_nt, dict(lower_only=0))):
        run(ops, case, dtype, gapset, **kw)
    assert lowm.shape == (m_pad, m_pad)


@both
@gaps_odd
@pytest.mark.parametrize("m", [37, 300])
def test_committee_entry_points(ops, m, dtype, gapset):
    """pg_grbcm_local_terms(_batched), pg_grbcm_finish, pg_grbcm_finish_full, pg_grbcm_weighted_prec: scalar kernels, odd leading
    dimensions included.  tolerances: test_grbcm_terms (rtol 1e-13 sums, 1e-12 finish, 1e-14 prec); fp32 inputs are rounded to fp32
    first and the fp64 reference is formed from the rounded values, so the same rtol holds for the fp64 outputs and 2^-23 for fp32 ones."""
    from oracle import pygpr_oracle as orc

    ne = 3
    rng = np.random.default_rng(6 + m)
    np_t = np.float64 if dtype == F64 else np.float32
    rnd = lambda a: a.astype(np_t).astype(np.float64)      # noqa: E731
    mc, vc = rnd(rng.standard_normal((ne, m))), rnd(0.1 + rng.random((ne, m)))
    vg, mg = rnd(0.2 + rng.random(m)), rnd(rng.standard_normal(m))
    r32 = 0 if dtype == F64 else 2.0 ** -23
    m_pad = -(-m // 256) * 256

    def terms(bed, batched):
        vgd = bed.put("vg", vg)
        out = bed.put("out", shape=(3, m), dtype=F64, role="out")
        if batched:
            me, va = bed.put("mean", mc, batch_gap=3), bed.put("var", vc, batch_gap=5)
            be, pr = bed.put("beta", shape=(ne, m), dtype=F64, role="out", batch_gap=7), bed.put("prec", shape=(ne, m), dtype=F64, role="out", batch_gap=7)
            ok(bed, bed.lib.pg_grbcm_local_terms_batched(bed.h, bed.code, m, p(me), me.ld, p(va), va.ld, p(vgd), ne, 1, 0, p(out), out.ld, p(be), p(pr),
                                                         be.ld, bed.st()))
            ref = sum(orc.grbcm_terms(mc[c], vc[c], vg, c == 1) for c in range(ne))
            beta = np.stack([orc.grbcm_terms(mc[c], vc[c], vg, c == 1)[0] for c in range(ne)])
            return [("out", ref, None, 0, 1e-13), ("beta", beta, None, 1e-15, 1e-13), ("prec", 1.0 / vc, None, 0, 1e-14)]
        me, va = bed.put("mean", mc[0]), bed.put("var", vc[0])
        be, pr = bed.put("beta", shape=(m,), dtype=F64, role="out"), bed.put("prec", shape=(m,), dtype=F64, role="out")
        ok(bed, bed.lib.pg_grbcm_local_terms(bed.h, bed.code, m, p(me), p(va), p(vgd), 0, 0, p(out), out.ld, p(be), p(pr), bed.st()))
        ref = orc.grbcm_terms(mc[0], vc[0], vg, False)
        return [("out", ref, None, 0, 1e-13), ("beta", ref[0], None, 1e-15, 1e-13), ("prec", 1.0 / vc[0], None, 0, 1e-14)]

    sums = sum(orc.grbcm_terms(mc[c], vc[c], vg, c == 0) for c in range(ne))
    cov0 = rnd(rng.standard_normal((m_pad, m_pad)))

    def finish(bed, full):
        sm, mgd, vgd = bed.put("sums", sums, dtype=F64), bed.put("mg", mg), bed.put("vg", vg)
        mean = bed.put("mean", shape=(m,), role="out")
        mu_ref, var_ref = orc.grbcm_finish(sums, mg, vg)
        if full:
            cov = bed.put("cov", cov0)
            ok(bed, bed.lib.pg_grbcm_finish_full(bed.h, bed.code, m, p(sm), sm.ld, p(mgd), p(vgd), p(cov), cov.ld, p(mean), bed.st()))
            return [("mean", np.diag(cov0)[:m] * (mu_ref / var_ref), None, 0, 1e-12 + r32)]
        var = bed.put("var", shape=(m,), role="out")
        b0, p0 = bed.put("beta0", shape=(m,), dtype=F64, role="out"), bed.put("prec0", shape=(m,), dtype=F64, role="out")
        ok(bed, bed.lib.pg_grbcm_finish(bed.h, bed.code, m, p(sm), sm.ld, p(mgd), p(vgd), p(mean), p(var), p(b0), p(p0), bed.st()))
        return [("mean", mu_ref, None, 0, 1e-12 + r32), ("var", var_ref, None, 0, 1e-12 + r32), ("beta0", 1.0 - sums[0], None, 1e-15, 1e-13),
                ("prec0", 1.0 / vg, None, 0, 1e-14)]

    P0, beta = rnd(rng.standard_normal((m_pad, m_pad))), rng.random(m)
    acc0 = rnd(rng.standard_normal((m_pad, m_pad)))
    lowp = np.tril(np.ones((m_pad, m_pad), bool))
    real = lowp.copy()
    real[m:] = False
    wref = np.zeros((m_pad, m_pad))
    wref[:m, :m] = 0.5 * (beta[:, None] + beta[None, :]) * P0[:m, :m]

    def wprec(bed, accumulate):
        pp, be = bed.put("P", P0), bed.put("beta", beta, dtype=F64)
        acc = bed.put("acc", acc0, role="inout", written=real if accumulate else lowp)
        ok(bed, bed.lib.pg_grbcm_weighted_prec(bed.h, bed.code, m, m_pad, p(pp), pp.ld, p(be), p(acc), acc.ld, accumulate, bed.st()))
        ref = np.where(real, wref + (acc0 if accumulate else 0.0), np.eye(m_pad))
        return [("acc", ref, real if accumulate else lowp, 1e-15 + 4 * r32, 1e-13 + 2 * r32)]

    for case, kw in ((terms, dict(batched=0)), (terms, dict(batched=1)), (finish, dict(full=0)), (finish, dict(full=1)), (wprec, dict(accumulate=0)),
                     (wprec, dict(accumulate=1))):
        run(ops, case, dtype, gapset, **kw)


# ------------------------------------------------------------------------------------------- the other scalar entry points, odd ld too
@both
@gaps_odd
def test_kernel_grad_build_sqdist_argmin_and_xgrad(ops, dtype, gapset):
    """pg_kernel_grad_build (dK stack, contiguous by contract: only X is strided), pg_sqdist_argmin (X, C, D strided) and
    pg_kernel_xgrad (every matrix strided, workspace exactly pg_kernel_xgrad_worksize).  tolerances: test_matern_family_gpu (dK: 1e-12),
    test_sqdist_kind_and_centres_any_d (1e-12), test_xgrad_gpu._abi_case (1e-12 / 1e-4 of max|ref|); fp32 dK and distances: the
    5e-6 of test_kernel_build_fp32 (the same expressions)."""
    parts, d, n, m = ["se", "m52", "wn"], 5, 70, 37
    rng = np.random.default_rng(12)
    x, hp = rng.random((n, d)), _hp(parts, d, rng)
    spec, nhp = make_spec(parts, d), hp.size
    dk = np.zeros((nhp, n, n))
    for k, slab in kr.grad_terms(parts, hp, x):
        dk[k] += slab

    def kgrad(bed):
        xd, hpd = bed.put("x", x), bed.put("hp", hp, dtype=F64)
        out = bed.put("dk", shape=(nhp * n * n,), role="out")
        ok(bed, bed.lib.pg_kernel_grad_build(bed.h, bed.code, C.byref(spec), p(hpd), p(xd), xd.ld, n, d, p(out), bed.st()))
        return [("dk", dk.reshape(-1), None, _ftol(dtype, 1e-12, 5e-6 * max(1.0, np.abs(dk).max())), 0)]

    nq, mc = 300, 90
    xs, cs = rng.random((nq, d)), rng.random((mc, d))
    d2 = ((xs[:, None, :] - cs[None, :, :]) ** 2).sum(2)
    srt = np.sort(d2, axis=1)
    clear = (srt[:, 1] - srt[:, 0]) > 1e-4                # rows whose nearest centre an fp32 rounding cannot change

    def sqd(bed):
        xd, cd = bed.put("x", xs), bed.put("c", cs)
        dd = bed.put("d", shape=(nq, mc), role="out")
        idx = bed.put("idx", shape=(nq,), dtype=torch.int32, role="out")
        ok(bed, bed.lib.pg_sqdist_argmin(bed.h, bed.code, p(xd), xd.ld, nq, p(cd), cd.ld, mc, d, p(dd), dd.ld, p(idx), bed.st()))
        return [("d", d2, None, _ftol(dtype, 1e-12, 5e-6), 0), ("idx", np.argmin(d2, axis=1), clear if dtype == F32 else None, 0, 0)]

    sp1 = make_spec(["se", "wn"], d)
    hp1 = _hp(["se", "wn"], d, rng)
    z, xq = rng.random((n, d)), rng.random((m, d))
    u, B = rng.standard_normal(n), rng.standard_normal((m, n))
    diff = xq[:, None, :] - z[None, :, :]                                             # [m, n, d]
    kv = hp1[0] ** 2 * np.exp(-((diff * hp1[1:1 + d]) ** 2).sum(2))
    dkx = -2.0 * kv[:, :, None] * hp1[1:1 + d] ** 2 * diff                              # dk(xq_p, z_i) / dxq_pk
    ref_u, ref_b = np.einsum("i,pik->pk", u, dkx), np.einsum("pi,pik->pk", B, dkx)

    def xgrad(bed):
        q, zd, hpd = bed.put("xq", xq), bed.put("z", z), bed.put("hp", hp1, dtype=F64)
        ud, bd = bed.put("u", u), bed.put("B", B)
        ou, ob = bed.put("out_u", shape=(m, d), role="out"), bed.put("out_b", shape=(m, d), role="out")
        lw = max(1, int(bed.lib.pg_kernel_xgrad_worksize(bed.h, m, n, d, 1)))
        w = bed.put("work", shape=(lw,), dtype=F64, role="out", written=np.zeros(lw, bool), scratch=np.ones(lw, bool))
        ok(bed, bed.lib.pg_kernel_xgrad(bed.h, bed.code, C.byref(sp1), p(hpd), 0, p(q), q.ld, 0, m, p(zd), zd.ld, 0, n, d, p(ud), 0, p(ou), ou.ld, 0,
                                        p(bd), bd.ld, 0, 0, p(ob), ob.ld, 0, 0, p(w), lw, 1, bed.st()))
        t = _ftol(dtype, 1e-12, 1e-4)
        return [("out_u", ref_u, None, t * np.abs(ref_u).max(), 0), ("out_b", ref_b, None, t * np.abs(ref_b).max(), 0)]

    for case in (kgrad, sqd, xgrad):
        run(ops, case, dtype, gapset)


# ------------------------------------------------------------------------------------------- append
@both
@gaps_odd
@pytest.mark.parametrize("n,k,n_pad", [(127, 1, 256), (250, 6, 256), (380, 8, 512), (300, 128, 512)])
def test_chol_append(ops, n, k, n_pad, dtype, gapset):
    """pg_chol_append (scalar kernels: odd leading dimensions of L, Minv, Kt, Knn too), n + k crossing a 128 and a 256 boundary,
    workspace exactly pg_chol_append_worksize.  Reference: tests/append_ref.append in fp64.  tolerances: fp64 1e-9 of max|ref| (the
    fp64 accumulation of both dtypes leaves the rounding of the inputs: test_append_gpu's class); fp32: 64 eps32 cond(L) max|ref|."""
    rng = np.random.default_rng(n + k)
    xa = rng.random((n + k, 3))
    Kf = ar.se_kernel(xa, xa) + 0.05 * np.eye(n + k)
    ya = rng.standard_normal(n + k)
    L, invd, M, u, alpha = ar.padded_fit(Kf[:n, :n], ya[:n], n_pad, garbage=0.0)
    Kt = np.zeros((k, n_pad))
    Kt[:, :n] = Kf[n:, :n]
    Knn = Kf[n:, n:]
    L2, iv2, M2, u2, a2, info = ar.append(L, invd, M, u, alpha, n, Kt, Knn, ya[n:])
    assert info == 0
    cond = float(np.sqrt(np.linalg.cond(Kf)))
    rows = np.zeros((n_pad, n_pad), bool)
    rows[n:n + k, :n + k] = True
    ivm = np.zeros(invd.shape, bool)
    for g in range(n, n + k):
        ivm[g // 128, g % 128, :] = True
    vecm = np.zeros(n_pad, bool)
    vecm[n:n + k] = True
    am = np.arange(n_pad) < n + k

    def case(bed):
        l = bed.put("l", L, role="inout", written=np.tril(rows), scratch=rows)
        iv = bed.put("invd", invd.reshape(-1), role="inout", written=np.zeros(ivm.size, bool), scratch=ivm.reshape(-1))
        mm = bed.put("minv", M, role="inout", written=np.tril(rows), scratch=rows)
        kt, knn, yn = bed.put("kt", Kt), bed.put("knn", Knn), bed.put("yn", ya[n:])
        ud = bed.put("u", u, role="inout", written=vecm)
        al = bed.put("alpha", alpha, role="inout", written=np.zeros(n_pad, bool), scratch=am)
        ws = int(bed.lib.pg_chol_append_worksize(bed.code, n_pad, k))
        w = bed.put("work", shape=(ws,), role="out", written=np.zeros(ws, bool), scratch=np.ones(ws, bool))
        info_d = bed.put("info", shape=(1,), dtype=torch.int32, role="out")
        ok(bed, bed.lib.pg_chol_append(bed.h, bed.code, n, k, n_pad, p(l), l.ld, p(iv), p(mm), mm.ld, p(kt), kt.ld, p(knn), knn.ld, p(yn), p(ud),
                                       p(al), p(w), p(info_d), bed.st()))
        t = lambda ref: _ftol(dtype, 1e-9, 64 * 2.0 ** -24 * cond) * max(1.0, np.abs(ref).max())      # noqa: E731
        low = np.tril(np.ones((n_pad, n_pad), bool))
        return [("info", 0, None, 0, 0), ("l", L2, low, t(L2), 0), ("minv", M2, low, t(M2), 0), ("invd", iv2.reshape(-1), None, t(iv2), 0),
                ("u", u2, None, t(u2), 0), ("alpha", a2, None, t(a2), 0)]

    run(ops, case, dtype, gapset)
