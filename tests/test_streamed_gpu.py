"""Every C-ABI entry point with a `void* stream` parameter, held to its stream contract (tests/streamed.py): one streamed run of the
framed case that already exists for it -- late inputs on a busy side stream, outputs consumed directly behind the call -- at that
case's shapes, gap set "mixed", fp64 and (where the entry point takes it) fp32.  The packed half of every run stays a plain call on the
default stream, so "same bits" compares a late-input side-stream call with a plain one.  tests/test_streamed_cpu.py holds TABLE to
the eleven headers.

Schedules: the factorisation tables are taken with look-ahead on and off (pg_set_lookahead), on the coupled and the classic chain
(n_pad = 3072), with the recursive split (n_pad = 1024) and with the build folded in (pg_build_potrf_trtri): every schedule that forks
to a stream of the handle, and the form of each that stays on the caller's.

The deferred join of pg_alpha_nlml_async has tests of its own, and the file proves that it is not blind: a call handed the null
stream, a consumer on an unrelated stream, and a probe without any library call that shows two torch streams running side by side
here (if they do not, the probe fails and every other test of the file skips with that reason).

Nothing here provokes a fault: a wrong stream only reads NaN from memory the test owns."""
import collections
import ctypes as C
import importlib
import inspect
import os

import numpy as np
import pytest
import torch

import streamed
import test_framed_gpu as fg
from streamed import StreamBed, StreamError
from test_framed_gpu import F32, F64, ok, ops, p  # noqa: F401  (ops: the module's fixture)

pytestmark = pytest.mark.gpu

Row = collections.namedtuple("Row", "id module test kw exports f32 la")
TABLE = []


def R(id_, module, test, exports, f32=True, la=(1,), **kw):
    TABLE.append(Row(id_, module, test, kw, tuple(exports), f32, tuple(la)))


ONOFF = (1, 0)
FG, FK = "test_framed_gpu", "test_framed_kinds_gpu"
# ---- include/pygpr_hip.h: tests/test_framed_gpu.py
for v in ("NT", "TT"):
    R("gemm-" + v, FG, "test_gemm_variants", ["pg_gemm_raw"], variant=v)
R("gemm-tri", FG, "test_gemm_tri_trapezoid_and_mixed_launch", ["pg_gemm_raw"], variant_name="GEMM_NT", tm=5, tn=3)
R("build-sym-valu", FG, "test_kernel_build_symmetric", ["pg_kernel_build"], parts=["se", "se", "wn"], d=31, n=300)
R("build-sym-pipe", FG, "test_kernel_build_symmetric", ["pg_kernel_build"], parts=["m52", "wn"], d=13, n=300)
R("build-cross-acc", FG, "test_kernel_build_cross_and_accumulate", ["pg_kernel_build"], parts=["se", "wn"], d=2, nr=37, nc=300)
R("build-empty", FG, "test_kernel_build_empty_operands", ["pg_kernel_build", "pg_kernel_build_batched"])
R("build-batched-pipe", FG, "test_kernel_build_batched", ["pg_kernel_build_batched"], parts=["m52", "wn"], d=13)
R("build-batched-valu", FG, "test_kernel_build_batched", ["pg_kernel_build_batched"], parts=["se", "m32", "wn"], d=31)
for n, n_pad in ((200, 256), (1100, 1280)):
    R("potrf-%d" % n_pad, FG, "test_potrf_and_potrf_trtri", ["pg_potrf"], la=ONOFF, n=n, n_pad=n_pad, fused=0)
    R("potrf_trtri-%d" % n_pad, FG, "test_potrf_and_potrf_trtri", ["pg_potrf_trtri"], la=ONOFF, n=n, n_pad=n_pad, fused=1)
SOLVES = ["pg_potrs_vec", "pg_trtri", "pg_lauum", "pg_potri", "pg_trmv"]
R("solves-768", FG, "test_solves_from_the_factor", SOLVES, n=700, n_pad=768)
R("solves-2304", FG, "test_solves_from_the_factor", SOLVES, n=2200, n_pad=2304)
R("scalar", FG, "test_scalar_entry_points_take_any_ld", ["pg_tril", "pg_symmetrize", "pg_logdet", "pg_nlml_value"])
R("potrs-trsm", FG, "test_potrs_and_trsm_matrix_rhs", ["pg_potrs", "pg_trsm_lower"], nrhs=128)
ENTRY = {"potrf": "pg_potrf", "build": "pg_build_potrf_trtri", "checked": "pg_build_potrf_trtri_checked"}
for entry, export in ENTRY.items():      # test_factor_schedules: every schedule, look-ahead on and off
    for n, n_pad, mode in ((900, 1024, "plain"), (900, 1024, "split"), (3000, 3072, "coupled"), (3000, 3072, "classic")):
        if entry == "checked" and mode == "classic":
            continue                     # (the checked entry is the build entry and a host read of info: one chain is enough at this size)
        # (with look-ahead off no panel is coupled, which the "coupled" row itself asserts against: its look-ahead-off form is "classic")
        R("schedule-%s-%s" % (entry, mode), FG, "test_factor_schedules", [export], la=(1,) if mode == "coupled" else ONOFF, entry=entry, n=n, n_pad=n_pad,
          mode=mode)
for with_x in (1, 0):
    R("factor-batched-x%d" % with_x, FG, "test_factor_batched", ["pg_build_potrf_trtri_batched"], la=ONOFF, with_x=with_x)
R("alpha-lauum-batched", FG, "test_alpha_nlml_and_lauum_batched", ["pg_alpha_batched", "pg_alpha_nlml_batched", "pg_alpha_nlml_async", "pg_lauum_batched"],
  la=ONOFF)
for n, pi in ((333, 0), (333, 2), (333, 3), (1500, 1)):
    R("nlml-grad-%d-%d" % (n, pi), FG, "test_nlml_grad_values", ["pg_nlml_grad"], n=n, pi=pi)
for pi in (0, 2):
    R("nlml-grad-batched-%d" % pi, FG, "test_nlml_grad_batched_values", ["pg_nlml_grad_batched"], pi=pi)
R("prediction", FG, "test_prediction_entry_points", ["pg_predict_mean_q", "pg_predict_mean_q_kt", "pg_predict_mean_q_kt_batched", "pg_trmm_lower",
                                                      "pg_trmm_lower_kt_batched", "pg_syrk_tn_sub", "pg_syrk_nt_sub_batched"], m=300)
R("committee", FG, "test_committee_entry_points", ["pg_grbcm_local_terms", "pg_grbcm_local_terms_batched", "pg_grbcm_finish", "pg_grbcm_finish_full",
                                                    "pg_grbcm_weighted_prec"], m=37)
R("dk-sqdist-xgrad", FG, "test_kernel_grad_build_sqdist_argmin_and_xgrad", ["pg_kernel_grad_build", "pg_sqdist_argmin", "pg_kernel_xgrad"])
for n, k, n_pad in ((380, 8, 512), (300, 128, 512)):
    R("append-%d-%d" % (n, k), FG, "test_chol_append", ["pg_chol_append"], n=n, k=k, n_pad=n_pad)
# ---- the newer kinds through the spec-taking entry points: tests/test_framed_kinds_gpu.py
for entry, export in (("build", "pg_build_potrf_trtri"), ("checked", "pg_build_potrf_trtri_checked"), ("batched", "pg_build_potrf_trtri_batched")):
    R("kinds-factor-" + entry, FK, "test_build_and_factor", [export], mid="P1", entry=entry)
R("kinds-xgrad", FK, "test_kernel_xgrad_batched", ["pg_kernel_xgrad"], mid="P1", trans_b=1)
# ---- the ten other headers
R("loo-terms", "test_loo_framed_gpu", "test_loo_terms", ["pg_loo_terms"], n=300, n_pad=512)
R("loo-weights", "test_loo_framed_gpu", "test_loo_weights", ["pg_loo_weights"], n=300, n_pad=512)
R("loo-fold", "test_loo_framed_gpu", "test_loo_fold", ["pg_loo_fold"], n=300, n_pad=512)
R("randn", "test_sample_framed_gpu", "test_randn", ["pg_randn"], rows=257, cols=130, rows_pad=512, cols_pad=256)
for name, m, n, d, acc in (("se*per", 70, 150, 3, True), ("rq", 1, 300, 17, False)):
    R("cross-grad-" + name, "test_sparse_gpu", "test_cross_grad_framed", ["pg_kernel_cross_grad"], name=name, m=m, n=n, d=d, accumulate=acc)
for name, n, m_max, d, special in (("se", 333, 64, 1, "stop"), ("se*per", 300, 40, 3, None)):
    R("select-" + name, "test_select_gpu", "test_greedy_select_framed", ["pg_greedy_select"], f32=False, name=name, n=n, m_max=m_max, d=d, special=special)
R("matmul-cross", "test_kmatmul_gpu", "test_matmul_framed", ["pg_kernel_matmul"], f32=False, name="se*per", nr=3, nc=600, nrhs=5, d=3, symmetric=False)
R("matmul-sym", "test_kmatmul_gpu", "test_matmul_framed", ["pg_kernel_matmul"], f32=False, name="se+wn", nr=257, nc=257, nrhs=17, d=3, symmetric=True)
R("lowrank-cross", "test_lowrank_grad_gpu", "test_lowrank_grad_framed", ["pg_kernel_lowrank_grad"], f32=False, name="se*per", nr=130, nc=70, r=33, d=3,
  accumulate=True, sym=False)
R("lowrank-sym", "test_lowrank_grad_gpu", "test_lowrank_grad_framed", ["pg_kernel_lowrank_grad"], f32=False, name="rq", nr=257, nc=257, r=17, d=17,
  accumulate=False, sym=True)
for nr, nf, nrhs, d in ((3, 600, 5, 3), (257, 150, 17, 5)):
    R("feature-%d" % nr, "test_feature_matmul_gpu", "test_feature_matmul_framed", ["pg_feature_matmul"], f32=False, nr=nr, nf=nf, nrhs=nrhs, d=d)
for mid in ("P1", "S1"):
    R("matmul-dx-" + mid, "test_dmatmul_framed_gpu", "test_matmul_dx_framed", ["pg_kernel_matmul_dx"], f32=False, mid=mid)
for name, nr, nc, d in (("se*per", 3, 600, 3), ("se+wn", 257, 70, 3)):
    R("rowsq-%d" % nr, "test_rowsq_gpu", "test_rowsq_framed", ["pg_kernel_rowsq"], f32=False, name=name, nr=nr, nc=nc, d=d)
R("lxgrad-segments", "test_lxgrad_gpu", "test_lowrank_xgrad_framed", ["pg_kernel_lowrank_xgrad"], f32=False, name="se+wn", nr=5, nc=5000, r=2, d=3,
  accumulate=False, sym=False)
R("lxgrad-sym", "test_lxgrad_gpu", "test_lowrank_xgrad_framed", ["pg_kernel_lowrank_xgrad"], f32=False, name="rq", nr=257, nc=257, r=17, d=17,
  accumulate=False, sym=True)

STREAMED = {e for row in TABLE for e in row.exports}       # what tests/test_streamed_cpu.py holds to the headers
PARAMS = [pytest.param(row, dtype, la, id="%s-%s%s" % (row.id, "f64" if dtype == F64 else "f32", "" if la else "-la0"))
          for row in TABLE for dtype in ([F64, F32] if row.f32 else [F64]) for la in row.la]
BLIND = "two torch streams do not run side by side here (a reader on a second stream saw a reveal that sat behind the delay): this file is blind"


# ------------------------------------------------------------------------------------------- the probe, and what it decides
@pytest.fixture(scope="session")
def side_by_side():
    ok_ = streamed.probe_concurrent_streams()
    d = streamed.calibrate()
    print("streamed probe: reader on a second stream %s the veil; delay %.1f ms (%d units, %s)" % ("saw" if ok_ else "DID NOT see", d["ms"], d["units"], d["kind"]))
    return ok_


@pytest.fixture(autouse=True)
def _not_blind(request, side_by_side):
    if not side_by_side and request.node.name != "test_two_streams_run_side_by_side":
        pytest.skip(BLIND)


def test_two_streams_run_side_by_side(side_by_side):
    d = streamed.calibrate()
    assert 0.0 < d["ms"] <= streamed.CAP_MS, d
    assert side_by_side, BLIND


# ------------------------------------------------------------------------------------------- one streamed run per row
def _drain():
    """Wait for everything a test left in flight.  An error of the device itself ends the session: nothing more is started on it."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("the GPU reported an error; no further test is started: %s" % e, returncode=3)


def drive(ops, monkeypatch, row, dtype, la, bed):
    """The existing test function of the row, its framed half on `bed`; returns the entry points that took the bed's stream."""
    mod = importlib.import_module(row.module)
    fn = getattr(mod, row.test)
    have = inspect.signature(fn).parameters
    kw = dict(row.kw, ops=ops)
    if "dtype" in have:
        kw["dtype"] = dtype
    else:
        assert dtype == F64, "this case is fp64 only"
    if "gapset" in have:
        kw["gapset"] = "mixed"
    monkeypatch.setattr(fg, "FRAMED_BED", bed)
    if mod is not fg and getattr(mod, "Bed", None) is fg.Bed:      # a case that builds its beds itself (test_select_gpu)
        monkeypatch.setattr(mod, "Bed", lambda o, dt, gs: (fg.Bed if gs is None else bed)(o, dt, gs))
    del StreamBed.log[:]
    try:
        if not la:
            assert ops.lib.pg_set_lookahead(ops.h, 0) == 0
        fn(**kw)
    finally:
        streamed.close_all()
        ops.lib.pg_set_lookahead(ops.h, 1)
        _drain()
    return list(StreamBed.log)


@pytest.mark.parametrize("row,dtype,la", PARAMS)
def test_streamed(ops, monkeypatch, row, dtype, la):
    called = drive(ops, monkeypatch, row, dtype, la, StreamBed)
    assert sorted(set(row.exports) - set(called)) == [], "entry points of the row that no streamed bed was handed to"


# ------------------------------------------------------------------------------------------- the deferred join of pg_alpha_nlml_async
def _values(bed, checks):
    for name, ref, mask, atol, rtol in checks:
        got = bed.items[name][0].view.double().cpu().numpy()
        m = np.ones(got.shape, bool) if mask is None else np.broadcast_to(mask, got.shape)
        np.testing.assert_allclose(got[m], np.broadcast_to(ref, got.shape)[m], atol=atol, rtol=rtol, err_msg=name)


def _async_bed(ops, dtype):
    """The operands of test_alpha_nlml_and_lauum_batched's pg_alpha_nlml_async case (n = 300 in 512, same allowances), plus K^-1 for
    pg_lauum and two words for the joining entry point (pg_logdet).  L, Minv and y are veiled; bed.st() reveals them late on S1."""
    n, n_pad = 300, 512
    s = fg.kstate(n, n_pad, 0)
    low, blk = np.tril(np.ones((n_pad, n_pad), bool)), fg.tiles_low(n_pad, n_pad)
    nw = (n_pad // 256) * n_pad
    bed = StreamBed(ops, dtype, "mixed")
    f = dict(l=bed.put("l", s["L"], poison=~blk), m=bed.put("minv", s["M"], poison=~blk), y=bed.put("y", s["y"]),
             u=bed.put("u", shape=(n_pad,), role="out"), al=bed.put("alpha", shape=(n_pad,), role="out"),
             w=bed.put("work", shape=(nw,), role="out", written=np.zeros(nw, bool), scratch=np.ones(nw, bool)),
             out=bed.put("out", shape=(2,), dtype=F64, role="out"))
    atol = fg._ftol(dtype, 1e-11, 5e-4)
    logdet = 2.0 * np.log(np.diag(s["L"])[:n]).sum()
    checks = [("u", s["u"], None, atol * np.abs(s["u"]).max(), 0), ("alpha", s["alpha"], None, atol * np.abs(s["alpha"]).max(), 0),
              ("out", np.array([s["nlml"], 2.0 * np.log(np.diag(s["L"])).sum()]), None, 0, fg._ftol(dtype, 1e-10, 1e-5))]
    kinv = s["M"].T @ s["M"]

    def call_async(st):
        ok(bed, ops.lib.pg_alpha_nlml_async(ops.h, bed.code, n, n_pad, p(f["l"]), f["l"].ld, p(f["m"]), f["m"].ld, p(f["y"]), p(f["u"]), p(f["al"]),
                                            p(f["w"]), p(f["out"]), st))
        bed.calls.append("pg_alpha_nlml_async")

    def add_lauum():
        f["k"] = bed.put("kinv", shape=(n_pad, n_pad), role="out", written=low, scratch=blk & ~low)
        checks.append(("kinv", kinv, low, fg._ftol(dtype, 1e-10, 2e-4) * max(1.0, np.abs(kinv).max()), 0))

    def call_lauum(st):
        ok(bed, ops.lib.pg_lauum(ops.h, bed.code, n_pad, p(f["m"]), f["m"].ld, p(f["k"]), f["k"].ld, st))

    def add_join(name):
        f[name] = bed.put(name, shape=(1,), dtype=F64, role="out")
        checks.append((name, logdet, None, 0, fg._ftol(dtype, 1e-12, 1e-5)))

    def call_join(name, st):      # a joining entry point: pg_logdet of the factor (test_scalar_entry_points_take_any_ld's allowance)
        ok(bed, ops.lib.pg_logdet(ops.h, bed.code, n, p(f["l"]), f["l"].ld, p(f[name]), st))

    return bed, f, checks, call_async, add_lauum, call_lauum, add_join, call_join


def _async_then_lauum_then_join(ops, dtype):
    bed, f, checks, call_async, add_lauum, call_lauum, add_join, call_join = _async_bed(ops, dtype)
    try:
        add_lauum()
        add_join("logdet")
        st = bed.st()                      # the delay and the late reveal on S1
        call_async(st)
        call_lauum(st)                     # documented not to join
        call_join("logdet", st)
        bed.consume()                      # alpha, u, out (and everything else the calls wrote), on S1, no host synchronisation before it
        bed.check()
        _values(bed, checks)
    finally:
        streamed.close_all()
        _drain()


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_deferred_join_reaches_the_next_reader(ops, dtype):
    """(a) pg_alpha_nlml_async, pg_lauum (which does not join), one joining entry point, then the consumer -- all on S1."""
    _async_then_lauum_then_join(ops, dtype)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_deferred_join_with_lookahead_off(ops, dtype):
    """(c) the same with pg_set_lookahead(0): the side stream is the caller's."""
    try:
        assert ops.lib.pg_set_lookahead(ops.h, 0) == 0
        _async_then_lauum_then_join(ops, dtype)
    finally:
        ops.lib.pg_set_lookahead(ops.h, 1)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_deferred_join_is_retired_by_its_owner_only(ops, dtype):
    """(b) async on S1; a joining entry point on S2, behind which alpha must be final on S2; then a joining entry point on S1, behind which
    everything must be final on S1.  Had S2's join retired the mark, S1's entry point would not wait: its consumer would run right
    behind the reveal, beside the side stream's work (the library has no read of the mark, so this is how it shows)."""
    bed, f, checks, call_async, add_lauum, call_lauum, add_join, call_join = _async_bed(ops, dtype)
    try:
        add_join("logdet_s2")
        add_join("logdet_s1")
        s2 = torch.cuda.Stream()
        st = bed.st()
        call_async(st)
        call_join("logdet_s2", C.c_void_p(s2.cuda_stream))
        with torch.cuda.stream(s2):
            on_s2 = streamed.EarlyClone([f["al"], f["logdet_s2"]])
        call_join("logdet_s1", st)
        bed.consume([f["u"], f["al"], f["out"], f["w"], f["logdet_s1"]])      # (logdet_s2 belongs to S2's consumer)
        bed.check()
        on_s2.check_final()
        _values(bed, checks)
    finally:
        streamed.close_all()
        _drain()


# ------------------------------------------------------------------------------------------- teeth
class NullStreamBed(StreamBed):
    null_stream = True


class ThirdConsumerBed(StreamBed):
    third_consumer = True


def _row(id_):
    return next(r for r in TABLE if r.id == id_)


@pytest.mark.parametrize("id_", ["scalar", "gemm-NT", "potrf-256"])
def test_a_call_on_the_wrong_stream_is_caught(ops, monkeypatch, id_):
    """The call is handed the null stream while the reveal sits behind the delay on `side`: a one-kernel entry point (pg_tril, the first
    case of the scalar row), pg_gemm_raw, and pg_potrf, which starts with a memset.  The call reads the veil (NaN in memory the test
    owns), so the "same bits" or the value check of the streamed run fails."""
    with pytest.raises(AssertionError) as e:
        drive(ops, monkeypatch, _row(id_), F64, 1, NullStreamBed)
    assert not isinstance(e.value, StreamError), e.value
    print("%s on the null stream: %s" % (id_, str(e.value).splitlines()[0][:200]))


def test_an_unordered_consumer_is_caught(ops, monkeypatch):
    """The early consumer's clone taken on a third stream (ordered behind nothing) differs from the final words."""
    with pytest.raises(StreamError) as e:
        drive(ops, monkeypatch, _row("gemm-NT"), F64, 1, ThirdConsumerBed)
    assert e.value.name == "c" and e.value.region == "view" and e.value.count > 0
    print("unordered consumer:", e.value)


# ------------------------------------------------------------------------------------------- the models, on a side stream
def _golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gp.npz"), allow_pickle=False)


def _exact_gp(busy):
    import pygpr_amd as pg
    from test_parity_gpu import N, T, se_wn

    g = _golden()
    busy()
    gp = pg.Exact_GP(T(g["a_x"]), T(g["a_y"]), se_wn())
    gp.set_params(T(g["a_hp"]))
    busy()
    mu, var = gp.predict(T(g["a_xp"]), var="diag")
    return dict(mean=N(mu), var=N(var))


def _mle(busy):
    import pygpr_amd as pg
    from test_parity_gpu import T, se_wn

    g = _golden()
    busy()
    gp = pg.Exact_GP(T(g["a_x"]), T(g["a_y"]), se_wn())
    loss, grad = pg.MLE(gp).loss_and_grad(g["a_hp"].copy())
    return dict(loss=np.asarray(loss), grad=np.asarray(grad))


def _iterative(busy):
    import pygpr_amd as pg
    import test_iterative_gpu as ti

    terms, hp, x, y, xp, *_ = ti.case("se+wn")
    busy()
    model = pg.Iterative_GP(ti.T(x), ti.T(y), ti.cov_of(terms), rank=ti.RANK, tol=ti.TOL)
    model.set_params(ti.T(hp))
    model.update()
    busy()
    mu, var = model.predict(ti.T(xp), var="diag")
    return dict(alpha=ti.N(model.alpha), mean=ti.N(mu), var=ti.N(var))


@pytest.mark.parametrize("which", ["exact_gp", "mle", "iterative_gp"])
def test_models_on_a_side_stream(ops, monkeypatch, which):
    """Exact_GP fit and predict, one MLE loss and gradient, Iterative_GP fit and predict (the smallest sizes of tests/test_parity_gpu.py and
    tests/test_iterative_gpu.py) inside `with torch.cuda.stream(side)` while the default stream is busy with the delay: against the same
    calls on the default stream, at the allowances those files hold the quantities to (mean 1e-10, variance 1e-11, loss rtol 1e-10,
    gradient rtol 1e-8 of |g|_inf; Iterative_GP: test_iterative_gpu.held with cond(A) from NumPy).  A buffer cached on one stream and
    consumed on another, or a launch on the null stream, queues behind the delay and shows."""
    import test_iterative_gpu as ti

    monkeypatch.setattr(ti.it_mod, "_RHS_BLOCK", 32)
    body = {"exact_gp": _exact_gp, "mle": _mle, "iterative_gp": _iterative}[which]
    want = body(lambda: None)
    torch.cuda.synchronize()
    default = torch.cuda.current_stream()

    def busy():
        with torch.cuda.stream(default):
            streamed.delay()

    side = torch.cuda.Stream()
    try:
        with torch.cuda.stream(side):
            got = body(busy)
    finally:
        _drain()
    if which == "exact_gp":
        np.testing.assert_allclose(got["mean"], want["mean"], atol=1e-10)
        np.testing.assert_allclose(got["var"], want["var"], atol=1e-11)
    elif which == "mle":
        np.testing.assert_allclose(got["loss"], want["loss"], rtol=1e-10)
        np.testing.assert_allclose(got["grad"], want["grad"], rtol=1e-8, atol=1e-8 * np.abs(want["grad"]).max())
    else:
        cond = ti.case("se+wn")[6]
        ti.held("alpha, side stream vs default", got["alpha"], want["alpha"], cond, yard_rel=1e-8)
        ti.held("mean, side stream vs default", got["mean"], want["mean"], cond, yard_abs=1e-10)
        ti.held("variance, side stream vs default", got["var"], want["var"], cond, yard_abs=1e-11)
