"""The frame helper (tests/framed.py) against NumPy stand-ins, no GPU: one correct "op" that passes every check, and deliberately
wrong ones, each of which must be caught at the right place.  This is the proof that the framed GPU tests can fail.  Also the
coverage check: every export of include/pygpr_hip.h that takes a device buffer has a case in tests/test_framed_gpu.py, every export
that takes a covariance spec has one in tests/test_framed_kinds_gpu.py, and that file's model table holds every kind the library offers."""
import ast
import os

import numpy as np
import pytest
import torch

from framed import ROW_GUARD, SENTINEL32, SENTINEL64, FrameError, frame, min_gap

DTYPES = [torch.float64, torch.float32]
GAPS = ["min", 132, 1]


def _gap(g, dtype):
    return min_gap(dtype) if g == "min" else g


def _whole(f):
    """The frame's whole buffer as a NumPy array that shares its memory."""
    return f.buf.numpy()


def good_scale(a, x, y, work):
    """The stand-in "op": y = 2 a x through a workspace, touching exactly what it owns."""
    work.view.numpy()[: a.rows] = a.view.numpy() @ x.view.numpy()
    y.view.numpy()[:] = 2.0 * work.view.numpy()[: a.rows]


def _operands(dtype, g, nexp=None):
    rng = np.random.default_rng(3)
    gap = _gap(g, dtype)
    a = frame((37, 29), dtype, "cpu", gap=gap, name="a").fill(rng.standard_normal((37, 29)))
    x = frame((29,), dtype, "cpu", name="x").fill(rng.standard_normal(29))
    y = frame((37,), dtype, "cpu", name="y")
    work = frame((37,), dtype, "cpu", name="work")
    return a, x, y, work


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("g", GAPS)
def test_layout(dtype, g):
    gap = _gap(g, dtype)
    f = frame((3, 5, 7), dtype, "cpu", gap=gap, batch_gap=11, name="f")
    item = f.item
    assert f.view.shape == (3, 5, 7) and f.view.stride() == (5 * (7 + gap) + 11, 7 + gap, 1)
    off = f.view.data_ptr() - f.buf.data_ptr()
    assert off % 16 == 0 and off % 256 == 16 and off // item == f.start
    assert f.start >= ROW_GUARD * f.ld and f.total - f.start - f.nexp * f.estride >= ROW_GUARD * f.ld
    sent = SENTINEL64 if item == 8 else SENTINEL32
    assert np.all(f.words.numpy() == sent)
    assert np.all(np.isnan(_whole(f)))                     # a quiet NaN in either format
    assert f.locate(f.start) == ((0, 0, 0), "view")
    assert f.locate(f.start + 7) == ((0, 0, 7), "gap" if gap else "view") or gap == 0
    assert f.locate(f.start - 1) == ((0, -1, f.ld - 1), "front")
    assert f.locate(f.start + f.estride - 1)[1] == "between"
    assert f.locate(f.start + 2 * f.estride + 5 * f.ld)[1] == "back"
    w = frame((12,), torch.int32, "cpu", name="info")
    assert w.view.numel() == 12 and int(w.view[0]) == SENTINEL32


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("g", GAPS)
def test_correct_op_passes(dtype, g):
    a, x, y, work = _operands(dtype, g)
    for f in (a, x):
        f.snapshot()
    good_scale(a, x, y, work)
    for f in (a, x, y, work):
        f.check_guards()
    a.check_unchanged()
    x.check_unchanged()
    y.check_written()
    ref = 2.0 * a.view.double().numpy() @ x.view.double().numpy()
    np.testing.assert_allclose(y.view.double().numpy(), ref, rtol=1e-5 if dtype == torch.float32 else 1e-13)
    p = a.packed()
    assert p.is_contiguous() and np.array_equal(p.numpy(), a.view.numpy())


@pytest.mark.parametrize("dtype", DTYPES)
def test_write_into_the_gap_is_caught(dtype):
    gap = min_gap(dtype)
    c = frame((37, 29), dtype, "cpu", gap=gap, name="c")
    c.view.numpy()[:] = 1.0
    c.check_guards()
    _whole(c)[c.start + 20 * c.ld + 29] = 1.0             # row 20, first word past the width: an `ld` taken for the width
    with pytest.raises(FrameError) as e:
        c.check_guards()
    assert (e.value.kind, e.value.count, e.value.where, e.value.region) == ("guard overwritten", 1, (0, 20, 29), "gap")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("side", ["front", "back"])
def test_write_into_the_row_guard_is_caught(dtype, side):
    c = frame((37, 29), dtype, "cpu", gap=min_gap(dtype), name="c")
    c.view.numpy()[:] = 1.0
    row = -3 if side == "front" else 37 + 90               # a 128-row tile that runs 91 rows past a 37-row operand
    _whole(c)[c.start + row * c.ld + 4] = 0.0
    _whole(c)[c.start + row * c.ld + 5] = 0.0
    with pytest.raises(FrameError) as e:
        c.check_guards()
    assert (e.value.count, e.value.where, e.value.region) == (2, (0, row, 4), side)
    assert ROW_GUARD >= 128 and c.start + (37 + 255) * c.ld + c.cols <= c.total      # a 256-row tile from the last row still lands inside


@pytest.mark.parametrize("dtype", DTYPES)
def test_write_past_the_workspace_is_caught(dtype):
    a, x, y, work = _operands(dtype, "min")
    good_scale(a, x, y, work)
    work.check_guards()
    _whole(work)[work.start + 37] = 3.0                    # one element past the stated size
    with pytest.raises(FrameError) as e:
        work.check_guards()
    assert (e.value.count, e.value.where, e.value.region) == (1, (0, 1, 0), "back")
    _whole(work)[work.start + 37] = np.nan                 # an ordinary NaN is not the sentinel either
    with pytest.raises(FrameError):
        work.check_guards()


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_flipped_input_bit_is_caught(dtype):
    a, x, y, work = _operands(dtype, 132)
    a.snapshot()
    good_scale(a, x, y, work)
    a.check_unchanged()
    a.words.numpy()[a.start + 11 * a.ld + 2] ^= 1          # lowest mantissa bit of a[11, 2]
    with pytest.raises(FrameError) as e:
        a.check_unchanged()
    assert (e.value.kind, e.value.count, e.value.where, e.value.region) == ("changed", 1, (0, 11, 2), "view")
    mask = np.zeros((37, 29), bool)
    mask[11, 2] = True
    a.check_unchanged(except_mask=mask)                    # ... unless the case says the call may write there
    a.words.numpy()[a.start + 11 * a.ld + 29 + 1] ^= 1     # the gap of an input is compared too
    with pytest.raises(FrameError) as e:
        a.check_unchanged(except_mask=mask)
    assert e.value.where == (0, 11, 30) and e.value.region == "gap"


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_unwritten_output_entry_is_caught(dtype):
    c = frame((37, 29), dtype, "cpu", gap=132, name="c")
    low = np.tril(np.ones((37, 29), bool))
    v = c.view.numpy()
    v[low] = 0.0                                           # zeros are written values: only the sentinel means "untouched"
    c.check_written(low)
    with pytest.raises(FrameError) as e:
        c.check_written()                                  # the strict upper part was never written
    assert e.value.kind == "left unwritten" and e.value.where == (0, 0, 1) and e.value.count == int((~low).sum())
    c.words.numpy()[c.start + 30 * c.ld + 17] = SENTINEL64 if c.item == 8 else SENTINEL32
    with pytest.raises(FrameError) as e:
        c.check_written(low)
    assert (e.value.count, e.value.where, e.value.region) == (1, (0, 30, 17), "view")


@pytest.mark.parametrize("dtype", DTYPES)
def test_write_between_experts_is_caught(dtype):
    c = frame((3, 8, 6), dtype, "cpu", gap=min_gap(dtype), batch_gap=40, name="c")
    c.view.numpy()[:] = 2.0
    c.check_guards()
    c.check_written()
    _whole(c)[c.start + 1 * c.estride + 8 * c.ld + 3] = 2.0      # expert 1 writes a ninth row: a stride taken as rows * ld
    with pytest.raises(FrameError) as e:
        c.check_guards()
    assert (e.value.count, e.value.where, e.value.region) == (1, (1, 8, 3), "between")


def test_poison_marks_only_the_mask():
    a = frame((5, 5), torch.float64, "cpu", gap=2, name="a").fill(np.ones((5, 5)))
    up = np.triu(np.ones((5, 5), bool), 1)
    a.poison(up)
    v = a.view.numpy()
    assert np.all(np.isnan(v[up])) and np.all(v[~up] == 1.0)
    a.check_guards()
    a.check_written()                                      # poison is an ordinary NaN, not the sentinel


# ------------------------------------------------------------------------------------------- coverage of the C ABI
# Exports that take no device buffer (nothing to frame), by kind:
NO_BUFFER = {
    "pg_version", "pg_last_error",                                   # constants / host text
    "pg_create", "pg_destroy",                                       # handle life cycle
    "pg_potrf_worksize", "pg_potrs_vec_worksize", "pg_potrs_worksize", "pg_chol_append_worksize", "pg_nlml_grad_worksize",
    "pg_kernel_xgrad_worksize",                                      # sizes: host arithmetic, each USED by a framed case (checked below)
    "pg_set_lookahead", "pg_set_outer_panel", "pg_set_recursive_split", "pg_set_coupled_chain", "pg_set_spin_budget",
    "pg_set_rearm_after",                                            # setters of handle state
    "pg_coupled_chain", "pg_chain_timeouts", "pg_chain_rearms", "pg_last_coupled_panels", "pg_wait_budget_us",   # counters / state reads
    "pg_profile", "pg_profile_read",                                 # host-side profile switch and read
}
# Diagnostics whose only buffers are fixed-size scratch of the probe itself (32 bytes / 8 ints / one 128 x 128 tile): timing tools,
# not part of what INTEGRATION.md offers a binder; they keep their own tests (test_hip_kernels.py) and get no frame.
PROBES = {"pg_spin_probe", "pg_leaf_raw", "pg_rowstep_raw"}
WORKSIZES = {n for n in NO_BUFFER if n.endswith("_worksize")}


def _gpu_test_names(module="test_framed_gpu.py"):
    """Every pg_* name that the test module (tests/test_framed_gpu.py) calls through the library object (lib.pg_xxx)."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), module)
    tree = ast.parse(open(path).read())
    return {n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute) and n.attr.startswith("pg_")}


def test_every_buffer_taking_export_has_a_framed_case():
    from pygpr_amd._lib import header_symbols

    exports = set(header_symbols())
    assert NO_BUFFER <= exports and PROBES <= exports, "the exemption lists name something the header no longer declares"
    need = exports - NO_BUFFER - PROBES
    used = _gpu_test_names()
    assert sorted(need - used) == [], "exports with a device buffer and no framed case"
    assert sorted(WORKSIZES - used) == [], "worksize exports that no framed case sizes its workspace with"


def test_every_spec_taking_export_is_framed_for_every_kind():
    """The exports with a `const pg_covspec*` parameter are where a kind's block width and offsets are used: each is called in
    tests/test_framed_kinds_gpu.py, whose models carry the kinds that tests/test_framed_gpu.py's table does not.  A new spec-taking
    entry point therefore fails here until it has a framed case there."""
    from pygpr_amd._lib import HEADER, parse_prototypes

    takers = {name for name, (_, params) in parse_prototypes(open(HEADER).read()).items() if "const pg_covspec*" in params}
    assert {"pg_kernel_build", "pg_kernel_grad_build", "pg_nlml_grad", "pg_kernel_xgrad", "pg_build_potrf_trtri"} <= takers, "the header's parse lost the known ones"
    used = _gpu_test_names("test_framed_kinds_gpu.py")
    assert sorted(takers - used) == [], "exports that take a covariance spec and have no framed case for the newer kinds"
    assert {"pg_nlml_grad_worksize", "pg_kernel_xgrad_worksize", "pg_potrf_worksize"} <= used, "workspaces not sized by their worksize export"


def test_framed_model_table_holds_every_kind():
    """The model table of tests/test_framed_kinds_gpu.py, flattened: every PG_KIND_* of pygpr_amd/_lib.py except PG_KIND_SQDIST (which has
    its own framed case, test_kernel_grad_build_sqdist_argmin_and_xgrad), at least one product and one model that needs more than one pass.
    A new kind therefore fails here until a framed model carries it.  The module imports without a GPU."""
    import kernel_ref as kr
    import test_framed_kinds_gpu as fk
    from pygpr_amd import _lib

    offered = {v for k, v in vars(_lib).items() if k.startswith("PG_KIND_")} - {_lib.PG_KIND_SQDIST}
    assert len(offered) >= 6
    assert set(fk.KIND_OF.values()) == offered, "a kind of _lib.py has no part name in the framed model table"
    held = {fk.KIND_OF[q] for model, _ in fk.MODELS.values() for q in kr.flat(model) if q != "wn"}
    assert sorted(offered - held) == [], "kinds that no framed model carries"
    assert any(isinstance(t, tuple) for model, _ in fk.MODELS.values() for t in model), "no product in the framed model table"
    npass = {mid: len(fk.passes_of(mid)) for mid in fk.MODELS}
    assert max(npass.values()) > 1, "no multi-pass model in the framed model table"
    for mid in fk.MODELS:      # a product spec is flagged, its offsets are the library's own layout (asserted inside passes_of)
        for sp, terms, idx in fk.passes_of(mid):
            assert bool(sp.ncomp & _lib.PG_SPEC_PRODUCT) == any(isinstance(t, tuple) for t in terms)


@pytest.mark.parametrize("mid,slip", [("P1", "period"), ("P2", "period"), ("X1", "period"), ("X2", "period"), ("R2", "width"), ("P2", "width"),
                                      ("X2", "width")])
def test_a_block_layout_slip_would_exceed_every_allowance(mid, slip):
    """Not a test of the library but of the framed models' power, in NumPy on their own inputs (n = 37): the two layout slips that no
    guard band can see, because they stay inside hp, change K by far more than the widest allowance any case grants (2.5e-5, the fp32
    build of the three-factor product).  `period`: the periods read at off + d + k instead of off + d + 1 + k (period 1 becomes the
    last length scale).  `width`: every component behind a block wider than d + 1 read one element early, as if that block were d + 1
    wide.  (A leading dimension or an expert stride taken for the packed width needs no such argument: every framed operand has a gap
    of at least one element that holds a quiet NaN, so the slip reads NaN into the arithmetic.)"""
    import kernel_ref as kr
    import test_framed_kinds_gpu as fk
    from pygpr_amd import _lib

    model, d = fk.MODELS[mid]
    x, hp, ref = fk.sym_inputs(mid, 37)
    worst = 0.0
    for sp, terms, idx in fk.passes_of(mid):
        bad = hp.copy()
        nc = sp.ncomp & ~_lib.PG_SPEC_PRODUCT
        comps = sorted((sp.off[c], sp.kind[c]) for c in range(nc))
        for j, (o, kind) in enumerate(comps):
            if slip == "period" and kind == _lib.PG_KIND_PERIODIC:
                bad[o + d + 1: o + 2 * d + 1] = hp[o + d: o + 2 * d]
            if slip == "width" and j > 0 and comps[j - 1][1] in (_lib.PG_KIND_RQ, _lib.PG_KIND_PERIODIC):
                w = 2 * d + 1 if kind == _lib.PG_KIND_PERIODIC else (d + 2 if kind == _lib.PG_KIND_RQ else d + 1)
                bad[o: o + w] = hp[o - 1: o - 1 + w]
        if not np.array_equal(bad, hp):
            worst = max(worst, float(np.abs(kr.kernel(terms, bad[idx], x[:37]) - kr.kernel(terms, hp[idx], x[:37])).max()))
    assert worst > 100 * 2.5e-5, worst
