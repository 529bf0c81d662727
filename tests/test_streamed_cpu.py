"""The streamed harness (tests/streamed.py) without a GPU: the veil / reveal / early-clone bookkeeping on CPU frames with NumPy stand-ins
-- after a reveal every frame check passes, a forgotten reveal is caught, a word written after the early consumer's clone is caught and
located, the veil is neither sentinel -- and the coverage check: every export of the eleven headers that has a `void* stream` parameter
is named in the table of tests/test_streamed_gpu.py or exempted here with a reason, so a new stream-taking export fails until it has
a streamed case."""
import importlib
import inspect
import os
import re

import numpy as np
import pytest
import torch

import streamed
from framed import SENTINEL32, SENTINEL64, FrameError, frame, min_gap
from streamed import VEIL32, VEIL64, VEIL_INT, EarlyClone, StreamError, Veil

DTYPES = [torch.float64, torch.float32]


def _operand(dtype, name="a"):
    rng = np.random.default_rng(5)
    f = frame((37, 29), dtype, "cpu", gap=min_gap(dtype), name=name).fill(rng.standard_normal((37, 29)))
    up = np.triu(np.ones((37, 29), bool), 1)
    f.poison(up)                                          # the veil sits on top of a poisoned, snapshotted operand, as in StreamBed.put
    return f.snapshot(), up


def test_the_veil_is_neither_sentinel_nor_the_poison():
    assert VEIL64 not in (SENTINEL64, 0x7FF8000000000000) and VEIL32 not in (SENTINEL32, 0x7FC00000) and VEIL_INT not in (SENTINEL32, VEIL32)
    assert np.isnan(np.array([VEIL64], np.int64).view(np.float64)[0]) and np.isnan(np.array([VEIL32], np.int32).view(np.float32)[0])
    for dtype, want in ((torch.float64, VEIL64), (torch.float32, VEIL32), (torch.int32, VEIL_INT)):
        f = frame((12,), dtype, "cpu", name="v")
        assert streamed.veil_word(f) == want


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_veiled_operand_is_all_veil_and_its_surroundings_are_not(dtype):
    a, up = _operand(dtype)
    before = a.words.numpy().copy()
    v = Veil()
    v.cover(a)
    assert np.all(a.wview.numpy() == streamed.veil_word(a)) and np.all(np.isnan(a.view.numpy()))
    a.check_guards()                                      # gaps and guards keep the sentinel
    outside = ~a.inside().numpy()
    assert np.array_equal(a.words.numpy()[outside], before[outside])


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_forgotten_reveal_is_caught_and_a_reveal_restores_every_bit(dtype):
    a, up = _operand(dtype)
    want = a.bits()
    v = Veil()
    v.cover(a)
    with pytest.raises(FrameError) as e:
        a.check_unchanged()                               # the reveal never came: the input no longer is its snapshot
    assert (e.value.kind, e.value.where, e.value.region, e.value.count) == ("changed", (0, 0, 0), "view", 37 * 29)
    assert len(v.pending) == 1 and not v.done
    v.reveal()
    assert not v.pending and len(v.done) == 1
    a.check_unchanged()
    a.check_guards()
    a.check_written()
    assert np.array_equal(a.bits(), want)                 # the poison's NaN payload included
    assert np.all(np.isnan(a.view.numpy()[up])) and not np.any(np.isnan(a.view.numpy()[~up]))


def test_an_int32_operand_is_veiled_with_garbage_and_revealed():
    w = frame((9,), torch.int32, "cpu", name="idx").fill(np.arange(9)).snapshot()
    v = Veil()
    v.cover(w)
    assert np.all(w.view.numpy() == VEIL_INT)
    with pytest.raises(FrameError):
        w.check_unchanged()
    v.reveal()
    w.check_unchanged()
    assert np.array_equal(w.view.numpy(), np.arange(9))


def test_operands_covered_after_a_reveal_wait_for_the_next_one():
    a, _ = _operand(torch.float64, "a")
    b, _ = _operand(torch.float64, "b")
    v = Veil()
    v.cover(a)
    v.reveal()
    v.cover(b)
    a.check_unchanged()
    with pytest.raises(FrameError):
        b.check_unchanged()
    v.reveal()
    b.check_unchanged()
    assert [f.name for f, _ in v.done] == ["a", "b"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_word_written_after_the_early_clone_is_caught_and_located(dtype):
    y = frame((3, 8, 6), dtype, "cpu", gap=min_gap(dtype), batch_gap=40, name="y")
    c = frame((5,), dtype, "cpu", name="c")
    y.view.numpy()[:] = 2.0                               # what the call wrote in stream order ...
    early = EarlyClone([c, y])
    early.check_final()                                   # ... and nothing after it: the clone is final
    y.view.numpy()[1, 7, 3] = 2.0
    early.check_final()                                   # (the same bits again are no change)
    y.view.numpy()[1, 7, 3] = 3.0                         # a straggler: work that was not joined into the caller's stream
    y.view.numpy()[2, 0, 0] = 3.0
    with pytest.raises(StreamError) as e:
        early.check_final()
    assert (e.value.name, e.value.count, e.value.where, e.value.region) == ("y", 2, (1, 7, 3), "view")
    assert isinstance(e.value, FrameError) and "not joined" in str(e.value)
    y.view.numpy()[1, 7, 3] = y.view.numpy()[2, 0, 0] = 2.0
    early.check_final()
    y.buf.numpy()[y.start + 1 * y.estride + 2 * y.ld + 6] = 0.0      # a late write into a row's gap is a late write too
    with pytest.raises(StreamError) as e:
        early.check_final()
    assert (e.value.count, e.value.where, e.value.region) == (1, (1, 2, 6), "gap")


def test_an_untouched_output_and_its_early_clone_agree():
    y = frame((7,), torch.float64, "cpu", name="y")
    early = EarlyClone([y])
    early.check_final()                                   # sentinel before, sentinel after: the clone says nothing about written-ness
    with pytest.raises(FrameError):
        y.check_written()                                 # ... that stays check_written's business


# ------------------------------------------------------------------------------------------- coverage of the stream-taking exports
# Stream-taking exports without a streamed case, each with its reason.
EXEMPT = {
    "pg_spin_probe": "timing probe of the chain's wait loop: its only buffer is 32 bytes of its own scratch (test_framed_cpu.PROBES)",
    "pg_leaf_raw": "measurement entry of one 128 x 128 leaf step, not offered to a binder (test_framed_cpu.PROBES)",
    "pg_rowstep_raw": "measurement entry of one rows step of the coupled chain, not offered to a binder (test_framed_cpu.PROBES)",
}


def _headers():
    from pygpr_amd import _lib

    return [getattr(_lib, k) for k in sorted(vars(_lib)) if k == "HEADER" or k.startswith("HEADER_")]


def stream_takers():
    """name -> header of every export whose prototype has a `void* stream` parameter."""
    from pygpr_amd import _lib

    takers = {}
    for path in _headers():
        text = open(path).read()
        protos = _lib.parse_prototypes(text)
        for name, params in re.findall(r"\b(pg_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", _lib._strip_comments(text)):
            assert name in protos, name
            if re.search(r"\bvoid\s*\*\s*stream\b", params):
                assert "void*" in protos[name][1]
                takers[name] = os.path.basename(path)
    return takers


def test_every_stream_taking_export_has_a_streamed_case():
    import test_framed_cpu
    import test_streamed_gpu as sg

    heads = _headers()
    assert len(heads) == 11 and all(os.path.exists(h) for h in heads)
    takers = stream_takers()
    assert {os.path.basename(h) for h in heads} == set(takers.values()), "a header without a stream-taking export: the parse lost it"
    assert {"pg_potrf", "pg_gemm_raw", "pg_build_potrf_trtri_checked", "pg_alpha_nlml_async", "pg_loo_fold", "pg_randn", "pg_kernel_lowrank_xgrad"} <= set(takers)
    assert len(takers) >= 56
    assert set(EXEMPT) <= set(takers), "the exemption list names something that takes no stream any more"
    assert set(EXEMPT) == test_framed_cpu.PROBES and all(len(reason) > 20 for reason in EXEMPT.values())
    assert sorted(sg.STREAMED & set(EXEMPT)) == []
    assert sorted(sg.STREAMED - set(takers)) == [], "the streamed table names something that is no stream-taking export"
    assert sorted(set(takers) - set(EXEMPT) - sg.STREAMED) == [], "stream-taking exports with no streamed case"


def test_every_row_of_the_streamed_table_names_an_existing_case():
    """Each row's module and test function exist, the function takes the row's arguments (with ops, dtype and gapset where it has them),
    the module calls the entry points the row claims, fp32 is asked only of cases that take a dtype, and the ids are unique."""
    import test_framed_cpu
    import test_streamed_gpu as sg

    assert len({row.id for row in sg.TABLE}) == len(sg.TABLE)
    for row in sg.TABLE:
        mod = importlib.import_module(row.module)
        fn = getattr(mod, row.test)
        have = inspect.signature(fn).parameters
        kw = dict(row.kw, ops=None)
        kw.update({k: None for k in ("dtype", "gapset") if k in have})
        inspect.signature(fn).bind(**kw)                  # raises TypeError on a missing or an unknown argument
        assert "dtype" in have or not row.f32, row.id
        called = test_framed_cpu._gpu_test_names(row.module + ".py")
        assert set(row.exports) <= called, (row.id, sorted(set(row.exports) - called))
        assert set(row.la) <= {0, 1} and 1 in row.la, row.id
    assert len(sg.PARAMS) == sum((2 if row.f32 else 1) * len(row.la) for row in sg.TABLE)


def test_the_schedules_that_fork_are_taken_with_look_ahead_on_and_off():
    """The coupled chain, look-ahead on, and the folded build of pg_build_potrf_trtri -- and the look-ahead-off form of each: rows of
    test_factor_schedules (n_pad = 3072: six outer panels), test_factor_batched, test_alpha_nlml_and_lauum_batched."""
    import test_streamed_gpu as sg

    rows = {row.id: row for row in sg.TABLE}
    for entry in ("potrf", "build"):
        assert rows["schedule-%s-coupled" % entry].kw["n_pad"] == 3072 and rows["schedule-%s-coupled" % entry].la == (1,)
        assert rows["schedule-%s-classic" % entry].la == (1, 0)
        assert rows["schedule-%s-split" % entry].la == (1, 0)
    assert rows["schedule-checked-coupled"].exports == ("pg_build_potrf_trtri_checked",)
    assert rows["factor-batched-x1"].la == (1, 0) and rows["factor-batched-x0"].la == (1, 0) and rows["alpha-lauum-batched"].la == (1, 0)
