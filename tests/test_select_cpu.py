"""Greedy inducing-point selection on the host: the new header, the restatement (tests/select_ref.py) against itself and against the
trace term it restates, its stops and degenerate inputs, and the Python logic of pygpr_amd/sparse.py (select_inducing,
Sparse_GP.select_inducing, Sparse_GP.greedy) on a test double of the device ops.  No GPU."""
import ast
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import pygpr_amd as pg
import select_ref as sel
import sparse_ref as sr
from oracle_ops import _np
from pygpr_amd import _lib, _ops
from pygpr_amd import sparse as sparse_mod
from test_sparse_cpu import SparseOracleOps

MODELS = {
    "se+wn": (["se", "wn"], lambda: pg.Compose([pg.Squared_exponential(), pg.White_noise()])),
    "m32+rq+wn": (["m32", "rq", "wn"], lambda: pg.Compose([pg.Matern32(), pg.Rational_quadratic(), pg.White_noise()])),
    "se*per+wn": ([("se", "per"), "wn"], lambda: pg.Compose([pg.Product([pg.Squared_exponential(), pg.Periodic()]), pg.White_noise()])),
}
FLOOR = _ops.JITTER


# ------------------------------------------------------------------------------------------- the header
def test_select_header_parses_and_binds():
    text = open(_lib.HEADER_SELECT).read()
    protos = _lib.parse_prototypes(text)
    assert sorted(protos) == ["pg_greedy_select", "pg_greedy_select_worksize"]
    assert _lib._SIGS_SELECT == _lib.signatures(protos)
    others = set(_lib.header_symbols()) | set(_lib._SIGS_LOO) | set(_lib._SIGS_SAMPLE) | set(_lib._SIGS_SPARSE)
    assert not set(protos) & others and "#define PG_KIND" not in text
    vp, i, lg, db = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_double
    assert _lib._SIGS_SELECT["pg_greedy_select_worksize"] == (lg, [i, i])
    assert _lib._SIGS_SELECT["pg_greedy_select"] == (i, [vp, i, ctypes.POINTER(_lib.CovSpec), vp, vp, lg, i, i, i, db, vp, vp, vp, vp, vp, vp])
    lib = _lib.load(check_symbols=True)
    for name, (res, args) in _lib._SIGS_SELECT.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    # host arithmetic: one aligning word, m_max columns of n rounded up to even, the residuals, three partials per 128 points, the
    # pivot row, eight state words
    assert lib.pg_greedy_select_worksize(300, 40) == 1 + 40 * 300 + 300 + 3 * 3 + 40 + 8
    assert lib.pg_greedy_select_worksize(257, 257) == 1 + 257 * 258 + 257 + 3 * 3 + 257 + 8
    assert lib.pg_greedy_select_worksize(262144, 2048) == 1 + 2048 * 262144 + 262144 + 3 * 2048 + 2048 + 8      # past 2^31 bytes
    assert lib.pg_greedy_select_worksize(0, 0) == 9 and lib.pg_greedy_select_worksize(7, 0) == 1 + 7 + 3 + 8
    assert lib.pg_greedy_select_worksize(-1, 0) == -1 and lib.pg_greedy_select_worksize(5, -1) == -1 and lib.pg_greedy_select_worksize(5, 6) == -1
    assert lib.pg_greedy_select(None, 0, None, None, None, 1, 1, 1, 1, 0.0, None, None, None, None, None, None) != 0      # null handle: refused
    assert b"pg_greedy_select" in lib.pg_last_error()
    assert "HEADER_SELECT" in inspect.getsource(_lib.build_id) and "_SIGS_SELECT" in inspect.getsource(_lib.load)


def test_every_select_export_has_a_framed_case():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_select_gpu.py")
    used = {n.attr for n in ast.walk(ast.parse(open(path).read())) if isinstance(n, ast.Attribute) and n.attr.startswith("pg_")}
    assert sorted(set(_lib._SIGS_SELECT) - used) == []


# ------------------------------------------------------------------------------------------- the restatement against itself
@pytest.mark.parametrize("name", sorted(MODELS))
def test_trace_restates_the_bounds_trace_term(name):
    """n = 300, m = 40, d = 3.  The yardstick forms tr(Kuu^-1 Phi) by a solve against Kuu without jitter and subtracts it from n kdiag:
    its own error is cond(Kuu) roundings of magnitude n kdiag, and 16 of those is the bound."""
    terms = MODELS[name][0]
    hp, x, y, z = sr.problem(terms, n=300, m=40, d=3)
    run = sel.greedy(terms, hp, x, 40, FLOOR)
    assert len(run.piv) == 40 and len(set(run.piv.tolist())) == 40 and run.piv[0] == 0
    assert np.all(np.diff(run.trace) < 0) and run.trace[0] < 300 * run.kdiag
    t, cond = sel.trace_term(terms, hp, x, x[run.piv])
    bound = 16 * cond * 300 * run.kdiag * 2.0 ** -52
    t_helper, _ = sel.trace_term(terms, hp, x, z)
    print("%-10s T greedy %.4f  yardstick %.4f  |diff| %.2e (bound %.2e, cond %.2e)  T of problem's z %.4f" %
          (name, run.trace[-1], t, abs(run.trace[-1] - t), bound, cond, t_helper))
    assert abs(run.trace[-1] - t) <= bound
    assert run.trace[-1] < t_helper
    assert np.array_equal(run.hist[-1], run.resid) and abs(np.sum(run.resid) - run.trace[-1]) == 0
    # the long-double run tells the same story (its pivots may differ where two residuals tie: the product model's do)
    ld = sel.greedy(terms, hp, x, 40, FLOOR, np.longdouble)
    t_ld, cond_ld = sel.trace_term(terms, hp, x, x[ld.piv])
    assert ld.trace.dtype == np.longdouble and abs(float(ld.trace[-1]) - t_ld) <= 16 * cond_ld * 300 * run.kdiag * 2.0 ** -52
    rep = sel.replay(terms, hp, x, run.piv, np.float64)
    assert np.array_equal(rep.hist, run.hist) and np.array_equal(rep.trace, run.trace)


def test_greedy_values_of_the_three_models():
    """The figures the feature was proposed with (T greedy against T of problem's own z), to two decimals."""
    want = {"se+wn": (36.78, 46.06), "m32+rq+wn": (89.09, 105.54), "se*per+wn": (221.19, 223.05)}
    for name, (tg, tz) in want.items():
        terms = MODELS[name][0]
        hp, x, y, z = sr.problem(terms, n=300, m=40, d=3)
        assert abs(sel.greedy(terms, hp, x, 40, FLOOR).trace[-1] - tg) < 0.006 and abs(sel.trace_term(terms, hp, x, z)[0] - tz) < 0.006


# ------------------------------------------------------------------------------------------- stops and degenerate inputs
def test_one_dimensional_se_stops_early():
    rng = np.random.default_rng(5)
    x = rng.random((333, 1))
    hp = np.array([1.0, 2.5 + 0.6 * rng.random()])
    run = sel.greedy(["se"], hp, x, 64, FLOOR)
    assert len(run.piv) == 13 and run.hist.shape == (14, 333)
    assert np.max(run.resid) <= FLOOR and run.hist[12][run.piv[12]] > FLOOR
    assert len(sel.greedy(["se"], hp, x, 64, 1e-3).piv) < 13          # a higher floor stops sooner


def duplicates_case():
    """100 points in the unit square and 30 exact copies of the first 30, shuffled among them."""
    rng = np.random.default_rng(7)
    base = rng.random((100, 2))
    x = np.concatenate([base, base[:30]])[rng.permutation(130)]
    return np.array([1.0, 2.7, 3.1]), x


def test_duplicates_are_never_selected_twice():
    hp, x = duplicates_case()
    run = sel.greedy(["se"], hp, x, 130, FLOOR)
    chosen = x[run.piv]
    print("duplicates: %d of 130 selected, largest residual left %.2e" % (len(run.piv), np.max(run.resid)))
    assert len(np.unique(chosen, axis=0)) == len(run.piv) <= 100
    assert len(run.piv) < 100 and np.max(run.resid) <= FLOOR           # the floor, not the count, ended it
    sel_set = {tuple(c) for c in chosen}
    twins = [i for i in range(130) if tuple(x[i]) in sel_set and i not in set(run.piv.tolist())]
    assert twins and np.all(np.abs(run.resid[twins]) <= 16 * 130 * 2.0 ** -53)      # a selected point's copy is explained to rounding


def test_full_rank_selects_everything():
    rng = np.random.default_rng(11)
    x = rng.random((257, 2))
    hp = np.array([1.1, 6.0, 7.0])
    run = sel.greedy(["m12"], hp, x, 257, FLOOR)
    print("full rank: count %d, final trace %.2e" % (len(run.piv), run.trace[-1]))
    assert sorted(run.piv.tolist()) == list(range(257)) and np.all(np.diff(run.trace[:-1]) < 0)
    # a pivot's residual is set to 0 at its own step and keeps taking the later steps' l_i^2 (no clamp): rounding noise squared
    assert run.resid[run.piv[-1]] == 0 and np.all(np.abs(run.resid) <= 2.0 ** -53) and abs(run.trace[-1]) <= 257 * 2.0 ** -53


def test_a_nan_point_is_never_selected():
    terms = ["se"]
    rng = np.random.default_rng(2)
    x = rng.random((60, 2))
    x[17, 1] = np.nan
    run = sel.greedy(terms, np.array([1.0, 2.0, 2.0]), x, 20, FLOOR)
    assert len(run.piv) == 20 and 17 not in run.piv and np.isnan(run.trace).all() and np.isnan(run.resid[17])
    assert np.isfinite(np.delete(run.resid, 17)).all()
    assert sel.argmax(np.array([np.nan, 1.0, 1.0, np.nan])) == 1 and sel.argmax(np.array([np.nan, np.nan])) == -1


# ------------------------------------------------------------------------------------------- host logic on a test double
class SelectOracleOps(SparseOracleOps):
    """The Sparse_GP tests' double (KindOracleOps plus the raw product and the contraction) plus the selection, through the restatement."""

    def __init__(self):
        super().__init__()
        self.select_calls = []

    def greedy_select_worksize(self, n, m_max):
        return 1 + m_max * ((n + 1) // 2 * 2) + n + 3 * ((n + 127) // 128) + m_max + 8

    def greedy_select(self, spec, hp, x, m_max, floor, work=None, out=None):
        (sp,) = spec if isinstance(spec, (list, tuple)) else [spec]
        assert sp.nnoise == 0 and out is None
        model, h, _ = self._model(sp, _np(hp), x.shape[1])
        run = sel.greedy(model, h, _np(x), m_max, floor)
        self.select_calls.append((x.shape[0], m_max, floor))
        c = len(run.piv)
        piv, trace = torch.full((m_max,), -77, dtype=torch.int32), torch.full((m_max,), float("nan"), dtype=torch.float64)
        piv[:c], trace[:c] = torch.from_numpy(run.piv.astype(np.int32)), torch.from_numpy(run.trace)
        return piv, torch.tensor([c], dtype=torch.int32), trace, torch.from_numpy(run.resid.copy())


@pytest.fixture
def select_ops(monkeypatch, tmp_path):
    ops = SelectOracleOps()
    monkeypatch.setattr(_ops, "_OPS", ops)
    monkeypatch.chdir(tmp_path)
    return ops


def model_of(name, n=300, m=40):
    terms, make = MODELS[name]
    hp, x, y, z = sr.problem(terms, n=n, m=m)
    gp = pg.Sparse_GP(torch.from_numpy(x), torch.from_numpy(y), make(), torch.from_numpy(z))
    gp.set_params(torch.from_numpy(hp))
    return terms, hp, x, y, z, gp


@pytest.mark.parametrize("name", sorted(MODELS))
def test_function_returns_the_restatements_selection(select_ops, name):
    terms, hp, x, y, z, gp = model_of(name)
    run = sel.greedy(terms, hp, x, 25, FLOOR)
    res = pg.select_inducing(torch.from_numpy(x), MODELS[name][1](), torch.from_numpy(hp), 25)
    assert isinstance(res, pg.Selection) and res._fields == ("index", "trace", "residual")
    assert res.index.dtype == torch.int64 and res.index.tolist() == run.piv.tolist()
    assert np.array_equal(res.trace.numpy(), run.trace) and np.array_equal(res.residual.numpy(), run.resid)
    assert res.residual.shape == (300,) and select_ops.select_calls == [(300, 25, FLOOR)]


def test_select_inducing_sets_z_and_drops_the_memo(select_ops):
    terms, hp, x, y, z, gp = model_of("se+wn")
    gp.update()
    vfe = pg.VFE(gp)
    l0 = float(vfe.loss(hp.copy()))
    version = gp._z_version
    res = gp.select_inducing()                                  # m: as many as the model has
    assert gp.need_upd and gp._z_version == version + 1 and gp.z.shape == (40, 3)
    assert torch.equal(gp.z, torch.from_numpy(x)[res.index]) and len(res.index) == 40
    l1 = float(vfe.loss(hp.copy()))                             # the same params: only the z token can have dropped the memo
    want = sr.loss_woodbury(terms, hp, x, y, x[res.index.numpy()])
    assert abs(l1 - want) <= 1e-9 * abs(want) and l1 < l0
    gp.update()
    res2 = gp.select_inducing(m=12)
    assert gp.need_upd and gp.z.shape == (12, 3) and res2.index.tolist() == res.index.tolist()[:12]
    gp.set_params(torch.from_numpy(hp * 1.3))                   # selection follows the model's CURRENT params
    res3 = gp.select_inducing(m=12)
    assert res3.index.tolist() == sel.greedy(terms, hp * 1.3, x, 12, FLOOR).piv.tolist()
    assert "select_inducing" in pg.__all__ and "Selection" in pg.__all__


def test_greedy_equals_construct_then_select(select_ops):
    terms, hp, x, y, z, gp = model_of("m32+rq+wn")
    gp.select_inducing(m=30)
    made = pg.Sparse_GP.greedy(torch.from_numpy(x), torch.from_numpy(y), MODELS["m32+rq+wn"][1](), 30, params=torch.from_numpy(hp))
    assert isinstance(made, pg.Sparse_GP) and torch.equal(made.z, gp.z) and torch.equal(made.params, gp.params) and made.need_upd
    la, lb = pg.VFE(made).loss(hp.copy()), pg.VFE(gp).loss(hp.copy())
    assert float(la) == float(lb)
    # without params: selected at, and left with, the covariance's initial ones
    cov = MODELS["se+wn"][1]()
    xt, yt = torch.from_numpy(x), torch.from_numpy(y)
    dflt = pg.Sparse_GP.greedy(xt, yt, cov, 15)
    init = cov.init_params(xt)
    assert torch.equal(dflt.params, init)
    assert torch.equal(dflt.z, xt[torch.from_numpy(sel.greedy(["se", "wn"], init.numpy(), x, 15, FLOOR).piv)])


def test_tol_becomes_the_floor(select_ops):
    terms, hp, x, y, z, gp = model_of("se+wn")
    kdiag = sr.kdiag(terms, hp, 3)
    xt, cov = torch.from_numpy(x), MODELS["se+wn"][1]()
    pg.select_inducing(xt, cov, hp, 10)
    pg.select_inducing(xt, cov, hp, 10, tol=1e-12)              # below the jitter: the jitter holds
    pg.select_inducing(xt, cov, hp, 10, tol=0.25)
    res = gp.select_inducing(m=300, tol=0.05)
    assert [c[2] for c in select_ops.select_calls] == [FLOOR, FLOOR, 0.25 * kdiag, 0.05 * kdiag] and FLOOR == 1e-7
    assert 1 <= len(res.index) < 300 and res.trace.shape == res.index.shape and gp.z.shape[0] == len(res.index)
    assert float(res.residual.max()) <= 0.05 * kdiag


def test_refusals(select_ops):
    rng = np.random.default_rng(0)
    x, y = torch.from_numpy(rng.random((50, 2))), torch.from_numpy(rng.random(50))
    se = pg.Squared_exponential()
    hp = se.init_params(x)
    long_sum = pg.Compose([pg.Squared_exponential() for _ in range(_lib.PG_MAX_COMP + 1)])
    with pytest.raises(NotImplementedError, match="pass"):
        pg.select_inducing(x, long_sum, long_sum.init_params(x), 5)
    mixed = pg.Compose([pg.Squared_exponential(), pg.Product([pg.Squared_exponential(), pg.Periodic()])])      # a sum beside a product: two passes
    with pytest.raises(NotImplementedError, match="pass"):
        pg.select_inducing(x, mixed, mixed.init_params(x), 5)
    with pytest.raises(ValueError, match="stationary"):
        pg.select_inducing(x, pg.White_noise(), pg.White_noise().init_params(x), 5)
    with pytest.raises(NotImplementedError, match="batched"):
        pg.select_inducing(x[None], se, hp, 5)
    with pytest.raises(NotImplementedError, match="batched"):
        pg.select_inducing(x, se, torch.stack([hp, hp]), 5)
    with pytest.raises(TypeError, match="float64"):
        pg.select_inducing(x.float(), se, hp, 5)
    with pytest.raises(TypeError, match="float64"):
        pg.select_inducing(x, se, hp.float(), 5)
    for m in (0, 51, -1, 2.5):
        with pytest.raises(ValueError, match="m must be"):
            pg.select_inducing(x, se, hp, m)
    assert select_ops.select_calls == []
    assert len(pg.select_inducing(x, se, hp, 50).index) >= 1 and len(pg.select_inducing(x, se, hp, 1).index) == 1      # no White_noise needed
    cov = pg.Compose([pg.Squared_exponential(), pg.White_noise()])
    gp = pg.Sparse_GP(x, y, cov, x[:8].clone())
    for m in (0, 51):
        with pytest.raises(ValueError, match="m must be"):
            gp.select_inducing(m=m)
    with pytest.raises(ValueError, match="m must be"):
        pg.Sparse_GP.greedy(x, y, cov, 51)
    with pytest.raises(TypeError, match="float64"):
        pg.Sparse_GP.greedy(x.float(), y.float(), cov, 5)
    with pytest.raises(ValueError, match="White_noise"):
        pg.Sparse_GP.greedy(x, y, se, 5)                            # the MODEL still needs its noise child
    gp.set_params(torch.stack([gp.params, gp.params]))
    with pytest.raises(NotImplementedError, match="batched"):
        gp.select_inducing()
    assert gp.z.shape == (8, 2)


def test_existing_models_are_untouched(select_ops):
    """Sparse_GP(x, y, cov, z) takes no part in selection: no call reaches the new op, and _prior is the shared arithmetic."""
    terms, hp, x, y, z, gp = model_of("se*per+wn")
    gp.update()
    pg.VFE(gp).loss_and_grad(hp.copy())
    assert select_ops.select_calls == []
    assert gp._prior(hp) == sparse_mod._prior_of(gp.cov, 3, hp) and gp._prior(hp)[1] == sr.kdiag(terms, hp, 3)
