"""The nearest-neighbour (Vecchia) GP on the host: the twelfth header parses, binds and is exported by the built library, the
worksizes and the refusals that need no device, the restatement (tests/vecchia_ref.py) against the exact oracle, against a central
difference of its own loss and against its np.longdouble form, and the host logic of pygpr_amd/vecchia.py on a stand-in `ops` that
calls the restatement.  No GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import kernel_ref as kr
import kind_tools as kt
import vecchia_ref as vr
from pygpr_amd import _lib, _ops
from pygpr_amd import vecchia as vmod
from test_rowsq_cpu import _hp

import pygpr_amd as pg

EXACT_MODELS = {"se+wn": ["se", "wn"], "m32+wn": ["m32", "wn"], "rq+wn": ["rq", "wn"], "se*per": [("se", "per")]}
EPS = 2.0 ** -52
EXPORTS = ["pg_knn", "pg_vecchia_nlml_grad", "pg_vecchia_nlml_grad_worksize", "pg_vecchia_predict", "pg_vecchia_predict_worksize"]


def _case(terms, n, d, seed):
    rng = np.random.default_rng(seed)
    x = rng.random((n, d))
    y = np.sin(3.0 * x.sum(1)) + 0.1 * rng.standard_normal(n)
    return _hp(terms, d, rng), x, y


def _full(n, m):
    """The causal table of an identity-ordered model whose every point sees all of its predecessors."""
    nbr = np.full((n, m), -1, np.int32)
    for i in range(n):
        nbr[i, :min(i, m)] = np.arange(min(i, m))
    return nbr


# ---- the header ----------------------------------------------------------------------------------------------------------------------
def test_vecchia_header_parses_binds_and_is_exported():
    text = open(_lib.VECCHIA_HEADER).read()
    protos = _lib.parse_prototypes(text)
    assert sorted(protos) == EXPORTS
    assert _lib._SIGS_VECCHIA == _lib.signatures(protos)
    assert "#define PG_KIND" not in text and not hasattr(_lib, "HEADER_VECCHIA")
    vp, i, lg, db = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_double
    sp = ctypes.POINTER(_lib.CovSpec)
    assert _lib._SIGS_VECCHIA["pg_knn"] == (i, [vp, i, vp, lg, i, vp, lg, i, i, vp, i, i, vp, lg, vp])
    assert _lib._SIGS_VECCHIA["pg_vecchia_nlml_grad_worksize"] == (lg, [i, i, i])
    assert _lib._SIGS_VECCHIA["pg_vecchia_predict_worksize"] == (lg, [i, i])
    assert _lib._SIGS_VECCHIA["pg_vecchia_nlml_grad"] == (i, [vp, i, sp, vp, i, vp, lg, i, i, vp, vp, lg, i, i, i, db, i, vp, vp, vp, vp, vp, vp, vp])
    assert _lib._SIGS_VECCHIA["pg_vecchia_predict"] == (i, [vp, i, sp, vp, vp, lg, i, i, vp, vp, lg, i, vp, lg, i, db, vp, vp, vp, vp, vp])
    lib = _lib.load(check_symbols=True)
    for name, (res, args) in _lib._SIGS_VECCHIA.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    assert "VECCHIA_HEADER" in inspect.getsource(_lib.build_id) and "_SIGS_VECCHIA" in inspect.getsource(_lib.load)
    # build_id hashes the header: the same bytes under another name change the identity
    before = _lib.build_id()["src_sha16"]
    assert re.fullmatch(r"[0-9a-f]{16}", before)


def test_the_names_collide_with_no_other_header():
    others = set(_lib.header_symbols())
    for k, v in vars(_lib).items():
        if k.startswith("_SIGS_") and k != "_SIGS_VECCHIA":
            others |= set(v)
    assert len(others) > 60 and not set(EXPORTS) & others


def test_every_stream_taking_export_of_the_header_has_a_framed_and_a_streamed_case():
    import test_framed_cpu

    text = _lib._strip_comments(open(_lib.VECCHIA_HEADER).read())
    takers = {name for name, params in re.findall(r"\b(pg_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", text) if re.search(r"\bvoid\s*\*\s*stream\b", params)}
    assert takers == {"pg_knn", "pg_vecchia_nlml_grad", "pg_vecchia_predict"}
    called = test_framed_cpu._gpu_test_names("test_vecchia_framed_gpu.py")
    assert sorted(takers - called) == [] and {"pg_vecchia_nlml_grad_worksize", "pg_vecchia_predict_worksize"} <= called
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_vecchia_framed_gpu.py")).read()
    assert "StreamBed" in src and "framed" in src


def test_worksizes():
    lib = _lib.load()
    # one row of nhp + 2 doubles (the hp slots, the loss, the failed index) per workgroup; four wavefronts a workgroup up to d = 3
    assert lib.pg_vecchia_nlml_grad_worksize(0, 3, 5) == 0
    assert lib.pg_vecchia_nlml_grad_worksize(1, 3, 5) == 7 and lib.pg_vecchia_nlml_grad_worksize(9, 3, 5) == 3 * 7
    assert lib.pg_vecchia_nlml_grad_worksize(1 << 18, 3, 5) == 4096 * 7          # never more than 4096 workgroups
    assert lib.pg_vecchia_nlml_grad_worksize(5, 64, 130) == 5 * 132               # d = 64: one wavefront a workgroup
    assert lib.pg_vecchia_predict_worksize(9, 3) == 3 * 2 and lib.pg_vecchia_predict_worksize(0, 1) == 0
    for bad in ((-1, 3, 5), (4, 0, 5), (4, 65, 5), (4, 3, -1)):
        assert lib.pg_vecchia_nlml_grad_worksize(*bad) == -1
    assert lib.pg_vecchia_predict_worksize(-1, 3) == -1 and lib.pg_vecchia_predict_worksize(3, 65) == -1


def _spec():
    return kt.one_spec(["se", "wn"], 2)


def _nlml_args(h=None, dtype=0, nhp=4, n=8, d=2, m=3, first=0, count=8):
    a = ctypes.c_void_p(64)      # never dereferenced: every call below is refused before anything is enqueued
    return [h, dtype, ctypes.byref(_spec()), a, nhp, a, d, n, d, a, a, m, m, first, count, 1e-7, 1, a, a, a, a, a, a, None]


def _predict_args(h=None, dtype=0, n=8, d=2, m=3, q=4):
    a = ctypes.c_void_p(64)
    return [h, dtype, ctypes.byref(_spec()), a, a, d, n, d, a, a, d, q, a, m, m, 1e-7, a, a, a, a, None]


def _knn_args(h=None, dtype=0, q=4, n=8, d=2, m=3, causal=1):
    a = ctypes.c_void_p(64)
    return [h, dtype, a, d, q, a, d, n, d, None, m, causal, a, m, None]


@pytest.mark.parametrize("kw,text", [({}, b"null handle"), ({"m": 0}, b"1 <= m <= 63"), ({"m": 64}, b"1 <= m <= 63"), ({"d": 0}, b"PG_MAX_DIM"),
                                     ({"d": 65}, b"PG_MAX_DIM"), ({"n": -1}, b"bad shape"), ({"dtype": 1}, b"float64 only")])
def test_refusals_that_need_no_device(kw, text):
    lib = _lib.load()
    for name, make in (("pg_knn", _knn_args), ("pg_vecchia_nlml_grad", _nlml_args), ("pg_vecchia_predict", _predict_args)):
        assert getattr(lib, name)(*make(**kw)) != 0
        err = lib.pg_last_error()
        assert name.encode() in err and text in err, (name, err)


def test_more_refusals_that_need_no_device():
    lib = _lib.load()
    assert lib.pg_knn(*_knn_args(q=-1)) != 0 and lib.pg_knn(*_knn_args(q=9, n=8)) != 0 and b"q <= n" in lib.pg_last_error()
    assert lib.pg_vecchia_nlml_grad(*_nlml_args(count=-1)) != 0 and lib.pg_vecchia_nlml_grad(*_nlml_args(first=3, count=6)) != 0
    assert b"first + count <= n" in lib.pg_last_error()
    assert lib.pg_vecchia_nlml_grad(*_nlml_args(nhp=3)) != 0 and b"outside hp" in lib.pg_last_error()      # se + wn at d = 2 needs four
    assert lib.pg_vecchia_predict(*_predict_args(q=-1)) != 0


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def _bound(terms, hp, x):
    """What two float64 evaluations of one quantity through different solves may differ by, relative to its scale: the backward
    error of a solve (n eps) times the condition of the matrix, with a factor 64 for the sums around it."""
    k = kr.kernel(terms, hp, x) + kr.JITTER * np.eye(x.shape[0])
    return 64.0 * x.shape[0] * EPS * np.linalg.cond(k)


@pytest.mark.parametrize("name", sorted(EXACT_MODELS))
def test_with_every_predecessor_the_restatement_is_the_exact_gp(name):
    terms = EXACT_MODELS[name]
    n, d = 40, 3
    hp, x, y = _case(terms, n, d, 7)
    bound = _bound(terms, hp, x)
    loss, grad, cm, cv = vr.nlml_and_grad(terms, hp, x, y, _full(n, n - 1), kr.JITTER)
    l_ref, g_ref = kr.nlml_and_grad(terms, hp, x, y)
    e_l, e_g = abs(loss - l_ref) / abs(l_ref), np.max(np.abs(grad - g_ref)) / np.max(np.abs(g_ref))
    xp = np.random.default_rng(8).random((9, d))
    mean, var = vr.predict(terms, hp, x, y, xp, np.tile(np.arange(n, dtype=np.int32), (9, 1)), kr.JITTER)
    m_ref, v_ref = kr.predict(terms, hp, x, y, xp, "diag")
    e_m, e_v = np.max(np.abs(mean - m_ref)) / np.max(np.abs(y)), np.max(np.abs(var - v_ref)) / np.max(v_ref)
    print("%-7s loss %.2e  grad %.2e  mean %.2e  var %.2e  (bound %.2e)" % (name, e_l, e_g, e_m, e_v, bound))
    assert max(e_l, e_g, e_m, e_v) <= bound
    # the last conditional IS the leave-one-out term of the last point
    lm, lv = kr.loo(terms, hp, x, y)
    assert abs(cm[-1] - lm[-1]) <= bound * np.max(np.abs(y)) and abs(cv[-1] - lv[-1]) <= bound * lv[-1]


@pytest.mark.parametrize("name", sorted(EXACT_MODELS))
def test_the_gradient_is_the_derivative_of_the_restatements_own_loss(name):
    terms = EXACT_MODELS[name]
    n, d, m = 40, 3, 8
    hp, x, y = _case(terms, n, d, 11)
    nbr = vr.knn(x, x, None, m, True)
    _, grad, _, _ = vr.nlml_and_grad(terms, hp, x, y, nbr, kr.JITTER)
    fd = np.zeros_like(hp)
    for p in range(hp.size):
        h = 1e-6 * max(1.0, abs(hp[p]))
        up, dn = hp.copy(), hp.copy()
        up[p] += h
        dn[p] -= h
        fd[p] = (vr.nlml_and_grad(terms, up, x, y, nbr, kr.JITTER)[0] - vr.nlml_and_grad(terms, dn, x, y, nbr, kr.JITTER)[0]) / (2 * h)
    err = np.max(np.abs(grad - fd)) / np.max(np.abs(grad))
    print("%-7s m = %d: gradient against the central difference %.2e" % (name, m, err))
    # truncation h^2 f''' / 6 ~ 1e-12 and rounding eps |loss| / h ~ 1e-8 of a loss of some 1e2, relative to a gradient of order 1e1
    assert err <= 1e-6


@pytest.mark.parametrize("name", sorted(EXACT_MODELS))
@pytest.mark.parametrize("m", [8, 39])
def test_the_float64_restatement_against_the_longdouble_one(name, m):
    terms = EXACT_MODELS[name]
    n, d = 40, 3
    hp, x, y = _case(terms, n, d, 13)
    nbr = vr.knn(x, x, None, m, True)
    got = vr.nlml_and_grad(terms, hp, x, y, nbr, kr.JITTER)
    ref = vr.nlml_and_grad(terms, hp, x, y, nbr, kr.JITTER, np.longdouble)
    assert all(np.asarray(r).dtype == np.longdouble for r in ref)
    errs = [float(abs(got[0] - ref[0]) / abs(ref[0]))] + [float(np.max(np.abs(g - r)) / np.max(np.abs(r))) for g, r in zip(got[1:], ref[1:])]
    bound = _bound(terms, hp, x)
    print("%-7s m = %2d: loss %.2e grad %.2e mean %.2e var %.2e (bound %.2e)" % ((name, m) + tuple(errs) + (bound,)))
    assert max(errs) <= bound


def test_knn_restatement_ties_padding_and_nan():
    x = np.array([[0.0], [1.0], [1.0], [0.5], [np.nan], [0.75]])
    nbr = vr.knn(x, x, None, 3, True)
    assert nbr.dtype == np.int32 and nbr.tolist() == [[-1, -1, -1], [0, -1, -1], [1, 0, -1], [0, 1, 2], [-1, -1, -1], [1, 2, 3]]
    assert vr.knn(x[:2], x, np.array([2.0]), 2, False).tolist() == [[0, 3], [1, 2]]


# ---- the host logic on a stand-in ops ------------------------------------------------------------------------------------------------
class RefOps:
    """What pygpr_amd/vecchia.py asks of the device layer, answered by the restatement on host tensors."""
    device = torch.device("cpu")

    def __init__(self, terms):
        self.terms, self.calls = terms, []

    def to_device(self, t, dtype=None):
        return t.detach().to(dtype=dtype if dtype is not None else t.dtype).contiguous().clone()

    def empty(self, *shape, dtype=torch.float64):
        return torch.full(shape, -77, dtype=dtype) if dtype == torch.int32 else torch.full(shape, float("nan"), dtype=dtype)

    def zeros(self, *shape, dtype=torch.float64):
        return torch.zeros(*shape, dtype=dtype)

    def knn(self, xq, xc, m, s=None, causal=False, out=None):
        self.calls.append(("knn", None if s is None else tuple(s.tolist()), bool(causal)))
        return torch.from_numpy(vr.knn(xq.numpy(), xc.numpy(), None if s is None else s.numpy(), m, causal))

    def vecchia_nlml_grad(self, spec, hp, x, y, nbr, first, count, jitter, want_grad, cmean, cvar, out, grad, info, work=None):
        self.calls.append(("nlml", int(first), int(count), bool(want_grad)))
        assert nbr.shape[0] == count
        loss, g, cm, cv = vr.nlml_and_grad(self.terms, hp.numpy(), x.numpy(), y.numpy(), nbr.numpy(), jitter, first=first)
        cmean.copy_(torch.from_numpy(cm))
        cvar.copy_(torch.from_numpy(cv))
        out[0] = float(loss)
        if want_grad:
            grad.copy_(torch.from_numpy(g))
        info[0] = 0

    def vecchia_predict(self, spec, hp, x, y, xq, nbr, jitter, mean, var, info, work=None):
        self.calls.append(("predict", int(xq.shape[0])))
        mu, v = vr.predict(self.terms, hp.numpy(), x.numpy(), y.numpy(), xq.numpy(), nbr.numpy(), jitter)
        mean.copy_(torch.from_numpy(mu))
        if var is not None:
            var.copy_(torch.from_numpy(v))
        info[0] = 0


TERMS = ["se", "wn"]


@pytest.fixture
def ref_ops(monkeypatch):
    ops = RefOps(TERMS)
    monkeypatch.setattr(_ops, "_OPS", ops)
    return ops


def _model(n=30, d=2, m=4, **kw):
    hp, x, y = _case(TERMS, n, d, 3)
    model = pg.Vecchia_GP(torch.from_numpy(x), torch.from_numpy(y), kt.cov_of(TERMS), neighbours=m, **kw)
    model.set_params(torch.from_numpy(hp))
    return model, hp, x, y


def test_outputs_come_back_in_the_users_order(ref_ops):
    model, hp, x, y = _model(order="random", seed=5)
    model.update()
    perm = model._perm.numpy()
    assert sorted(perm.tolist()) == list(range(30)) and perm.tolist() != list(range(30))
    nbr = vr.knn(x[perm], x[perm], None, 4, True)
    loss, _, cm, cv = vr.nlml_and_grad(TERMS, hp, x[perm], y[perm], nbr, kr.JITTER)
    assert model.nlml == float(loss)
    assert np.array_equal(model.cond_mean.numpy()[perm], cm) and np.array_equal(model.cond_var.numpy()[perm], cv)
    user = model.neighbours.numpy()
    assert user.shape == (30, 4) and user.dtype == np.int64
    for pos in range(30):
        want = [int(perm[j]) if j >= 0 else -1 for j in nbr[pos]]
        assert user[perm[pos]].tolist() == want
    assert np.array_equal(model.x.numpy(), x) and np.array_equal(model.y.numpy(), y)      # the user's tensors are never permuted
    # the same permutation handed over as a tensor is the same model; None is the identity
    again, _, _, _ = _model(order=torch.from_numpy(perm))
    again.update()
    assert again.nlml == model.nlml and np.array_equal(again.neighbours.numpy(), user)
    plain, _, _, _ = _model()
    plain.update()
    assert plain._perm.tolist() == list(range(30)) and np.array_equal(plain.neighbours.numpy(), vr.knn(x, x, None, 4, True))


def test_a_chunked_evaluation_is_the_sum_of_its_chunks_in_order(ref_ops, monkeypatch):
    model, hp, x, y = _model()
    whole = pg.Vecchia_MLE(model).loss_and_grad(hp)
    monkeypatch.setattr(vmod, "_TARGET_CHUNK", 7)
    model2, _, _, _ = _model()
    ref_ops.calls.clear()
    loss, grad = pg.Vecchia_MLE(model2).loss_and_grad(hp)
    assert [c[1:3] for c in ref_ops.calls if c[0] == "nlml"] == [(0, 7), (7, 7), (14, 7), (21, 7), (28, 2)]
    nbr = vr.knn(x, x, None, 4, True)
    parts = [vr.nlml_and_grad(TERMS, hp, x, y, nbr[s: s + 7], kr.JITTER, first=s) for s in range(0, 30, 7)]
    want_l, want_g = 0.0, np.zeros(hp.size)
    for p in parts:
        want_l, want_g = want_l + float(p[0]), want_g + p[1]
    assert float(loss) == want_l and np.array_equal(grad, want_g)
    assert abs(float(loss) - float(whole[0])) <= 1e-12 * abs(float(whole[0]))


def test_the_neighbour_sets_stay_while_the_parameters_move(ref_ops):
    model, hp, x, y = _model()
    model.update()
    table, version = model._nbr, model._nbr_version
    model.set_params(torch.from_numpy(hp * 1.3))
    with pytest.raises(RuntimeError):
        model.cond_mean
    model.update()
    assert model._nbr is table and model._nbr_version == version and sum(c[0] == "knn" for c in ref_ops.calls) == 1
    assert ref_ops.calls[0] == ("knn", None, True)
    model.refresh_neighbours()
    assert model._nbr is not table and model._nbr_version == version + 1
    assert ref_ops.calls[-1] == ("knn", tuple((hp * 1.3)[1:3].tolist()), True)      # the first stationary component's length scales
    model.refresh_neighbours(scaled=False)
    assert ref_ops.calls[-1] == ("knn", None, True)


def test_the_memo_follows_parameters_data_and_the_table(ref_ops):
    model, hp, x, y = _model()
    loss = pg.Vecchia_MLE(model)
    assert isinstance(loss, pg.Loss) and "Vecchia_GP" in pg.__all__ and "Vecchia_MLE" in pg.__all__
    count = lambda: sum(c[0] == "nlml" for c in ref_ops.calls)      # noqa: E731
    l0, g0 = loss.loss_and_grad(hp)
    assert count() == 1 and np.array_equal(loss.grad(hp), g0) and float(loss.loss(hp)) == float(l0) and count() == 1
    loss.loss(hp * 1.1)
    loss.grad(hp * 1.1)
    assert count() == 3
    loss.loss_and_grad(hp)
    assert count() == 4
    model.refresh_neighbours()
    loss.loss_and_grad(hp)
    assert count() == 5
    model.y = torch.from_numpy(y + 1.0)
    l1, _ = loss.loss_and_grad(hp)
    assert count() == 6 and float(l1) != float(l0) and sum(c[0] == "knn" for c in ref_ops.calls) == 3
    model.x = torch.from_numpy(x[::-1].copy())
    loss.loss_and_grad(hp)
    assert count() == 7 and sum(c[0] == "knn" for c in ref_ops.calls) == 4
    assert np.array_equal(loss.start_params(), model.params.numpy())
    loss.write_back(hp * 0.9)
    assert np.array_equal(model.params.numpy(), hp * 0.9) and model.need_upd


def test_predict_chunks_and_its_refusals(ref_ops, monkeypatch):
    model, hp, x, y = _model()
    xp = torch.from_numpy(np.random.default_rng(9).random((11, 2)))
    monkeypatch.setattr(vmod, "_CHUNK", 4)
    mean, var = model.predict(xp, "diag")
    assert [c for c in ref_ops.calls if c[0] == "predict"] == [("predict", 4), ("predict", 4), ("predict", 3)]
    nb = vr.knn(xp.numpy(), x, None, 4, False)
    mu, v = vr.predict(TERMS, hp, x, y, xp.numpy(), nb, kr.JITTER)
    assert np.array_equal(mean.numpy(), mu) and np.array_equal(var.numpy(), v)
    (only,) = model.predict(xp, "none")
    assert np.array_equal(only.numpy(), mu)
    with pytest.raises(NotImplementedError):
        model.predict(xp, "full")
    with pytest.raises(ValueError):
        model.predict(xp, "half")
    for call in (lambda: model.append(xp, xp[:, 0]), model.loo_predict, lambda: model.sampler(xp), lambda: model.predict_grad(xp)):
        with pytest.raises(NotImplementedError):
            call()


def test_what_the_model_refuses(ref_ops):
    hp, x, y = _case(TERMS, 12, 2, 3)
    X, Y, cov = torch.from_numpy(x), torch.from_numpy(y), kt.cov_of(TERMS)
    for bad in (0, 64):
        with pytest.raises(ValueError):
            pg.Vecchia_GP(X, Y, cov, neighbours=bad)
    with pytest.raises(NotImplementedError):
        pg.Vecchia_GP(X.float(), Y.float(), cov)
    with pytest.raises(NotImplementedError):
        pg.Vecchia_GP(X[None], Y[None], cov)
    with pytest.raises(NotImplementedError):
        pg.Vecchia_GP(X, Y, pg.Compose([pg.Squared_exponential() for _ in range(5)] + [pg.White_noise()]))
    for order in (torch.zeros(12, dtype=torch.int64), torch.arange(11), torch.arange(12).double(), "maxmin"):
        with pytest.raises(ValueError):
            pg.Vecchia_GP(X, Y, cov, order=order).update()
    model = pg.Vecchia_GP(X, Y, cov, neighbours=3)
    with pytest.raises(NotImplementedError):
        model.set_params(torch.from_numpy(np.stack([hp, hp])))
        model.update()
    model.set_params(torch.from_numpy(hp))
    for cls in (pg.MLE, pg.LOO):
        with pytest.raises(NotImplementedError):
            cls(model)
    with pytest.raises(TypeError):
        pg.Vecchia_MLE(pg.Exact_GP(X, Y, cov))
