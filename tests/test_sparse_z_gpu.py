"""Sparse_GP's derivatives in its point sets on the MI355X: the gradient of the bound in the inducing inputs (VFE(train_z=True)) and
predict_grad against the NumPy restatement (tests/sparse_z_ref.py), chunked against unchunked, in training, and through the memo.

Tolerances (none is a guess; every test prints what it measured): the model rule of tests/test_sparse_gpu.py.  Per comparison 50 x the
disagreement between the restatement's dense (n x n) and Woodbury (m x m) forms on that input, floored at 1e-10 (sparse_ref.tol_of),
relative to the largest reference entry: the loss's disagreement for the z-gradient -- its weights G_uu and G_uf are the
hyper-parameter gradient's, which that test holds to the same figure -- the predictive mean's for d mean / dx*, the predictive
covariance's for d var / dx*.

Matern-1/2 has no derivative where an inducing input sits on a training point; the library gives that pair 0 and
so does the restatement, but the case takes z off the data as the host test of the difference quotients does.  The other three models
keep z on the data: every inducing input then meets one coincident training point and its own diagonal entry of G_uu, whose
derivatives are 0."""
import functools

import numpy as np
import pytest
import torch

import pygpr_amd as pg
import sparse_ref as sr
import sparse_z_ref as szr
from kind_tools import cov_of, ops  # noqa: F401  (ops: the module's fixture)
from pygpr_amd import sparse as sparse_mod
from test_sparse_gpu import MODELS, hold, mcase

pytestmark = pytest.mark.gpu

ZMODELS = dict(MODELS, **{"m12+wn": ["m12", "wn"]})


def _d17():
    """d = 17 reaches the contraction's second block of 16 coordinates.  sparse_ref.problem's length scales make Kuf vanish there."""
    rng = np.random.default_rng(3)
    x = rng.random((300, 17))
    hp = np.concatenate([[1.0], 0.6 + 0.1 * rng.random(17), [0.3]])
    z = x[:40] + 0.05 * rng.standard_normal((40, 17))
    y = np.sin(3.0 * x.sum(1)) + 0.1 * rng.standard_normal(300)
    return hp, x, y, z


@functools.lru_cache(maxsize=None)
def zcase(name):
    """(terms, hp, x, y, z, the restatement's loss, packed gradient and own error), computed once per case."""
    if name == "d17":
        terms = ZMODELS["se+wn"]
        hp, x, y, z = _d17()
    elif name == "m1":
        terms = ZMODELS["se+wn"]
        hp, x, y, z = sr.problem(terms, n=300, m=1, d=3)
    elif name == "m12+wn":
        terms = ZMODELS[name]
        hp, x, y, z = sr.problem(terms, n=700, m=90)
        z = z + 0.05 * np.random.default_rng(1).standard_normal(z.shape)
    else:
        terms, hp, x, y, z = mcase(name)[:5]
    loss, grad = szr.loss_and_grad(terms, szr.pack(hp, z), x, y)
    own = sr.self_error(terms, hp, x, y, z)
    kuu, kuf = sr.kuu_kuf(terms, hp, x, z)
    print("restatement's own error", name, "%.2e" % own, "cond(Kuu) %.2e" % np.linalg.cond(kuu), "median Kuf %.2e" % np.median(kuf))
    return terms, hp, x, y, z, loss, grad, own


def model(terms, hp, x, y, z):
    gp = pg.Sparse_GP(torch.from_numpy(x), torch.from_numpy(y), cov_of(terms), torch.from_numpy(z.copy()))
    gp.set_params(torch.from_numpy(hp))
    return gp


def against_the_restatement(name, tag):
    terms, hp, x, y, z, loss, grad, own = zcase(name)
    gp = model(terms, hp, x, y, z)
    vfe = pg.VFE(gp, train_z=True)
    p = vfe.start_params()
    assert np.array_equal(p, szr.pack(hp, z))
    got_l, got_g = vfe.loss_and_grad(p)
    nhp = hp.size
    assert got_g.shape == (nhp + z.size,)
    hold("%s %s loss" % (name, tag), got_l, loss, own)
    hold("%s %s hp gradient" % (name, tag), got_g[:nhp], grad[:nhp], own)
    hold("%s %s z gradient" % (name, tag), got_g[nhp:], grad[nhp:], own)
    l_hp, g_hp = pg.VFE(gp).loss_and_grad(hp.copy())          # what today's loss gives: the same bits
    assert got_l == l_hp and np.array_equal(got_g[:nhp], g_hp)
    assert torch.equal(gp.z, torch.from_numpy(z)) and torch.equal(gp.params, torch.from_numpy(hp))


@pytest.mark.parametrize("chunk", [256, None], ids=["chunk256", "default"])
@pytest.mark.parametrize("name", sorted(ZMODELS))
def test_z_gradient_against_the_restatement(ops, monkeypatch, name, chunk):
    """n = 700, m = 90, d = 3; chunk 256 walks three chunks, the last one ragged (188 columns); the default chunk holds all in one."""
    if chunk is not None:
        monkeypatch.setattr(sparse_mod, "_SPARSE_CHUNK", chunk)
    against_the_restatement(name, "chunk %s" % chunk if chunk else "one chunk")


@pytest.mark.parametrize("name", ["d17", "m1"])
def test_z_gradient_at_shapes_that_reach_other_bodies(ops, monkeypatch, name):
    """d = 17 (n = 300, m = 40): the coordinate blocks of 16; m = 1 (n = 300, d = 3): one inducing input, a lone lane.  Two chunks."""
    monkeypatch.setattr(sparse_mod, "_SPARSE_CHUNK", 256)
    against_the_restatement(name, "chunk 256")


def test_chunked_and_unchunked_agree_to_rounding(ops, monkeypatch):
    terms, hp, x, y, z, *_ = zcase("se+wn")
    gp = model(terms, hp, x, y, z)
    p = szr.pack(hp, z)
    l1, g1 = pg.VFE(gp, train_z=True).loss_and_grad(p)
    monkeypatch.setattr(sparse_mod, "_SPARSE_CHUNK", 256)
    l2, g2 = pg.VFE(gp, train_z=True).loss_and_grad(p)
    gz1, gz2 = g1[hp.size:], g2[hp.size:]
    print("chunked vs one chunk: loss %.2e z gradient %.2e" % (abs(l1 - l2) / abs(l1), np.abs(gz1 - gz2).max() / np.abs(gz1).max()))
    # the same sums in another order: the bound the hyper-parameter gradient is held to in tests/test_sparse_gpu.py
    assert abs(l1 - l2) <= 2e-10 * abs(l1) and np.abs(gz1 - gz2).max() <= 2e-10 * np.abs(gz1).max()


def test_training_z_with_the_hyper_parameters_ends_lower(ops, tmp_path, monkeypatch):
    """se + wn, n = 700, m = 20, six CG iterations from the problem's hp: the restatement ends at 300.27 with the hyper-parameters
    alone and at -20.00 with z beside them."""
    monkeypatch.chdir(tmp_path)                              # the optimiser writes its trace into the working directory
    terms = ZMODELS["se+wn"]
    hp, x, y, z = sr.problem(terms, n=700, m=20)
    ends = {}
    for train_z in (False, True):
        gp = model(terms, hp, x, y, z)
        opt = pg.CG(pg.VFE(gp, train_z=train_z))
        opt.args.update(maxiter=6, disp=False)
        opt.minimize()
        ends[train_z] = float(opt.res.fun)
    print("CG, 6 iterations: hp alone %.4f, hp and z %.4f" % (ends[False], ends[True]))
    assert np.isfinite(ends[True]) and ends[True] < ends[False]
    nhp = hp.size
    assert opt.res.x.shape == (nhp + z.size,)
    assert not torch.equal(gp.z, torch.from_numpy(z)) and gp.z.dtype == torch.float64 and gp.z.shape == z.shape
    assert np.array_equal(gp.z.numpy().reshape(-1), opt.res.x[nhp:]) and np.array_equal(gp.params.numpy(), opt.res.x[:nhp])
    own = sr.self_error(terms, gp.params.numpy(), x, y, gp.z.numpy())
    hold("VFE(model) at the written-back z", pg.VFE(gp).loss(gp.params.numpy().copy()), ends[True], own)
    fresh = model(terms, gp.params.numpy().copy(), x, y, gp.z.numpy())
    xp = torch.from_numpy(np.random.default_rng(9).random((130, 3)))
    for a, b in zip(gp.predict(xp, var="diag"), fresh.predict(xp, var="diag")):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_predict_grad_against_the_restatement(ops, name):
    terms, hp, x, y, z, xp, loss, grad, mu, cov, own = mcase(name)
    dm_ref, dv_ref = szr.predict_grads(terms, hp, x, y, z, xp)
    gp = model(terms, hp, x, y, z)
    xpt = torch.from_numpy(xp)
    mean, var, dmean, dvar = gp.predict_grad(xpt)
    m0, v0 = gp.predict(xpt, var="diag")
    assert torch.equal(mean, m0) and torch.equal(var, v0)
    for t in (dmean, dvar):
        assert t.shape == (130, 3) and t.dtype == torch.float64 and t.device == xpt.device
    hold(name + " d mean / dx*", dmean.numpy(), dm_ref, own["mean"])
    hold(name + " d var / dx*", dvar.numpy(), dv_ref, own["cov"])
    two = gp.predict_grad(xpt, var="none")
    assert len(two) == 2 and torch.equal(two[0], m0)
    hold(name + " d mean / dx* (var none)", two[1].numpy(), dm_ref, own["mean"])
    with pytest.raises(ValueError):
        gp.predict_grad(xpt, var="full")


def test_memo_holds_the_inducing_inputs(ops, monkeypatch):
    terms, hp, x, y, z, *_ = zcase("se+wn")
    gp = model(terms, hp, x, y, z)
    calls = []
    inner = pg.Sparse_GP._evaluate
    monkeypatch.setattr(pg.Sparse_GP, "_evaluate", lambda self, *a, **k: (calls.append(1), inner(self, *a, **k))[1])
    vfe = pg.VFE(gp, train_z=True)
    p = vfe.start_params()
    l0 = vfe.loss(p)
    g0 = vfe.grad(p)                                         # with train_z every evaluation forms the gradient: this one is served
    assert len(calls) == 1 and g0.shape == p.shape
    l2, g2 = vfe.loss_and_grad(p.copy())
    assert len(calls) == 1 and l2 == l0 and np.array_equal(g2, g0)
    q = p.copy()
    q[hp.size + 4] += 1e-3                                   # one coordinate of one inducing input
    l1 = vfe.loss(q)
    assert len(calls) == 2 and l1 != l0
