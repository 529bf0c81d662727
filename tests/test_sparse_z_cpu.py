"""Sparse_GP's derivatives in its point sets on the host: the restatement (tests/sparse_z_ref.py) against central differences, the
optimisers' start / write-back hooks, the packed parameter vector of VFE(train_z=True), and the class logic of pygpr_amd/sparse.py --
the z-gradient, predict_grad, training, the memo -- on a test double of the device ops.  No GPU.

Bound of the difference quotients: 1e-6 of the largest entry, the project's figure for the hyper-parameter gradient in
tests/test_sparse_cpu.py (a loss known to 1e-12 relative at step 1e-5: 1e-12 |L| / 1e-5 of rounding, h^2 of truncation).  Measured:
at most 1.5e-8 for the z-gradient.  Matern-1/2 has no derivative where an inducing input sits on a training point (the library's
convention gives that pair 0, central differences straddle the cusp), so its case takes z off the data."""
import numpy as np
import pytest
import torch

import kernel_ref as kr
import pygpr_amd as pg
import sparse_ref as sr
import sparse_z_ref as szr
from oracle_ops import _np
from pygpr_amd import _ops
from pygpr_amd import sparse as sparse_mod
from test_sparse_cpu import MODELS, SparseOracleOps

H = 1e-5
BOUND = 1e-6
TERMS = {"se+wn": ["se", "wn"], "m32+rq+wn": ["m32", "rq", "wn"], "se*per+wn": [("se", "per"), "wn"], "m12+wn": ["m12", "wn"]}
CASES = [(name, moved) for name in ("se+wn", "m32+rq+wn", "se*per+wn") for moved in (False, True)] + [("m12+wn", True)]


def small(name, moved):
    terms = TERMS[name]
    hp, x, y, z = sr.problem(terms, n=120, m=12, d=3, seed=3)
    if moved:
        z = z + 0.05 * np.random.default_rng(1).standard_normal(z.shape)
    return terms, hp, x, y, z


# ------------------------------------------------------------------------------------------- the restatement against differences
@pytest.mark.parametrize("name,moved", CASES, ids=["%s-%s" % (n, "moved" if mv else "on-data") for n, mv in CASES])
def test_z_gradient_against_central_differences(name, moved):
    terms, hp, x, y, z = small(name, moved)
    g = szr.z_grad(terms, hp, x, y, z)
    fd = np.zeros_like(g)
    for i in range(z.shape[0]):
        for k in range(z.shape[1]):
            up, dn = z.copy(), z.copy()
            up[i, k] += H
            dn[i, k] -= H
            fd[i, k] = (sr.loss_woodbury(terms, hp, x, y, up) - sr.loss_woodbury(terms, hp, x, y, dn)) / (2 * H)
    err = np.abs(g - fd).max() / np.abs(fd).max()
    print("z-gradient vs central differences", name, "moved" if moved else "on the data", "%.2e" % err)
    assert g.shape == z.shape and err <= BOUND


@pytest.mark.parametrize("name,moved", CASES, ids=["%s-%s" % (n, "moved" if mv else "on-data") for n, mv in CASES])
def test_predict_grads_against_central_differences(name, moved):
    """A prediction at x*_p depends on x*_p alone: coordinate k of every test point is stepped at once."""
    terms, hp, x, y, z = small(name, moved)
    xp = np.random.default_rng(9).random((25, 3))
    dmean, dvar = szr.predict_grads(terms, hp, x, y, z, xp)
    fm, fv = np.zeros_like(dmean), np.zeros_like(dvar)
    for k in range(3):
        up, dn = xp.copy(), xp.copy()
        up[:, k] += H
        dn[:, k] -= H
        (mu1, v1), (mu0, v0) = sr.predict(terms, hp, x, y, z, up), sr.predict(terms, hp, x, y, z, dn)
        fm[:, k], fv[:, k] = (mu1 - mu0) / (2 * H), (v1 - v0) / (2 * H)
    em, ev = np.abs(dmean - fm).max() / np.abs(fm).max(), np.abs(dvar - fv).max() / np.abs(fv).max()
    print("predict_grads vs central differences", name, "mean %.2e variance %.2e" % (em, ev))
    assert dmean.shape == dvar.shape == xp.shape and em <= BOUND and ev <= BOUND


def test_packed_loss_and_grad_is_the_two_gradients_side_by_side():
    terms, hp, x, y, z = small("se+wn", True)
    loss, g = szr.loss_and_grad(terms, szr.pack(hp, z), x, y)
    l_ref, g_ref = sr.loss_and_grad(terms, hp, x, y, z)
    assert loss == l_ref and np.array_equal(g[: hp.size], g_ref) and np.array_equal(g[hp.size:], szr.z_grad(terms, hp, x, y, z).reshape(-1))
    h2, z2 = szr.unpack(szr.pack(hp, z), hp.size, 3)
    assert np.array_equal(h2, hp) and np.array_equal(z2, z)


# ------------------------------------------------------------------------------------------- host logic on a test double
class SparseZOracleOps(SparseOracleOps):
    """SparseOracleOps plus the contraction of the first-argument derivative (pg_kernel_xgrad) by kernel_ref."""

    def __init__(self):
        super().__init__()
        self.xgrad_calls = []

    def kernel_xgrad(self, spec, hp, xq, z, u=None, b=None, out_u=None, out_b=None, trans_b=False, accumulate=False):
        assert not trans_b and (u is None) == (out_u is None) and (b is None) == (out_b is None) and (u is not None or b is not None)
        m, d = xq.shape
        n = z.shape[0]
        assert b is None or (b.is_contiguous() and b.shape[0] >= m and b.shape[1] >= n)      # what HipOps asks of its operands
        (sp,) = spec if isinstance(spec, (list, tuple)) else [spec]
        model, h, _ = self._model(sp, _np(hp), d)
        dks = kr.kernel_xgrad(model, h, _np(z), _np(xq))                                      # [d, m, n]
        self.xgrad_calls.append((m, n, u is not None, b is not None, bool(accumulate)))
        for w, out, sub in ((u, out_u, "kpi,i->pk"), (b, out_b, "kpi,pi->pk")):
            if w is not None:
                val = torch.from_numpy(np.einsum(sub, dks, _np(w)[:n] if w.dim() == 1 else _np(w)[:m, :n]))
                assert out.shape == (m, d)
                out.copy_(out + val if accumulate else val)
        return out_u, out_b


@pytest.fixture
def z_ops(monkeypatch, tmp_path):
    ops = SparseZOracleOps()
    monkeypatch.setattr(_ops, "_OPS", ops)
    monkeypatch.chdir(tmp_path)
    return ops


def model_of(name, n=300, m=40, **kw):
    terms, make = MODELS[name]
    hp, x, y, z = sr.problem(terms, n=n, m=m, **kw)
    gp = pg.Sparse_GP(torch.from_numpy(x), torch.from_numpy(y), make(), torch.from_numpy(z))
    gp.set_params(torch.from_numpy(hp))
    return terms, hp, x, y, z, gp


def test_default_hooks_are_what_the_drivers_read_and_wrote(z_ops):
    terms, hp, x, y, z, gp = model_of("se+wn")
    for loss in (pg.MLE(pg.Exact_GP(gp.x, gp.y, gp.cov)), pg.VFE(gp)):
        mdl = loss.model
        mdl.set_params(torch.from_numpy(hp))
        start = loss.start_params()
        assert isinstance(start, np.ndarray) and np.array_equal(start, mdl.params.numpy()) and not np.shares_memory(start, mdl.params.numpy())
        seen = []
        mdl.set_params = lambda p, seen=seen: seen.append(p)
        loss.write_back(hp * 1.5)
        assert len(seen) == 1 and isinstance(seen[0], torch.Tensor) and seen[0].dtype == torch.float64
        assert np.array_equal(seen[0].numpy(), hp * 1.5)


def test_packing_round_trips_and_write_back_assigns_both(z_ops):
    terms, hp, x, y, z, gp = model_of("se+wn")
    vfe = pg.VFE(gp, train_z=True)
    p = vfe.start_params()
    assert p.dtype == np.float64 and p.shape == (hp.size + z.size,) and np.array_equal(p, szr.pack(hp, z))
    h2, z2 = vfe.unpack(p)
    assert np.array_equal(h2, hp) and np.array_equal(z2, z) and np.array_equal(vfe.pack(h2, z2), p)
    gp.update()
    old_z = gp.z
    vfe.write_back(p * 1.01)
    assert gp.need_upd and gp.z is not old_z and torch.equal(old_z, torch.from_numpy(z))          # a new tensor, the old one untouched
    assert gp.z.dtype == torch.float64 and gp.z.device.type == "cpu" and gp.z.shape == (40, 3)
    assert np.array_equal(gp.z.numpy(), z * 1.01) and np.array_equal(gp.params.numpy(), hp * 1.01)
    assert not pg.VFE(gp).train_z and pg.VFE(gp).start_params().shape == (hp.size,)


def test_wrong_length_is_refused_before_anything_touches_the_device(monkeypatch):
    terms, hp, x, y, z = small("se+wn", False)
    gp = pg.Sparse_GP(torch.from_numpy(x), torch.from_numpy(y), MODELS["se+wn"][1](), torch.from_numpy(z))

    def no_device():
        raise AssertionError("the device was asked for")

    monkeypatch.setattr(sparse_mod, "get_ops", no_device)
    vfe = pg.VFE(gp, train_z=True)
    good = szr.pack(hp, z)
    for bad in (hp, good[:-1], np.concatenate([good, [0.0]]), good.reshape(1, -1)):
        for call in (vfe.loss, vfe.grad, vfe.loss_and_grad, vfe.write_back):
            with pytest.raises(ValueError, match="train_z"):
                call(bad)
    with pytest.raises(AssertionError, match="device"):
        vfe.loss(good)                                        # the right length is what reaches it


@pytest.mark.parametrize("name", sorted(MODELS))
@pytest.mark.parametrize("chunk", [128, 32768])
def test_class_agrees_with_the_restatement(z_ops, monkeypatch, name, chunk):
    monkeypatch.setattr(sparse_mod, "_SPARSE_CHUNK", chunk)
    terms, hp, x, y, z, gp = model_of(name)
    z = z + 0.05 * np.random.default_rng(1).standard_normal(z.shape)      # evaluate off the model's own z
    tol = sr.tol_of(sr.self_error(terms, hp, x, y, z))
    l_ref, g_ref = szr.loss_and_grad(terms, szr.pack(hp, z), x, y)
    vfe = pg.VFE(gp, train_z=True)
    loss, grad = vfe.loss_and_grad(szr.pack(hp, z))
    nhp = hp.size
    assert grad.shape == (nhp + z.size,) and abs(loss - l_ref) <= tol * abs(l_ref)
    assert np.abs(grad[:nhp] - g_ref[:nhp]).max() <= tol * np.abs(g_ref[:nhp]).max()
    assert np.abs(grad[nhp:] - g_ref[nhp:]).max() <= tol * np.abs(g_ref[nhp:]).max()
    want = [(40, 40, False, True, False)] + [(40, min(chunk, 300 - s), False, True, True) for s in range(0, 300, chunk)]
    assert z_ops.xgrad_calls == want
    assert torch.equal(gp.z, torch.from_numpy(sr.problem(terms)[3]))                                # the model's own z was not assigned
    # the hyper-parameter part and the loss are those of the plain loss on a model that holds this z, bit for bit
    gp2 = pg.Sparse_GP(gp.x, gp.y, gp.cov, torch.from_numpy(z))
    l2, g2 = pg.VFE(gp2).loss_and_grad(hp.copy())
    assert l2 == loss and np.array_equal(g2, grad[:nhp])
    assert pg.VFE(gp, train_z=True).loss(szr.pack(hp, z)) == loss


def test_predict_grad(z_ops, monkeypatch):
    terms, hp, x, y, z, gp = model_of("m32+rq+wn")
    xp = np.random.default_rng(2).random((70, 3))
    xpt = torch.from_numpy(xp)
    tol = sr.tol_of(sr.self_error(terms, hp, x, y, z))
    dm_ref, dv_ref = szr.predict_grads(terms, hp, x, y, z, xp)
    mean, var, dmean, dvar = gp.predict_grad(xpt)
    m0, v0 = gp.predict(xpt, var="diag")
    assert torch.equal(mean, m0) and torch.equal(var, v0)
    assert dmean.shape == dvar.shape == (70, 3) and dmean.dtype == dvar.dtype == torch.float64
    assert np.abs(dmean.numpy() - dm_ref).max() <= tol * np.abs(dm_ref).max()
    assert np.abs(dvar.numpy() - dv_ref).max() <= tol * np.abs(dv_ref).max()
    assert z_ops.xgrad_calls == [(70, 40, True, True, False)]
    del z_ops.xgrad_calls[:]
    two = gp.predict_grad(xpt, var="none")
    assert len(two) == 2 and torch.equal(two[0], m0) and torch.equal(two[1], dmean) and z_ops.xgrad_calls == [(70, 40, True, False, False)]
    monkeypatch.setattr(sparse_mod, "_CHUNK", 32)                                   # three chunks of test points, the last one of 6
    parts = gp.predict_grad(xpt)
    for a, b in zip(parts, (mean, var, dmean, dvar)):
        assert torch.allclose(a, b, rtol=0, atol=1e-13)
    with pytest.raises(ValueError, match="var"):
        gp.predict_grad(xpt, var="full")
    with pytest.raises(NotImplementedError, match="differentiable"):
        gp.predict(xpt.clone().requires_grad_(True), var="diag")
    assert len(gp.predict_grad(xpt.clone().requires_grad_(True))) == 4             # no autograd: a leaf that asks for it is served


def test_memo_holds_the_inducing_inputs(z_ops, monkeypatch):
    terms, hp, x, y, z, gp = model_of("se+wn")
    calls = []
    inner = pg.Sparse_GP._evaluate
    monkeypatch.setattr(pg.Sparse_GP, "_evaluate", lambda self, *a, **k: (calls.append(1), inner(self, *a, **k))[1])
    vfe = pg.VFE(gp, train_z=True)
    p = vfe.start_params()
    l0 = vfe.loss(p)                                         # with train_z every evaluation forms the gradient ...
    g = vfe.grad(p)                                          # ... so this one is served
    assert len(calls) == 1 and g.shape == p.shape and vfe.loss_and_grad(p.copy())[0] == l0 and len(calls) == 1
    q = p.copy()
    q[hp.size + 4] += 1e-3
    l1 = vfe.loss(q)
    assert len(calls) == 2 and l1 != l0
    plain = pg.VFE(gp)                                       # the plain loss is today's: a loss-only evaluation holds no gradient
    plain.loss(hp.copy())
    plain.grad(hp.copy())
    assert len(calls) == 4


def test_training_z_with_the_hyper_parameters_ends_lower(z_ops):
    ends = []
    for train_z in (False, True):
        terms, hp, x, y, z, gp = model_of("se+wn", n=150, m=10)
        vfe = pg.VFE(gp, train_z=train_z)
        opt = pg.CG(vfe)
        opt.args.update(maxiter=4, disp=False)
        opt.minimize()
        ends.append(float(opt.res.fun))
        assert opt.res.x.shape == (hp.size + (z.size if train_z else 0),)
        assert torch.equal(gp.z, torch.from_numpy(z)) != train_z                    # written back when trained, untouched when not
        assert abs(float(pg.VFE(gp).loss(gp.params.numpy().copy())) - ends[-1]) <= 1e-9 * abs(ends[-1])
    print("CG, 4 iterations: hp alone %.4f, hp and z %.4f" % tuple(ends))
    assert ends[1] < ends[0]
