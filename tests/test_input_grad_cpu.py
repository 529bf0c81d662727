"""Gradients of the training objectives in the training inputs on the host: MLE.grad_x, Stochastic_MLE.grad_x / loss_and_grads /
weight_factors and the autograd bridge nlml_of_inputs, on oracle ops.  No GPU.

The oracle ops are tests/test_varcache_cpu.VcOracleOps (kinds, matrix-free products, preconditioner) with the generator of
tests/test_sample_cpu.SampleOracleOps, pg_kernel_xgrad's two forms in one call, and the two low-rank contractions restated in NumPy
(tests/lowrank_ref.py, tests/lxgrad_ref.py): the host logic -- memo, counters, the kept solve, the bridge -- runs where there is no device."""
import functools

import numpy as np
import pytest
import scipy.linalg as sla
import torch

import dmatmul_ref as dr
import kernel_ref as kr
import lowrank_ref as lr
import lxgrad_ref as lx
import pygpr_amd as pg
import slq_ref as sq
from kind_tools import cov_of
from oracle_ops import _np
from pygpr_amd import _ops
from test_sample_cpu import SampleOracleOps
from test_varcache_cpu import VcOracleOps

T = torch.from_numpy
EPS = 2.0 ** -53
EXACT = {"se+wn": ["se", "wn"], "m52+wn": ["m52", "wn"], "se*per+wn": [("se", "per"), "wn"]}


class InputOracleOps(VcOracleOps, SampleOracleOps):
    """VcOracleOps plus the generator, pg_kernel_xgrad with both weights in one call, and the low-rank contractions."""

    def __init__(self):
        SampleOracleOps.__init__(self)

    def kernel_xgrad(self, spec, hp, xq, z, u=None, b=None, out_u=None, out_b=None, trans_b=False, accumulate=False):
        assert not accumulate and not trans_b and out_u is None and out_b is None
        q = _np(xq)
        model, h, _ = self._model(spec, _np(hp), q.shape[1])
        dk = dr.dkernel(model, h, q, _np(z))                               # [d, m, n]
        n = dk.shape[2]
        ou = None if u is None else torch.from_numpy(np.einsum("kpi,i->pk", dk, _np(u)[:n]))
        ob = None if b is None else torch.from_numpy(np.einsum("kpi,pi->pk", dk, _np(b)[:, :n]))
        return ou, ob

    def kernel_lowrank_grad_worksize(self, nr, nc, r, nhp):
        return 0

    def kernel_lowrank_grad(self, spec, hp, xr, xc, u, v, grad=None, accumulate=False, work=None):
        assert not accumulate
        x = _np(xr)
        model, h, _ = self._model(spec, _np(hp), x.shape[1])
        g = lr.lowrank_grad(model, h, x, None if xc is None else _np(xc), _np(u), _np(v))
        grad[: g.size] = torch.from_numpy(g)
        return grad

    def kernel_lowrank_xgrad_worksize(self, nr, nc, d, r):
        return 0

    def kernel_lowrank_xgrad(self, spec, hp, xr, xc, u, v, out=None, accumulate=False, work=None):
        assert not accumulate and out is None
        x = _np(xr)
        model, h, _ = self._model(spec, _np(hp), x.shape[1])
        return torch.from_numpy(np.ascontiguousarray(lx.lowrank_xgrad(model, h, x, None if xc is None else _np(xc), _np(u), _np(v))[0]))


@pytest.fixture
def in_ops(monkeypatch):
    ops = InputOracleOps()
    monkeypatch.setattr(_ops, "_OPS", ops)
    return ops


def _hp(terms, d, rng):
    hp = []
    for part in kr.flat(terms):
        if part == "wn":
            hp += [0.3]
            continue
        hp += [0.9 + 0.3 * rng.random()] + list(1.0 + 0.8 * rng.random(d))
        hp += list(0.8 + 0.5 * rng.random(d)) if part == "per" else []
    return np.array(hp)


@functools.lru_cache(maxsize=None)
def exact_problem(name, n=40, d=2):
    terms = EXACT[name]
    rng = np.random.default_rng(21)
    x = rng.random((n, d))
    y = np.sin(3.0 * x).sum(1) + 0.1 * rng.standard_normal(n)
    return terms, _hp(terms, d, rng), x, y


def closed_form(terms, hp, x, y, a=None):
    """dNLML/dx_ik = sum_j (A^-1 - alpha alpha^T)_ij dk(x_i, x_j)/dx_ik, dense, and its two parts: (g, trace part, data-fit part, alpha)."""
    if a is None:
        a = kr.kernel(terms, hp, x)
        a[np.diag_indices_from(a)] += kr.JITTER
    c = sla.cho_factor(a, lower=True)
    alpha, ainv = sla.cho_solve(c, y), sla.cho_solve(c, np.eye(x.shape[0]))
    dk = dr.dkernel(terms, hp, x, x)                                       # [d, n, n]: dk(x_i, x_j)/dx_ik
    trace = np.einsum("ij,kij->ik", ainv, dk)
    fit = -alpha[:, None] * np.einsum("j,kij->ik", alpha, dk)
    return trace + fit, trace, fit, alpha


def exact_model(name):
    terms, hp, x, y = exact_problem(name)
    model = pg.Exact_GP(T(x.copy()), T(y.copy()), cov_of(terms))
    model.set_params(T(hp))
    return terms, hp, x, y, model


# ------------------------------------------------------------------------------------------- MLE.grad_x
@pytest.mark.parametrize("name", sorted(EXACT))
def test_exact_grad_x_is_the_dense_closed_form(in_ops, name):
    terms, hp, x, y, model = exact_model(name)
    loss = pg.MLE(model)
    before = loss.loss_and_grad(hp)
    got = loss.grad_x(hp)
    want = closed_form(terms, hp, x, y)[0]
    err, big = float(np.max(np.abs(got - want))), float(np.max(np.abs(want)))
    print("%-10s MLE.grad_x against the dense closed form: %.2e of max|g| = %.3g" % (name, err / big, big))
    assert got.shape == x.shape and got.dtype == np.float64
    assert err <= 1e-10 * big
    after = loss.loss_and_grad(hp)
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()


# The h/2 errors measured on the host (central differences of kernel_ref.nlml in float64, h = 1e-3 and 5e-4, relative to max|g|; both
# steps sit in the truncation regime, the ratio is 4.00 for all three): the assertion allows ten times each.
FD_MEASURED = {"se+wn": 4.32e-6, "m52+wn": 4.35e-6, "se*per+wn": 4.99e-5}


@pytest.mark.parametrize("name", sorted(EXACT))
def test_the_closed_form_is_the_derivative_of_the_oracles_nlml(name):
    terms, hp, x, y = exact_problem(name)
    g = closed_form(terms, hp, x, y)[0]
    errs = []
    for h in (1e-3, 5e-4):
        fd = np.zeros_like(x)
        for i in range(x.shape[0]):
            for k in range(x.shape[1]):
                a, b = x.copy(), x.copy()
                a[i, k] += h
                b[i, k] -= h
                fd[i, k] = (kr.nlml(terms, hp, a, y) - kr.nlml(terms, hp, b, y)) / (2 * h)
        errs.append(float(np.max(np.abs(fd - g))) / float(np.max(np.abs(g))))
    print("%-10s closed form vs central differences: h = 1e-3 %.2e, h = 5e-4 %.2e (ratio %.2f) of max|g|" % (name, errs[0], errs[1],
                                                                                                            errs[0] / errs[1]))
    assert errs[0] >= 3 * errs[1]
    assert errs[1] <= 10 * FD_MEASURED[name]


def test_exact_grad_x_refusals(in_ops):
    terms, hp, x, y, model = exact_model("se+wn")
    loss = pg.MLE(model)
    with pytest.raises(NotImplementedError, match="batched"):
        loss.grad_x(np.stack([hp, hp]))
    with pytest.raises(TypeError, match="float64 only"):
        loss.grad_x(hp.astype(np.float32))
    m32 = pg.Exact_GP(T(x).float(), T(y).float(), cov_of(terms))
    with pytest.raises(TypeError, match="float64 only"):
        pg.MLE(m32).grad_x(hp)
    bat = pg.Exact_GP(T(np.stack([x, x])), T(np.stack([y, y])), cov_of(terms))
    with pytest.raises(NotImplementedError, match="batched"):
        pg.MLE(bat).grad_x(hp)


# ------------------------------------------------------------------------------------------- Stochastic_MLE
N, D, RANK, PROBES, SEED, TOL = 120, 2, 30, 32, 0, 1e-8
SE_WN = ["se", "wn"]


@functools.lru_cache(maxsize=None)
def stochastic_problem():
    rng = np.random.default_rng(0)
    x = rng.random((N, D))
    y = np.sin(3.0 * x).sum(1) + 0.1 * rng.standard_normal(N)
    return np.array([1.1, 1.4, 0.9, 0.3]), x, y


def stochastic_model(seed=SEED):
    hp, x, y = stochastic_problem()
    model = pg.Iterative_GP(T(x.copy()), T(y.copy()), cov_of(SE_WN), rank=RANK, tol=TOL)
    model.set_params(T(hp))
    return hp, x, y, model, pg.Stochastic_MLE(model, probes=PROBES, seed=seed)


def test_stochastic_grad_x_is_the_restatement_on_its_factors(in_ops):
    """Within the derived bound of tests/test_lxgrad_gpu.py, (16 own_dK + (n + 2 r + 2) 2^-53) S_ik, against np.longdouble."""
    hp, x, y, model, loss = stochastic_model()
    gx = loss.grad_x(hp)
    u, v = loss.weight_factors()
    assert gx.shape == (N, D) and u.shape == v.shape == (N, 1 + PROBES) and u.flags.owndata and v.flags.owndata
    ref, scale = lx.lowrank_xgrad(SE_WN, hp, x, None, u, v, np.longdouble)
    bound = 16 * dr.own_dk(SE_WN, hp, x, x) + (N + 2 * (1 + PROBES) + 2) * EPS
    fig = float(np.max(np.abs(gx - ref) / scale))
    print("Stochastic_MLE.grad_x against the restatement on weight_factors(): %.2e of S (bound %.2e)" % (fig, bound))
    assert np.all(np.abs(gx - ref) <= bound * np.asarray(scale, np.float64))
    # the factors are the documented ones: U = [-alpha / 2, S / (2 t)], V = [alpha, P^-1 Z]
    alpha = closed_form(SE_WN, hp, x, y, sq.setup(SE_WN, hp, x, RANK)[0])[3]
    assert np.max(np.abs(v[:, 0] - alpha)) <= 1e-8 * np.max(np.abs(alpha)) and np.array_equal(u[:, 0], -0.5 * v[:, 0])


def test_the_estimator_is_centred_and_its_data_fit_part_exact(in_ops):
    """Per-probe contributions from the restatement on single factor columns (times t: U carries 1 / (2 t)); for every entry the mean of
    the 32 and its standard error, against the exact trace part sum_j A^-1_ij d1k_ijk of the dense closed form.  At most 1 % of the
    n d = 240 entries beyond 4 standard errors (Student-t, 31 degrees of freedom: 0.1 entries expected), none beyond 6.  Deterministic:
    pg_randn is tests/philox_ref.py's generator; seed 0 meets the condition."""
    hp, x, y, model, loss = stochastic_model()
    loss.grad_x(hp)
    u, v = loss.weight_factors()
    a = sq.setup(SE_WN, hp, x, RANK)[0]
    g, trace, fit, alpha = closed_form(SE_WN, hp, x, y, a)
    per = np.stack([PROBES * lx.lowrank_xgrad(SE_WN, hp, x, None, u[:, c: c + 1], v[:, c: c + 1])[0] for c in range(1, 1 + PROBES)])
    mean, se = per.mean(0), per.std(0, ddof=1) / np.sqrt(PROBES)
    z = np.abs(mean - trace) / se
    print("trace part: |mean - exact| / stderr: max %.2f, beyond 4: %d of %d, beyond 6: %d" % (float(z.max()), int((z > 4).sum()), z.size,
                                                                                           int((z > 6).sum())))
    assert int((z > 4).sum()) <= 0.01 * z.size and not (z > 6).any()
    col0 = lx.lowrank_xgrad(SE_WN, hp, x, None, u[:, :1], v[:, :1])[0]
    err = float(np.max(np.abs(col0 - fit)))
    print("data-fit part: column 0 against -alpha_i sum_j alpha_j d1k: %.2e of max %.3g" % (err / float(np.max(np.abs(fit))),
                                                                                         float(np.max(np.abs(fit)))))
    assert err <= 1e-8 * float(np.max(np.abs(fit)))


def test_counters_and_the_memo(in_ops):
    hp, x, y, model, loss = stochastic_model()
    l, g, gx = loss.loss_and_grads(hp)
    assert (loss.solves, loss.grad_calls, loss.xgrad_calls) == (1, 1, 1)
    assert np.array_equal(loss.grad_x(hp), gx) and loss.grad_x(hp) is not loss.grad_x(hp)
    l2, g2 = loss.loss_and_grad(hp)
    assert float(l2) == float(l) and np.array_equal(g2, g) and float(loss.loss(hp)) == float(l)
    assert (loss.solves, loss.grad_calls, loss.xgrad_calls) == (1, 1, 1)
    # after loss(p) or grad(p) alone, grad_x(p) adds its launch and no solve
    other = hp * 1.01
    loss.loss(other)
    assert (loss.solves, loss.grad_calls, loss.xgrad_calls) == (2, 1, 1)
    gxo = loss.grad_x(other)
    assert (loss.solves, loss.grad_calls, loss.xgrad_calls) == (2, 1, 2)
    loss.grad(other)
    assert (loss.solves, loss.grad_calls, loss.xgrad_calls) == (2, 2, 2) and np.array_equal(loss.grad_x(other), gxo)
    # grad_x first: a solve of its own, which loss and grad then find
    third = hp * 0.99
    gxt = loss.grad_x(third)
    assert (loss.solves, loss.grad_calls, loss.xgrad_calls) == (3, 2, 3)
    loss.loss(third)
    loss.grad(third)
    assert (loss.solves, loss.grad_calls, loss.xgrad_calls) == (3, 3, 3)
    # an in-place edit of x invalidates the memo
    model.x[0, 0] += 0.25
    gxe = loss.grad_x(third)
    assert (loss.solves, loss.grad_calls, loss.xgrad_calls) == (4, 3, 4) and not np.array_equal(gxe[0], gxt[0])
    with pytest.raises(TypeError, match="float64 only"):
        loss.grad_x(hp.astype(np.float32))
    fresh = pg.Stochastic_MLE(model, probes=3)
    with pytest.raises(RuntimeError, match="no evaluation is kept"):
        fresh.weight_factors()


def test_the_module_docstring_says_what_grad_x_is():
    from pygpr_amd import stochastic

    doc = " ".join(stochastic.__doc__.split())
    assert "`grad_x` is an estimator built from the same probes" in doc
    assert "pivots of the preconditioner change discretely with x as well" in doc


# ------------------------------------------------------------------------------------------- the bridge
@pytest.mark.parametrize("which", ["exact", "stochastic"])
def test_the_bridge_hands_out_grad_x_and_grad_hp(in_ops, which):
    if which == "exact":
        terms, hp, x, y, model = exact_model("se+wn")
        loss = pg.MLE(model)
    else:
        hp, x, y, model, loss = stochastic_model()
    n, d = x.shape
    # a leaf x and leaf params
    xt, pt = T(x.copy()).requires_grad_(True), T(hp.copy()).requires_grad_(True)
    val = pg.nlml_of_inputs(loss, xt, pt)
    assert val.dim() == 0 and val.dtype == torch.float64 and val.requires_grad
    assert model.x.data_ptr() == xt.data_ptr() and not model.x.requires_grad
    val.backward()
    l, ghp = loss.loss_and_grad(hp)
    gx = loss.grad_x(hp)
    assert float(val.detach()) == float(l) and np.array_equal(xt.grad.numpy(), gx) and np.array_equal(pt.grad.numpy(), ghp)
    # through a linear map x = raw @ M, and an upstream scalar
    rng = np.random.default_rng(3)
    raw = T(rng.random((n, 4)))
    m0 = np.linalg.lstsq(raw.numpy(), x, rcond=None)[0]
    mt = T(m0.copy()).requires_grad_(True)
    (3.0 * pg.nlml_of_inputs(loss, raw @ mt)).backward()
    gxm = loss.grad_x(model.params.numpy())
    want = 3.0 * raw.numpy().T @ gxm
    assert np.max(np.abs(mt.grad.numpy() - want)) <= 1e-12 * np.max(np.abs(want))
    # params that do not require grad get none; params None reads model.params
    xt2 = T(x.copy()).requires_grad_(True)
    pg.nlml_of_inputs(loss, xt2, T(hp.copy())).backward()
    assert np.array_equal(xt2.grad.numpy(), gx)


def test_the_bridge_refuses_other_losses(in_ops):
    terms, hp, x, y, model = exact_model("se+wn")
    xt = T(x.copy()).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="LOO has no gradient in the training inputs"):
        pg.nlml_of_inputs(pg.LOO(model), xt)
    sparse = pg.Sparse_GP(T(x.copy()), T(y.copy()), cov_of(terms), T(x[:7].copy()))
    with pytest.raises(NotImplementedError, match="VFE has no gradient in the training inputs"):
        pg.nlml_of_inputs(pg.VFE(sparse), xt)
    with pytest.raises(NotImplementedError, match="no batches"):
        pg.nlml_of_inputs(pg.MLE(model), xt[None])
