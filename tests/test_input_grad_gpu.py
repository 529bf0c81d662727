"""Gradients of the training objectives in the training inputs on the MI355X: Stochastic_MLE.grad_x against the longdouble restatement
(tests/lxgrad_ref.py) on the loss's own weight_factors(), MLE.grad_x against the dense NumPy closed form, counters and the memo, the bits of
loss / grad / loss_and_grad around a grad_x call, and the autograd bridge with device tensors.

Bounds (none is fitted; every test prints what it measured):
  stochastic  tests/test_lxgrad_gpu.py's derived bound in its symmetric form, (16 own_dK + (n + 2 r + 2) 2^-53) S_ik with r = 1 + probes
  exact       1e-9 max|g|, the tolerance of the existing oracle comparisons of the gradient (tests/test_parity_gpu.py)"""
import functools

import numpy as np
import pytest
import scipy.linalg as sla
import torch

import dmatmul_ref as dr
import kernel_ref as kr
import lxgrad_ref as lx
import pygpr_amd as pg
from kind_tools import T, cov_of, ops  # noqa: F401  (ops: the module's fixture)

pytestmark = pytest.mark.gpu

MODELS = {"se+wn": ["se", "wn"], "se*per+wn": [("se", "per"), "wn"]}
N, D, RANK, PROBES = 300, 3, 20, 7
EPS = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def problem(name):
    terms = MODELS[name]
    rng = np.random.default_rng(11)
    x = rng.random((N, D))
    y = np.sin(3.0 * x).sum(1) + 0.1 * rng.standard_normal(N)
    hp = []
    for part in kr.flat(terms):
        hp += [0.3] if part == "wn" else [1.1] + list(1.0 + 0.8 * rng.random(D)) + (list(0.8 + 0.5 * rng.random(D)) if part == "per" else [])
    return terms, np.array(hp), x, y


def iterative(name):
    terms, hp, x, y = problem(name)
    model = pg.Iterative_GP(T(x.copy()), T(y.copy()), cov_of(terms), rank=RANK, tol=1e-10)
    model.set_params(T(hp))
    return terms, hp, x, y, model, pg.Stochastic_MLE(model, probes=PROBES, seed=0)


def exact(name):
    terms, hp, x, y = problem(name)
    model = pg.Exact_GP(T(x.copy()), T(y.copy()), cov_of(terms))
    model.set_params(T(hp))
    return terms, hp, x, y, model, pg.MLE(model)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_stochastic_grad_x_against_the_restatement_on_its_factors(ops, name):
    terms, hp, x, y, model, loss = iterative(name)
    l, g, gx = loss.loss_and_grads(hp)
    assert (loss.solves, loss.grad_calls, loss.xgrad_calls) == (1, 1, 1) and gx.shape == (N, D) and gx.dtype == np.float64
    u, v = loss.weight_factors()
    assert u.shape == v.shape == (N, 1 + PROBES)
    ref, scale = lx.lowrank_xgrad(terms, hp, x, None, u, v, np.longdouble)
    bound = 16 * dr.own_dk(terms, hp, x, x) + (N + 2 * (1 + PROBES) + 2) * EPS
    fig = float(np.max(np.abs(gx - ref) / scale))
    print("%-10s Stochastic_MLE.grad_x against the restatement on weight_factors(): %.2e of S (bound %.2e)" % (name, fig, bound))
    assert np.isfinite(gx).all() and np.all(np.abs(gx - ref) <= bound * np.asarray(scale, np.float64))
    # a following grad_x at the same params takes nothing; loss, grad and loss_and_grad keep their bits
    assert np.array_equal(loss.grad_x(hp), gx)
    l2, g2 = loss.loss_and_grad(hp)
    assert (loss.solves, loss.grad_calls, loss.xgrad_calls) == (1, 1, 1)
    assert np.asarray(l2).tobytes() == np.asarray(l).tobytes() and g2.tobytes() == g.tobytes()
    # the same bits from a loss that never computes grad_x, and from grad_x after loss alone (one launch, no solve)
    *_, plain = iterative(name)
    lp, gp = plain.loss_and_grad(hp)
    assert np.asarray(lp).tobytes() == np.asarray(l).tobytes() and gp.tobytes() == g.tobytes()
    *_, later = iterative(name)
    la = later.loss(hp)
    gxa = later.grad_x(hp)
    assert (later.solves, later.grad_calls, later.xgrad_calls) == (1, 0, 1)
    assert np.asarray(la).tobytes() == np.asarray(l).tobytes() and gxa.tobytes() == gx.tobytes()
    assert later.grad(hp).tobytes() == g.tobytes() and later.solves == 1
    # an in-place edit of x invalidates the memo
    later.model.x[0, 0] += 0.125
    assert not np.array_equal(later.grad_x(hp)[0], gx[0]) and (later.solves, later.xgrad_calls) == (2, 2)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_exact_grad_x_against_the_dense_closed_form(ops, name):
    """n = 300 padded to 512: the padding rows and columns of A^-1 stay out of the contraction."""
    terms, hp, x, y, model, loss = exact(name)
    before = (loss.loss(hp), loss.grad(hp), loss.loss_and_grad(hp))
    got = loss.grad_x(hp)
    a = kr.kernel(terms, hp, x)
    a[np.diag_indices_from(a)] += kr.JITTER
    c = sla.cho_factor(a, lower=True)
    alpha, ainv = sla.cho_solve(c, y), sla.cho_solve(c, np.eye(N))
    dk = dr.dkernel(terms, hp, x, x)
    want = np.einsum("ij,kij->ik", ainv - np.outer(alpha, alpha), dk)
    err, big = float(np.max(np.abs(got - want))), float(np.max(np.abs(want)))
    print("%-10s MLE.grad_x against the dense closed form: %.2e of max|g| = %.3g" % (name, err / big, big))
    assert got.shape == (N, D) and got.dtype == np.float64 and err <= 1e-9 * big
    after = (loss.loss(hp), loss.grad(hp), loss.loss_and_grad(hp))
    for b, a_ in zip(before[:2] + before[2], after[:2] + after[2]):
        assert np.asarray(b).tobytes() == np.asarray(a_).tobytes()
    # ... and from a fresh loss, whose evaluations never met grad_x's buffers
    *_, fresh = exact(name)
    assert np.asarray(fresh.loss(hp)).tobytes() == np.asarray(before[0]).tobytes() and fresh.grad(hp).tobytes() == before[1].tobytes()
    assert loss.grad_x(hp).tobytes() == got.tobytes()


@pytest.mark.parametrize("which", ["exact", "stochastic"])
def test_the_bridge_with_device_tensors(ops, which):
    terms, hp, x, y, model, loss = exact("se+wn") if which == "exact" else iterative("se+wn")
    xd = torch.from_numpy(x.copy()).cuda().requires_grad_(True)
    pd = torch.from_numpy(hp.copy()).cuda().requires_grad_(True)
    val = pg.nlml_of_inputs(loss, xd, pd)
    assert val.is_cuda and val.dim() == 0 and val.dtype == torch.float64
    val.backward()
    l, ghp = loss.loss_and_grad(hp)
    gx = loss.grad_x(hp)
    assert xd.grad.is_cuda and pd.grad.is_cuda and float(val.detach()) == float(l)
    assert np.array_equal(xd.grad.cpu().numpy(), gx) and np.array_equal(pd.grad.cpu().numpy(), ghp)
    # through a linear map on the device
    raw = torch.from_numpy(np.random.default_rng(3).random((N, 4))).cuda()
    m0 = torch.linalg.lstsq(raw, xd.detach()).solution
    mt = m0.clone().requires_grad_(True)
    (2.0 * pg.nlml_of_inputs(loss, raw @ mt)).backward()
    want = 2.0 * raw.cpu().numpy().T @ loss.grad_x(model.params.numpy())
    assert mt.grad.is_cuda and np.max(np.abs(mt.grad.cpu().numpy() - want)) <= 1e-12 * np.max(np.abs(want))
    with pytest.raises(NotImplementedError, match="LOO has no gradient"):
        pg.nlml_of_inputs(pg.LOO(exact("se+wn")[4]), xd)
