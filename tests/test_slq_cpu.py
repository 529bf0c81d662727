"""Stochastic_MLE on the host: the restatement (tests/slq_ref.py) against dense linear algebra -- the quadrature's identities, log|P|,
its dense limit, the unbiasedness of both estimators -- the package's own host arithmetic against the restatement, and the refusals
that need no device.  No GPU."""
import numpy as np
import pytest
import torch

import kernel_ref as kr
import pygpr_amd as pg
import slq_ref as sq
import sparse_ref as sr
from pygpr_amd import stochastic as st_mod

SE_WN = ["se", "wn"]
TOL = 1e-10


@pytest.fixture(scope="module")
def problem():
    hp, x, y, _ = sr.problem(SE_WN, n=700, m=40)
    return hp, x, y


@pytest.fixture(scope="module")
def estimates(problem):
    hp, x, y = problem
    return {rank: sq.estimate(SE_WN, hp, x, y, rank, 0, 15, TOL) for rank in (0, 40, 100)}


def test_stream_constants_match_the_package():
    assert (sq.STREAM_G1, sq.STREAM_G2) == (st_mod.STREAM_G1, st_mod.STREAM_G2) and sq.STREAM_G1 != sq.STREAM_G2


@pytest.mark.parametrize("rank", [0, 40, 100])
def test_quadrature_at_the_reciprocal_is_the_solve(estimates, problem, rank):
    """e_1^T T_k^-1 e_1 (r^T z)_0 = b^T x_k, an identity of CG from x_0 = 0; the solve runs on past the column's k steps, which moves
    b^T x by no more than cond(A) tol of it."""
    hp, x, y = problem
    e = estimates[rank]
    b = np.concatenate([y[:, None], e["z"]], 1)
    sol = np.concatenate([e["alpha"][:, None], e["s"]], 1)
    want = np.sum(b * sol, 0)
    got = np.array([sq.quadrature(e["rec"], c, TOL, f=lambda v: 1.0 / v) for c in range(16)])
    err = float(np.max(np.abs(got - want) / np.abs(want)))
    bound = np.linalg.cond(e["a"]) * TOL
    print("rank %3d: quadrature at 1/x against b^T A^-1 b of the same solve: %.2e (bound %.2e)" % (rank, err, bound))
    assert err <= bound


@pytest.mark.parametrize("rank", [1, 20, 100])
def test_logdet_of_the_preconditioner(problem, rank):
    hp, x, y = problem
    _, l, shift, pre = sq.setup(SE_WN, hp, x, rank)
    sign, want = np.linalg.slogdet(pre.dense())
    got = sq.logdet_p(l, shift)
    # both sum n logarithms of pivots that carry cond(P) 2^-53 each
    bound = 700 * np.linalg.cond(pre.dense()) * 2.0 ** -53
    print("rank %3d: log|P| %.12g against slogdet %.12g (difference %.2e, bound %.2e)" % (rank, got, want, abs(got - want), bound))
    assert sign == 1 and abs(got - want) <= bound


@pytest.mark.parametrize("rank", [40, 100])
def test_quadrature_reaches_its_dense_limit(estimates, rank):
    e = estimates[rank]
    err = float(np.max(np.abs(e["q"] - e["q_limit"])))
    print("rank %3d: %d iterations, quadrature against z^T P^-1/2 log(P^-1/2 A P^-1/2) P^-1/2 z: %.2e absolute" % (rank, e["iterations"], err))
    assert err <= 1e-9


def test_the_untruncated_tridiagonal_is_noise(estimates):
    """The columns share the iteration count: past its own convergence a column's coefficients are rounding noise and the cut is what
    keeps T meaningful -- the steps used differ between the columns and stay below the shared count."""
    rec = estimates[40]["rec"]
    used = [sq.steps_used(rec["rz"][:, c], rec["rz0"][c], TOL) for c in range(16)]
    print("steps used per column:", used, "of", rec["rz"].shape[0])
    assert max(used) <= rec["rz"].shape[0] and min(used) >= 1


@pytest.mark.parametrize("rank", [0, 40])
def test_the_packages_host_arithmetic_is_the_restatements(estimates, rank):
    e = estimates[rank]
    rec = e["rec"]
    for c in (0, 1, 15):
        k = sq.steps_used(rec["rz"][:, c], rec["rz0"][c], TOL)
        assert k == st_mod.steps_used(rec["rz"][:, c], rec["rz0"][c], TOL)
        assert np.array_equal(st_mod.tridiagonal(rec["step"][:, c], rec["beta"][:, c], k), sq.tridiagonal(rec["step"][:, c], rec["beta"][:, c], k))
    mine = np.array([st_mod.quadrature(rec["step"][:, c], rec["beta"][:, c], rec["rz"][:, c], rec["rz0"][c], TOL) for c in range(1, 16)])
    err = float(np.max(np.abs(mine - e["q"])))
    print("rank %3d: the package's quadrature against the restatement's: %.2e absolute" % (rank, err))
    assert err <= 1e-9


@pytest.mark.parametrize("rank", [40, 100])
def test_pcg_gradient_is_the_dense_solve_gradient(estimates, problem, rank):
    hp, x, y = problem
    e = estimates[rank]
    dense, scale, *_ = sq.grad_dense(SE_WN, hp, x, y, e["a"], e["pre"], e["z"])
    got, _ = sq.grad_from(SE_WN, hp, x, e["alpha"], e["s"], e["pz"])
    err = np.abs(got - dense) / scale
    bound = 2 * np.linalg.cond(e["a"]) * TOL
    print("rank %3d: gradient from PCG solves against dense solves: %.2e of S_p (bound %.2e)" % (rank, float(err.max()), bound))
    assert np.all(err <= bound)


def test_both_estimators_are_unbiased():
    """n = 300, 2000 probes in blocks of 500: the mean log-determinant and every gradient entry lie within 4 of their own standard
    errors of slogdet(A) and of kernel_ref.nlml_and_grad."""
    import scipy.linalg as sla

    hp, x, y, _ = sr.problem(SE_WN, n=300, m=20)
    a, l, shift, pre = sq.setup(SE_WN, hp, x, 20)
    ldp = sq.logdet_p(l, shift)
    c = sla.cho_factor(a, lower=True)
    alpha = sla.cho_solve(c, y)
    slabs = list(kr.grad_terms(SE_WN, hp, x))
    per, gper = [], []
    for blk in range(4):
        z = sq.probes(0, l, shift, 500, first=500 * blk)
        per.append(ldp + sq.dense_limit(a, l, shift, z))
        s, pz = sla.cho_solve(c, z), pre.solve(z)
        gper.append(np.stack([0.5 * np.sum(s * (slab @ pz), 0) - 0.5 * float(alpha @ slab @ alpha) for _, slab in slabs]))
    per, gper = np.concatenate(per), np.concatenate(gper, 1)
    want = np.linalg.slogdet(a)[1]
    se = per.std(ddof=1) / np.sqrt(per.size)
    print("log|A| %.6f, mean of 2000 probes %.6f, standard error %.4f: %.2f standard errors" % (want, per.mean(), se, (per.mean() - want) / se))
    assert abs(per.mean() - want) <= 4 * se
    _, gwant = kr.nlml_and_grad(SE_WN, hp, x, y)
    for (i, _), row in zip(slabs, gper):
        gse = row.std(ddof=1) / np.sqrt(row.size)
        print("gradient entry %d: exact %.6f, mean %.6f, standard error %.4f: %.2f standard errors" % (i, gwant[i], row.mean(), gse,
                                                                                                      (row.mean() - gwant[i]) / gse))
        assert abs(row.mean() - gwant[i]) <= 4 * gse


# ------------------------------------------------------------------------------------------- the loss's host logic
def _cov():
    return pg.Compose([pg.Squared_exponential(), pg.White_noise()])


def test_refusals_that_need_no_device():
    x, y = torch.rand(20, 3, dtype=torch.float64), torch.rand(20, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="MLE"):
        pg.Stochastic_MLE(pg.Exact_GP(x, y, _cov()))
    model = pg.Iterative_GP(x, y, _cov(), rank=5)
    for bad in (0, -3, 1.5, 64):
        with pytest.raises(ValueError):
            pg.Stochastic_MLE(model, probes=bad)
    with pytest.raises(ValueError):
        pg.Stochastic_MLE(model, seed=0.5)
    with pytest.raises(TypeError):
        pg.Iterative_GP(x.float(), y.float(), _cov())
    loss = pg.Stochastic_MLE(model)
    assert (loss.probes, loss.seed) == (15, 0) and loss.slq_info is None and isinstance(loss, pg.Loss)
    with pytest.raises(TypeError):
        loss.loss(np.ones(5, np.float32))
    for refusing in (pg.MLE, pg.LOO):                       # unchanged: they keep pointing to VFE, and now name the new class too
        with pytest.raises(NotImplementedError, match="VFE"):
            refusing(model)
        with pytest.raises(NotImplementedError, match="Stochastic_MLE"):
            refusing(model)
    assert "Stochastic_MLE" in pg.__all__
