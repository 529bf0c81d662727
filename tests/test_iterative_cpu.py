"""Iterative_GP on the host: the new header, the restatement (tests/iterative_ref.py) against dense linear algebra -- the Woodbury
preconditioner, block PCG and its stopping rule, what the preconditioner buys, degenerate columns -- and the refusals that need no
device.  No GPU."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import iterative_ref as ir
import matmul_ref as mr
import pygpr_amd as pg
import sparse_ref as sr
from pygpr_amd import _lib

SE_WN = ["se", "wn"]


# ------------------------------------------------------------------------------------------- the header
def test_matmul_header_parses_binds_and_is_exported():
    text = open(_lib.HEADER_MATMUL).read()
    protos = _lib.parse_prototypes(text)
    assert sorted(protos) == ["pg_kernel_matmul", "pg_kernel_matmul_worksize"]
    assert _lib._SIGS_MATMUL == _lib.signatures(protos)
    others = (set(_lib.header_symbols()) | set(_lib._SIGS_LOO) | set(_lib._SIGS_SAMPLE) | set(_lib._SIGS_SPARSE) | set(_lib._SIGS_SELECT))
    assert not set(protos) & others and "#define PG_KIND" not in text
    vp, i, lg, db = ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_double
    assert _lib._SIGS_MATMUL["pg_kernel_matmul_worksize"] == (lg, [i, i, i])
    assert _lib._SIGS_MATMUL["pg_kernel_matmul"] == (i, [vp, i, ctypes.POINTER(_lib.CovSpec), vp, vp, lg, i, vp, lg, i, i, vp, lg, i, db, vp, lg,
                                                         vp, vp])
    lib = _lib.load(check_symbols=True)
    for name, (res, args) in _lib._SIGS_MATMUL.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args
    # host arithmetic: no workspace while the row tiles fill the chip or the column range is short; otherwise segments of at least four
    # column tiles, one 64 x 32 partial tile per row tile, block of right-hand sides and segment
    assert lib.pg_kernel_matmul_worksize(65536, 65536, 16) == 0 and lib.pg_kernel_matmul_worksize(1, 300, 3) == 0
    assert lib.pg_kernel_matmul_worksize(5, 5000, 2) == 16 * 64 * 32                  # 79 column tiles: 16 segments of five
    assert lib.pg_kernel_matmul_worksize(8192, 32768, 1) == 4 * 128 * 64 * 32        # 128 row tiles: four segments fill 512 workgroups
    assert lib.pg_kernel_matmul_worksize(0, 0, 0) == 0
    assert lib.pg_kernel_matmul_worksize(-1, 0, 0) == -1 and lib.pg_kernel_matmul_worksize(5, -1, 1) == -1 and lib.pg_kernel_matmul_worksize(5, 5, -1) == -1
    assert lib.pg_kernel_matmul(None, 0, None, None, None, 1, 1, None, 1, 1, 1, None, 1, 1, 0.0, None, 1, None, None) != 0      # null handle: refused
    assert b"pg_kernel_matmul" in lib.pg_last_error()
    assert "HEADER_MATMUL" in inspect.getsource(_lib.build_id) and "_SIGS_MATMUL" in inspect.getsource(_lib.load)


# ------------------------------------------------------------------------------------------- the restatement
@pytest.fixture(scope="module")
def se_problem():
    hp, x, y, _ = sr.problem(SE_WN, n=700, m=40)
    a = ir.operator(SE_WN, hp, x)
    return hp, x, y, a, float(np.linalg.cond(a))


def test_the_operator_is_the_matrix_exact_gp_factors(se_problem):
    import kernel_ref as kr

    hp, x, y, a, cond = se_problem
    k = kr.kernel(SE_WN, hp, x)
    k[np.diag_indices_from(k)] += kr.JITTER
    assert np.max(np.abs(a - k)) <= 4 * 2.0 ** -52 * np.max(np.abs(k))
    print("cond(A) = %.2e" % cond)
    assert 1e2 < cond < 1e5                     # the problem of the iteration counts below


@pytest.mark.parametrize("rank", [1, 20, 100])
def test_woodbury_is_the_dense_inverse(se_problem, rank):
    hp, x, y, a, _ = se_problem
    l, piv = ir.factor_l(SE_WN, hp, x, rank)
    assert l.shape == (700, rank) and len(set(piv.tolist())) == rank
    pre = ir.Woodbury(l, mr.shift_of(SE_WN, hp, 3, ir.JITTER))
    r = np.random.default_rng(0).standard_normal((700, 5))
    dense = np.linalg.solve(pre.dense(), r)
    err = np.max(np.abs(pre.solve(r) - dense)) / np.max(np.abs(dense))
    bound = 50 * np.linalg.cond(pre.dense()) * 2.0 ** -53
    print("rank %3d  P^-1 against the dense inverse: %.2e (bound %.2e)" % (rank, err, bound))
    assert err <= bound
    # the factor is the pivoted Cholesky factor: L L^T reproduces k at the pivots' rows (up to the jitter in Lu)
    k = mr.stationary_kernel(SE_WN, hp, x, x)
    assert np.max(np.abs((l @ l.T)[piv] - k[piv])) <= 10 * ir.JITTER


@pytest.mark.parametrize("rank", [0, 40])
def test_pcg_against_the_dense_solve(se_problem, rank):
    """The error is within cond(A) x the reported (true) residual: ||x - x*|| / ||x*|| <= cond ||b - A x|| / ||b||."""
    hp, x, y, a, cond = se_problem
    l, _ = ir.factor_l(SE_WN, hp, x, rank)
    pre = ir.Woodbury(l, mr.shift_of(SE_WN, hp, 3, ir.JITTER))
    b = np.stack([y, np.random.default_rng(1).standard_normal(700)], 1)
    sol, it, res, ok = ir.pcg(a, b, pre, 1e-10, 1000)
    want = np.linalg.solve(a, b)
    assert ok and res <= 2e-10 and it % ir.CHECK_EVERY == 0
    for c in range(2):
        err = np.linalg.norm(sol[:, c] - want[:, c]) / np.linalg.norm(want[:, c])
        print("rank %2d column %d: %d iterations, residual %.2e, error %.2e (bound %.2e)" % (rank, c, it, res, err, cond * res))
        assert err <= cond * res
    one, it1, _, _ = ir.pcg(a, y, pre, 1e-10, 1000)          # a vector is one column
    assert one.shape == (700,) and np.allclose(one, want[:, 0], rtol=0, atol=cond * 2e-10 * np.abs(want[:, 0]).max())


def test_iterations_fall_strictly_with_the_rank(se_problem):
    hp, x, y, a, _ = se_problem
    counts = []
    for rank in (0, 20, 40):
        l, _ = ir.factor_l(SE_WN, hp, x, rank)
        _, it, res, ok = ir.pcg(a, y, ir.Woodbury(l, mr.shift_of(SE_WN, hp, 3, ir.JITTER)), 1e-10, 1000, check_every=1)
        assert ok
        counts.append(it)
    print("iterations to 1e-10 at rank 0 / 20 / 40:", counts)
    assert counts[0] > counts[1] > counts[2]


def test_max_iter_ends_the_solve_unconverged(se_problem):
    hp, x, y, a, _ = se_problem
    _, it, res, ok = ir.pcg(a, y, ir.Woodbury(np.zeros((700, 0)), 1.0), 1e-10, 2)
    assert it == 2 and not ok and res > 1e-10


def test_zero_and_duplicate_columns_give_no_nan(se_problem):
    hp, x, y, a, _ = se_problem
    l, _ = ir.factor_l(SE_WN, hp, x, 20)
    pre = ir.Woodbury(l, mr.shift_of(SE_WN, hp, 3, ir.JITTER))
    b = np.stack([y, np.zeros(700), y], 1)
    sol, it, res, ok = ir.pcg(a, b, pre, 1e-10, 1000)
    assert ok and np.isfinite(sol).all()
    assert not sol[:, 1].any() and np.array_equal(sol[:, 0], sol[:, 2])
    # ... and many more iterations than any column needs: converged columns keep taking zero or harmless steps
    sol2, _, _, _ = ir.pcg(a, b, pre, 1e-300, 300)
    assert np.isfinite(sol2).all() and not sol2[:, 1].any()


# ------------------------------------------------------------------------------------------- the model's host logic
def _cov():
    return pg.Compose([pg.Squared_exponential(), pg.White_noise()])


def test_refusals_that_need_no_device():
    x, y = torch.rand(20, 3, dtype=torch.float64), torch.rand(20, dtype=torch.float64)
    with pytest.raises(TypeError):
        pg.Iterative_GP(x.float(), y.float(), _cov())
    with pytest.raises(NotImplementedError):
        pg.Iterative_GP(x.reshape(2, 10, 3), y.reshape(2, 10), _cov())
    with pytest.raises(NotImplementedError):      # five stationary children: two pg_covspec passes
        pg.Iterative_GP(x, y, pg.Compose([pg.Squared_exponential() for _ in range(5)] + [pg.White_noise()]))
    with pytest.raises(ValueError):
        pg.Iterative_GP(x, y, _cov(), rank=-1)
    model = pg.Iterative_GP(x, y, _cov(), rank=5, tol=1e-9, max_iter=50)
    assert isinstance(model, pg.GPR) and model.need_upd and (model.rank, model.tol, model.max_iter) == (5, 1e-9, 50)
    for loss in (pg.MLE, pg.LOO):
        with pytest.raises(NotImplementedError, match="VFE"):
            loss(model)
    with pytest.raises(NotImplementedError):
        model.append(x[:2], y[:2])
    with pytest.raises(NotImplementedError):
        model.loo_predict()
    with pytest.raises(NotImplementedError):
        model.sampler(x[:2])
    with pytest.raises(NotImplementedError):      # autograd through predict
        model.predict(x[:2].clone().requires_grad_(True), "diag")
    pg.Iterative_GP(x, y, pg.Squared_exponential())      # a covariance without White_noise is legal: the shift is JITTER
    assert issubclass(pg.NotConverged, torch.linalg.LinAlgError)
    err = pg.NotConverged(7, 0.5, 1e-8)
    assert (err.iterations, err.residual) == (7, 0.5)
