"""The state walks of Iterative_GP / Stochastic_MLE and Sparse_GP / VFE (tests/state_walk_models.py) on the CPU double `ModelsOracleOps`:
every number is the oracle's on both sides, the double's solves stop at the model's tol like the device's, and the bounds are the GPU
tier's.  Whatever differs is a bug of the host layer: a memo that outlives its data, a kept solve scaled twice, a buffer of the shared
scratch pool overwritten under a fitted state, a snapshot that follows its model, an update() that refits when it need not or does
not when it must.  Also checked here: the shadow alone factors and converges at every state a walk visits (its own assertions)."""
import pytest

import state_walk_models as sm
from state_walk_models import model_ops  # noqa: F401  (the fixture)


@pytest.fixture
def env(model_ops, monkeypatch):  # noqa: F811
    return sm.make_env(model_ops, monkeypatch)


def test_grad_x_memo_at_a_reused_address(env):
    reused, _ = sm.seq_grad_x_at_a_reused_address(env)
    assert reused >= 1


def test_loss_memo_with_x_replaced_twice(env):
    sm.seq_loss_at_a_reused_address(env)


@pytest.mark.parametrize("which", ["x", "z"])
def test_vfe_memo_with_data_replaced_twice(env, which):
    sm.seq_vfe_at_a_reused_address(env, which)


@pytest.mark.parametrize("kind", ["se+wn", "(se*per)+wn"])
def test_kept_solve_in_every_order(env, kind):
    sm.seq_kept_solve(env, kind)


def test_a_loss_evaluation_leaves_the_iterative_fit(env):
    sm.seq_evaluation_leaves_the_iterative_fit(env)


@pytest.mark.parametrize("whitened", [False, True], ids=["unwhitened", "whitened"])
def test_a_loss_evaluation_leaves_the_sparse_fit(env, whitened):
    sm.seq_evaluation_leaves_the_sparse_fit(env, whitened)


def test_update_refits_once_and_only_when_dirty(env):
    sm.seq_update_refits_once(env)


def test_snapshots(env):
    sm.seq_snapshots(env)


def test_not_converged_leaves_model_and_loss_usable(env):
    sm.seq_failure_leaves_the_iterative_model_usable(env)


@pytest.mark.parametrize("whitened", [False, True], ids=["unwhitened", "whitened"])
def test_failed_factorisation_leaves_the_sparse_model_usable(env, whitened):
    sm.seq_failure_leaves_the_sparse_model_usable(env, whitened)


@pytest.mark.parametrize("whitened", [False, True], ids=["unwhitened", "whitened"])
def test_write_back_then_predict(env, whitened):
    sm.seq_write_back(env, whitened)


@pytest.mark.parametrize("kind", sorted(sm.KINDS))
def test_negative_hyper_parameters_iterative(env, kind):
    sm.seq_signs(env, kind, "iterative")


@pytest.mark.parametrize("whitened", [False, True], ids=["unwhitened", "whitened"])
@pytest.mark.parametrize("kind", sorted(sm.KINDS))
def test_negative_hyper_parameters_sparse(env, kind, whitened):
    sm.seq_signs(env, kind, "sparse", whitened)


def test_walks_cover_every_operation():
    cov = sm.coverage()
    for fam, kinds in (("iterative", sm.ITER_KINDS), ("sparse", sm.SPARSE_KINDS)):
        seen, changes = cov[fam]
        assert sorted(k for k in kinds if not seen[k]) == [], "operation kinds no committed %s walk performs" % fam
        assert min(changes) >= 10, (fam, changes)


@pytest.mark.parametrize("walk", sm.ITER_WALKS, ids=lambda w: "seed%d" % w[0])
def test_random_walk_iterative(env, walk):
    sm.run_iter_walk(env, *walk)


@pytest.mark.parametrize("walk", sm.SPARSE_WALKS, ids=lambda w: "seed%d" % w[0])
def test_random_walk_sparse(env, walk):
    sm.run_sparse_walk(env, *walk)
