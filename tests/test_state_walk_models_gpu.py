"""The state walks of Iterative_GP / Stochastic_MLE and Sparse_GP / VFE (tests/state_walk_models.py) through the library on the MI355X:
the scripted sequences and one random walk per family, every observation against the from-scratch fp64 shadow at the bounds of the
fresh-model tests (the helper's docstring lists them; DESIGN 4.15a records what was measured).  The walk of each family, sequence 1 and
one Exact_GP walk of tests/state_walk.py run a second time with x, y (and z) created ON THE DEVICE: HipOps.to_device then returns the
caller's tensor itself, so every `_dev` and every `_state["x"]` is an alias of user memory.  Every figure is printed before it is
asserted (pytest -s), and each test ends with the table of its largest errors."""
import pytest

import state_walk as sw
import state_walk_models as sm

pytestmark = pytest.mark.gpu

PLACES = ["host", "device"]


def _env(monkeypatch, place="host"):
    from pygpr_amd._ops import get_ops

    return sm.make_env(get_ops(), monkeypatch, device="cuda" if place == "device" else None)


@pytest.fixture
def env(monkeypatch):
    return _env(monkeypatch)


@pytest.mark.parametrize("place", PLACES)
def test_grad_x_memo_at_a_reused_address(monkeypatch, place):
    reused, _ = sm.seq_grad_x_at_a_reused_address(_env(monkeypatch, place))
    assert reused >= 1


@pytest.mark.parametrize("place", PLACES)
def test_loss_memo_with_x_replaced_twice(monkeypatch, place):
    sm.seq_loss_at_a_reused_address(_env(monkeypatch, place))


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("which", ["x", "z"])
def test_vfe_memo_with_data_replaced_twice(monkeypatch, which, place):
    sm.seq_vfe_at_a_reused_address(_env(monkeypatch, place), which)


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


@pytest.mark.parametrize("place", PLACES)
def test_random_walk_iterative(monkeypatch, place):
    sm.run_iter_walk(_env(monkeypatch, place), *sm.ITER_WALKS[0])


@pytest.mark.parametrize("place", PLACES)
def test_random_walk_sparse(monkeypatch, place):
    sm.run_sparse_walk(_env(monkeypatch, place), *sm.SPARSE_WALKS[1 if place == "device" else 0])


def test_exact_gp_random_walk_with_device_resident_data(monkeypatch):
    from pygpr_amd._ops import get_ops

    sw.run_walk(sw.Env(get_ops(), monkeypatch, sw.TOL64, sw.TOL32, device="cuda"), *sw.WALKS[0])
