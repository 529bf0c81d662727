"""The committee's state walk (tests/state_walk_grbcm.py) through the library on the MI355X: the same scripted sequences and random walks
as the CPU tier, every observation against the from-scratch fp64 shadow (TOL64 = 1e-9, TOL32 = 1e-3; the full covariance at the golden
test's rtol 1e-6 / atol 1e-10) and the aggregation alone against its long-double restatement on the library's own per-expert outputs.
Every figure is printed before it is asserted (pytest -s), and each test ends with the table of its largest errors."""
import pytest

import state_walk as sw
import state_walk_grbcm as sg

pytestmark = pytest.mark.gpu


@pytest.fixture
def env(monkeypatch):
    from pygpr_amd._ops import get_ops

    return sg.make_env(get_ops(), monkeypatch, sw.TOL64, sw.TOL32)


def test_which_expert_refits(env):
    sg.seq_which_expert_refits(env)


def test_terms_paths(env):
    sg.seq_terms_paths(env)


def test_full_covariance_paths(env):
    sg.seq_full_paths(env)


def test_test_point_shapes(env):
    sg.seq_test_point_shapes(env)


def test_fp32_committee(env):
    sg.seq_fp32(env)


def test_product_kind(env):
    sg.seq_other_kind(env)


def test_memo_of_the_shared_objective(env):
    sg.seq_memo(env)


def test_replaced_data_at_a_reused_address(env):
    sg.seq_address_reuse(env)


def test_failed_fit_of_one_expert(env):
    sg.seq_failed_fit(env)


def test_tail_repeated_after_a_timeout(env):
    sg.seq_replay_after_a_timeout(env)


def test_walks_cover_every_operation():
    seen, changes, gates, dtypes = sg.coverage()
    assert sorted(k for k in sg.ALL_KINDS if not seen[k]) == [], "operation kinds no committed walk performs"
    assert min(changes) >= 10, changes
    assert gates >= {"_BATCH_MAX_N", "_CHUNK", "_AGG_BATCH_MAX"} and dtypes == {sw.F64, sw.F32}


@pytest.mark.parametrize("walk", sg.WALKS, ids=lambda w: "seed%d" % w[0])
def test_random_walk(env, walk):
    sg.run_walk(env, *walk)
