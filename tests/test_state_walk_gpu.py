"""The state walk (tests/state_walk.py) through the library on the MI355X: the same scripted sequences and random walks as the CPU tier,
every observation against the from-scratch fp64 shadow at the append tests' bounds (TOL64 = 1e-9, TOL32 = 1e-3, ten times that for
derivatives).  Every figure is printed before it is asserted (pytest -s), and each test ends with the table of its largest errors."""
import pytest

import state_walk as sw

pytestmark = pytest.mark.gpu


@pytest.fixture
def env(monkeypatch):
    from pygpr_amd._ops import get_ops

    return sw.Env(get_ops(), monkeypatch, sw.TOL64, sw.TOL32)


def test_eager_inverse_switched_on_after_a_lazy_inverse(env):
    sw.seq_eager_after_lazy_single(env)


def test_eager_inverse_switched_on_after_a_lazy_inverse_batched(env):
    sw.seq_eager_after_lazy_batched(env)


@pytest.mark.parametrize("kind", sorted(sw.KINDS))
def test_appends(env, kind):
    sw.seq_appends(env, kind)


@pytest.mark.parametrize("kind", sorted(sw.KINDS))
def test_append_growth(env, kind):
    sw.seq_append_growth(env, kind)


def test_appends_fp32(env):
    sw.seq_appends(env, "se+wn", sw.F32)
    sw.seq_append_growth(env, "se+wn", sw.F32)


@pytest.mark.parametrize("experts", [1, 3])
def test_chunk_edges(env, experts):
    sw.seq_chunks(env, experts)


def test_lazy_batched_experts(env):
    sw.seq_lazy_batched(env)


def test_experts_one_by_one(env):
    sw.seq_one_by_one(env)


def test_launch_groups(env):
    sw.seq_group_budget(env)


def test_five_children_take_the_serial_paths(env):
    sw.seq_five_children(env)


def test_rows_and_data(env):
    sw.seq_rows_and_data(env)


def test_memo_orders_and_factor_reuse(env):
    sw.seq_memo(env)


def test_replaced_data_at_a_reused_address(env):
    sw.seq_address_reuse(env)


def test_walks_cover_every_operation():
    seen, changes = sw.coverage()
    assert sorted(k for k in sw.ALL_KINDS if not seen[k]) == [], "operation kinds no committed walk performs"
    assert min(changes) >= 10, changes


@pytest.mark.parametrize("walk", sw.WALKS, ids=lambda w: "seed%d" % w[0])
def test_random_walk(env, walk):
    sw.run_walk(env, *walk)
