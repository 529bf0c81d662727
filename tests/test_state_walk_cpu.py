"""The state walk (tests/state_walk.py) on the CPU double: every number is the oracle's on both sides, so the walker and its shadow must
agree to rounding (1e-11; fp32 models store the oracle's numbers in fp32 and are held to the GPU tier's TOL32), and whatever differs is a
bug of the host layer: a wrong expert, a wrong chunk, a stale or missing buffer.  Both sides take their covariances from
tests/kernel_ref.py here, so the append sequences run on two of the three kinds (a sum and the product); the GPU tier runs all three."""
import pytest

import state_walk as sw
from state_walk import walk_ops  # noqa: F401  (the fixture)


@pytest.fixture
def env(walk_ops, monkeypatch):  # noqa: F811
    return sw.Env(walk_ops, monkeypatch, sw.TOL_DOUBLE, sw.TOL32, deriv=1)


def test_eager_inverse_switched_on_after_a_lazy_inverse(env):
    sw.seq_eager_after_lazy_single(env)


def test_eager_inverse_switched_on_after_a_lazy_inverse_batched(env):
    sw.seq_eager_after_lazy_batched(env)


@pytest.mark.parametrize("kind", ["se+wn", "(se*per)+wn"])
def test_appends(env, kind):
    sw.seq_appends(env, kind)


@pytest.mark.parametrize("kind", ["m52+wn", "(se*per)+wn"])
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
