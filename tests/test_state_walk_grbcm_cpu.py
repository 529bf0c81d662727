"""The committee's state walk (tests/state_walk_grbcm.py) on the CPU double: every number is the oracle's on both sides, so the committee
and its shadow must agree to rounding (1e-11; an fp32 committee stores the oracle's numbers in fp32 and is held to the GPU tier's TOL32),
and whatever differs is a bug of the host layer: a stale expert, a wrong row, a wrong weight, a buffer re-used too early.  Here too: the
restatement of the aggregation is pinned to the oracle package, and the reference alone is held to the full-covariance bound at every
committed m."""
import numpy as np
import pytest

import state_walk as sw
import state_walk_grbcm as sg
from oracle import pygpr_oracle as orc
from state_walk import walk_ops  # noqa: F401  (the fixture)


@pytest.fixture
def env(walk_ops, monkeypatch):  # noqa: F811
    """The thread pools held to one thread while the test runs, as tests/state_walk_models.py does: the double issues thousands of
    factorisations and copies of 256 x 256 matrices, which threaded pools side by side serve twenty times slower (measured: 34 s against
    1.7 s per sequence)."""
    env = sg.make_env(walk_ops, monkeypatch, sw.TOL_DOUBLE, sw.TOL32, deriv=1)
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:                 # (slower, not wrong)
        yield env
        return
    with threadpool_limits(limits=1):
        yield env


def test_restated_aggregation_is_the_oracles():
    """aggregate / aggregate_full (np.longdouble) against oracle.pygpr_oracle.grbcm_aggregate / grbcm_aggregate_full at 1e-12, and the
    plain fp64 form of the same code against its long-double form."""
    rng = np.random.default_rng(7)
    for nc, m in ((1, 5), (3, 37), (5, 64)):
        mg, ml = rng.standard_normal(m), rng.standard_normal((nc, m))
        a = rng.standard_normal((nc + 1, m, 2 * m))
        covs = a @ a.transpose(0, 2, 1) / (2 * m) + 0.3 * np.eye(m)
        vg, vl = np.diagonal(covs[0]).copy(), np.diagonal(covs[1:], axis1=1, axis2=2).copy()
        for mine, theirs in ((sg.aggregate(mg, vg, ml, vl), orc.grbcm_aggregate(mg, vg, ml, vl)),
                             (sg.aggregate_full(mg, covs[0], ml, covs[1:])[:2], orc.grbcm_aggregate_full(mg, covs[0], ml, covs[1:]))):
            for got, ref in zip(mine, theirs):
                np.testing.assert_allclose(np.asarray(got, dtype=np.float64), ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max())
        for got, ref in zip(sg.aggregate_full(mg, covs[0], ml, covs[1:], dtype=np.float64), sg.aggregate_full(mg, covs[0], ml, covs[1:])):
            assert got.dtype == np.float64 and ref.dtype == np.longdouble
            np.testing.assert_allclose(got, np.asarray(ref, dtype=np.float64), rtol=1e-11, atol=1e-12 * float(np.abs(ref).max()))


def test_reference_alone_holds_the_full_covariance_bound():
    """At sigma_n = 0.3 every m x m predictive covariance has cond <= about m 1.3 / 0.09: the shadow's own fp64 arithmetic against its
    long-double aggregation stays inside layer (a)'s rtol 1e-6 / atol 1e-10 at every committed m, 513 included."""
    rng = np.random.default_rng(8)
    terms = sw.SE_WN
    xg = rng.random((sg.NG, sw.D))
    xl = np.concatenate([np.broadcast_to(xg, (3, sg.NG, sw.D)), rng.random((3, 60, sw.D))], axis=1)
    y = lambda x: np.sin(3.0 * x).sum(-1) + 0.1 * rng.standard_normal(x.shape[:-1])      # noqa: E731
    yg, yl = y(xg), y(xl)
    hp = [sw.hp_for(terms, rng) for _ in range(4)]
    fits = [sw.Fit(terms, hp[0], xg, yg)] + [sw.Fit(terms, hp[c + 1], xl[c], yl[c]) for c in range(3)]
    for m in sorted(set(sg.M_FULL) | set(sg.WALK_M)):
        xs = rng.random((m, sw.D))
        pred = [f.predict(xs) for f in fits]
        args = (pred[0][0], pred[0][2], np.stack([p[0] for p in pred[1:]]), np.stack([p[2] for p in pred[1:]]))
        mu64, cov64 = sg.aggregate_full(*args, dtype=np.float64)[:2]
        mu80, cov80 = sg.f64(*sg.aggregate_full(*args)[:2])
        cond = np.linalg.cond(args[1])
        print("m = %3d: cond(C_global) %.1e, |cov64 - cov80| %.2e, |mu64 - mu80| %.2e" % (m, cond, np.abs(cov64 - cov80).max(), np.abs(mu64 - mu80).max()))
        assert cond <= m * 1.3 / 0.09 * 1.5
        np.testing.assert_allclose(cov64, cov80, rtol=1e-6, atol=1e-10)
        np.testing.assert_allclose(mu64, mu80, rtol=1e-6, atol=1e-9)


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
