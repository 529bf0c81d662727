"""The padded restatement of pg_chol_append (tests/append_ref.py) against numpy.linalg on the concatenated problem: no GPU needed."""
import numpy as np
import pytest

import torch

import pygpr_amd as pg

import append_ref as ar


def _problem(n, k, seed=3, d=3, noise=0.05):
    rng = np.random.default_rng(seed)
    X = rng.random((n + k, d))
    y = np.sin(3 * X).sum(1) + 0.1 * rng.standard_normal(n + k)
    K = ar.se_kernel(X, X) + (noise ** 2 + ar.JITTER) * np.eye(n + k)
    return X, y, K


def _check(state, K, y, n_tot):
    L, invd, M, u, alpha = state
    n_pad = L.shape[0]
    Lr = np.linalg.cholesky(K)
    Mr = np.linalg.inv(Lr)
    np.testing.assert_allclose(np.tril(L[:n_tot, :n_tot]), Lr, rtol=0, atol=1e-10 * np.abs(Lr).max())
    np.testing.assert_allclose(np.tril(M[:n_tot, :n_tot]), Mr, rtol=0, atol=1e-9 * np.abs(Mr).max())
    ar_ = np.linalg.solve(K, y)
    np.testing.assert_allclose(alpha[:n_tot], ar_, rtol=0, atol=1e-8 * np.abs(ar_).max())
    np.testing.assert_allclose(u[:n_tot], Mr @ y, rtol=0, atol=1e-9 * np.abs(Mr @ y).max())
    assert not alpha[n_tot:].any() and not u[n_tot:].any()
    # the pad: identity rows / columns from n_tot on (lower triangle), exactly
    assert np.array_equal(np.tril(L)[n_tot:, :], np.eye(n_pad)[n_tot:, :])
    assert np.array_equal(np.tril(M)[n_tot:, :], np.eye(n_pad)[n_tot:, :])
    # inv_diag: the diagonal 128-blocks of L^-1 (upper parts zero)
    for b in range(n_pad // 128):
        blk = np.tril(M[b * 128:(b + 1) * 128, b * 128:(b + 1) * 128])
        np.testing.assert_allclose(invd[b], blk, rtol=0, atol=1e-12 * max(1.0, np.abs(blk).max()))
        Lb = np.tril(L[b * 128:(b + 1) * 128, b * 128:(b + 1) * 128])
        np.testing.assert_allclose(invd[b] @ Lb, np.eye(128), atol=1e-8)


@pytest.mark.parametrize("n,k", [(300, 1), (300, 7), (120, 20), (200, 128), (250, 7)])
def test_append_matches_concatenated_fit(n, k):
    """k = 1, 7, rows 120..139 straddling a 128-block, k = 128, and 250 + 7 crossing n_pad = 256 (growth to 512)."""
    X, y, K = _problem(n, k)
    n_pad = ((n + 255) // 256) * 256
    state = ar.padded_fit(K[:n, :n], y[:n], n_pad)
    n_pad2 = ((n + k + 255) // 256) * 256
    if n_pad2 > n_pad:
        state = ar.grow(*state, n_pad2)
    Kt = np.zeros((k, n_pad2))
    Kt[:, :n] = K[n:, :n]
    out = ar.append(*state, n, Kt, K[n:, n:], y[n:])
    assert out[5] == 0
    _check(out[:5], K, y, n + k)


def test_append_chunks_and_garbage_upper_part():
    """Two appends in a row equal one fit; NaN in the scratch above the diagonal blocks is never read."""
    n, k1, k2 = 260, 40, 90
    X, y, K = _problem(n, k1 + k2, seed=5)
    state = ar.padded_fit(K[:n, :n], y[:n], 512, garbage=np.nan)
    for n0, kc in ((n, k1), (n + k1, k2)):
        Kt = np.zeros((kc, 512))
        Kt[:, :n0] = K[n0:n0 + kc, :n0]
        out = ar.append(*state, n0, Kt, K[n0:n0 + kc, n0:n0 + kc], y[n0:n0 + kc])
        assert out[5] == 0
        state = out[:5]
    _check(state, K, y, n + k1 + k2)


def test_append_bad_pivot_leaves_state():
    n, k = 200, 5
    X, y, K = _problem(n, k)
    state = ar.padded_fit(K[:n, :n], y[:n], 256)
    Kt = np.zeros((k, 256))
    Kt[:, :n] = K[n:, :n]
    Kt[2, 17] = np.nan
    out = ar.append(*state, n, Kt, K[n:, n:], y[n:])
    assert out[5] == n + 3
    for a, b in zip(out[:5], state):
        assert np.array_equal(a, b, equal_nan=True)
    # a duplicated point without noise: the Schur complement is singular
    Kd = ar.se_kernel(X[:n], X[:n]) + ar.JITTER * np.eye(n)
    state = ar.padded_fit(Kd, y[:n], 256)
    Kt = np.zeros((1, 256))
    Kt[0, :n] = Kd[0, :n] - ar.JITTER * (np.arange(n) == 0)
    out = ar.append(*state, n, Kt, np.array([[Kd[0, 0] - 2 * ar.JITTER]]), y[:1])
    assert out[5] == n + 1


def test_batched_models_and_committee_refuse_append():
    """Raised before any device work: the model is unchanged."""
    rng = np.random.default_rng(0)
    cov = pg.Compose([pg.Squared_exponential(), pg.White_noise()])
    x = torch.from_numpy(rng.random((2, 50, 3)))
    y = torch.from_numpy(rng.random((2, 50)))
    gp = pg.Exact_GP(x, y, cov)
    with pytest.raises(NotImplementedError):
        gp.append(x[0, :5], y[0, :5])
    assert gp.x is x and gp.y is y
    gr = pg.GRBCM(x, y, torch.from_numpy(rng.random((20, 3))), torch.from_numpy(rng.random(20)), cov)
    with pytest.raises(NotImplementedError):
        gr.append(x[0, :5], y[0, :5])
