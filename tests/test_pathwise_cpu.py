"""Pathwise function samples without a GPU: the spectral laws of the restatement (tests/pathwise_ref.py) against the kernels they
claim to realise, the closed-form covariance of the sampler, the refusals, and the new header's binding.

Bounds (derived; every test prints what it measured):
  kernel approximation   Kt_ij = sum_c (sigma_c^2 / F) sum_j cos(omega_j . tau) is a mean of F terms bounded by sigma_c^2 per
                         component: its standard deviation is at most sigma_c^2 / sqrt(F), and 6 of them cover the 900 entries of a
                         30 x 30 matrix.  The bound is 6 sum_c sigma_c^2 / sqrt(F).
  closed form            with Kt = K the sampler's covariance is the exact posterior's: 1e-10, two dense solves at n = 300 apart."""
import ctypes

import numpy as np
import pytest

import kernel_ref as kr
import matmul_ref as mr
import pathwise_ref as pr
import sparse_ref as sr

F = 200000
D = 3
LENGTHS = [0.5, 0.9, 1.4]
SIGMA = {"se": 1.1, "m12": 0.9, "m32": 1.2, "m52": 0.8}


def model_hp(terms):
    return np.concatenate([[SIGMA[p]] + LENGTHS for p in terms])


def points():
    return 4.0 * np.random.default_rng(12).random((30, D)) - 2.0


def worst(feature_terms, kernel_terms):
    """(largest |Kt - K| over the 30 x 30 entries, the bound) for features of one model against the kernel of another."""
    x = points()
    hp = model_hp(feature_terms)
    nu, u, amp = pr.spectral_features(feature_terms, hp, D, F, seed=7)
    assert nu.shape == (2 * F * len(feature_terms), D) and set(np.unique(u)) == {-0.25, 0.0}
    kt = pr.feature_kernel(x, x, nu, u, amp)
    k = mr.stationary_kernel(kernel_terms, model_hp(kernel_terms), x, x)
    bound = 6.0 * sum(SIGMA[p] ** 2 for p in kernel_terms) / np.sqrt(F)
    return float(np.max(np.abs(kt - k))), bound


@pytest.mark.parametrize("terms", [["se"], ["m12"], ["m32"], ["m52"], ["se", "m52"]], ids="+".join)
def test_the_features_realise_their_kernel(terms):
    err, bound = worst(terms, terms)
    print("%-8s max |Phi Phi^T - K| = %.4f  (bound %.4f, F = %d)" % ("+".join(terms), err, bound, F))
    assert err <= bound


def test_the_bound_separates_matern32_from_matern52():
    """The same length scales and sigma: only the degrees of freedom differ."""
    x = points()
    hp = model_hp(["m52"])
    nu, u, amp = pr.spectral_features(["m32"], hp, D, F, seed=7)
    err = float(np.max(np.abs(pr.feature_kernel(x, x, nu, u, amp) - mr.stationary_kernel(["m52"], hp, x, x))))
    bound = 6.0 * SIGMA["m52"] ** 2 / np.sqrt(F)
    print("m32 features against the m52 kernel: %.4f  (bound %.4f)" % (err, bound))
    assert err > bound


@pytest.mark.parametrize("terms", [["se", "wn"], ["m32", "m52", "wn"]], ids="+".join)
def test_the_closed_form_covariance_is_the_posterior_when_the_features_are_exact(terms):
    hp, x, y, _ = sr.problem(terms, n=300, m=40)
    xp = np.random.default_rng(9).random((40, x.shape[1]))
    got = pr.sampler_cov(terms, hp, x, xp, lambda a, b: mr.stationary_kernel(terms, hp, a, b))
    _, ref = kr.predict(terms, hp, x, y, xp, var="full")
    latent = ref - float(mr.shift_of(terms, hp, x.shape[1])) * np.eye(xp.shape[0])      # predict keeps sigma_n^2 on the diagonal of K**
    err = float(np.max(np.abs(got - latent)))
    print("%-12s closed form with Kt = K against predict's covariance: %.2e  (bound 1e-10)" % ("+".join(terms), err))
    assert err <= 1e-10
    assert np.all(np.diag(got) > 0)


def test_the_pairs_share_a_frequency_and_sample_s_is_its_own():
    hp = model_hp(["m52", "se"])
    nu, u, amp = pr.spectral_features(["m52", "se"], hp, D, 8, seed=3)
    assert np.array_equal(nu[0::2], nu[1::2]) and np.all(u[0::2] == 0) and np.all(u[1::2] == -0.25)
    assert np.allclose(amp[:16], SIGMA["m52"] / np.sqrt(8)) and np.allclose(amp[16:], SIGMA["se"] / np.sqrt(8))
    assert np.array_equal(pr.weights(3, 32, 5, amp)[:, :2], pr.weights(3, 32, 2, amp))
    assert np.array_equal(pr.noise_draws(3, 10, 5)[:, :1], pr.noise_draws(3, 10, 1))
    assert not np.array_equal(pr.spectral_features(["m52", "se"], hp, D, 8, seed=4)[0], nu)


def test_refusals():
    import pygpr_amd as pg

    se = pg.Squared_exponential()
    hp = np.array([1.0] + LENGTHS)
    for cov, nhp, name in ((pg.Rational_quadratic(), D + 2, "Rational_quadratic"), (pg.Periodic(), 2 * D + 1, "Periodic"),
                           (pg.Product([pg.Squared_exponential(), pg.Matern32()]), 2 * D + 2, "Product")):
        with pytest.raises(NotImplementedError, match=name):
            pg.spectral_features(cov, np.ones(nhp), D, 16, 0)
    with pytest.raises(NotImplementedError):      # five components: two passes
        pg.spectral_features(pg.Compose([pg.Squared_exponential() for _ in range(5)]), np.ones(5 * (D + 1)), D, 16, 0)
    for bad in (0, -3, 1.5):
        with pytest.raises(ValueError):
            pg.spectral_features(se, hp, D, bad, 0)
    with pytest.raises(TypeError):
        pg.spectral_features(se, hp.astype(np.float32), D, 16, 0)
    with pytest.raises(NotImplementedError):      # batched hyper-parameters
        pg.spectral_features(se, np.stack([hp, hp]), D, 16, 0)


def test_the_feature_header_is_bound_and_the_library_answers_without_a_device():
    from pygpr_amd import _lib

    protos = _lib.parse_prototypes(open(_lib.HEADER_FEATURE).read())
    assert sorted(protos) == ["pg_feature_matmul", "pg_feature_matmul_worksize"]
    i, lg, vp = ctypes.c_int, ctypes.c_long, ctypes.c_void_p
    assert _lib._SIGS_FEATURE["pg_feature_matmul_worksize"] == (lg, [i, i, i])
    assert _lib._SIGS_FEATURE["pg_feature_matmul"] == (i, [vp, i, vp, lg, i, vp, lg, i, i, vp, vp, lg, i, vp, lg, vp, vp])
    lib = _lib.load(check_symbols=True)
    # the plan is pg_kernel_matmul's, the feature in the place of the column point
    for shape in ((65536, 4096, 16), (1, 300, 3), (5, 5000, 2), (8192, 32768, 1), (0, 0, 0), (70, 150, 33)):
        assert lib.pg_feature_matmul_worksize(*shape) == lib.pg_kernel_matmul_worksize(*shape)
    assert lib.pg_feature_matmul_worksize(5, 5000, 2) == 16 * 64 * 32
    assert lib.pg_feature_matmul_worksize(-1, 0, 0) == -1 and lib.pg_feature_matmul_worksize(5, -1, 1) == -1 and lib.pg_feature_matmul_worksize(5, 5, -1) == -1
    assert lib.pg_feature_matmul(None, 0, None, 1, 1, None, 1, 1, 1, None, None, 1, 1, None, 1, None, None) != 0      # null handle: refused
    assert b"pg_feature_matmul" in lib.pg_last_error()
