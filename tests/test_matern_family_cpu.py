"""CPU tier of the Matern family (Matern-1/2, -3/2 next to -5/2): the NumPy restatement of tests/kernel_ref.py against sklearn,
central differences and the oracle, and the Python side of the new kinds (layout, constants against the C header)."""
import os
import re

import numpy as np
import pytest

import pygpr_amd as pg
from pygpr_amd import _lib
from oracle import pygpr_oracle as orc

import kernel_ref as kr


def _data(n=23, m=9, d=3, seed=0):
    rng = np.random.default_rng(seed)
    x, xp = rng.random((n, d)), rng.random((m, d))
    x[5] = x[2]                                                 # an exact duplicate: r = 0 off the diagonal
    hp = np.concatenate([[1.3], 0.5 + rng.random(d)])
    return x, xp, hp


@pytest.mark.parametrize("part", ["m12", "m32"])
def test_restatement_matches_sklearn(part):
    from sklearn.gaussian_process.kernels import Matern

    x, xp, hp = _data()
    sk = Matern(length_scale=1.0 / hp[1:], nu=kr.NU[part])
    np.testing.assert_allclose(kr.stationary(part, hp, x), hp[0] ** 2 * sk(x), rtol=0, atol=1e-13)
    np.testing.assert_allclose(kr.stationary(part, hp, x, xp), hp[0] ** 2 * sk(xp, x), rtol=0, atol=1e-13)
    np.testing.assert_allclose(kr.kernel([part, "wn"], np.append(hp, 0.2), x, xp), hp[0] ** 2 * sk(xp, x), rtol=0, atol=1e-13)


@pytest.mark.parametrize("part", ["m12", "m32", "m52", "se"])
def test_restatement_gradient_matches_central_differences(part):
    x, _, hp = _data()
    parts = [part, "wn"]
    hp = np.append(hp, 0.3)
    k, dk = kr.kernel_and_grad(parts, hp, x)
    assert dk.shape == (hp.size,) + k.shape and np.isfinite(dk).all()
    h = 1e-6
    for p in range(hp.size):
        e = np.zeros(hp.size)
        e[p] = h
        fd = (kr.kernel(parts, hp + e, x) - kr.kernel(parts, hp - e, x)) / (2 * h)
        # Matern-1/2 has a kink at r = 0 only ALONG r; the duplicate pair (2, 5) has D = 0, so every dl_k moves nothing there
        np.testing.assert_allclose(dk[p], fd, rtol=1e-6, atol=1e-7)
    if part == "m12":
        assert not dk[1:-1, 2, 5].any() and not np.diag(dk[1]).any()


def test_matern52_branch_is_the_oracles():
    x, _, hp = _data(n=31, d=4)
    k, dk = kr.kernel_and_grad(["m52"], hp, x)
    ko, dko = orc.matern52_kernel_and_grad(hp, x)
    np.testing.assert_allclose(k, ko, rtol=1e-14, atol=1e-15)
    np.testing.assert_allclose(dk, dko, rtol=1e-13, atol=1e-15)


def test_restatement_nlml_gradient_matches_the_dense_stack():
    rng = np.random.default_rng(3)
    x, y = orc.synth(40, 3, seed=2)
    parts = ["m12", "m32", "wn"]
    hp = np.concatenate([[1.1], 0.5 + rng.random(3), [0.7], 0.5 + rng.random(3), [0.2]])
    loss, g = kr.nlml_and_grad(parts, hp, x, y)
    k, dk = kr.kernel_and_grad(parts, hp, x)
    k[np.diag_indices_from(k)] += kr.JITTER
    kinv = np.linalg.inv(k)
    a = kinv @ y
    np.testing.assert_allclose(g, -0.5 * (np.einsum("i,kij,j->k", a, dk, a) - np.einsum("ij,kji->k", kinv, dk)), rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(loss, kr.nlml(parts, hp, x, y), rtol=1e-14)
    h = 1e-6
    for p in range(hp.size):
        e = np.zeros(hp.size)
        e[p] = h
        np.testing.assert_allclose(g[p], (kr.nlml(parts, hp + e, x, y) - kr.nlml(parts, hp - e, x, y)) / (2 * h), rtol=1e-5, atol=1e-6)


def test_layout_of_the_new_kinds():
    from pygpr_amd.covar import layout

    cov = pg.Compose([pg.White_noise(), pg.Matern32(), pg.Compose([pg.Matern12(), pg.Squared_exponential()])])
    kinds, offs, noise, nhp = layout(cov, 3)
    assert kinds == [3, 4, 0] and offs == [1, 5, 9] and noise == [0] and nhp == 13
    assert "Matern32" in pg.__all__ and "Matern12" in pg.__all__
    assert pg.Matern12().get_params_shape(np.empty((7, 5))) == [6]


def test_kind_constants_match_the_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "pygpr_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+(PG_KIND_[A-Z0-9_]+)\s+(\d+)", text)}
    assert defs == {"PG_KIND_RBF": 0, "PG_KIND_MATERN52": 1, "PG_KIND_SQDIST": 2, "PG_KIND_MATERN32": 3, "PG_KIND_MATERN12": 4}
    for k, v in defs.items():
        assert getattr(_lib, k) == v
