"""Joint draws without a GPU: the generator's definition (tests/philox_ref.py) against the published known answers of Philox4x32-10 and
against itself, the third public header and its binding, the framed-coverage rule for that header, and the host logic of
Exact_GP.sampler / PosteriorSampler on a NumPy test double whose `randn` is that restatement."""
import ast
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import philox_ref as pr
import pygpr_amd as pg
from oracle_ops import OracleOps, _np
from pygpr_amd import _lib, _ops
from pygpr_amd import gpr as gpr_mod


# ------------------------------------------------------------------------------------------- the generator's definition
@pytest.mark.parametrize("counter,key,out", [
    ([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, out):
    assert " ".join("%08x" % v for v in pr.philox4x32_10(counter, key)) == out


def test_pinned_values_and_counter_construction():
    z = pr.randn(7, 0, 0, 2, 5)
    pinned = [0.22970816055506, 0.20041438525856883, 0.6326745268770012, 1.1822866467543975, 1.1322135771470712]
    np.testing.assert_allclose(z[0], pinned, rtol=0, atol=1e-15)
    assert np.array_equal(z[:, :3], pr.randn(7, 0, 0, 4, 3)[:2])                 # neither the row nor the column count enters a value
    assert np.array_equal(pr.randn(7, 0, 3, 2, 5), pr.randn(7, 0, 0, 5, 5)[3:])   # first_row shifts rows
    assert not np.array_equal(pr.randn(7, 1, 0, 2, 5), z) and not np.array_equal(pr.randn(8, 0, 0, 2, 5), z)
    assert not np.array_equal(pr.randn(7 + (1 << 32), 0, 0, 2, 5), z)            # the high key word
    assert np.array_equal(pr.randn(-1, 0, 0, 2, 5), pr.randn((1 << 64) - 1, 0, 0, 2, 5))      # two's complement


def test_moments_of_the_restatement():
    """Deterministic: seed 20240607, 1024 x 1024.  Measured 0.50, -2.81 and 4.89."""
    z = pr.randn(20240607, 0, 0, 1024, 1024)
    n = z.size
    assert abs(z.mean()) * np.sqrt(n) <= 4
    assert abs(z.var() - 1.0) / np.sqrt(2.0 / n) <= 4
    assert np.isfinite(z).all() and np.abs(z).max() < 8.57


# ------------------------------------------------------------------------------------------- the third header
def test_sample_header_parses_and_binds():
    text = open(_lib.HEADER_SAMPLE).read()
    protos = _lib.parse_prototypes(text)
    assert sorted(protos) == ["pg_randn"]
    assert _lib._SIGS_SAMPLE == _lib.signatures(protos)          # the closed vocabulary: signatures() raises on any other type
    assert not set(protos) & set(_lib.header_symbols()) and not set(protos) & set(_lib._SIGS_LOO)
    vp, i, lg = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    assert _lib._SIGS_SAMPLE["pg_randn"] == (i, [vp, i, lg, i, i, i, i, vp, lg, i, i, vp])
    # what csrc/sample.hip defines (pg_<name>_t, one per export) is what the header declares
    src = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "csrc", "sample.hip")).read()
    defined = set(re.findall(r"^int (pg_[a-z_0-9]+)_t\(", src, flags=re.M))
    assert defined == set(protos)
    lib = _lib.load(check_symbols=True)
    for name, (res, args) in _lib._SIGS_SAMPLE.items():
        fn = getattr(lib, name)                                  # a symbol of the built library ...
        assert isinstance(fn, ctypes._CFuncPtr) and fn.restype is res and list(fn.argtypes) == args
    assert lib.pg_randn(None, 0, 0, 0, 0, 1, 1, None, 1, 1, 1, None) != 0       # null handle: refused on the host
    assert "HEADER_SAMPLE" in inspect.getsource(_lib.build_id)


def test_every_sample_export_has_a_framed_case():
    """The rule of tests/test_framed_cpu.py, continued for include/pygpr_hip_sample.h."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_sample_framed_gpu.py")
    tree = ast.parse(open(path).read())
    used = {n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute) and n.attr.startswith("pg_")}
    assert sorted(set(_lib._SIGS_SAMPLE) - used) == [], "exports with a device buffer and no framed case"


def test_public_names():
    assert "PosteriorSampler" in pg.__all__ and "randn" in pg.__all__
    assert pg.GRBCM.sampler is pg.GPR.sampler and pg.GRBCM.sample is pg.GPR.sample      # the committee keeps the base class's refusal
    with pytest.raises(NotImplementedError):
        pg.sample_gp()
    with pytest.raises(ValueError):
        pg.randn(-1, 3)
    with pytest.raises(TypeError):
        pg.randn(2, 3, dtype=torch.float16)
    assert pg.randn(0, 5).shape == (0, 5) and pg.randn(4, 0, dtype=torch.float32).dtype == torch.float32      # nothing to generate: no device


# ------------------------------------------------------------------------------------------- host logic on a test double
class SampleOracleOps(OracleOps):
    """OracleOps plus the generator (tests/philox_ref.py) and the batched factorisation, in NumPy; counts factorisations."""

    def __init__(self):
        self.factorisations = 0
        self.randn_calls = []

    def build_factor(self, *a, **k):
        self.factorisations += 1
        return super().build_factor(*a, **k)

    def build_factor_batched(self, *a, **k):
        self.factorisations += 1
        return OracleOps.build_factor_batched(self, *a, **k)

    def potrf_trtri_batched(self, a_all, invd_all, info_all, minv_all=None):
        assert minv_all is None
        for e in range(a_all.shape[0]):
            self.potrf(a_all[e], None, info_all[e: e + 1])

    def randn(self, out, rows, cols, seed, stream_id=0, row0=0):
        self.randn_calls.append((rows, cols, seed, stream_id, row0))
        out.zero_()
        out[:rows, :cols] = torch.from_numpy(pr.randn(seed, stream_id, row0, rows, cols)).to(out.dtype)
        return out


@pytest.fixture
def fake_ops(monkeypatch, tmp_path):
    ops = SampleOracleOps()
    monkeypatch.setattr(_ops, "_OPS", ops)
    monkeypatch.chdir(tmp_path)
    return ops


HP = np.array([1.1, 0.8, 1.3, 0.3])
M = 37


def _model(n=40, d=2, seed=5, hp=HP):
    rng = np.random.default_rng(seed)
    x = rng.random((n, d))
    y = np.sin(3 * x.sum(1)) + 0.3 * rng.standard_normal(n)
    gp = pg.Exact_GP(torch.from_numpy(x.copy()), torch.from_numpy(y.copy()), pg.Compose([pg.Squared_exponential(), pg.White_noise()]))
    gp.set_params(torch.from_numpy(np.array(hp, dtype=np.float64)))
    xp = torch.from_numpy(np.random.default_rng(seed + 1).random((M, d)))
    return gp, xp


@pytest.mark.parametrize("noise", [True, False])
@pytest.mark.parametrize("prior", [True, False])
def test_sampler_host_path(fake_ops, noise, prior):
    gp, xp = _model()
    smp = gp.sampler(xp, noise=noise, prior=prior, jitter=1e-6)
    assert isinstance(smp, pg.PosteriorSampler) and (smp.m, smp.dtype, smp.noise, smp.jitter) == (M, torch.float64, noise, 1e-6)
    if prior:
        assert gp.need_upd and fake_ops.factorisations == 0       # neither needs nor triggers a fit
        mean, c = np.zeros(M), gp.cov.kernel(gp.params, xp).numpy()
        assert not smp.mean.any()
    else:
        mean, c = (t.numpy() for t in gp.predict(xp, "full"))
        assert np.array_equal(smp.mean.numpy(), mean)
    chol = smp.chol.numpy()
    assert chol.shape == (M, M) and not np.triu(chol, 1).any()
    shift = 1e-6 - (0.0 if noise else HP[-1] ** 2)
    np.testing.assert_allclose(chol @ chol.T, c + shift * np.eye(M), rtol=0, atol=1e-13 * np.abs(c).max())
    z = np.random.default_rng(3).standard_normal((6, M))
    np.testing.assert_allclose(smp.draw(z=torch.from_numpy(z)).numpy(), mean + z @ chol.T, rtol=0, atol=1e-13)
    np.testing.assert_allclose(smp.draw(z=torch.from_numpy(z[None])).numpy(), mean + z @ chol.T, rtol=0, atol=1e-13)
    got = smp.draw(5, seed=11, first=3)
    assert got.shape == (5, M) and fake_ops.randn_calls[-1] == (5, M, 11, 0, 3)
    assert np.array_equal(got.numpy(), smp.draw(z=torch.from_numpy(pr.randn(11, 0, 3, 5, M))).numpy())
    assert np.array_equal(gp.sample(xp, 5, 11, noise=noise, prior=prior, jitter=1e-6).numpy(), smp.draw(5, 11).numpy())


def test_draw_chunks_do_not_change_the_samples(fake_ops, monkeypatch):
    gp, xp = _model()
    smp = gp.sampler(xp, noise=True)
    whole = smp.draw(300, seed=4, first=2)
    monkeypatch.setattr(gpr_mod, "_DRAW_BYTES", 1)               # the smallest chunk: 128 rows
    parts = smp.draw(300, seed=4, first=2)
    assert [c[0] for c in fake_ops.randn_calls[-3:]] == [128, 128, 44] and [c[4] for c in fake_ops.randn_calls[-3:]] == [2, 130, 258]
    assert np.array_equal(whole.numpy(), parts.numpy())
    z = torch.from_numpy(np.random.default_rng(0).standard_normal((300, M)))
    assert np.array_equal(smp.draw(z=z).numpy()[:128], smp.draw(z=z[:128]).numpy())


def test_draw_argument_checks(fake_ops):
    gp, xp = _model()
    smp = gp.sampler(xp, noise=True)
    assert smp.draw(0).shape == (0, M) and smp.draw().shape == (1, M)
    with pytest.raises(ValueError, match="n_samples"):
        smp.draw(-1)
    for bad in (torch.zeros(4, M + 1, dtype=torch.float64), torch.zeros(M, dtype=torch.float64), torch.zeros(2, 4, M, dtype=torch.float64)):
        with pytest.raises(ValueError, match="z must be"):
            smp.draw(z=bad)
    with pytest.raises(NotImplementedError, match="GPR has no joint sampler"):
        pg.GPR.sampler(pg.GPR(gp.x, gp.y, gp.cov), xp)
    with pytest.raises(NotImplementedError, match="GPR has no joint sampler"):
        pg.GPR.sample(pg.GPR(gp.x, gp.y, gp.cov), xp, 3)


def test_sampler_is_a_snapshot_and_leaves_the_model_alone(fake_ops):
    gp, xp = _model()
    before = [t.numpy().copy() for t in gp.predict(xp, "full")]
    smp = gp.sampler(xp)
    after = [t.numpy() for t in gp.predict(xp, "full")]
    assert all(np.array_equal(a, b) for a, b in zip(before, after)) and fake_ops.factorisations == 1
    d0, c0, m0 = smp.draw(4, 1).numpy().copy(), smp.chol.numpy().copy(), smp.mean.numpy().copy()
    gp.set_params(torch.from_numpy(HP * 1.3))
    gp.update()
    gp.predict(xp, "full")
    assert np.array_equal(smp.draw(4, 1).numpy(), d0) and np.array_equal(smp.chol.numpy(), c0) and np.array_equal(smp.mean.numpy(), m0)
    assert not np.array_equal(gp.sampler(xp).draw(4, 1).numpy(), d0)


def test_failed_pivot_names_jitter_and_noise(fake_ops):
    """A clearly indefinite matrix (diagonal shifted by -10), not a singular one: the outcome does not hang on rounding."""
    gp, xp = _model()
    with pytest.raises(torch.linalg.LinAlgError, match="(?s)jitter.*noise") as e:
        gp.sampler(xp, jitter=-10.0)
    assert e.value.pg_info == 1
    assert gp.sampler(xp).draw(2).shape == (2, M)                # nothing of the failure stays behind


def test_batched_model_draws_one_stream_per_expert(fake_ops):
    hp3 = np.stack([HP, HP * 1.1, HP * 0.9])
    gp, xp = _model(hp=hp3)
    smp = gp.sampler(xp, noise=True)
    mean, chol = smp.mean.numpy(), smp.chol.numpy()
    pm, pc = (t.numpy() for t in gp.predict(xp, "full"))
    assert mean.shape == (3, M) and chol.shape == (3, M, M) and np.array_equal(mean, pm)
    got = smp.draw(5, seed=9).numpy()
    assert got.shape == (3, 5, M) and [c[3] for c in fake_ops.randn_calls[-3:]] == [0, 1, 2]
    for e in range(3):
        np.testing.assert_allclose(chol[e] @ chol[e].T, pc[e] + 1e-7 * np.eye(M), rtol=0, atol=1e-13 * np.abs(pc[e]).max())
        np.testing.assert_allclose(got[e], mean[e] + pr.randn(9, e, 0, 5, M) @ chol[e].T, rtol=0, atol=1e-13)
    with pytest.raises(ValueError, match="z must be"):
        smp.draw(z=torch.zeros(5, M, dtype=torch.float64))
    pri = gp.sampler(xp, prior=True, noise=True)
    assert pri.mean.shape == (3, M) and not pri.mean.any() and pri.draw(2).shape == (3, 2, M)
