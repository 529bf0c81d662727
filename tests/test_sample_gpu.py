"""The device normal generator (pg_randn, pygpr_amd.randn) against its NumPy restatement (tests/philox_ref.py), and Exact_GP.sampler /
PosteriorSampler.draw against host fp64 arithmetic on what the sampler itself reports.

Generator bounds, from the definition (include/pygpr_hip_sample.h), not from a measurement: fp64 2e-13 absolute -- |z| <= 8.57, the
argument 2 pi u2 is rounded once, log / sqrt / sincos are within a few ulp: about 5e-14, and a factor 4 for a different but correct
libm; fp32 1e-6 absolute -- one float ulp at 8.57.  Measured maxima on the MI355X: fp64 8.9e-16, fp32 2.4e-7.

Sampler data: oracle.synth, n = 200, d = 3, sigma and l in [0.5, 1.5], sigma_n = 0.3 (the conditioning of tests/test_loo_gpu.py); kernels
se + wn and m32 + rq + wn; m = 37 (one pad block) and 300 (two).  fp64 runs noise x prior; fp32 runs noise=True only: the latent fp32
covariance at jitter 1e-7 is not reliably positive definite (its rounding errors, about 1e-7 max |C| per entry, are of the jitter's size).

Sampler bounds.  `factor` is the Cholesky backward error max |L L^T - (C + shift I)| / max |C| (C = predict(xp, "full")[1] or
cov.kernel(params, xp), shift = jitter - [noise=False] sum sigma_n^2, formed on the host in fp64): independent of C's condition number.
`draw` is max |draw(z=z) - (mean + z L^T)| / max |mean + z L^T| with the sampler's own mean and L on the host in fp64.  Each is measured
over all cases of this file on the MI355X; the bound is that maximum times 10, rounded up to a power of ten.  Every test prints its
figure before it asserts.  Measured maxima / bounds ("Joint posterior and prior sampling", has the same table):

    fp64   factor 2.5e-14 / 1e-12   draw 4.7e-16 / 1e-14
    fp32   factor 1.2e-6 / 1e-4   draw 6.0e-7 / 1e-5

(under the sanity ceilings 1e-9 for fp64 and 1e-3 for fp32)."""
import functools

import numpy as np
import pytest
import torch

import philox_ref as pr
import pygpr_amd as pg
from oracle import pygpr_oracle as orc

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
RANDN_ATOL = {F64: 2e-13, F32: 1e-6}
BOUND = {(F64, "factor"): 1e-12, (F64, "draw"): 1e-14, (F32, "factor"): 1e-4, (F32, "draw"): 1e-5}
COV = {"se": pg.Squared_exponential, "m32": pg.Matern32, "rq": pg.Rational_quadratic, "wn": pg.White_noise}
KINDS = [("se", "wn"), ("m32", "rq", "wn")]
N, D = 200, 3
SIGMA_N = 0.3
SEEDS = [0, (1 << 40) + 3, -1]      # the high key word, two's complement


@pytest.fixture(scope="module")
def ops():
    from pygpr_amd._ops import get_ops

    return get_ops()


# ------------------------------------------------------------------------------------------- the generator
@functools.lru_cache(maxsize=None)
def ref_randn(seed, stream, first_row, rows, cols):
    z = pr.randn(seed, stream, first_row, rows, cols)
    z.setflags(write=False)
    return z


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 5), (2, 1000), (257, 130)])
def test_randn_values(dtype, rows, cols):
    """(1, 1) smallest; (3, 5) odd cols: the last block is half used; (2, 1000) several workgroups along a row; (257, 130) rows past one
    pad block.  Seeds 0, 2^40 + 3, -1; streams 0 and 5; first_row 0 and 1000."""
    worst = 0.0
    for seed in SEEDS:
        for stream in (0, 5):
            for first in (0, 1000):
                got = pg.randn(rows, cols, seed=seed, stream=stream, first_row=first, dtype=dtype)
                assert got.shape == (rows, cols) and got.dtype == dtype and got.device.type == "cpu"
                e = float(np.abs(got.double().numpy() - ref_randn(seed, stream, first, rows, cols)).max())
                worst = max(worst, e)
    print("randn_err %s %dx%d measured %.3e bound %.0e" % ("f64" if dtype == F64 else "f32", rows, cols, worst, RANDN_ATOL[dtype]))
    assert worst <= RANDN_ATOL[dtype]


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_randn_fp32_is_the_rounded_fp64_and_padding_and_stride(ops, dtype):
    rows, cols, seed = 257, 130, (1 << 40) + 3
    ref = ref_randn(seed, 5, 1000, rows, cols)
    out = torch.full((512, 384), float("nan"), dtype=dtype, device="cuda")
    ops.randn(out[:, :256], rows, cols, seed, stream_id=5, row0=1000)          # rows_pad = 512, cols_pad = 256, ldz = 384
    got = out.cpu().double().numpy()
    assert np.abs(got[:rows, :cols] - ref).max() <= RANDN_ATOL[dtype]
    assert not got[rows:, :256].any() and not got[:rows, cols:256].any()       # the rest of 512 x 256: exactly 0
    assert np.isnan(got[:, 256:]).all()                                        # beyond cols_pad: untouched
    # the single-element store path: odd ldz and a base one element off the 16-byte grid give the same bits
    flat = torch.full((1 + 512 * 259 + 8,), float("nan"), dtype=dtype, device="cuda")
    view = torch.as_strided(flat, (512, 256), (259, 1), 1)
    assert view.data_ptr() % 16 != 0
    ops.randn(view, rows, cols, seed, stream_id=5, row0=1000)
    assert torch.equal(view, out[:, :256])
    rest = torch.ones_like(flat, dtype=torch.bool)
    torch.as_strided(rest, (512, 256), (259, 1), 1).fill_(False)
    assert bool(torch.isnan(flat[rest]).all())
    if dtype == F32:
        wide = torch.empty(rows, cols, dtype=F64, device="cuda")
        ops.randn(wide, rows, cols, seed, stream_id=5, row0=1000)
        assert torch.equal(wide.float(), out[:rows, :cols])                     # not another stream: the rounding of the fp64 draw


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_randn_chunk_invariance(ops, dtype):
    whole = ops.randn(torch.empty(8, 70, dtype=dtype, device="cuda"), 8, 70, 12345)
    a = ops.randn(torch.empty(4, 70, dtype=dtype, device="cuda"), 4, 70, 12345, row0=0)
    b = ops.randn(torch.empty(128, 256, dtype=dtype, device="cuda"), 4, 70, 12345, row0=4)      # another padding as well
    assert torch.equal(whole[:4], a) and torch.equal(whole[4:], b[:4, :70])


# ------------------------------------------------------------------------------------------- the sampler
def hp_of(parts, seed=7):
    rng = np.random.default_rng(seed)
    return np.concatenate([[SIGMA_N] if p == "wn" else 0.5 + rng.random(D + (2 if p == "rq" else 1)) for p in parts])


@functools.lru_cache(maxsize=None)
def data(m):
    x, y = orc.synth(N, D, seed=11)
    xp = np.random.default_rng(100 + m).random((m, D))
    for a in (x, y, xp):
        a.setflags(write=False)
    return x, y, xp


def model(parts, dtype, hp=None):
    x, y, _ = data(37)
    gp = pg.Exact_GP(torch.from_numpy(x.copy()).to(dtype), torch.from_numpy(y.copy()).to(dtype), pg.Compose([COV[p]() for p in parts]))
    gp.set_params(torch.from_numpy(hp_of(parts) if hp is None else hp))
    return gp


def judge(dtype, what, got, ref, case, scale=None):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    e = float(np.abs(got - ref).max() / (np.abs(ref).max() if scale is None else scale))
    print("sample_err %s %-6s %-44s measured %.3e bound %.0e" % ("f64" if dtype == F64 else "f32", what, case, e, BOUND[dtype, what]))
    assert np.isfinite(got).all() and e <= BOUND[dtype, what], (what, case, e)


CASES = [(F64, noise, prior) for noise in (True, False) for prior in (True, False)] + [(F32, True, prior) for prior in (True, False)]


@pytest.mark.parametrize("dtype,noise,prior", CASES, ids=lambda v: {F64: "f64", F32: "f32"}.get(v, str(v)))
@pytest.mark.parametrize("m", [37, 300])
@pytest.mark.parametrize("parts", KINDS, ids="+".join)
def test_sampler_case(parts, m, dtype, noise, prior):
    """Mean, factor, draw with a given z, draw with a seed, prefix invariance.  fp32 runs noise=True only: the latent fp32 covariance at
    jitter 1e-7 is not reliably positive definite."""
    case = "%s m=%d noise=%d prior=%d" % ("+".join(parts), m, noise, prior)
    gp = model(parts, dtype)
    xp = torch.from_numpy(data(m)[2].copy()).to(dtype)
    smp = gp.sampler(xp, noise=noise, prior=prior)
    assert (smp.m, smp.dtype, smp.noise, smp.jitter) == (m, dtype, noise, 1e-7)
    mean, chol = smp.mean, smp.chol
    assert mean.shape == (m,) and chol.shape == (m, m) and mean.dtype == dtype and chol.dtype == dtype and mean.device == xp.device
    if prior:
        assert gp.need_upd and not mean.any()                     # exactly 0, and no fit was triggered
        c = gp.cov.kernel(gp.params, xp)
    else:
        pm, c = gp.predict(xp, "full")
        assert torch.equal(mean, pm)                              # predict's mean, bit for bit
    c = c.double().numpy()
    L, mu = chol.double().numpy(), mean.double().numpy()
    assert not np.triu(L, 1).any()
    shift = 1e-7 - (0.0 if noise else SIGMA_N ** 2)
    judge(dtype, "factor", L @ L.T, c + shift * np.eye(m), case, scale=np.abs(c).max())
    z = np.random.default_rng(m).standard_normal((6, m))
    zt = torch.from_numpy(z).to(dtype)
    got = smp.draw(z=zt)
    assert got.shape == (6, m) and got.dtype == dtype and got.device == xp.device
    judge(dtype, "draw", got.numpy(), mu + zt.double().numpy() @ L.T, case)
    d8 = smp.draw(8, seed=5, first=3)
    assert torch.equal(d8, smp.draw(z=pg.randn(8, m, seed=5, stream=0, first_row=3)))      # the same product on identical Z
    judge(dtype, "draw", d8[:4].numpy(), smp.draw(4, seed=5, first=3).double().numpy(), case + " prefix")
    assert torch.equal(gp.sample(xp, 4, 5, noise=noise, prior=prior), smp.draw(4, 5))


def test_sampler_statistics():
    """m = 64, noise=True, 4096 draws, seed 20240607: |sample mean - mean|_i <= 6 sqrt(C_ii / 4096) and max |sample covariance - C| <=
    6 sqrt(2) max diag(C) / sqrt(4096) (an entry's standard deviation is at most sqrt(2) maxdiag / sqrt(ns)).  The same case on the CPU
    (tests/philox_ref.py, the oracle's predictive covariance and NumPy's Cholesky) sits at 2.78 and 2.35 of those standard deviations."""
    gp = model(("se", "wn"), F64)
    xp = torch.from_numpy(np.random.default_rng(64).random((64, D)))
    mean, c = (t.numpy() for t in gp.predict(xp, "full"))
    s = gp.sampler(xp, noise=True).draw(4096, seed=20240607).numpy()
    em = float((np.abs(s.mean(0) - mean) / np.sqrt(np.diag(c) / 4096)).max())
    ec = float(np.abs(np.cov(s.T) - c).max() / (np.sqrt(2.0) * np.diag(c).max() / 64.0))
    print("sample_stats mean %.2f sigma, covariance %.2f sigma (limit 6)" % (em, ec))
    assert em <= 6 and ec <= 6


def test_sampler_is_a_snapshot():
    parts = ("se", "wn")
    gp = model(parts, F64)
    xp = torch.from_numpy(data(37)[2].copy())
    before = gp.predict(xp, "full")
    smp = gp.sampler(xp)
    after = gp.predict(xp, "full")
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    d0, c0 = smp.draw(4, 1), smp.chol
    gp.set_params(torch.from_numpy(hp_of(parts) * 1.2))
    gp.update()
    gp.predict(xp, "full")
    assert torch.equal(smp.draw(4, 1), d0) and torch.equal(smp.chol, c0)
    fresh = model(parts, F64)                                    # never fitted: the prior needs no update and triggers none
    assert fresh.need_upd
    assert fresh.sampler(xp, prior=True).draw(3).shape == (3, 37) and fresh.need_upd


def test_sampler_batched():
    parts = ("se", "wn")
    hp = hp_of(parts)
    gp = model(parts, F64, hp=np.stack([hp, hp * 1.1, hp * 0.9]))
    m = 37
    xp = torch.from_numpy(data(m)[2].copy())
    smp = gp.sampler(xp, noise=True)
    pm, pc = gp.predict(xp, "full")
    mean, chol = smp.mean, smp.chol
    assert mean.shape == (3, m) and chol.shape == (3, m, m) and torch.equal(mean, pm)
    got = smp.draw(5, seed=9)
    assert got.shape == (3, 5, m)
    for e in range(3):
        L, c = chol[e].numpy(), pc[e].numpy()
        assert not np.triu(L, 1).any()
        judge(F64, "factor", L @ L.T, c + 1e-7 * np.eye(m), "batched expert %d" % e, scale=np.abs(c).max())
        z = pg.randn(5, m, seed=9, stream=e).numpy()
        judge(F64, "draw", got[e].numpy(), mean[e].numpy() + z @ L.T, "batched expert %d" % e)


def test_sampler_errors():
    rng = np.random.default_rng(2)
    T = torch.from_numpy
    cov = pg.Compose([pg.Squared_exponential(), pg.White_noise()])
    gr = pg.GRBCM(T(rng.random((2, 30, D))), T(rng.random((2, 30))), T(rng.random((20, D))), T(rng.random(20)), cov)
    xp = T(data(37)[2].copy())
    with pytest.raises(NotImplementedError):
        gr.sampler(xp)
    with pytest.raises(NotImplementedError):
        gr.sample(xp, 2)
    smp = model(("se", "wn"), F64).sampler(xp, noise=True)
    with pytest.raises(ValueError):
        smp.draw(-1)
    with pytest.raises(ValueError):
        smp.draw(z=torch.zeros(4, 36, dtype=F64))
    assert smp.draw(0).shape == (0, 37)
