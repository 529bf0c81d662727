"""NumPy restatement of pygpr_amd/pathwise.py: the spectral laws on tests/philox_ref.py's normals, and the dense pathwise formula and
its closed-form covariance on tests/kernel_ref.py, in the grammar of that file (a model is a list of part names, "wn" the noise).

    f_s(xp) = Phi(xp) w_s + k(xp, X) A^-1 (y - Phi(X) w_s - sqrt(shift) e_s),      A = k(X, X) + shift I,  shift = sum sigma_n^2 + JITTER

Given the frequencies the samples are exactly Gaussian with mean k(xp, X) A^-1 y and the covariance `sampler_cov` states; with the
feature covariance Kt = Phi Phi^T replaced by the kernel itself that covariance is the exact posterior's."""
import numpy as np

import feature_ref as fr
import kernel_ref as kr
import matmul_ref as mr
import philox_ref as ph

STREAM_DIR, STREAM_CHI, STREAM_W, STREAM_EPS = 0x5200, 0x5210, 0x5220, 0x5221
DOF = {"m12": 1, "m32": 3, "m52": 5}
JITTER = kr.JITTER


def stationary_blocks(terms, d):
    """(part, offset) of every stationary component in order; a product or a part without a spectral law is refused."""
    out = []
    for t, blocks in kr._chunks(terms, d):
        if t == "wn":
            continue
        if len(blocks) != 1 or blocks[0][0] not in ("se",) + tuple(DOF):
            raise NotImplementedError(str(t))
        out.append((blocks[0][0], blocks[0][1]))
    return out


def spectral_features(terms, hp, d, features, seed):
    """(NU [nf, d], U [nf], amp [nf]): feature 2 F c + 2 j is the cosine of pair j of component c, 2 F c + 2 j + 1 its sine."""
    F = int(features)
    comps = stationary_blocks(terms, d)
    nf = 2 * F * len(comps)
    nu, u, amp = np.zeros((nf, d)), np.zeros(nf), np.zeros(nf)
    for c, (part, o) in enumerate(comps):
        g = ph.randn(seed, STREAM_DIR + c, 0, F, d)
        if part == "se":
            s = np.full(F, np.sqrt(2.0))
        else:
            m = DOF[part]
            s = np.sqrt(m / (ph.randn(seed, STREAM_CHI + c, 0, F, m) ** 2).sum(1))
        f = s[:, None] * g * np.abs(hp[o + 1: o + 1 + d])[None, :] / (2.0 * np.pi)
        blk = slice(2 * F * c, 2 * F * (c + 1))
        nu[blk][0::2], nu[blk][1::2] = f, f
        u[blk][1::2] = -0.25
        amp[blk] = abs(hp[o]) / np.sqrt(F)
    return nu, u, amp


def weights(seed, nf, n_samples, amp):
    return ph.randn(seed, STREAM_W, 0, nf, n_samples) * amp[:, None]


def noise_draws(seed, n, n_samples):
    return ph.randn(seed, STREAM_EPS, 0, n, n_samples)


def features(x, nu, u, amp):
    """Phi with its amplitudes [n, nf]."""
    return fr.phi(x, nu, u) * amp[None, :]


def feature_kernel(xa, xb, nu, u, amp):
    """Kt(xa, xb) = Phi(xa) Phi(xb)^T, in slabs of features (F = 200000 would not fit as one matrix)."""
    out = np.zeros((xa.shape[0], xb.shape[0]))
    for s in range(0, nu.shape[0], 1 << 16):
        sl = slice(s, s + (1 << 16))
        out += features(xa, nu[sl], u[sl], amp[sl]) @ features(xb, nu[sl], u[sl], amp[sl]).T
    return out


def operator(terms, hp, x):
    n, d = x.shape
    return mr.stationary_kernel(terms, hp, x, x) + float(mr.shift_of(terms, hp, d, JITTER)) * np.eye(n)


def samples(terms, hp, x, y, xp, nu, u, amp, w, e):
    """The dense pathwise formula: [n_samples, q] (w carries the amplitudes; e are standard normals)."""
    d = x.shape[1]
    shift = float(mr.shift_of(terms, hp, d, JITTER))
    b = y[:, None] - fr.phi(x, nu, u) @ w - np.sqrt(shift) * e
    v = np.linalg.solve(operator(terms, hp, x), b)
    return (fr.phi(xp, nu, u) @ w + mr.stationary_kernel(terms, hp, xp, x) @ v).T


def sampler_cov(terms, hp, x, xp, kt):
    """Cov[f_s(xp)] given the frequencies, kt(a, b) the prior covariance the features realise:
        Kt** - Kt*x A^-1 K*x^T - K*x A^-1 Ktx* + K*x A^-1 (Ktxx + shift I) A^-1 Kx*."""
    d = x.shape[1]
    shift = float(mr.shift_of(terms, hp, d, JITTER))
    a = operator(terms, hp, x)
    ksx = mr.stationary_kernel(terms, hp, xp, x)
    g = np.linalg.solve(a, ksx.T).T                       # K*x A^-1
    cross = kt(xp, x) @ g.T
    return kt(xp, xp) - cross - cross.T + g @ (kt(x, x) + shift * np.eye(x.shape[0])) @ g.T
