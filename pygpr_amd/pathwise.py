"""Pathwise function samples: posterior (and prior) functions of a GP that can be evaluated anywhere.  New, not in the reference.

Matheron's rule (Wilson, Borovitskiy, Terenin, Mostowsky, Deisenroth: "Efficiently sampling functions from Gaussian process
posteriors", ICML 2020): a prior function is drawn from random Fourier features and corrected by the data,

    f_s(.) = Phi(.) w_s + k(., X) A^-1 (y - Phi(X) w_s - eps_s),    eps_s ~ N(0, shift I),    A = k(X, X) + shift I.

After ONE block solve for all samples, evaluating S functions at q points is one cross product (pg_kernel_matmul) and one feature
product (pg_feature_matmul, include/pygpr_hip_feature.h): no further solve, nothing q x q or q x n, and Phi -- n x nf -- is never written.

Features.  Phi[i][f] = amp_f cos(2 pi (x_i . nu_f + u_f)), frequencies nu in cycles per unit, phases u in cycles.  For each stationary
component c of the covariance, with block [sigma, l_1..l_d] (k = sigma^2 rho(sum_k l_k^2 tau_k^2)) and F = `features`, pair j takes

    g_j [d] = normal(seed, STREAM_DIR + c, j, 0..d-1),        nu_j = s_j g_j |l| / (2 pi),

with the radial factor s_j = sqrt(2) for the squared exponential (omega_k = sqrt(2) l_k g_k is its spectral law) and
s_j = sqrt(m / chi_j), chi_j = sum_{i < m} normal(seed, STREAM_CHI + c, j, i)^2, for Matern-1/2, 3/2 and 5/2 (m = 1, 3, 5: the
multivariate Student-t with m = 2 nu degrees of freedom).  Every frequency is used twice, as a cosine (u = 0) and as a sine (u = -0.25,
exact in cycles), so the feature covariance (1/F) sum_j cos(omega_j . tau) is exactly stationary and no uniform variates are drawn.
A component contributes 2 F features of amplitude |sigma_c| / sqrt(F): feature 2 F c + 2 j is pair j's cosine, 2 F c + 2 j + 1 its sine.

The normals are pg_randn's (pygpr_amd.randn): counter-based, so sample s is a function of (seed, features, s) alone.
"""
from typing import Callable, Optional, Tuple

import numpy as np
import torch
from numpy import ndarray
from torch import Tensor

from . import _lib
from ._ops import get_ops
from .covar import Covar, spec_of, terms
from .sparse import _stationary

STREAM_DIR = 0x5200      # pg_randn stream of the directions g of component c: STREAM_DIR + c  (c < PG_MAX_COMP)
STREAM_CHI = 0x5210      # ... of the normals whose square sum is a Matern component's chi^2: STREAM_CHI + c
STREAM_W = 0x5220        # ... of the feature weights W [nf, S]
STREAM_EPS = 0x5221      # ... of the noise draws E [n, S]
_GRAD_COLUMNS = 512      # columns of the derivative's feature weights (coordinates x samples) one feature product carries

_KIND_NAMES = {_lib.PG_KIND_RQ: "Rational_quadratic", _lib.PG_KIND_PERIODIC: "Periodic"}
_DOF = {_lib.PG_KIND_MATERN12: 1, _lib.PG_KIND_MATERN32: 3, _lib.PG_KIND_MATERN52: 5}      # m = 2 nu


def _checked_terms(cov: Covar, d: int):
    """The stationary terms of a covariance whose spectral law is implemented, or the refusal."""
    passes, nhp = spec_of(cov, d)
    if len(passes) != 1:
        raise NotImplementedError("spectral_features: covariances that need more than one pg_covspec pass are not supported")
    tms, _, _ = terms(cov, d)
    for product, kinds, _ in tms:
        if product:
            raise NotImplementedError("spectral_features: a Product has no spectral law here (the convolution of its factors' is a follow-up)")
        if kinds[0] != _lib.PG_KIND_RBF and kinds[0] not in _DOF:
            raise NotImplementedError("spectral_features: %s has no spectral law here (gamma variates / a discrete spectrum are a follow-up)"
                                      % _KIND_NAMES.get(kinds[0], "kind %d" % kinds[0]))
    return tms, passes[0], nhp


def _hp_vector(params, nhp: int) -> ndarray:
    p = params.detach().cpu().numpy() if isinstance(params, Tensor) else np.asarray(params)
    if p.dtype != np.float64:
        raise TypeError("spectral_features computes in float64 only; params is %s" % p.dtype)
    if p.shape[-1] != nhp:
        raise ValueError("spectral_features: the covariance takes %d hyper-parameters, got %d" % (nhp, p.shape[-1]))
    if p.reshape(-1, nhp).shape[0] != 1:
        raise NotImplementedError("spectral_features: batched hyper-parameters are not supported")
    return np.array(p.reshape(nhp), dtype=np.float64)


def _check_count(name: str, v) -> int:
    if not (isinstance(v, (int, np.integer)) and v >= 1):
        raise ValueError("%s must be a positive integer, got %r" % (name, v))
    return int(v)


def spectral_features(cov: Covar, params, d: int, features: int = 1024, seed: int = 0) -> Tuple[ndarray, ndarray, ndarray]:
    """(NU [nf, d], U [nf], amp [nf]) as float64 host arrays, nf = 2 * features * (stationary components): the random Fourier features
    of `cov` at the hyper-parameters `params` (see the module's text).  Squared_exponential, Matern12, Matern32 and Matern52 components
    of one pg_covspec; Rational_quadratic, Periodic and Product raise NotImplementedError.  White_noise children carry no features."""
    F = _check_count("spectral_features: features", features)
    if not isinstance(seed, (int, np.integer)):
        raise ValueError("spectral_features: the seed must be an integer, got %r" % (seed,))
    tms, _, nhp = _checked_terms(cov, d)
    hp = _hp_vector(params, nhp)
    from .gpr import randn

    nf = 2 * F * len(tms)
    nu, u, amp = np.zeros((nf, d)), np.zeros(nf), np.zeros(nf)
    for c, (_, kinds, offs) in enumerate(tms):
        o = offs[0]
        g = randn(F, d, seed, STREAM_DIR + c).numpy()
        if kinds[0] == _lib.PG_KIND_RBF:
            s = np.full(F, np.sqrt(2.0))
        else:
            m = _DOF[kinds[0]]
            chi = (randn(F, m, seed, STREAM_CHI + c).numpy() ** 2).sum(1)
            s = np.sqrt(m / chi)
        f = s[:, None] * g * np.abs(hp[o + 1: o + 1 + d])[None, :] / (2.0 * np.pi)
        blk = slice(2 * F * c, 2 * F * (c + 1))
        nu[blk][0::2], nu[blk][1::2] = f, f
        u[blk][1::2] = -0.25
        amp[blk] = abs(hp[o]) / np.sqrt(F)
    return nu, u, amp


class FunctionSamples:
    """S functions drawn from a GP's posterior (or prior), to be evaluated wherever wanted: `fs(xp)` -> [n_samples, q] on xp's device.

    The samples are of the LATENT function f: no observation noise is added at the test points (add sigma_n * normal yourself for draws
    of new observations).  An instance is a snapshot -- it owns copies of the points, the hyper-parameters, the features and the solved
    weights, so later set_params or data edits of the model do not change it.  Sample s depends on (seed, features, s) and not on
    n_samples.  Memory: O(n (d + S) + nf (d + S)); nothing is n x nf or q x n.

    `frequencies` [nf, d], `phases` [nf], `weights` [nf, S] (the normals times the features' amplitudes) and `data_weights` [n, S] (the
    solved A^-1 (y - Phi(X) w_s - eps_s); None for a prior) are host copies: f_s(.) = Phi(.) weights[:, s] + k(., X) data_weights[:, s];
    `cg_info`: solves, iterations (the most any block solve took) and residual (the worst true one) -- None for a prior."""

    def __init__(self, spec, hpd: Optional[Tensor], x: Optional[Tensor], nu: Tensor, u: Tensor, w: Tensor, v: Optional[Tensor],
                 features: int, seed: int, cg_info: Optional[dict]) -> None:
        self._spec, self._hpd, self._x, self._nu, self._u, self._w, self._v = spec, hpd, x, nu, u, w, v
        self.n_samples, self.features, self.seed = int(w.shape[1]), int(features), int(seed)
        self.prior = v is None
        self.cg_info = cg_info

    @property
    def frequencies(self) -> ndarray:
        return self._nu.cpu().numpy()

    @property
    def phases(self) -> ndarray:
        return self._u.cpu().numpy()

    @property
    def weights(self) -> ndarray:
        return self._w.cpu().numpy()

    @property
    def data_weights(self) -> Optional[ndarray]:
        return None if self._v is None else self._v.cpu().numpy()

    def _checked_device(self, xp: Tensor):
        d = self._nu.shape[1]
        if not isinstance(xp, Tensor) or xp.dim() != 2 or xp.shape[1] != d:
            raise NotImplementedError("FunctionSamples: xp must be [q, %d] (no batches)" % d)
        if xp.dtype != torch.float64:
            raise TypeError("FunctionSamples computes in float64 only; xp is %s" % xp.dtype)
        ops = get_ops()
        return ops, ops.to_device(xp.detach(), torch.float64)

    def grad(self, xp: Tensor) -> Tensor:
        """[n_samples, q, d] on xp's device: entry [s, p, k] is d f_s(xp_p) / d xp_pk, the derivative of what `fs(xp)` returns.  The
        feature part is the feature product at phases u + 0.25 (exact in cycles: d/dt cos(2 pi t) = 2 pi cos(2 pi (t + 1/4))) against
        the weights 2 pi nu_fk w_fs, d S columns taken in blocks of coordinates; the data part is one pg_kernel_matmul_dx against the
        solved weights (include/pygpr_hip_dmatmul.h).  No solve, nothing q x n."""
        ops, xpd = self._checked_device(xp)
        q, d, S = xpd.shape[0], self._nu.shape[1], self.n_samples
        out = ops.empty(q, d, S)
        uq = self._u + 0.25
        kb = max(1, _GRAD_COLUMNS // S)
        for k0 in range(0, d, kb):
            k1 = min(d, k0 + kb)
            wk = (2.0 * np.pi) * self._nu[:, k0:k1, None] * self._w[:, None, :]           # [nf, kb, S]
            part = ops.feature_matmul(xpd, self._nu, uq, wk.reshape(wk.shape[0], (k1 - k0) * S))
            out[:, k0:k1, :] = part.reshape(q, k1 - k0, S)
        if self._v is not None:
            out += ops.kernel_matmul_dx(self._spec, self._hpd, xpd, self._x, self._v)
        return out.permute(2, 0, 1).contiguous().to(xp.device)

    def __call__(self, xp: Tensor) -> Tensor:
        ops, xpd = self._checked_device(xp)
        out = ops.feature_matmul(xpd, self._nu, self._u, self._w)                      # [q, S]
        if self._v is not None:
            out += ops.kernel_matmul(self._spec, self._hpd, xpd, self._x, self._v)
        return out.t().contiguous().to(xp.device)


def draw_function_samples(cov: Covar, hp: ndarray, x: Tensor, y: Optional[Tensor], shift: float, n_samples: int, features: int, seed: int,
                          solve: Optional[Callable[[Tensor], Tuple[Tensor, dict]]]) -> FunctionSamples:
    """The samples of one model: x [n, d] and y [n] on the device, hp the host vector, shift = sum sigma_n^2 + the model's jitter, and
    `solve`: B [n, S] -> (A^-1 B [n, S], cg_info) -- whatever solver the model has.  solve None: the prior (y and shift are not read)."""
    S = _check_count("function_samples: n_samples", n_samples)
    ops = get_ops()
    d = x.shape[1]
    nu, u, amp = spectral_features(cov, hp, d, features, seed)
    _, sp, _ = _checked_terms(cov, d)
    nf = nu.shape[0]
    nud, ud, ampd = (ops.to_device(torch.from_numpy(a), torch.float64) for a in (nu, u, amp))
    w = ops.randn(ops.empty(nf, S), nf, S, seed, stream_id=STREAM_W)
    w.mul_(ampd[:, None])
    if solve is None:
        return FunctionSamples(None, None, None, nud, ud, w, None, features, seed, None)
    n = x.shape[0]
    xs = x.clone()
    b = ops.randn(ops.empty(n, S), n, S, seed, stream_id=STREAM_EPS)
    b.mul_(-float(np.sqrt(shift)))
    b -= ops.feature_matmul(xs, nud, ud, w)
    b += y[:, None]
    v, info = solve(b)
    hpd = ops.to_device(torch.from_numpy(np.array(hp, dtype=np.float64)), torch.float64)
    return FunctionSamples(_stationary(sp), hpd, xs, nud, ud, w, v, features, seed, info)
