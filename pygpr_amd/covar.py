"""Covariance kernels with PyGPR's `Covar` protocol (reference: PyGPR/covar.py), evaluated on the
MI355X through libpygpr_hip.

Same names, hyper-parameter layout and shapes as the reference:
  * `Squared_exponential`  hp = [sigma, l_1..l_d], K = sigma^2 exp(-sum_d l_d^2 (x_d - x'_d)^2),
    l are INVERSE length scales, sigma enters squared, no 1/2 in the exponent (covar.py:129-167)
  * `White_noise`          hp = [sigma_n], sigma_n^2 I; with `xp` given it is `tensor(0)` (covar.py:227-245)
  * `Compose`              sum of children, hp concatenated in list order, dK concatenated on dim -3
                           (covar.py:28-81)
  * `Matern52`             NEW (no reference counterpart), same hp layout as the SE.
  * `Matern32`, `Matern12` NEW, the rest of the Matern family (nu = 3/2 and 1/2, the exponential kernel), same hp layout.
  * `Rational_quadratic`   NEW, hp = [sigma, l_1..l_d, alpha] (d + 2 values): sigma^2 (1 + sq / alpha^2)^(-alpha^2) with the SE's
                           scaled squared distance sq; the squared exponential as alpha grows.
  * `Periodic`             NEW, hp = [sigma, l_1..l_d, p_1..p_d] (2 d + 1 values), one period per dimension:
                           sigma^2 exp(-sum_k l_k^2 sin^2(pi (x_k - x'_k) / p_k)); the phase is taken from the difference.
  * `Product`              NEW, the product of two to PG_MAX_COMP stationary kernels (no White_noise, no nesting), hp concatenated in
                           list order like Compose's, every factor keeping its own block and its own sigma: K = prod_c K_c,
                           dK/dtheta_{c,j} = (prod_{c' != c} K_c') dK_c/dtheta_{c,j}.  The locally periodic kernel is
                           Product([Squared_exponential(), Periodic()]); alone or as a child of Compose.
Leading batch dims on hp and/or x follow the reference's flatten-to-one-batch-dim rule.  Tensors come
back on the device of `x` (CPU in -> CPU out); the arithmetic always runs on the GPU in the dtype of
`x` (float64, or float32 as an explicit opt-in) -- unlike the reference, nothing here touches torch's
global default dtype.  Distances are direct sums of squared differences instead of the reference's GEMM
expansion (covar.py:102-127): same value to rounding, exactly symmetric, never negative.
"""
from typing import List, Protocol, Sequence

import torch
from torch import Tensor

from . import _lib
from ._ops import get_ops, make_spec, make_specs, pad_to


class Covar(Protocol):
    """Protocol for covariance kernels (PyGPR/covar.py:9-25)."""

    def get_params_shape(self, x: Tensor) -> List[int]:
        ...

    def init_params(self, x: Tensor) -> Tensor:
        ...

    def kernel(self, params: Tensor, x: Tensor, xp: Tensor = None) -> Tensor:
        ...

    def kernel_and_grad(self, params: Tensor, x: Tensor) -> List[Tensor]:
        ...


def _params_shape(x: Tensor, nhp: int) -> List[int]:
    shape = list(x.shape)
    shape[-1] = nhp
    shape.pop(-2)
    return shape


def layout(cov, d):
    """Flatten a covariance object into (kinds, offsets, noise_offsets, nhp) for pg_covspec."""
    kinds, offs, noise = [], [], []
    nhp = cov._collect(d, 0, kinds, offs, noise)
    return kinds, offs, noise, nhp


def terms(cov, d):
    """(terms, noise_offsets, nhp): the covariance as the sum it is.  One entry per stationary term in list order, each a tuple
    (product, kinds, offsets): a plain stationary child is (False, (kind,), (offset,)), a Product (True, its factors' kinds, their
    offsets).  layout() flattens the same walk and cannot tell Product([a, b]) from Compose([a, b])."""
    tms, noise = [], []
    nhp = cov._terms(d, 0, tms, noise)
    return tuple(tms), noise, nhp


def spec_of(cov, d):
    """(passes, nhp): the pg_covspec list the device ops take.  A sum of stationary and noise children is one entry unless it has more
    than PG_MAX_COMP of either.  A Product alone, or beside nothing but up to PG_MAX_COMP White_noise children, is ONE product spec (the
    fused, batched and checked paths take one spec); in any other sum the plain children go first, as they always did and with the noise
    in the earliest passes, and every Product follows in a product pass of its own without noise (`accumulate` and the disjoint gradient
    entries serve those as they serve a long Compose)."""
    tms, noise, nhp = terms(cov, d)
    plain = [t for t in tms if not t[0]]
    prods = [t for t in tms if t[0]]
    if len(prods) == 1 and not plain and len(noise) <= _lib.PG_MAX_COMP:
        return [make_spec(prods[0][1], prods[0][2], noise, product=True)], nhp
    passes = make_specs([t[1][0] for t in plain], [t[2][0] for t in plain], noise) if (plain or noise or not prods) else []
    return passes + [make_spec(t[1], t[2], [], product=True) for t in prods], nhp


class _DeviceKernel:
    """Shared evaluation code: every concrete kernel only says how it lays out its parameters."""

    def _collect(self, d, base, kinds, offs, noise):  # -> number of parameters consumed
        raise NotImplementedError

    def _nhp(self, d):
        return self._collect(d, 0, [], [], [])

    def _terms(self, d, base, tms, noise):  # -> number of parameters consumed; a leaf: one plain term per stationary kind it collects
        kinds, offs = [], []
        used = self._collect(d, base, kinds, offs, noise)
        tms.extend((False, (k,), (o,)) for k, o in zip(kinds, offs))
        return used

    # ---- protocol ---------------------------------------------------------------------------
    def get_params_shape(self, x: Tensor) -> List[int]:
        return _params_shape(x, self._nhp(x.shape[-1]))

    def _batches(self, hp, x, xp=None):
        nhp = self._nhp(x.shape[-1])
        assert hp.shape[-1] == nhp  # covar.py:52,66,131,171
        hb = hp.reshape(-1, nhp)
        xb = x.reshape(-1, x.shape[-2], x.shape[-1])
        xpb = None if xp is None else xp.reshape(-1, xp.shape[-2], xp.shape[-1])
        nb = max(hb.shape[0], xb.shape[0], 1 if xpb is None else xpb.shape[0])
        for t in (hb, xb, xpb):
            if t is not None and t.shape[0] not in (1, nb):
                raise RuntimeError("batch dimensions of hp / x / xp do not broadcast")
        return hb, xb, xpb, nb

    def kernel(self, hp: Tensor, x: Tensor, xp: Tensor = None) -> Tensor:
        ops = get_ops()
        hb, xb, xpb, nb = self._batches(hp, x, xp)
        n, d = xb.shape[-2:]
        spec, _ = spec_of(self, d)
        dt = x.dtype if x.dtype in (torch.float32, torch.float64) else torch.float64
        hd = ops.to_device(hb, torch.float64)
        xd = ops.to_device(xb, dt)
        xpd = None if xpb is None else ops.to_device(xpb, dt)
        outs = []
        for b in range(nb):
            hpb = hd[b % hd.shape[0]]
            xr = xd[b % xd.shape[0]]
            if xpd is None:
                buf = ops.empty(pad_to(n, 64), pad_to(n, 64), dtype=dt)
                ops.kernel_build(spec, hpb, xr, None, buf)
                outs.append(buf[:n, :n])
            else:
                xq = xpd[b % xpd.shape[0]]
                m = xq.shape[0]
                buf = ops.empty(pad_to(m, 64), pad_to(n, 64), dtype=dt)
                ops.kernel_build(spec, hpb, xq, xr, buf)     # rows = test points (covar.py:152-161)
                outs.append(buf[:m, :n])
        res = torch.stack(outs) if nb > 1 else outs[0].contiguous()
        return res.to(x.device)

    def kernel_and_grad(self, hp: Tensor, x: Tensor) -> List[Tensor]:
        ops = get_ops()
        hb, xb, _, nb = self._batches(hp, x)
        n, d = xb.shape[-2:]
        spec, nhp = spec_of(self, d)
        dt = x.dtype if x.dtype in (torch.float32, torch.float64) else torch.float64
        hd = ops.to_device(hb, torch.float64)
        xd = ops.to_device(xb, dt)
        ks, dks = [], []
        for b in range(nb):
            hpb, xr = hd[b % hd.shape[0]], xd[b % xd.shape[0]]
            buf = ops.empty(pad_to(n, 64), pad_to(n, 64), dtype=dt)
            ops.kernel_build(spec, hpb, xr, None, buf)
            ks.append(buf[:n, :n])
            dks.append(ops.kernel_grad_build(spec, hpb, xr, ops.empty(nhp, n, n, dtype=dt)))
        k = torch.stack(ks) if nb > 1 else ks[0].contiguous()
        dk = torch.stack(dks) if nb > 1 else dks[0]
        return [k.to(x.device), dk.to(x.device)]


class Squared_exponential(_DeviceKernel):
    """ARD squared exponential, K(x,x') = sig^2 exp(-|(x-x').ls|^2) (PyGPR/covar.py:84-206)."""

    _kind = _lib.PG_KIND_RBF

    def _collect(self, d, base, kinds, offs, noise):
        kinds.append(self._kind)
        offs.append(base)
        return d + 1

    def init_params(self, x: Tensor) -> Tensor:  # covar.py:96-100
        return torch.ones(self.get_params_shape(x), dtype=torch.float64)

    def distance(self, x: Tensor, xp: Tensor = None) -> Tensor:
        """Squared Euclidean distances (covar.py:102-127): x [(b), n, d] -> [(b), n, n]; with xp [(b), m, d] the rows
        are the test points, [(b), m, n]; a batch of one is squeezed away like the reference does.  Evaluated on the
        device by the covariance tile kernel as direct sums of squared differences (the reference expands
        -2 x x'^T + |x|^2 + |x'|^2: same value to rounding, but this one is exactly symmetric with a zero diagonal)."""
        ops = get_ops()
        xb = x.reshape(-1, x.shape[-2], x.shape[-1])
        xpb = None if xp is None else xp.reshape(-1, xp.shape[-2], xp.shape[-1])
        nb = max(xb.shape[0], 1 if xpb is None else xpb.shape[0])
        for t in (xb, xpb):
            if t is not None and t.shape[0] not in (1, nb):
                raise RuntimeError("batch dimensions of x / xp do not broadcast")
        dt = x.dtype if x.dtype in (torch.float32, torch.float64) else torch.float64
        xd = ops.to_device(xb, dt)
        xpd = None if xpb is None else ops.to_device(xpb, dt)
        n = xb.shape[1]
        outs = []
        for b in range(nb):
            xr = xd[b % xd.shape[0]]
            if xpd is None:
                buf = ops.empty(pad_to(n, 64), pad_to(n, 64), dtype=dt)
                ops.sqdist(xr, None, buf)
                outs.append(buf[:n, :n])
            else:
                xq = xpd[b % xpd.shape[0]]
                m = xq.shape[0]
                buf = ops.empty(pad_to(m, 64), pad_to(n, 64), dtype=dt)
                ops.sqdist(xq, xr, buf)
                outs.append(buf[:m, :n])
        res = torch.stack(outs) if nb > 1 else outs[0].contiguous()
        return res.to(x.device)


class Matern52(Squared_exponential):
    """Matern-5/2 with the SE parameterisation: r = |(x-x').ls|,
    K = sig^2 (1 + sqrt5 r + 5 r^2/3) exp(-sqrt5 r).  Not in the reference."""

    _kind = _lib.PG_KIND_MATERN52


class Matern32(Squared_exponential):
    """Matern-3/2 with the SE parameterisation: r = |(x-x').ls|, K = sig^2 (1 + sqrt3 r) exp(-sqrt3 r)."""

    _kind = _lib.PG_KIND_MATERN32


class Matern12(Squared_exponential):
    """Matern-1/2 (the exponential / Ornstein-Uhlenbeck kernel) with the SE parameterisation: r = |(x-x').ls|,
    K = sig^2 exp(-r).  dK/dl_k = -sig^2 exp(-r) l_k (x_k-x'_k)^2 / r, 0 at r = 0 (its limit)."""

    _kind = _lib.PG_KIND_MATERN12


class Rational_quadratic(Squared_exponential):
    """ARD rational quadratic, hp = [sigma, l_1..l_d, alpha]: d + 2 values, the shape alpha behind the SE's block.  The conventions are
    the SE's: l are INVERSE length scales, no 1/2 in the distance, and every parameter enters SQUARED, the shape included, so that an
    unconstrained optimiser cannot leave the domain.  With D_k = x_k - x'_k:

        sq = sum_k l_k^2 D_k^2,   a = alpha^2,   t = sq / a
        K         = sigma^2 (1 + t)^(-a) = sigma^2 exp(-a log1p(t))
        dK/dsigma = 2 K / sigma
        dK/dl_k   = -2 [K / (1 + t)] l_k D_k^2
        dK/dalpha = 2 alpha K [t / (1 + t) - log1p(t)]        (0 at sq = 0)
        dK/dx*_k  = -2 [K / (1 + t)] l_k^2 D_k

    A scale mixture of squared exponentials: K tends to this library's SE, sigma^2 exp(-sq), from above as a grows,
    0 <= K - K_SE <= K_SE (exp(sq^2 / (2 a)) - 1).  alpha = 0 gives NaN (0 * inf) and is not worked around."""

    _kind = _lib.PG_KIND_RQ

    def _collect(self, d, base, kinds, offs, noise):
        kinds.append(self._kind)
        offs.append(base)
        return d + 2


class Periodic(Squared_exponential):
    """ARD periodic kernel with one period per dimension, hp = [sigma, l_1..l_d, p_1..p_d]: 2 d + 1 values, the periods behind the SE's
    block.  The conventions are the SE's: l are INVERSE length scales, sigma and l enter squared, and there is no 1/2 and no factor 2 in
    the exponent.  With D_k = x_k - x'_k, w_k = pi / p_k and s_k = sin(w_k D_k):

        sq        = sum_k l_k^2 s_k^2
        K         = sigma^2 exp(-sq)
        dK/dsigma = 2 K / sigma
        dK/dl_k   = -2 K l_k s_k^2
        dK/dp_k   = K l_k^2 sin(2 w_k D_k) w_k D_k / p_k
        dK/dx*_k  = -K l_k^2 sin(2 w_k D_k) w_k         (D = x* - x, rows = test points)

    MacKay's exp(-2 sin^2(pi D / p) / ell^2) is this kernel with l^2 = 2 / ell^2.  K is even in p_k, so the period enters as it is;
    p_k = 0 gives NaN and is not worked around.  The phase is formed from the coordinate DIFFERENCE, t = D_k / p_k reduced exactly to
    |t - rint(t)| <= 1/2: K is exactly symmetric, exactly sigma^2 where a point meets itself, and keeps its accuracy on data far from
    the origin (the squared exponential on the warped point (l_k / 2) [cos, sin](2 pi x_k / p_k) is the same function and loses
    |x| / p ulps).  Sums with a trend kernel are written Compose([Squared_exponential(), Periodic(), White_noise()])."""

    _kind = _lib.PG_KIND_PERIODIC

    def _collect(self, d, base, kinds, offs, noise):
        kinds.append(self._kind)
        offs.append(base)
        return 2 * d + 1

    def distance(self, x: Tensor, xp: Tensor = None) -> Tensor:
        raise TypeError("Periodic has no Euclidean distance: Squared_exponential.distance is the squared exponential's")


class White_noise(_DeviceKernel):
    """Gaussian noise sigma_n^2 I (PyGPR/covar.py:209-269)."""

    def _collect(self, d, base, kinds, offs, noise):
        noise.append(base)
        return 1

    def init_params(self, x: Tensor) -> Tensor:  # covar.py:221-225
        return 1e-4 * torch.ones(self.get_params_shape(x), dtype=torch.float64)

    def kernel(self, hp: Tensor, x: Tensor, xp: Tensor = None) -> Tensor:
        if xp is not None:
            return torch.tensor(0)  # covar.py:243
        return super().kernel(hp, x)


class Compose(_DeviceKernel):
    """Sum of covariance kernels (PyGPR/covar.py:28-81)."""

    def __init__(self, covars: Sequence[Covar]) -> None:
        self.covars = covars

    def _collect(self, d, base, kinds, offs, noise):
        used = 0
        for c in self.covars:
            used += c._collect(d, base + used, kinds, offs, noise)
        return used

    def _terms(self, d, base, tms, noise):
        used = 0
        for c in self.covars:
            used += c._terms(d, base + used, tms, noise)
        return used

    def init_params(self, x: Tensor) -> Tensor:  # covar.py:45-48
        return torch.cat([c.init_params(x) for c in self.covars], dim=-1)

    def kernel(self, hp: Tensor, x: Tensor, xp: Tensor = None) -> Tensor:
        if xp is not None and not layout(self, x.shape[-1])[0]:
            assert hp.shape[-1] == self._nhp(x.shape[-1])
            return torch.tensor(0)  # a sum of White_noise children only
        return super().kernel(hp, x, xp)


class Product(_DeviceKernel):
    """Product of stationary covariance kernels, K = prod_c K_c: not in the reference, whose Compose can only add.  hp is the factors'
    blocks concatenated in list order, as in Compose; each factor keeps its block as it is, its own sigma included (the product's
    amplitude is prod_c sigma_c^2: the sigmas are not identified separately by data, and are not tied here).  With K_{-c} the product of
    the other factors:

        dK/dtheta_{c,j} = K_{-c} dK_c/dtheta_{c,j},      dK/dx* = sum_c K_{-c} dK_c/dx*

    K_{-c} is formed explicitly on the device, never as K / K_c: a factor that underflows to 0 gives K = 0 and zero derivatives.
    Factors are the stationary kinds (Squared_exponential, Matern52/32/12, Rational_quadratic, Periodic), two to PG_MAX_COMP of them; a
    White_noise, Compose or Product factor is a TypeError.  The locally periodic kernel is Product([Squared_exponential(), Periodic()]);
    a Product stands alone or as a child of Compose, beside stationary kernels, other Products and White_noise."""

    def __init__(self, covars: Sequence[Covar]) -> None:
        covars = list(covars)
        for c in covars:
            if not isinstance(c, Squared_exponential):      # (every stationary kind derives from it; White_noise, Compose and Product do not)
                raise TypeError("Product multiplies stationary kernels only, got %s" % type(c).__name__)
        if not 2 <= len(covars) <= _lib.PG_MAX_COMP:
            raise ValueError("Product takes 2 to %d factors, got %d" % (_lib.PG_MAX_COMP, len(covars)))
        self.covars = covars

    def _collect(self, d, base, kinds, offs, noise):
        used = 0
        for c in self.covars:
            used += c._collect(d, base + used, kinds, offs, noise)
        return used

    def _terms(self, d, base, tms, noise):
        kinds, offs = [], []
        used = self._collect(d, base, kinds, offs, noise)
        tms.append((True, tuple(kinds), tuple(offs)))
        return used

    def init_params(self, x: Tensor) -> Tensor:
        return torch.cat([c.init_params(x) for c in self.covars], dim=-1)
