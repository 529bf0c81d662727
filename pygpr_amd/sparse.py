"""Inducing-point GP regression: Titsias' collapsed variational bound ("VFE" / SGPR) on the MI355X.  New, not in the reference.

With m inducing inputs z, Kuu = k(z, z) + JITTER I, Kuf = k(z, x), sigma^2 = sum sigma_n^2 over the White_noise children,
Phi = Kuf Kuf^T, b = Kuf y, Sigma = Kuu + Phi / sigma^2, c = Sigma^-1 b and T = n kdiag - tr(Kuu^-1 Phi):

    L     = sum log diag Ls - sum log diag Lu + n/2 log sigma^2 + y^T y / (2 sigma^2) - b^T c / (2 sigma^4) + n/2 log 2pi + T / (2 sigma^2)
    mean* = Ksu c / sigma^2,      cov* = Kss - Ksu (Kuu^-1 - Sigma^-1) Kus      (Kss keeps the noise, as Exact_GP.predict keeps it)

L is the NEGATIVE bound: `VFE(model)` follows MLE's protocol, so `CG(VFE(model))` trains the hyper-parameters.  O(n m^2) time and
O(m^2 + m chunk) memory: the training points are streamed in chunks of `_SPARSE_CHUNK` columns and nothing of size n x anything
outlives one chunk.

How one evaluation runs.  Every chunk's Kuf_c is built into an AUGMENTED operand A_c = [Kuf_c; y_c^T; 0] (m_aug = pad(m + 1) rows), so
that one deep-K product of the GEMM core per chunk, Phi_aug += A_c A_c^T (lower tiles), carries Phi, b (row m) and y^T y (entry
[m, m]) together.  The m x m algebra runs on padded buffers with the identity in the padding: two factorisations, their inverses
(trtri + lauum, mirrored), c = Sigma^-1 b by substitution against Ls (never through the explicit inverse: b^T c cancels against
y^T y), and the product Kuu^-1 Phi_aug (trace: T; times Kuu^-1: the last term of G_uu).  The gradient is

    dL = sum G_uu o dKuu + sum_c sum G_uf,c o dKuf_c + explicit terms in sigma_n and the prior variances,
    G_uu   = 1/2 Sigma^-1 - 1/2 Kuu^-1 + c c^T / (2 sigma^4) + Kuu^-1 Phi Kuu^-1 / (2 sigma^2)
    G_uf,c = (Sigma^-1 - Kuu^-1) Kuf_c / sigma^2 - c (y_c - Kuf_c^T c / sigma^2)^T / sigma^4 = [M | -c / sigma^4] A_c,
             M = (Sigma^-1 - Kuu^-1) / sigma^2 + c c^T / sigma^6

-- the rank-one correction rides in the same NN product as the matrix term, because A_c holds y_c -- and both contractions against
dK/dtheta are pg_kernel_cross_grad (include/pygpr_hip_sparse.h), which rebuilds the derivative from the point tiles.  Batched
models, float32 and covariances longer than one pg_covspec are not served.

z is data to `VFE(model)`.  `select_inducing` / `Sparse_GP.greedy` choose it among the training points: greedy conditional-variance
selection, the partial pivoted Cholesky factorisation of k(x, x) on the device (include/pygpr_hip_select.h; 8 n m bytes of workspace
for the factor).  `VFE(model, train_z=True)` trains it from there, jointly with the hyper-parameters, on the packed vector
concat(hp, z.reshape(-1)).  The same weights give the gradient:

    dL/dz_ik = 2 sum_j G_uu[i][j] dk(z_i, z_j)/dz_ik + sum_c sum_j G_uf,c[i][j] dk(z_i, x_j)/dz_ik

(z_j held constant in the first sum: G_uu is symmetric, z_i enters row i and column i; JITTER, kdiag and the sigma^2 terms do not
depend on z).  Both sums are pg_kernel_xgrad, the contraction of the kernel's first-argument derivative that Exact_GP.predict_grad uses,
with the lanes on the inducing inputs: one call on G_uu, one accumulating call per chunk on the rows [:m] of the W_c pass 2 already
holds; dL/dz rides in the evaluation's one transfer.  `predict_grad` is the same contraction on the test points, with u = c / sigma^2
for the mean and B = V = Ksu (Kuu^-1 - Sigma^-1), the product `predict` forms anyway, for the variance.  z is unconstrained, and by
default Sigma is factored unwhitened: a line search that drives two inducing inputs together ends in the LinAlgError an hp-only run
ends in when sigma_n falls too far, and the error propagates out of the optimiser -- the whitened evaluation below is the one to train
z on.  Matern-1/2 has no derivative at a coincident pair: it contributes 0.

Whitened evaluation.  `Sparse_GP(..., whitened=True)` is a second path through the same model for small noise, many
or trainable inducing inputs, where Sigma spans 1e12 and more and is no longer numerically positive definite.  With Li = Lu^-1,
V_c = Li A_c (row m still y_c: the padding of Li is the identity), Psi_aug = sum_c V_c V_c^T (Psi, b~ = Li b in row m, y^T y at [m, m]),
D = I + Psi / sigma^2, Ld = chol(D), c~ = D^-1 b~ by substitution and E = I - D^-1:

    L     = sum log diag Ld + n/2 log sigma^2 + y^T y / (2 sigma^2) - b~^T c~ / (2 sigma^4) + n/2 log 2pi + (n kdiag - tr Psi) / (2 sigma^2)
    G_uu  = 1/2 Li^T [(D^-1 - I) + c~ c~^T / sigma^4 + Psi / sigma^2] Li
    W_c   = Li^T ([M~ | -c~ / sigma^4] V_c) = G_uf,c,      M~ = (D^-1 - I) / sigma^2 + c~ c~^T / sigma^6
    mean* = w c~ / sigma^2,   cov* = Kss - (w E) w^T,   w = Ksu Li^T per chunk of test points;   predict_grad: u = Li^T c~ / sigma^2, V = (w E) Li

D has no eigenvalue below 1 whatever Kuu's condition.  Every chunk is whitened BEFORE it is accumulated (Lu^-1 Phi Lu^-T, formed after
Phi has lost the digits, fails like Sigma), and the weights stay whitened per chunk: G_uu and W_c come back to original coordinates only
after the product with the chunk, because Li^T . Li folded into one m x m matrix and applied to the unwhitened Kuf_c or Ksu loses the
gradient and the variance at small noise.  No new kernel: the products with Li are K-range products of the GEMM core (Li from pg_trtri
has scratch above its diagonal blocks), three per chunk of training points more than the unwhitened passes and one per chunk of test
points.  Still one synchronisation per evaluation and O(m^2 + m chunk) memory, with one more chunk-sized buffer.  The default,
whitened=False, is the evaluation described above, call for call.
"""
import math
from typing import NamedTuple, Sequence

import numpy as np
import torch
from numpy import ndarray
from torch import Tensor

from . import _lib
from ._lib import CovSpec
from ._ops import JITTER, get_ops, pad_to
from .covar import Covar, spec_of, terms
from .gpr import _CHUNK, GPR, _checked, _lin_alg_error
from .loss import _MemoLoss

_SPARSE_CHUNK = 32768   # training points per streamed chunk (columns of Kuf held at a time)


def _pass1_variant(ma):
    """The tiling of pass 1's lower-tile product at m_aug rows.  With fewer 128 x 128 lower tiles than the MI355X has compute units
    (m_aug <= 2816) the launch is one partly filled round however deep K is; the 64 x 64 tiling has four times the tiles and gives the
    same bits (an element's k order does not depend on the tile shape).  Measured at K = 32768: 3.44 against 4.66 ms at m_aug = 2304,
    1.66 against 4.63 ms at 1280."""
    t = ma // 128
    return _lib.GEMM_NT_64 if t * (t + 1) // 2 <= 256 else _lib.GEMM_NT


def _stationary(sp):
    """The pass without its noise children: Kuu carries JITTER alone, and the contraction has no noise entries."""
    out = CovSpec()
    out.ncomp = sp.ncomp
    for i in range(_lib.PG_MAX_COMP):
        out.kind[i], out.off[i] = sp.kind[i], sp.off[i]
    out.nnoise = 0
    return out


def _prior_of(cov, d, hp):
    """(sigma^2, kdiag, the terms, the noise offsets) of a covariance at the host vector hp: see Sparse_GP._prior."""
    tms, noise, _ = terms(cov, d)
    sig2 = float(sum(hp[o] ** 2 for o in noise))
    kdiag = float(sum(np.prod([hp[o] ** 2 for o in offs]) for _, _, offs in tms))
    return sig2, kdiag, tms, noise


class Selection(NamedTuple):
    """What select_inducing returns, on the device of the points it was given: `index` [count] int64, the chosen training points in
    selection order; `trace` [count], the trace term of the collapsed bound (n kdiag - tr(Kuu^-1 Kuf Kfu), without jitter) after
    each choice -- the curve to pick m from; `residual` [n], the prior variance the chosen set leaves unexplained at every point."""
    index: Tensor
    trace: Tensor
    residual: Tensor


def select_inducing(x: Tensor, cov: Covar, params, m: int, tol: float = 0.0) -> Selection:
    """Greedy conditional-variance selection of up to m inducing points among the rows of x [n, d] (float64) at the hyper-parameters
    `params`: repeatedly the point whose prior variance the points chosen so far explain least -- the partial pivoted Cholesky
    factorisation of k(x, x) (pg_greedy_select, include/pygpr_hip_select.h).  The stationary part of `cov` alone decides; a
    White_noise child is neither required nor used.  Selection stops early once the largest residual variance is no longer above
    max(tol * kdiag, JITTER): a point whose conditional variance is below the jitter Sparse_GP adds to Kuu cannot improve the bound.
    Needs 8 n m bytes of device workspace (the factor), unlike the model's O(m^2 + m chunk)."""
    if not isinstance(x, Tensor) or x.dtype != torch.float64:
        raise TypeError("select_inducing computes in float64 only; x is %s" % getattr(x, "dtype", type(x).__name__))
    if x.dim() != 2:
        raise NotImplementedError("select_inducing: batched points are not supported (x [n, d])")
    n, d = x.shape
    tms, _, _ = terms(cov, d)
    if not tms:
        raise ValueError("select_inducing: the covariance has no stationary term to select by")
    passes, nhp = spec_of(cov, d)
    if len(passes) != 1:
        raise NotImplementedError("select_inducing: covariances that need more than one pg_covspec pass are not supported")
    p = params.detach().cpu().numpy() if isinstance(params, Tensor) else np.asarray(params)
    if p.dtype != np.float64:
        raise TypeError("select_inducing computes in float64 only; params is %s" % p.dtype)
    if p.shape[-1] != nhp:
        raise ValueError("select_inducing: the covariance takes %d hyper-parameters, got %d" % (nhp, p.shape[-1]))
    if p.reshape(-1, nhp).shape[0] != 1:
        raise NotImplementedError("select_inducing: batched hyper-parameters are not supported")
    hp = np.array(p.reshape(nhp), dtype=np.float64)
    if not (isinstance(m, (int, np.integer)) and 1 <= m <= n):
        raise ValueError("select_inducing: m must be an integer in [1, %d], got %r" % (n, m))
    _, kdiag, _, _ = _prior_of(cov, d, hp)
    floor = max(float(tol) * kdiag, JITTER)
    ops = get_ops()
    xd = ops.to_device(x, torch.float64)
    hpd = ops.to_device(torch.from_numpy(hp), torch.float64)
    piv, count, trace, resid = ops.greedy_select(_stationary(passes[0]), hpd, xd, int(m), floor)
    c = int(count.cpu()[0])                                        # the one synchronisation
    return Selection(piv[:c].to(device=x.device, dtype=torch.int64), trace[:c].to(x.device), resid.to(x.device))


class Sparse_GP(GPR):
    """Variational inducing-point GP: x [n, d], y [n], z [m, d] inducing inputs (data like x, unless VFE(train_z=True) trains them),
    all float64; params as Exact_GP's.
    `Sparse_GP.greedy(x, y, cov, m)` chooses z among the training points; `select_inducing` chooses it again at the current params.
    whitened=True evaluates the bound, its gradients and the predictions in the coordinates of Lu^-1 (module docstring, "Whitened
    evaluation"): for small noise, many or trainable inducing inputs, where Sigma itself can no longer be factored."""

    def __init__(self, x: Tensor, y: Tensor, cov: Covar, z: Tensor, whitened: bool = False) -> None:
        super().__init__(x, y, cov)
        self._z = z
        self._whitened = bool(whitened)
        self._check_data()
        d = x.shape[-1]
        _, noise, _ = terms(cov, d)
        if not noise:
            raise ValueError("Sparse_GP: the covariance needs a White_noise child (the bound divides by the noise variance)")
        passes, _ = spec_of(cov, d)
        if len(passes) != 1:
            raise NotImplementedError("Sparse_GP: covariances that need more than one pg_covspec pass are not supported")
        self.params: Tensor = cov.init_params(x)
        self._dev = None
        self._dev_key = None
        self._state = None
        self._bufs = {}
        self._z_version = 0
        self.need_upd = True

    # ---- inducing inputs from the training points -------------------------------------------
    @classmethod
    def greedy(cls, x: Tensor, y: Tensor, cov: Covar, m: int, params=None, tol: float = 0.0, whitened: bool = False) -> "Sparse_GP":
        """A model whose m (or fewer: `tol`) inducing inputs are chosen among x by `select_inducing` at `params`, which the model
        then holds, or at cov.init_params(x).  whitened: as the constructor's (the selection itself does not depend on it)."""
        res = select_inducing(x, cov, cov.init_params(x) if params is None else params, m, tol)
        model = cls(x, y, cov, x[res.index], whitened=whitened)
        if params is not None:
            model.set_params(params if isinstance(params, Tensor) else torch.as_tensor(np.asarray(params)))
        return model

    def select_inducing(self, m: int = None, tol: float = 0.0) -> Selection:
        """Choose the inducing inputs again among the training points at the current params (m: as many as now) and assign them: the
        model turns dirty and a VFE on it drops its memo.  Returns the Selection."""
        res = select_inducing(self._x, self.cov, self._hp_host(), self._z.shape[0] if m is None else m, tol)
        self.z = self._x[res.index]
        return res

    # ---- data -------------------------------------------------------------------------------
    @property
    def z(self) -> Tensor:
        return self._z

    @z.setter
    def z(self, value: Tensor) -> None:
        self._z = value
        self._z_version += 1
        self._data_changed()

    @property
    def whitened(self) -> bool:
        """Whether the model evaluates in whitened coordinates; fixed at construction."""
        return self._whitened

    @property
    def dtype(self):
        return torch.float64

    def _data_changed(self) -> None:
        self._dev = None
        self._state = None
        self.need_upd = True

    def _check_data(self) -> None:
        x, y, z = self._x, self._y, self._z
        for name, t in (("x", x), ("y", y), ("z", z)):
            if t.dtype != torch.float64:
                raise TypeError("Sparse_GP computes in float64 only (the sigma^-4 terms of the bound leave no digits in single "
                                "precision); %s is %s" % (name, t.dtype))
        if x.dim() != 2 or y.dim() != 1:
            raise NotImplementedError("Sparse_GP: batched models are not supported (x [n, d], y [n])")
        if z.dim() != 2 or z.shape[1] != x.shape[1] or z.shape[0] < 1:
            raise ValueError("Sparse_GP: z must be [m, %d] with m >= 1, got %s" % (x.shape[1], tuple(z.shape)))
        if y.shape[0] != x.shape[0]:
            raise ValueError("Sparse_GP: x holds %d points, y %d values" % (x.shape[0], y.shape[0]))

    def _device_data(self):
        """(x, y, z) on the device, uploaded once per (tensor identity, version)."""
        key = tuple(v for t in (self._x, self._y, self._z) for v in (id(t), t._version))
        if self._dev is None or self._dev_key != key:
            self._check_data()
            ops = get_ops()
            self._dev = tuple(ops.to_device(t, torch.float64) for t in (self._x, self._y, self._z))
            self._dev_key = key
            self._state = None
            self.need_upd = True
        return self._dev

    def _hp_host(self, params=None) -> ndarray:
        p = self.params if params is None else params
        p = p.detach().cpu().numpy() if isinstance(p, Tensor) else np.asarray(p)
        _, nhp = spec_of(self.cov, self._x.shape[-1])
        assert p.shape[-1] == nhp
        if p.reshape(-1, nhp).shape[0] != 1:
            raise NotImplementedError("Sparse_GP: batched hyper-parameters are not supported")
        return np.array(p.reshape(nhp), dtype=np.float64)

    def _prior(self, hp):
        """(sigma^2, kdiag, the offsets): the noise variance, the constant prior variance of the stationary part (what
        Exact_GP._kss_diag forms, without its noise) and (terms, noise offsets)."""
        return _prior_of(self.cov, self._x.shape[-1], hp)

    def _buf(self, name, *shape, zero=False):
        """Device scratch kept per name and shape (a ragged last chunk has buffers of its own): one evaluation after the other runs on
        the stream, so one set serves them all."""
        t = self._bufs.get((name, shape))
        if t is None:
            t = self._bufs[(name, shape)] = get_ops().empty(*shape, dtype=torch.float64)
        if zero:
            t.zero_()
        return t

    # ---- the bound --------------------------------------------------------------------------
    def _build_chunk(self, ops, spec, hpd, zd, xd, yd, s, nc, m, ma):
        """A_c = [k(z, x_c); y_c^T; 0] as [m_aug, pad(nc)] (the cross build zeroes the padding)."""
        a = self._buf("chunk", ma, pad_to(nc))
        ops.kernel_build(spec, hpd, zd, xd[s: s + nc], a)
        a[m, :nc] = yd[s: s + nc]
        return a

    def _evaluate(self, hp: ndarray, want_grad: bool, keep: bool, want_zgrad: bool = False, z: ndarray = None):
        """One evaluation of the bound at the host vector hp: (loss, grad | None); keep: leave the prediction state behind.  Everything
        is enqueued before the ONE synchronisation that reads the status words and the scalars.  z: inducing inputs [m, d] (host) to
        evaluate at in place of the model's own, which stay as they are.  want_zgrad (with want_grad): the gradient comes back packed,
        concat(dL/dhp [nhp], dL/dz [m d]) -- the z part accumulated on the device by pg_kernel_xgrad from the weights the
        hyper-parameter gradient forms anyway, and carried by the same transfer."""
        assert want_grad or not want_zgrad, "the z-gradient shares the weights of the hyper-parameter gradient"
        assert z is None or not keep, "the prediction state belongs to the model's own z"
        if self._whitened:
            return self._evaluate_whitened(hp, want_grad, keep, want_zgrad, z)
        ops = get_ops()
        xd, yd, zd = self._device_data()
        n, d = xd.shape
        if z is not None:
            z = np.ascontiguousarray(z, dtype=np.float64)
            if z.ndim != 2 or z.shape[1] != d or z.shape[0] < 1:
                raise ValueError("Sparse_GP: z must be [m, %d] with m >= 1, got %s" % (d, z.shape))
            zd = ops.to_device(torch.from_numpy(z), torch.float64)
        m = zd.shape[0]
        ma = pad_to(m + 1)
        (sp,), nhp = spec_of(self.cov, d)
        spec = _stationary(sp)
        sig2, kdiag, tms, noise = self._prior(hp)
        hpd = ops.to_device(torch.from_numpy(hp), torch.float64)
        ch = int(_SPARSE_CHUNK)
        chunks = [(s, min(ch, n - s)) for s in range(0, n, ch)]
        info = torch.zeros(2, dtype=torch.int32, device=ops.device)
        res = [None]
        keepers = {}

        def enqueue():
            # pass 1: Phi_aug = sum_c A_c A_c^T (lower tiles; mirrored once at the end)
            phi = self._buf("phi", ma, ma, zero=True)
            a = None
            for s, nc in chunks:
                a = self._build_chunk(ops, spec, hpd, zd, xd, yd, s, nc, m, ma)
                ops.gemm_raw(_pass1_variant(ma), ma, ma, a.shape[1], 1.0, a, a, 1.0, phi, tri=1)
            ops.symmetrize(phi, ma)
            phm, b, yy = phi[:m, :m], phi[:m, m], phi[m, m]
            # the m x m algebra: Lu, Ls, the two inverses
            lu = self._buf("lu", ma, ma)
            ops.kernel_build(spec, hpd, zd, None, lu, jitter=JITTER)       # Kuu + JITTER I, identity in the padding
            ls = self._buf("ls", ma, ma)
            ls.copy_(lu)
            ls[:m, :m].add_(phm, alpha=1.0 / sig2)                          # Sigma
            invd = self._buf("invd", 2, ops.potrf_worksize(ma, torch.float64))
            minv = self._buf("minv", ma, ma)
            kuui, sgi = (self._buf("kuui", ma, ma), self._buf("sgi", ma, ma)) if not keep else (ops.empty(ma, ma), ops.empty(ma, ma))
            for i, (fac, inv) in enumerate(((lu, kuui), (ls, sgi))):
                ops.potrf(fac, invd[i], info[i: i + 1])
                ops.trtri(fac, invd[i], minv)
                ops.lauum(minv, inv)
                ops.symmetrize(inv, ma)
            ldu = lu.diagonal()[:m].log().sum()
            lds = ls.diagonal()[:m].log().sum()
            # c = Sigma^-1 b by substitution against Ls: cond(Sigma) is cond(Kuu) times n / sigma^2, and b^T c cancels against y^T y in the
            # loss -- c from the explicit inverse costs the loss three digits (measured: 5e-10 against 3e-13 at cond(Sigma) = 1e7)
            bvec = self._buf("bvec", ma, zero=True)
            bvec[:m] = b
            cvec = self._buf("cvec", ma)
            ops.potrs_vec(ls, invd[1], bvec, cvec)
            c = cvec[:m].clone()
            kp = self._buf("kphi", ma, ma)
            ops.gemm_raw(_lib.GEMM_NN, ma, ma, ma, 1.0, kuui, phi, 0.0, kp)      # Kuu^-1 Phi_aug
            tr_sp = (sgi[:m, :m] * phm).sum() if want_grad else ldu.new_zeros(())      # tr(Sigma^-1 Phi): both symmetric
            scal = [ldu, lds, yy, (b * c).sum(), tr_sp, kp[:m, :m].diagonal().sum(), (c * (phm * c).sum(1)).sum()]
            grad = ops.zeros(nhp, dtype=torch.float64)
            if want_grad:
                g = self._buf("guu", ma, ma)
                ops.gemm_raw(_lib.GEMM_NN, ma, ma, ma, 1.0, kp, kuui, 0.0, g)     # Kuu^-1 Phi Kuu^-1 in [:m, :m]
                cc = torch.outer(c, c)
                gm = g[:m, :m]
                gm.mul_(0.5 / sig2).add_(sgi[:m, :m], alpha=0.5).sub_(kuui[:m, :m], alpha=0.5).add_(cc, alpha=0.5 / sig2 ** 2)
                work = self._buf("gwork", max(1, ops.kernel_cross_grad_worksize(m, max(m, min(ch, n)), nhp)))
                ops.kernel_cross_grad(spec, hpd, zd, zd, g, grad, accumulate=False, work=work)
                gz = None
                if want_zgrad:      # 2 sum_j G_uu[i][j] dk(z_i, z_j)/dz_i: z_i enters row i and column i of the symmetric G_uu
                    gz = self._buf("gz", m, d)
                    ops.kernel_xgrad(spec, hpd, zd, zd, b=g[:m], out_b=gz)
                    gz.mul_(2.0)
                mw = self._buf("mw", ma, ma, zero=True)                           # [M | -c / sigma^4 | 0], zero rows below m
                mw[:m, :m].add_(sgi[:m, :m], alpha=1.0 / sig2).sub_(kuui[:m, :m], alpha=1.0 / sig2).add_(cc, alpha=1.0 / sig2 ** 3)
                mw[:m, m] = c * (-1.0 / sig2 ** 2)
                for s, nc in chunks:       # pass 2: rebuild A_c (one chunk: it is still there), W_c = [M | -c / sigma^4] A_c, contract
                    if len(chunks) > 1:
                        a = self._build_chunk(ops, spec, hpd, zd, xd, yd, s, nc, m, ma)
                    w = self._buf("w", ma, a.shape[1])
                    ops.gemm_raw(_lib.GEMM_NN, ma, a.shape[1], ma, 1.0, mw, a, 0.0, w)
                    ops.kernel_cross_grad(spec, hpd, zd, xd[s: s + nc], w, grad, accumulate=True, work=work)
                    if want_zgrad:         # + sum_j G_uf,c[i][j] dk(z_i, x_j)/dz_i: the rows [:m] of the W_c the chunk already holds
                        ops.kernel_xgrad(spec, hpd, zd, xd[s: s + nc], b=w[:m], out_b=gz, accumulate=True)
                if want_zgrad:
                    grad = torch.cat([grad, gz.reshape(-1)])
            if keep:
                keepers.update(c=c, kuui=kuui, sgi=sgi, hpd=hpd)
            res[0] = torch.cat([torch.stack(scal), grad]).cpu().numpy()          # the one sync + transfer

        for st in _checked(enqueue, lambda: info.tolist()):
            if st:
                raise _lin_alg_error(st, " -- Kuu or Sigma of the inducing points")
        ldu, lds, yy, bc, tr_sp, tr_kp, cpc = res[0][:7]
        t = n * kdiag - tr_kp
        loss = lds - ldu + 0.5 * n * math.log(sig2) + yy / (2 * sig2) - bc / (2 * sig2 ** 2) + 0.5 * n * math.log(2 * math.pi) + t / (2 * sig2)
        grad = None
        if want_grad:
            grad = res[0][7:].copy()
            dsig2 = (-tr_sp / (2 * sig2 ** 2) + n / (2 * sig2) - yy / (2 * sig2 ** 2) + bc / sig2 ** 3 - cpc / (2 * sig2 ** 4)
                     - t / (2 * sig2 ** 2))
            for o in noise:
                grad[o] = 2.0 * hp[o] * dsig2
            for _, _, offs in tms:          # the trace of Kff: n / (2 sigma^2) dkdiag/dsigma_c (a product term: 2 term / sigma_c)
                for o in offs:
                    others = np.prod([hp[o2] ** 2 for o2 in offs if o2 != o])
                    grad[o] += n / (2 * sig2) * 2.0 * hp[o] * others
        if keep:
            self._state = dict(keepers, m=m, ma=ma, sig2=sig2, kss=kdiag + sig2, spec=spec, full_spec=sp)
        return np.array(loss), grad

    def _evaluate_whitened(self, hp: ndarray, want_grad: bool, keep: bool, want_zgrad: bool = False, z: ndarray = None):
        """_evaluate for a whitened model (module docstring, "Whitened evaluation"): the same contract, one synchronisation, and
        O(m^2 + m chunk) memory with one chunk-sized buffer more than the unwhitened passes (A_c, V_c and W_c; the product
        [M~ | -c~ / sigma^4] V_c lands in A_c's buffer).  Li = Lu^-1 comes from pg_trtri, which leaves scratch in the blocks above
        the diagonal: every product with it is a K-range product of the GEMM core that never reads them."""
        ops = get_ops()
        xd, yd, zd = self._device_data()
        n, d = xd.shape
        if z is not None:
            z = np.ascontiguousarray(z, dtype=np.float64)
            if z.ndim != 2 or z.shape[1] != d or z.shape[0] < 1:
                raise ValueError("Sparse_GP: z must be [m, %d] with m >= 1, got %s" % (d, z.shape))
            zd = ops.to_device(torch.from_numpy(z), torch.float64)
        m = zd.shape[0]
        ma = pad_to(m + 1)
        (sp,), nhp = spec_of(self.cov, d)
        spec = _stationary(sp)
        sig2, kdiag, tms, noise = self._prior(hp)
        hpd = ops.to_device(torch.from_numpy(hp), torch.float64)
        ch = int(_SPARSE_CHUNK)
        chunks = [(s, min(ch, n - s)) for s in range(0, n, ch)]
        info = torch.zeros(2, dtype=torch.int32, device=ops.device)
        res = [None]
        keepers = {}

        def whiten(li, a):
            """V_c = Li A_c: the rows [:m] whitened, row m (y_c) and the zero rows below it unchanged (Li is the identity there)."""
            v = self._buf("v", ma, a.shape[1])
            ops.trmm_lower(li, a, v)
            return v

        def enqueue():
            # Lu and Li = Lu^-1 first: every chunk is whitened before it is accumulated
            lu = self._buf("lu", ma, ma)
            ops.kernel_build(spec, hpd, zd, None, lu, jitter=JITTER)       # Kuu + JITTER I, identity in the padding
            invd = self._buf("invd", 2, ops.potrf_worksize(ma, torch.float64))
            ops.potrf(lu, invd[0], info[0:1])
            li = self._buf("li", ma, ma) if not keep else ops.empty(ma, ma)
            ops.trtri(lu, invd[0], li)
            # pass 1: Psi_aug = sum_c V_c V_c^T (lower tiles; mirrored once at the end): Psi, b~ = Li b (row m) and y^T y ([m, m])
            psi = self._buf("psi", ma, ma, zero=True)
            v = None
            for s, nc in chunks:
                v = whiten(li, self._build_chunk(ops, spec, hpd, zd, xd, yd, s, nc, m, ma))
                ops.gemm_raw(_pass1_variant(ma), ma, ma, v.shape[1], 1.0, v, v, 1.0, psi, tri=1)
            ops.symmetrize(psi, ma)
            psm, b, yy = psi[:m, :m], psi[:m, m], psi[m, m]
            # D = I + Psi / sigma^2 (identity in the padding as well), Ld, c~ = D^-1 b~ by substitution against Ld
            ld = self._buf("ld", ma, ma, zero=True)
            ld.diagonal().fill_(1.0)
            ld[:m, :m].add_(psm, alpha=1.0 / sig2)
            ops.potrf(ld, invd[1], info[1:2])
            ldd = ld.diagonal()[:m].log().sum()
            bvec = self._buf("bvec", ma, zero=True)
            bvec[:m] = b
            cvec = self._buf("cvec", ma)
            ops.potrs_vec(ld, invd[1], bvec, cvec)
            c = cvec[:m].clone()
            di = None
            if want_grad or keep:                                           # D^-1 (the loss alone does not need it)
                minv = self._buf("minv", ma, ma)
                di = self._buf("dinv", ma, ma)
                ops.trtri(ld, invd[1], minv)
                ops.lauum(minv, di)
                ops.symmetrize(di, ma)
            tr_di = di[:m, :m].diagonal().sum() if want_grad else ldd.new_zeros(())
            scal = [ldd, yy, (b * c).sum(), tr_di, psm.diagonal().sum(), (c * (psm * c).sum(1)).sum()]
            grad = ops.zeros(nhp, dtype=torch.float64)
            if want_grad:
                cc = torch.outer(c, c)
                # G_uu = 1/2 Li^T [(D^-1 - I) + c~ c~^T / sigma^4 + Psi / sigma^2] Li, back in original coordinates
                xm = self._buf("xm", ma, ma, zero=True)
                xm[:m, :m].add_(di[:m, :m]).add_(cc, alpha=1.0 / sig2 ** 2).add_(psm, alpha=1.0 / sig2)
                xm[:m, :m].diagonal().sub_(1.0)
                t = self._buf("minv", ma, ma)                               # (D^-1 is formed: the inverse factor's buffer is free)
                ops.gemm_raw(_lib.GEMM_NN, ma, ma, ma, 1.0, xm, li, 0.0, t, klo=2)      # X Li: Li's rows from the tile column down
                g = self._buf("guu", ma, ma)
                ops.gemm_raw(_lib.GEMM_TN, ma, ma, ma, 0.5, li, t, 0.0, g, klo=1)       # 1/2 Li^T (X Li)
                work = self._buf("gwork", max(1, ops.kernel_cross_grad_worksize(m, max(m, min(ch, n)), nhp)))
                ops.kernel_cross_grad(spec, hpd, zd, zd, g, grad, accumulate=False, work=work)
                gz = None
                if want_zgrad:      # 2 sum_j G_uu[i][j] dk(z_i, z_j)/dz_i: z_i enters row i and column i of the symmetric G_uu
                    gz = self._buf("gz", m, d)
                    ops.kernel_xgrad(spec, hpd, zd, zd, b=g[:m], out_b=gz)
                    gz.mul_(2.0)
                mw = self._buf("mw", ma, ma, zero=True)                           # [M~ | -c~ / sigma^4 | 0], zero rows below m
                mw[:m, :m].add_(di[:m, :m], alpha=1.0 / sig2).add_(cc, alpha=1.0 / sig2 ** 3)
                mw[:m, :m].diagonal().sub_(1.0 / sig2)
                mw[:m, m] = c * (-1.0 / sig2 ** 2)
                for s, nc in chunks:       # pass 2: V_c again (one chunk: it is still there), W_c = Li^T ([M~ | -c~ / sigma^4] V_c), contract
                    if len(chunks) > 1:
                        v = whiten(li, self._build_chunk(ops, spec, hpd, zd, xd, yd, s, nc, m, ma))
                    u = self._buf("chunk", ma, v.shape[1])                        # A_c is spent once V_c stands
                    ops.gemm_raw(_lib.GEMM_NN, ma, v.shape[1], ma, 1.0, mw, v, 0.0, u)
                    w = self._buf("w", ma, v.shape[1])
                    ops.gemm_raw(_lib.GEMM_TN, ma, v.shape[1], ma, 1.0, li, u, 0.0, w, klo=1)      # Li^T (.): Li's rows from the tile row down
                    ops.kernel_cross_grad(spec, hpd, zd, xd[s: s + nc], w, grad, accumulate=True, work=work)
                    if want_zgrad:
                        ops.kernel_xgrad(spec, hpd, zd, xd[s: s + nc], b=w[:m], out_b=gz, accumulate=True)
                if want_zgrad:
                    grad = torch.cat([grad, gz.reshape(-1)])
            if keep:
                em = ops.zeros(ma, ma, dtype=torch.float64)                       # [E | c~ / sigma^2 | 0], E = I - D^-1
                em[:m, :m].sub_(di[:m, :m])
                em[:m, :m].diagonal().add_(1.0)
                em[:m, m] = c / sig2
                keepers.update(c=c, li=li, bm=em, hpd=hpd)
            res[0] = torch.cat([torch.stack(scal), grad]).cpu().numpy()          # the one sync + transfer

        for st in _checked(enqueue, lambda: info.tolist()):
            if st:
                raise _lin_alg_error(st, " -- Kuu of the inducing points, or D = I + Psi / sigma^2")
        ldd, yy, bc, tr_di, tr_psi, cpc = res[0][:6]
        t = n * kdiag - tr_psi
        loss = ldd + 0.5 * n * math.log(sig2) + yy / (2 * sig2) - bc / (2 * sig2 ** 2) + 0.5 * n * math.log(2 * math.pi) + t / (2 * sig2)
        grad = None
        if want_grad:
            grad = res[0][6:].copy()
            # tr(Sigma^-1 Phi) = tr(D^-1 Psi) = sigma^2 (m - tr D^-1), b^T c = b~^T c~, c^T Phi c = c~^T Psi c~
            dsig2 = (-(m - tr_di) / (2 * sig2) + n / (2 * sig2) - yy / (2 * sig2 ** 2) + bc / sig2 ** 3 - cpc / (2 * sig2 ** 4)
                     - t / (2 * sig2 ** 2))
            for o in noise:
                grad[o] = 2.0 * hp[o] * dsig2
            for _, _, offs in tms:          # the trace of Kff: n / (2 sigma^2) dkdiag/dsigma_c (a product term: 2 term / sigma_c)
                for o in offs:
                    others = np.prod([hp[o2] ** 2 for o2 in offs if o2 != o])
                    grad[o] += n / (2 * sig2) * 2.0 * hp[o] * others
        if keep:
            self._state = dict(keepers, m=m, ma=ma, sig2=sig2, kss=kdiag + sig2, spec=spec, full_spec=sp)
        return np.array(loss), grad

    def update(self) -> None:
        self._device_data()                  # first: an in-place edit of x / y / z (version bump) marks the model dirty here
        if self.need_upd:
            self._state = None
            self._evaluate(self._hp_host(), want_grad=False, keep=True)
            ops = get_ops()
            st = self._state
            if not self._whitened:          # (the whitened evaluation leaves its own: Li and [E | c~ / sigma^2 | 0])
                m, ma = st["m"], st["ma"]
                bm = ops.zeros(ma, ma, dtype=torch.float64)       # [Kuu^-1 - Sigma^-1 | c / sigma^2 | 0]: variance and mean from one product
                bm[:m, :m].add_(st["kuui"][:m, :m]).sub_(st["sgi"][:m, :m])
                bm[:m, m] = st["c"] / st["sig2"]
                st["bm"] = bm
            self.need_upd = False
        return None

    # ---- prediction -------------------------------------------------------------------------
    def predict(self, xp: Tensor, var: str = "full") -> Sequence[Tensor]:
        """[mean, var | covariance | NotImplemented] of y* at xp [q, d]: mean = Ksu c / sigma^2, cov = Kss - Ksu (Kuu^-1 - Sigma^-1) Kus
        with the noise on the diagonal of Kss.  var="diag" chunks the test points; var="full" takes them in one piece.  A whitened
        model whitens every chunk of test points, w = Ksu Li^T, and forms mean = w c~ / sigma^2, cov = Kss - (w E) w^T."""
        if torch.is_grad_enabled() and isinstance(xp, Tensor) and xp.requires_grad:
            raise NotImplementedError("Sparse_GP.predict is not differentiable through autograd; predict_grad returns the derivatives in the "
                                      "test points")
        return self._predict(xp, var)[:2]

    def predict_grad(self, xp: Tensor, var: str = "diag") -> Sequence[Tensor]:
        """[mean, var, dmean, dvar] (var="diag") or [mean, dmean] (var="none") without autograd, Exact_GP.predict_grad's contract:
        dmean[p, :] = d mean_p / d xp_p = sum_i (c_i / sigma^2) dk(xp_p, z_i)/dxp_p and dvar[p, :] = d var_p / d xp_p =
        -2 sum_i V_pi dk(xp_p, z_i)/dxp_p with V = Ksu (Kuu^-1 - Sigma^-1), both [q, d] float64 on xp's device.  Mean and variance are
        `predict`'s own (same path, same bits); V is the product that path forms, and both derivatives come out of one pg_kernel_xgrad
        call per chunk of test points.  Matern-1/2: a test point on an inducing point contributes 0 for that pair.
        A whitened model: u = Li^T c~ / sigma^2 and V = (w E) Li, w = Ksu Li^T whitened per chunk."""
        if var not in ("diag", "none"):
            raise ValueError("predict_grad: var must be 'diag' or 'none', got %r" % (var,))
        with torch.no_grad():
            mean, vr, dmean, dvar = self._predict(xp, var, grads=True)
        return [mean, dmean] if var == "none" else [mean, vr, dmean, dvar]

    @staticmethod
    def _whiten_rows(ops, li, kt, w):
        """w = kt Li^T: a chunk of test points [q_pad, m_aug] in whitened coordinates (column m and beyond stay zero)."""
        ops.trmm_lower_kt(li, kt, w)
        return w

    def _predict(self, xp: Tensor, var: str, grads: bool = False):
        """[mean, var | covariance | NotImplemented] and, for grads (not with var="full"), the two derivatives in the test points."""
        if xp.dim() != 2 or xp.shape[1] != self._x.shape[1]:
            raise NotImplementedError("Sparse_GP.predict: xp must be [q, %d] (no batches)" % self._x.shape[1])
        ops = get_ops()
        self.update()
        st = self._state
        m, ma, bm, spec, hpd = st["m"], st["ma"], st["bm"], st["spec"], st["hpd"]
        li = st.get("li")                    # a whitened model: every kt below is followed by w = kt Li^T, which takes its place
        _, _, zd = self._device_data()
        xpd = ops.to_device(xp, torch.float64)
        q = xpd.shape[0]
        want = var if var in ("full", "diag") else "none"
        mean = ops.empty(q, dtype=torch.float64)
        if want == "full":
            qp = pad_to(q)
            kt = ops.empty(qp, ma, dtype=torch.float64)
            v = ops.empty(qp, ma, dtype=torch.float64)
            cov = ops.empty(qp, qp, dtype=torch.float64)
            ops.kernel_build(spec, hpd, xpd, zd, kt)                                   # Ksu, test-point-major; zero in column m and beyond
            if li is not None:
                kt = self._whiten_rows(ops, li, kt, ops.empty(qp, ma, dtype=torch.float64))
            ops.gemm_raw(_lib.GEMM_NN, qp, ma, ma, 1.0, kt, bm, 0.0, v)                # [Ksu (Kuu^-1 - Sigma^-1) | mean | 0]
            mean.copy_(v[:q, m])
            ops.kernel_build(st["full_spec"], hpd, xpd, None, cov)                     # Kss incl. sigma_n^2, identity in the padding
            ops.gemm_raw(_lib.GEMM_NT, qp, qp, ma, -1.0, v, kt, 1.0, cov, tri=1)       # (column m of kt is zero: the mean does not enter)
            ops.symmetrize(cov, qp)                                                    # the upper triangle is the mirror: exactly symmetric
            return [mean.to(xp.device), cov[:q, :q].contiguous().to(xp.device)]
        vr = ops.empty(q, dtype=torch.float64) if want == "diag" else None
        dmean = dvar = u = None
        if grads:
            d = xpd.shape[1]
            dmean = ops.empty(q, d, dtype=torch.float64)
            dvar = ops.empty(q, d, dtype=torch.float64) if want == "diag" else None
            u = st.get("u")
            if u is None and li is None:
                u = st["u"] = st["c"] / st["sig2"]
            elif u is None:                 # Li^T c~ / sigma^2: the mean's weights back in original coordinates
                cs = ops.zeros(ma, dtype=torch.float64)
                cs[:m] = st["c"] / st["sig2"]
                u = st["u"] = ops.empty(ma, dtype=torch.float64)
                ops.trmv(li, cs, u, 1, ops.empty((ma // 256) * ma, dtype=torch.float64))
        for s in range(0, q, _CHUNK):
            xq = xpd[s: s + _CHUNK]
            qc = xq.shape[0]
            qp = pad_to(qc)
            kt = self._buf("pkt", qp, ma)
            v = self._buf("pv", qp, ma)
            ops.kernel_build(spec, hpd, xq, zd, kt)
            if li is not None:
                kt = self._whiten_rows(ops, li, kt, self._buf("pw", qp, ma))
            ops.gemm_raw(_lib.GEMM_NN, qp, ma, ma, 1.0, kt, bm, 0.0, v)
            mean[s: s + qc] = v[:qc, m]
            if want == "diag":
                vr[s: s + qc] = st["kss"] - (v[:qc, :m] * kt[:qc, :m]).sum(1)
            if grads and li is not None and want == "diag":      # V = (w E) Li: Li's rows from the tile column down (v's column m meets zeros)
                vo = self._buf("pvo", qp, ma)
                ops.gemm_raw(_lib.GEMM_NN, qp, ma, ma, 1.0, v, li, 0.0, vo, klo=2)
                v = vo
            if grads:       # u = c / sigma^2 for the mean, B = V = columns [:m] of the product above for the variance: one pass for both
                ops.kernel_xgrad(spec, hpd, xq, zd, u=u, b=v[:qc] if want == "diag" else None, out_u=dmean[s: s + qc],
                                 out_b=dvar[s: s + qc] if want == "diag" else None)
        out = [mean.to(xp.device), vr.to(xp.device) if want == "diag" else NotImplemented]
        if grads:
            out += [dmean.to(xp.device), dvar.mul_(-2.0).to(xp.device) if want == "diag" else None]
        return out


class VFE(_MemoLoss):
    """The negative collapsed variational bound of a Sparse_GP as a training objective with MLE's protocol (`CG(VFE(model))`).

    train_z=True trains the inducing inputs with the hyper-parameters: the parameter vector is concat(hp [nhp], z.reshape(-1) [m d]),
    `loss` / `grad` / `loss_and_grad` take and return that length and evaluate at the z inside the vector without assigning it to the
    model, and an optimiser starts from (model.params, model.z) and writes both back (`start_params` / `write_back`).  Every
    evaluation forms the gradient, so that `loss(p)` followed by `grad(p)` is one device evaluation through the memo.  z is
    unconstrained: no box, no reparametrisation.  Matern-1/2 has no derivative where an inducing input sits on a training point or on
    another inducing input; that pair contributes 0."""

    def __init__(self, model: Sparse_GP, train_z: bool = False) -> None:
        if not isinstance(model, Sparse_GP):
            raise TypeError("VFE is the loss of a Sparse_GP, got %s" % type(model).__name__)
        super().__init__(model)
        self._z_seen = None
        self.train_z = bool(train_z)

    # ---- the packed vector (train_z) --------------------------------------------------------
    def pack(self, hp, z) -> ndarray:
        """concat(hp [nhp], z.reshape(-1) [m d]) as a new host float64 vector."""
        as_np = lambda t: t.detach().cpu().numpy() if isinstance(t, Tensor) else np.asarray(t)      # noqa: E731
        return np.concatenate([as_np(hp).reshape(-1), as_np(z).reshape(-1)]).astype(np.float64)

    def unpack(self, params: ndarray):
        """(hp [nhp], z [m, d]) views of a packed vector; a vector of any other length than nhp + m d is a ValueError."""
        mdl = self.model
        (m, d), (_, nhp) = mdl._z.shape, spec_of(mdl.cov, mdl._x.shape[-1])
        p = np.asarray(params, dtype=np.float64)
        if p.ndim != 1 or p.size != nhp + m * d:
            raise ValueError("VFE(train_z=True) takes concat(hp [%d], z.reshape(-1) [%d x %d]) = %d entries, got shape %s"
                             % (nhp, m, d, nhp + m * d, p.shape))
        return p[:nhp], p[nhp:].reshape(m, d)

    def start_params(self) -> ndarray:
        if not self.train_z:
            return super().start_params()
        return self.pack(self.model.params, self.model.z)

    def write_back(self, x: ndarray) -> None:
        if not self.train_z:
            return super().write_back(x)
        dev = x.device if isinstance(x, Tensor) else "cpu"
        hp, z = self.unpack(x.detach().cpu().numpy() if isinstance(x, Tensor) else x)
        self.model.set_params(torch.tensor(hp))
        self.model.z = torch.tensor(z, dtype=torch.float64, device=dev)      # the setter marks the model dirty; the memo goes with it

    def _evaluate(self, params: ndarray, want_grad: bool):
        m = self.model
        if self.train_z:
            self.unpack(params)                              # a wrong length is refused before anything touches the device
            # every evaluation forms the gradient: loss(p) and then grad(p) at the same p -- get_learn_rate's order -- is ONE device
            # evaluation (with the plain loss the second call repeats both passes), and scipy's CG never asks for the loss alone
            want_grad = True
        # the memo's key holds x, y and the covariance: z, and which of the two evaluations the model runs, are this model's own
        token = (id(m._z), m._z._version, m._z_version, m.whitened)
        if token != self._z_seen:
            self._memo = None
            self._z_seen = token
        return super()._evaluate(params, want_grad)

    def _evaluate_device(self, params: ndarray, want_grad: bool, key=None, reuse_factor=False):
        m = self.model
        if self.train_z:
            hp, z = self.unpack(params)
            return m._evaluate(m._hp_host(hp), want_grad, keep=False, want_zgrad=want_grad, z=z)
        loss, grad = m._evaluate(m._hp_host(np.asarray(params, dtype=np.float64)), want_grad, keep=False)
        return loss, grad
