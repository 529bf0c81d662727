"""Matrix-free exact GP regression: Exact_GP's posterior from preconditioned conjugate gradients on the MI355X.  New, not in the
reference.

The same function as Exact_GP: A = k(x, x) + (sum sigma_n^2 + JITTER) I, alpha = A^-1 y, mean* = k(x*, x) alpha,
cov* = K** - K*^T A^-1 K* with the noise on the diagonal of K**.  A is never formed: every product A V is pg_kernel_matmul
(include/pygpr_hip_matmul.h), which evaluates the covariance from the point tiles inside the product.  Memory is O(n (rank + nrhs));
no n x n array exists at any time, so n is bounded by time, not by the three n x n matrices Exact_GP keeps.

Preconditioner.  The partial pivoted Cholesky factor of k(x, x) that greedy selection computes (`select_inducing`): with m = min(rank, n)
pivots z = x[piv], Lu = chol(k(z, z) + JITTER I) and L = k(x, z) Lu^-T (n x m, kept), P = L L^T + shift I and, by Woodbury with
C = shift I + L^T L (m x m, factored once),

    P^-1 r = (r - L C^-1 L^T r) / shift.

L is built in row chunks from cross builds and whitened per chunk like a Sparse_GP's test points; L^T L, L^T r and L u are products of
the GEMM core on padded buffers (zero rows and columns in the padding, the identity in C's).  rank = 0 is plain CG; a selection that
stops early (the residual variance fell below the jitter) leaves a preconditioner of that rank.

Solver.  `_solve` runs block PCG on A X = B: every column has its own step lengths -- device tensors, no host round trip -- and all
columns share one pg_kernel_matmul per iteration.  A column whose p^T A p or r^T z is zero (a zero or converged column) takes a zero
step.  Every `check_every` iterations the host reads one number, the largest ||r_c|| / ||b_c|| over the columns (a zero column counts
with ||b_c|| = 1), and stops at <= tol; the true residual b - A x is then formed once, and that is the figure reported.  Past max_iter:
`NotConverged`, and the model stays dirty.

Training.  MLE and LOO need the factor and refuse this model; `Stochastic_MLE` (pygpr_amd/stochastic.py) trains it through
`CG(Stochastic_MLE(model))`: the log-determinant by stochastic Lanczos quadrature on the coefficients `_solve(..., record=True)` keeps,
the gradient from the same probe solves through pg_kernel_lowrank_grad.  `VFE` on a Sparse_GP, or MLE on an Exact_GP of a subset, remain
the cheaper ways to a starting point.  Batched models, float32 and covariances longer than one pg_covspec are refused.

Derivatives.  `predict_grad` gives d mean / dx* and d var / dx* without autograd: both from pg_kernel_xgrad, the mean's
against alpha, the variance's against the block solve its value takes anyway.  `predict` itself stays closed to autograd.  The
derivative of a function sample, S right-hand sides at once, is pg_kernel_matmul_dx's (include/pygpr_hip_dmatmul.h).

Cached variances.  `variance_cache` builds a `VarianceCache` (pygpr_amd/varcache.py): a Galerkin projection of A^-1 onto a
block-Krylov space started from the preconditioner's factor, y and optional anchor points, built once from a handful of wide products;
every variance afterwards is one cross product and no solve, an upper bound of the exact variance, and with `bounds` it comes with a
certified lower bound whose |k*|^2 term is pg_kernel_rowsq (include/pygpr_hip_rowsq.h).  `predict` keeps its block solves.

Sampling.  `function_samples` draws posterior functions by pathwise conditioning (pygpr_amd/pathwise.py): one block solve
for all samples, then every evaluation is one cross product and one feature product.  A joint `sampler` stays refused.
"""
from typing import Sequence

import numpy as np
import torch
from numpy import ndarray
from torch import Tensor

from . import _lib
from ._ops import JITTER, get_ops, pad_to
from .covar import Covar, spec_of, terms
from .gpr import _CHUNK, GPR, _checked, _lin_alg_error
from .pathwise import FunctionSamples, _check_count, _checked_terms, draw_function_samples
from .sparse import _prior_of, _stationary, select_inducing
from .varcache import VarianceCache

_RHS_BLOCK = 64      # test points whose variance columns one block solve carries
_RHS_PAD = 128       # the GEMM core's column tile: every block of right-hand sides is a buffer of that many columns (or a multiple)
CHECK_EVERY = 10     # iterations between two reads of the residual


class NotConverged(torch.linalg.LinAlgError):
    """The conjugate gradients did not reach the tolerance within max_iter iterations.  `iterations`: how many were taken;
    `residual`: the largest ||r_c|| / ||b_c|| of the recurrence at that point."""

    def __init__(self, iterations: int, residual: float, tol: float) -> None:
        super().__init__("Iterative_GP: conjugate gradients stopped after %d iterations at relative residual %.3e (tol %.1e); raise "
                         "max_iter or rank, or loosen tol" % (iterations, residual, tol))
        self.iterations = int(iterations)
        self.residual = float(residual)


class Iterative_GP(GPR):
    """Exact GP regression without the n x n matrix: x [n, d], y [n] float64, params as Exact_GP's.  rank: pivots of the
    pivoted-Cholesky preconditioner (0: plain CG); tol: relative residual every solve is taken to; max_iter: iterations a solve may
    take before it raises NotConverged.  After update(), `cg_info` holds iterations, residual (the true one) and rank of the last
    solve."""

    _matrix_free = True      # MLE / LOO refuse such a model: they need the factor

    def __init__(self, x: Tensor, y: Tensor, cov: Covar, rank: int = 100, tol: float = 1e-8, max_iter: int = 1000) -> None:
        super().__init__(x, y, cov)
        if not (isinstance(rank, (int, np.integer)) and rank >= 0):
            raise ValueError("Iterative_GP: rank must be a non-negative integer, got %r" % (rank,))
        if not (tol > 0 and isinstance(max_iter, (int, np.integer)) and max_iter >= 1):
            raise ValueError("Iterative_GP: tol must be positive and max_iter a positive integer")
        self.rank, self.tol, self.max_iter = int(rank), float(tol), int(max_iter)
        self._check_data()
        passes, _ = spec_of(cov, x.shape[-1])
        if len(passes) != 1:
            raise NotImplementedError("Iterative_GP: covariances that need more than one pg_covspec pass are not supported")
        self.params: Tensor = cov.init_params(x)
        self._dev = None
        self._dev_key = None
        self._state = None
        self.cg_info = None
        self.need_upd = True

    # ---- data -------------------------------------------------------------------------------
    @property
    def dtype(self):
        return torch.float64

    def _data_changed(self) -> None:
        self._dev = None
        self._state = None
        self.need_upd = True

    def _check_data(self) -> None:
        x, y = self._x, self._y
        for name, t in (("x", x), ("y", y)):
            if t.dtype != torch.float64:
                raise TypeError("Iterative_GP computes in float64 only (the solver's tolerance is below single precision); %s is %s"
                                % (name, t.dtype))
        if x.dim() != 2 or y.dim() != 1:
            raise NotImplementedError("Iterative_GP: batched models are not supported (x [n, d], y [n])")
        if y.shape[0] != x.shape[0]:
            raise ValueError("Iterative_GP: x holds %d points, y %d values" % (x.shape[0], y.shape[0]))

    def _device_data(self):
        """(x, y) on the device, uploaded once per (tensor identity, version)."""
        key = tuple(v for t in (self._x, self._y) for v in (id(t), t._version))
        if self._dev is None or self._dev_key != key:
            self._check_data()
            ops = get_ops()
            self._dev = tuple(ops.to_device(t, torch.float64) for t in (self._x, self._y))
            self._dev_key = key
            self._state = None
            self.need_upd = True
        return self._dev

    def _hp_host(self) -> ndarray:
        p = self.params
        p = p.detach().cpu().numpy() if isinstance(p, Tensor) else np.asarray(p)
        if p.dtype != np.float64:
            raise TypeError("Iterative_GP computes in float64 only; params is %s" % p.dtype)
        _, nhp = spec_of(self.cov, self._x.shape[-1])
        assert p.shape[-1] == nhp
        if p.reshape(-1, nhp).shape[0] != 1:
            raise NotImplementedError("Iterative_GP: batched hyper-parameters are not supported")
        return np.array(p.reshape(nhp), dtype=np.float64)

    # ---- the preconditioner -----------------------------------------------------------------
    def _preconditioner(self, ops, hp, hpd, spec, shift, xd):
        """(L [n_pad, m_pad], the factor of C = shift I + L^T L, its workspace, m), or None for rank 0."""
        n, d = xd.shape
        tms, _, _ = terms(self.cov, d)
        want = min(self.rank, n)
        if want == 0 or not tms:
            return None
        piv = select_inducing(xd, self.cov, hp, want).index          # (one synchronisation: the count)
        m = int(piv.shape[0])
        if m == 0:
            return None
        zd = xd[piv].contiguous()
        ma, npad = pad_to(m), pad_to(n)
        info = torch.zeros(2, dtype=torch.int32, device=ops.device)
        out = {}

        def enqueue():
            lu = ops.empty(ma, ma)
            ops.kernel_build(spec, hpd, zd, None, lu, jitter=JITTER)       # k(z, z) + JITTER I, identity in the padding
            invd = ops.empty(2, ops.potrf_worksize(ma, torch.float64))
            ops.potrf(lu, invd[0], info[0:1])
            li = ops.empty(ma, ma)
            ops.trtri(lu, invd[0], li)
            lmat = ops.empty(npad, ma)
            for s in range(0, n, _CHUNK):                                  # L = k(x, z) Lu^-T, chunk by chunk straight into its rows
                nc = min(_CHUNK, n - s)
                rows = pad_to(nc)
                kt = ops.empty(rows, ma)
                ops.kernel_build(spec, hpd, xd[s: s + nc], zd, kt)         # zero in the padding: the rows behind n, the columns behind m
                ops.trmm_lower_kt(li, kt, lmat[s: s + rows])
            c = ops.empty(ma, ma)
            ops.gemm_raw(_lib.GEMM_TN_64 if ma <= 2048 else _lib.GEMM_TN, ma, ma, npad, 1.0, lmat, lmat, 0.0, c)
            dg = c.diagonal()
            dg[:m].add_(shift)
            dg[m:].fill_(1.0)
            ops.potrf(c, invd[1], info[1:2])
            out.update(L=lmat, C=c, invd=invd[1], m=m, ma=ma)

        for st in _checked(enqueue, lambda: info.tolist()):
            if st:
                raise _lin_alg_error(st, " -- the pivots' covariance or the preconditioner's capacitance matrix")
        return out

    @staticmethod
    def _apply_preconditioner(ops, pre, shift, r, z):
        """z = P^-1 r on [n_pad, cols] buffers (cols a multiple of _RHS_PAD; zero rows and columns stay zero)."""
        if pre is None:
            z.copy_(r)
            return
        lmat, ma = pre["L"], pre["ma"]
        npad, cols = r.shape
        t = ops.empty(ma, cols)
        ops.gemm_raw(_lib.GEMM_TN_64, ma, cols, npad, 1.0, lmat, r, 0.0, t)       # L^T r
        u = ops.potrs(pre["C"], pre["invd"], t)                                    # C^-1 L^T r
        z.copy_(r)
        ops.gemm_raw(_lib.GEMM_NN, npad, cols, ma, -1.0, lmat, u, 1.0, z)          # r - L u
        z.mul_(1.0 / shift)

    # ---- the solver -------------------------------------------------------------------------
    def _solve(self, ops, st, b, nrhs, record=False, freeze=False):
        """X with A X = B for the first nrhs columns of the zero-padded buffer b [n_pad, cols]: (x buffer, iterations, true residual).
        Raises NotConverged past max_iter.  record: a fourth result, what the stochastic log-determinant reads from the recurrence --
        `z0`, the first preconditioned residual P^-1 B (a device buffer like b), and on the host `step`, `beta` and `rz` [iterations, nrhs]
        (the step lengths, the betas and r^T z after each step) with `rz0` [nrhs], r^T z before the first.  They are kept as device
        tensors while the solve runs and come over in one transfer at its end.  freeze: a column that meets the tolerance at a check
        takes zero steps from then on, so what it converges to does not depend on the columns it shares the solve with (function
        samples: sample s is the same whatever n_samples)."""
        xd, hpd, spec, shift, pre = st["x"], st["hpd"], st["full_spec"], st["shift"], st["pre"]
        n = xd.shape[0]
        bv = b[:n, :nrhs]
        work = st.get("work")
        x = torch.zeros_like(b)
        r = b.clone()
        z = torch.zeros_like(b)
        ap = torch.zeros_like(b)
        xv, rv, zv, apv = x[:n, :nrhs], r[:n, :nrhs], z[:n, :nrhs], ap[:n, :nrhs]
        self._apply_preconditioner(ops, pre, shift, r, z)
        p = z.clone()
        pv = p[:n, :nrhs]
        rz = (rv * zv).sum(0)
        if record:
            z0, rz0, steps, betas, rzs = z.clone(), rz, [], [], []
        bn = bv.norm(dim=0)
        bn = torch.where(bn == 0, torch.ones_like(bn), bn)
        zero = torch.zeros_like(rz)
        active = torch.ones_like(rz, dtype=torch.bool) if freeze else None
        it, res = 0, float("inf")
        while it < self.max_iter:
            ops.kernel_matmul(spec, hpd, xd, None, pv, out=apv, jitter=JITTER, work=work)
            pap = (pv * apv).sum(0)
            step = torch.where((pap != 0) & (rz != 0), rz / pap, zero)
            if freeze:
                step = torch.where(active, step, zero)
            xv.addcmul_(pv, step)
            rv.addcmul_(apv, -step)
            self._apply_preconditioner(ops, pre, shift, r, z)
            rz_new = (rv * zv).sum(0)
            beta = torch.where(rz != 0, rz_new / rz, zero)
            pv.mul_(beta).add_(zv)
            rz = rz_new
            it += 1
            if record:
                steps.append(step)
                betas.append(beta)
                rzs.append(rz_new)
            if it % CHECK_EVERY == 0 or it == self.max_iter:
                resc = rv.norm(dim=0) / bn
                if freeze:                                                 # (a frozen column's r stands still: it keeps the figure it froze at)
                    active = active & (resc > self.tol)
                res = float(resc.max())                                    # the one synchronisation per CHECK_EVERY iterations
                if not res > self.tol:                                     # (a NaN residual ends the solve as well: it cannot improve)
                    break
        if not res <= self.tol:
            raise NotConverged(it, res, self.tol)
        ops.kernel_matmul(spec, hpd, xd, None, xv, out=apv, jitter=JITTER, work=work)
        true = float(((bv - apv).norm(dim=0) / bn).max())
        if record:
            rec = torch.stack(steps + betas + rzs + [rz0]).cpu().numpy()
            return x, it, true, dict(z0=z0, step=rec[:it], beta=rec[it: 2 * it], rz=rec[2 * it: 3 * it], rz0=rec[3 * it])
        return x, it, true

    # ---- fit --------------------------------------------------------------------------------
    def update(self) -> None:
        xd, yd = self._device_data()             # first: an in-place edit of x / y (version bump) marks the model dirty here
        if not self.need_upd:
            return None
        self._state = None
        ops = get_ops()
        n, d = xd.shape
        hp = self._hp_host()
        (sp,), _ = spec_of(self.cov, d)
        sig2, kdiag, _, _ = _prior_of(self.cov, d, hp)
        shift = sig2 + JITTER
        hpd = ops.to_device(torch.from_numpy(hp), torch.float64)
        spec = _stationary(sp)
        pre = self._preconditioner(ops, hp, hpd, spec, shift, xd)
        size = ops.kernel_matmul_worksize(n, n, _RHS_PAD)
        st = dict(x=xd, hpd=hpd, spec=spec, full_spec=sp, shift=shift, pre=pre, kss=kdiag + sig2,
                  work=ops.empty(size) if size > 0 else None)
        b = ops.zeros(pad_to(n), _RHS_PAD)
        b[:n, 0] = yd
        xs, its, res = self._solve(ops, st, b, 1)
        st["alpha"] = xs[:n, 0].clone()
        self.cg_info = dict(iterations=its, residual=res, rank=0 if pre is None else pre["m"])
        self._state = st
        self.need_upd = False
        return None

    @property
    def alpha(self) -> Tensor:
        """A^-1 y [n] of the fitted model, on x's device."""
        self.update()
        return self._state["alpha"].to(self._x.device)

    # ---- prediction -------------------------------------------------------------------------
    def _check_xp(self, xp, who):
        if xp.dim() != 2 or xp.shape[1] != self._x.shape[1]:
            raise NotImplementedError("Iterative_GP.%s: xp must be [q, %d] (no batches)" % (who, self._x.shape[1]))
        if xp.dtype != torch.float64:
            raise TypeError("Iterative_GP computes in float64 only; xp is %s" % xp.dtype)

    def _diag_variance(self, ops, st, xpd, dvar=None):
        """var [q] at the device points xpd: the test points in blocks of _RHS_BLOCK, each a block solve A S = k(x, xp_b) at the model's
        tol.  dvar [q, d]: also filled, dvar[p] = -2 sum_i S_ip dk(xp_p, x_i)/dxp_p from the same solution (pg_kernel_xgrad's B form
        on the n x 64 block, stored transposed) -- K** has a constant diagonal, so there is no other term."""
        xd, hpd, spec = st["x"], st["hpd"], st["spec"]
        n, q = xd.shape[0], xpd.shape[0]
        npad = pad_to(n)
        blk = int(_RHS_BLOCK)
        cols = pad_to(blk, _RHS_PAD)
        vr = ops.empty(q)
        for s in range(0, q, blk):
            qb = min(blk, q - s)
            ks = ops.empty(npad, cols)
            ops.kernel_build(spec, hpd, xd, xpd[s: s + qb], ks)            # k(x, xp_b), zero in the padding
            sol, _, _ = self._solve(ops, st, ks, qb)
            vr[s: s + qb] = st["kss"] - (ks[:n, :qb] * sol[:n, :qb]).sum(0)
            if dvar is not None:
                ops.kernel_xgrad(spec, hpd, xpd[s: s + qb], xd, b=sol[:n], out_b=dvar[s: s + qb], trans_b=True)
        if dvar is not None:
            dvar.mul_(-2.0)
        return vr

    def predict_grad(self, xp: Tensor, var: str = "diag") -> Sequence[Tensor]:
        """[mean, var, dmean, dvar] (var="diag") or [mean, dmean] (var="none") without autograd, Exact_GP.predict_grad's contract:
        dmean[p, :] = d mean_p / d xp_p and dvar[p, :] = d var_p / d xp_p, [q, d] float64 on xp's device.  Mean and variance are
        `predict`'s own (same path, same bits).  dmean is pg_kernel_xgrad's vector form against alpha (no q x n matrix; for ONE
        right-hand side that VALU pass is three times faster than pg_kernel_matmul_dx); the variance and its derivative
        share one block solve per _RHS_BLOCK test points, and var="none" solves nothing."""
        if var not in ("diag", "none"):
            raise ValueError("predict_grad: var must be 'diag' or 'none', got %r" % (var,))
        self._check_xp(xp, "predict_grad")
        ops = get_ops()
        self.update()
        st = self._state
        xd, hpd, spec = st["x"], st["hpd"], st["spec"]
        xpd = ops.to_device(xp.detach(), torch.float64)
        mean = ops.kernel_matmul(spec, hpd, xpd, xd, st["alpha"])
        dmean, _ = ops.kernel_xgrad(spec, hpd, xpd, xd, u=st["alpha"])
        if var == "none":
            return [mean.to(xp.device), dmean.to(xp.device)]
        dvar = ops.empty(xpd.shape[0], xd.shape[1])
        vr = self._diag_variance(ops, st, xpd, dvar)
        return [mean.to(xp.device), vr.to(xp.device), dmean.to(xp.device), dvar.to(xp.device)]

    def predict(self, xp: Tensor, var: str = "full") -> Sequence[Tensor]:
        """[mean, var | covariance | NotImplemented] of y* at xp [q, d]: the mean is one cross product against alpha (no q x n matrix);
        the variances take the test points in blocks of _RHS_BLOCK, each a block solve A S = k(x, xp_b) at the model's tol."""
        if torch.is_grad_enabled() and isinstance(xp, Tensor) and xp.requires_grad:
            raise NotImplementedError("Iterative_GP.predict is not differentiable through autograd; use an Exact_GP for derivatives in "
                                      "the test points")
        self._check_xp(xp, "predict")
        ops = get_ops()
        self.update()
        st = self._state
        xd, hpd, spec = st["x"], st["hpd"], st["spec"]
        n = xd.shape[0]
        npad = pad_to(n)
        xpd = ops.to_device(xp, torch.float64)
        q = xpd.shape[0]
        want = var if var in ("full", "diag") else "none"
        mean = ops.kernel_matmul(spec, hpd, xpd, xd, st["alpha"])
        if want == "none":
            return [mean.to(xp.device), NotImplemented]
        blk = int(_RHS_BLOCK)
        cols = pad_to(blk, _RHS_PAD)
        blocks = [(s, min(blk, q - s)) for s in range(0, q, blk)]

        def cross(s, qb):
            ks = ops.empty(npad, cols)
            ops.kernel_build(spec, hpd, xd, xpd[s: s + qb], ks)            # k(x, xp_b), zero in the padding
            return ks

        if want == "diag":
            return [mean.to(xp.device), self._diag_variance(ops, st, xpd).to(xp.device)]
        qp = pad_to(q)
        cov = ops.empty(qp, qp)
        ops.kernel_build(st["full_spec"], hpd, xpd, None, cov)              # K** incl. sigma_n^2, identity in the padding
        g = ops.empty(cols, cols)
        for j, (s, qb) in enumerate(blocks):                                # the lower block triangle, column of blocks by column
            ks = cross(s, qb)
            sol, _, _ = self._solve(ops, st, ks, qb)
            for s2, qb2 in blocks[j:]:
                k2 = ks if s2 == s else cross(s2, qb2)
                ops.gemm_raw(_lib.GEMM_TN_64, cols, cols, npad, 1.0, k2, sol, 0.0, g)      # k(x, xp_b2)^T S_b
                cov[s2: s2 + qb2, s: s + qb].sub_(g[:qb2, :qb])
        ops.symmetrize(cov, qp)                                             # the upper triangle is the mirror: exactly symmetric
        return [mean.to(xp.device), cov[:q, :q].contiguous().to(xp.device)]

    # ---- cached variances ------------------------------------------------------------------
    def variance_cache(self, steps: int = 2, anchors: Tensor = None, bounds: bool = True, max_columns: int = 4096) -> VarianceCache:
        """A VarianceCache of the fitted model (fits if dirty): the Galerkin projection of A^-1 onto span[B0, A B0, ..., A^steps B0],
        B0 = [L | y | k(X, anchors)] with L the preconditioner's factor and `anchors` [na, d] float64 points where the variance matters
        (their cross-covariance columns).  Its variances are upper bounds of the exact ones that tighten with steps and anchors;
        bounds=True also keeps A Q for the lower bound of `variance(xp, bounds=True)`, certified up to a stated rounding model.  A request whose
        (steps + 1) x (rank + 1 + na) columns exceed max_columns is a ValueError before any product.  The cache is a SNAPSHOT, like a
        FunctionSamples: later set_params or refits of the model do not change it.  NotConverged and a failed preconditioner
        propagate as from update(); a failed factorisation of the projected matrix raises like Exact_GP's."""
        return VarianceCache(self, steps, anchors, bounds, max_columns)

    # ---- function samples -------------------------------------------------------------------
    def function_samples(self, n_samples: int = 1, features: int = 1024, seed: int = 0, prior: bool = False) -> FunctionSamples:
        """n_samples functions drawn from the posterior by pathwise conditioning (pygpr_amd/pathwise.py), as a FunctionSamples to
        evaluate at any points: `features` frequencies per stationary component (twice as many features), all randomness from pg_randn
        at `seed`.  The samples are of the latent function (no observation noise).  One fit and, for every _RHS_BLOCK samples, one block
        solve at the model's tol -- each of the block's full width, whatever n_samples, and with columns frozen once converged, so that
        sample s does not depend on n_samples; NotConverged and a failed preconditioner propagate as from update().  prior=True: draws
        of the prior at the current params -- no fit, no solve."""
        if not isinstance(seed, (int, np.integer)):
            raise ValueError("Iterative_GP.function_samples: the seed must be an integer, got %r" % (seed,))
        _check_count("Iterative_GP.function_samples: n_samples", n_samples)
        _check_count("Iterative_GP.function_samples: features", features)
        _checked_terms(self.cov, self._x.shape[1])      # a kind without a spectral law is refused before anything is fitted
        if prior:      # (of x only the width is read)
            return draw_function_samples(self.cov, self._hp_host(), self._x, None, 0.0, n_samples, features, seed, None)
        ops = get_ops()
        self.update()
        st = self._state
        xd, yd = self._device_data()
        n = xd.shape[0]
        npad = pad_to(n)

        def solve(b):
            blk = int(_RHS_BLOCK)
            cols = pad_to(blk, _RHS_PAD)
            v = torch.empty_like(b)
            its, worst, count = 0, 0.0, 0
            for s in range(0, b.shape[1], blk):
                sb = min(blk, b.shape[1] - s)
                buf = ops.zeros(npad, cols)
                buf[:n, :sb] = b[:, s: s + sb]
                sol, it, res = self._solve(ops, st, buf, blk, freeze=True)      # the full width: zero columns take zero steps
                v[:, s: s + sb] = sol[:n, :sb]
                its, worst, count = max(its, it), max(worst, res), count + 1
            return v, dict(solves=count, iterations=its, residual=worst, rank=self.cg_info["rank"])

        return draw_function_samples(self.cov, self._hp_host(), xd, yd, st["shift"], n_samples, features, seed, solve)

    def sample(self, xp: Tensor, n_samples: int = 1, seed: int = 0, features: int = 1024, prior: bool = False) -> Tensor:
        """function_samples(n_samples, features, seed, prior)(xp): [n_samples, q] draws of the latent function at xp [q, d]."""
        return self.function_samples(n_samples, features, seed, prior)(xp)

    def sampler(self, xp: Tensor, **kwargs):
        raise NotImplementedError("Iterative_GP has no joint sampler (a q x q factor is what this model cannot afford); draw functions "
                                  "with function_samples(...) and evaluate them at xp")

    def predict_var(self, xp: Tensor, **kwargs: Tensor) -> Tensor:
        return self.predict(xp, var="diag")[1]

    def predict_covar(self, xp: Tensor, **kwargs: Tensor) -> Tensor:
        return self.predict(xp, var="full")[1]
