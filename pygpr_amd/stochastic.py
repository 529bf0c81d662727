"""Training a matrix-free model: the negative log marginal likelihood of an Iterative_GP from probe vectors.  New, not in the reference.

    NLML = 1/2 y^T alpha + 1/2 log|A| + n/2 log 2pi,   A = k(x, x) + (sum sigma_n^2 + JITTER) I,   alpha = A^-1 y

alpha is the model's block PCG solve.  The log-determinant is stochastic Lanczos quadrature read off that same solve: with the
preconditioner P = L L^T + shift I of the model's rank (log|P| = (n - m) log shift + log|C| exactly, from the factor of the capacitance
matrix C) and probes z_i ~ N(0, P),

    log|A| = log|P| + E[ z^T P^-1/2 log(P^-1/2 A P^-1/2) P^-1/2 z ],

and the quadratic form of a probe is (z^T P^-1 z) e_1^T log(T) e_1 with T the tridiagonal matrix of the PCG coefficients of its column:
T[j][j] = 1/a_j + b_{j-1}/a_{j-1}, T[j][j+1] = sqrt(b_j)/a_j (a: step lengths, b: betas).  The columns of a block solve share the
iteration count; a column's T is cut at the first step whose r^T z fell to tol^2 of its start -- what follows is rounding noise.

The gradient is sum_ij W_ij dK_ij/dtheta with W = 1/2 [ (1/t) sum_i (A^-1 z_i)(P^-1 z_i)^T - alpha alpha^T ], of rank t + 1 and never
formed: one pg_kernel_lowrank_grad call in its symmetric form (include/pygpr_hip_lowrank.h) on views into the solver's buffers, plus
2 sigma_n tr(W) for the noise entries on the host.  Both are by-products of ONE block solve of [y, z_1..z_t]; with the default 15 probes
that is one 16-column panel of pg_kernel_matmul per iteration.

The probes come from pg_randn at a fixed seed, so the loss is a deterministic function of (params, seed), which a line search needs.
Loss and gradient are separate estimators -- the gradient is not the derivative of the loss estimate -- and the pivots of the
preconditioner change discretely with the parameters: a line search stalls once the steps are of the size of that noise, near the
optimum.

The gradient in the training inputs (`grad_x`, `loss_and_grads`) comes from the same weight: both arguments of k carry x_i,
so dNLML/dx_ik = sum_j (W_ij + W_ji) dk(x_i, x_j)/dx_ik -- one pg_kernel_lowrank_xgrad call in its symmetric form
(include/pygpr_hip_lxgrad.h) on the same views U, V, after the same solve; noise and jitter have no derivative in x.  `grad_x` is an
estimator built from the same probes as `grad`: its data-fit part (the factor column of alpha) is exact to the solver's tol, its trace
part has the probes' variance, and it is not the derivative of the loss estimate either.  The pivots of the preconditioner change
discretely with x as well, so what holds for a line search in the parameters holds for one in the inputs.
"""
from typing import Tuple

import numpy as np
import torch
from numpy import ndarray

from . import _lib
from ._ops import JITTER, get_ops, pad_to
from .covar import spec_of, terms
from .gpr import GPR
from .iterative import _RHS_PAD
from .loss import _MemoLoss
from .sparse import _prior_of, _stationary

STREAM_G1 = 0x5131      # pg_randn stream of the probes' low-rank part, g1 [m, t]
STREAM_G2 = 0x5132      # ... and of their diagonal part, g2 [n, t]
MAX_PROBES = 63         # y and the probes are the factor columns of one pg_kernel_lowrank_grad call (r <= 64)


def tridiagonal(step, beta, k):
    """T [k, k] of one column from its first k step lengths and k - 1 betas."""
    a, b = np.asarray(step[:k], np.float64), np.asarray(beta[:k], np.float64)
    t = np.zeros((k, k))
    dg = 1.0 / a
    dg[1:] += b[:-1] / a[:-1]
    off = np.sqrt(b[:-1]) / a[:-1]
    t[np.arange(k), np.arange(k)] = dg
    t[np.arange(k - 1), np.arange(1, k)] = off
    t[np.arange(1, k), np.arange(k - 1)] = off
    return t


def steps_used(rz, rz0, tol):
    """Steps of one column that carry information: up to and including the first whose r^T z <= tol^2 (r^T z)_0; all when none is."""
    hit = np.flatnonzero(np.asarray(rz) <= tol * tol * rz0)
    return int(hit[0]) + 1 if hit.size else len(rz)


def quadrature(step, beta, rz, rz0, tol, f=np.log):
    """(z^T P^-1 z) e_1^T f(T) e_1 of one column: rz0 is z^T P^-1 z, the first r^T z of a solve that starts at x = 0."""
    k = steps_used(rz, rz0, tol)
    if k == 0 or not rz0 > 0:
        return 0.0
    # (the dense divide-and-conquer solver: LAPACK's tridiagonal stemr does not converge on every T met here, and at k = 1850 the
    # dense one is the faster of the two that do)
    lam, vec = np.linalg.eigh(tridiagonal(step, beta, k))
    return float(rz0 * np.sum(vec[0] ** 2 * f(lam)))


class Stochastic_MLE(_MemoLoss):
    """Negative log marginal likelihood of a matrix-free model (Iterative_GP) and its gradient from `probes` probe vectors drawn at
    `seed`: MLE's protocol, so `CG(Stochastic_MLE(model))` trains the model.  One evaluation is one preconditioner and one block solve
    at the model's rank, tol and max_iter (NotConverged and a failed factorisation propagate as from update()); the gradient adds one
    kernel launch.  After an evaluation `slq_info` holds iterations, residual (the true one), rank, per_probe (the probes' estimates
    of log|A|) and stderr (their standard error)."""

    def __init__(self, model: GPR, probes: int = 15, seed: int = 0) -> None:
        if not getattr(model, "_matrix_free", False):
            raise NotImplementedError("Stochastic_MLE estimates what a matrix-free model (Iterative_GP) cannot compute; %s holds its "
                                      "factor: use MLE" % type(model).__name__)
        if not (isinstance(probes, (int, np.integer)) and 1 <= probes <= MAX_PROBES):
            raise ValueError("Stochastic_MLE: probes must be an integer in 1..%d, got %r" % (MAX_PROBES, probes))
        if not isinstance(seed, (int, np.integer)):
            raise ValueError("Stochastic_MLE: the seed must be an integer, got %r" % (seed,))
        super().__init__(model)
        self.probes, self.seed = int(probes), int(seed)
        self.slq_info = None
        self.grad_calls = 0       # gradient kernels launched so far (tests / diagnostics)
        self.solves = 0           # block solves so far
        self.xgrad_calls = 0      # training-input gradient kernels launched so far
        self._kept = None         # the solve of the last evaluation: a grad() or grad_x() at the same point only adds the kernel
        self._memo_x = None       # (key, grad_x, the keyed x / y / cov) of the last training-input gradient
        self.grad_x_value: ndarray = NotImplemented

    # ---- the memo: MLE's, with the probes and the seed in the key -------------------------------
    def _key(self, params: ndarray):
        m = self.model
        if np.asarray(params).dtype == np.float32:
            raise TypeError("Stochastic_MLE computes in float64 only (the solver's tolerance is below single precision); params is float32")
        tms, noise, _ = terms(m.cov, m._x.shape[-1])
        return (np.asarray(params, dtype=np.float64).tobytes(), np.shape(params), id(m._x), m._x._version, id(m._y), m._y._version,
                id(m.cov), (tms, tuple(noise)), self.probes, self.seed, m.rank, m.tol, m.max_iter)

    def _evaluate(self, params: ndarray, want_grad: bool):
        m = self.model
        key = self._key(params)
        hit = self._memo if (self.memoize and self._memo is not None and self._memo[0] == key) else None
        if hit is not None and (hit[2] is not None or not want_grad):
            return hit[1].copy(), (hit[2].copy() if hit[2] is not None else None)
        reuse = hit is not None and want_grad and self._factor_key == key and self._kept is not None
        loss, grad = self._evaluate_device(params, want_grad, key if self.memoize else None, reuse)
        self._memo = (key, loss.copy(), grad.copy() if want_grad else None, (m._x, m._y, m.cov))
        self._drop_memo_x(key)
        return loss, grad

    def _drop_memo_x(self, key) -> None:
        """The memo of grad_x belongs to the point _memo holds: it goes as soon as _memo moves on, and with it its hold on the data."""
        if self._memo_x is not None and self._memo_x[0] != key:
            self._memo_x = None

    def _evaluate_x(self, params: ndarray) -> ndarray:
        """grad_x at params: the memo's, or one kernel launch on the kept solve of the last evaluation at these parameters and data, or
        -- when there is none -- a solve of its own, which a following loss() or grad() at the same point finds."""
        m = self.model
        key = self._key(params)
        if self.memoize and self._memo_x is not None and self._memo_x[0] == key:
            return self._memo_x[1].copy()
        kept = self._kept if (self.memoize and self._factor_key == key and self._kept is not None) else None
        if kept is None:
            self._kept = self._factor_key = None       # the buffers of the last evaluation go before the next one allocates
            kept = self._solve_all(params)
            if self.memoize:
                self._kept, self._factor_key = kept, key
                if self._memo is None or self._memo[0] != key:
                    self._memo = (key, kept["loss"].copy(), None, (m._x, m._y, m.cov))
                    self._drop_memo_x(key)
        gx = self._gradient_x(kept)
        if self.memoize:
            # (the key holds id()s: like _memo, this memo keeps the tensors and the covariance they name alive, so that no later x / y /
            # cov can come to lie at one of their addresses -- with the same version counter -- and be served this gradient; it is
            # dropped when _memo moves to another point, so it never holds data that _memo has let go)
            self._memo_x = (key, gx.copy(), (m._x, m._y, m.cov))
        return gx

    def grad_x(self, params: ndarray) -> ndarray:
        """dNLML/dx [n, d], the estimator of the module docstring: after loss(p), grad(p) or loss_and_grad(p) one kernel launch and no
        solve."""
        gx = self._evaluate_x(params)
        self.grad_x_value = gx
        return gx

    def loss_and_grads(self, params: ndarray) -> Tuple[float, ndarray, ndarray]:
        """(loss, grad in the hyper-parameters, grad in the training inputs) from one solve and one launch of each gradient kernel."""
        llhd, jac = self.loss_and_grad(params)
        return (llhd, jac, self.grad_x(params))

    def weight_factors(self) -> Tuple[ndarray, ndarray]:
        """Host copies (U, V), each [n, 1 + probes], of the last evaluation's factors of the weight W ~ U V^T = dNLML/dA:
        U = [-alpha / 2, A^-1 Z / (2 t)], V = [alpha, P^-1 Z].  A diagnostic in the manner of FunctionSamples.data_weights: grad and grad_x
        can be restated from them."""
        if self._kept is None:
            raise RuntimeError("weight_factors: no evaluation is kept (evaluate first, with memoize on)")
        u, v = self._factors(self._kept)
        return u.cpu().numpy().copy(), v.cpu().numpy().copy()

    # ---- one evaluation -------------------------------------------------------------------------
    def _solve_all(self, params: ndarray):
        ops = get_ops()
        model = self.model
        xd, yd = model._device_data()
        n, d = xd.shape
        (sp,), nhp = spec_of(model.cov, d)
        p = np.asarray(params, dtype=np.float64)
        assert p.shape[-1] == nhp
        if p.reshape(-1, nhp).shape[0] != 1:
            raise NotImplementedError("Stochastic_MLE: batched hyper-parameters are not supported")
        hp = np.array(p.reshape(nhp), dtype=np.float64)
        t = self.probes
        sig2, kdiag, _, _ = _prior_of(model.cov, d, hp)
        shift = sig2 + JITTER
        hpd = ops.to_device(torch.from_numpy(hp), torch.float64)
        pre = model._preconditioner(ops, hp, hpd, _stationary(sp), shift, xd)      # exactly update()'s
        size = ops.kernel_matmul_worksize(n, n, _RHS_PAD)
        st = dict(x=xd, hpd=hpd, full_spec=sp, shift=shift, pre=pre, work=ops.empty(size) if size > 0 else None)
        npad = pad_to(n)
        b = ops.zeros(npad, _RHS_PAD)
        b[:n, 0] = yd
        zb = b[:, 1: 1 + t]
        ops.randn(zb, n, t, self.seed, stream_id=STREAM_G2)                         # g2, zero behind row n
        if pre is None:
            m, logp = 0, 0.0                                                        # P = I: z = g2
        else:
            m, ma = pre["m"], pre["ma"]
            zb.mul_(float(np.sqrt(shift)))
            g1 = ops.zeros(ma, _RHS_PAD)
            ops.randn(g1[:, 1: 1 + t], m, t, self.seed, stream_id=STREAM_G1)
            ops.gemm_raw(_lib.GEMM_NN, npad, _RHS_PAD, ma, 1.0, pre["L"], g1, 1.0, b)      # z = L g1 + sqrt(shift) g2 ~ N(0, P)
            logp = pre["C"].diagonal()[:m].log().sum()                              # (read with the scalars below)
        xs, its, res, rec = model._solve(ops, st, b, 1 + t, record=True)
        self.solves += 1
        alpha = xs[:n, 0].clone()
        scal = torch.stack([(yd * alpha).sum(), torch.as_tensor(logp, dtype=torch.float64, device=ops.device)]).cpu().numpy()
        logdet_p = (n - m) * float(np.log(shift)) + 2.0 * float(scal[1]) if pre is not None else 0.0
        q = np.array([quadrature(rec["step"][:, c], rec["beta"][:, c], rec["rz"][:, c], rec["rz0"][c], model.tol) for c in range(1, 1 + t)])
        per_probe = logdet_p + q
        logdet = float(per_probe.mean())
        loss = 0.5 * float(scal[0]) + 0.5 * logdet + 0.5 * n * float(np.log(2.0 * np.pi))
        self.slq_info = dict(iterations=its, residual=res, rank=m, per_probe=per_probe,
                             stderr=float(per_probe.std(ddof=1) / np.sqrt(t)) if t > 1 else float("nan"))
        return dict(st=st, hp=hp, nhp=nhp, n=n, xs=xs, z0=rec["z0"], alpha=alpha, loss=np.array(loss), scaled=False)

    def _factors(self, kept):
        """U = [-alpha / 2, S / (2 t)] and V = [alpha, P^-1 Z]: views into the solver's buffers (leading dimension _RHS_PAD), scaled in
        place the first time."""
        n, t = kept["n"], self.probes
        xs, z0 = kept["xs"], kept["z0"]
        if not kept["scaled"]:
            xs[:, 0].mul_(-0.5)
            xs[:, 1: 1 + t].mul_(0.5 / t)
            z0[:n, 0] = kept["alpha"]
            kept["scaled"] = True
        return xs[:n, : 1 + t], z0[:n, : 1 + t]

    def _gradient_x(self, kept) -> ndarray:
        """One symmetric pg_kernel_lowrank_xgrad call on the same views: [n, d]."""
        ops = get_ops()
        st = kept["st"]
        u, v = self._factors(kept)
        out = ops.kernel_lowrank_xgrad(st["full_spec"], st["hpd"], st["x"], None, u, v)
        self.xgrad_calls += 1
        return out.cpu().numpy()                                                    # the one sync + transfer

    def _gradient(self, kept) -> ndarray:
        """One symmetric pg_kernel_lowrank_grad call with U = [-alpha / 2, S / (2 t)] and V = [alpha, P^-1 Z]."""
        ops = get_ops()
        model = self.model
        st, nhp = kept["st"], kept["nhp"]
        u, v = self._factors(kept)
        grad = ops.zeros(nhp)
        ops.kernel_lowrank_grad(st["full_spec"], st["hpd"], st["x"], None, u, v, grad)
        self.grad_calls += 1
        trace = (u * v).sum()                                                       # tr(W): the noise entries' weight
        out = torch.cat([grad, trace.reshape(1)]).cpu().numpy()                     # the one sync + transfer
        g = out[:nhp].copy()
        _, noise, _ = terms(model.cov, st["x"].shape[1])
        for o in noise:
            g[o] = 2.0 * kept["hp"][o] * out[nhp]
        return g

    def _evaluate_device(self, params: ndarray, want_grad: bool, key=None, reuse=False) -> Tuple[ndarray, ndarray]:
        kept = self._kept if reuse else None
        if kept is None:
            self._kept = self._factor_key = None       # the buffers of the last evaluation go before the next one allocates
            kept = self._solve_all(params)
        grad = self._gradient(kept) if want_grad else None
        if key is not None:
            self._kept, self._factor_key = kept, key
        return kept["loss"], grad
