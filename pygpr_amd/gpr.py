"""GP models with PyGPR's class surface (reference: PyGPR/gpr.py) on the MI355X.

`Exact_GP.update` = covariance build + 1e-7 jitter + Cholesky + alpha = K^-1 y (gpr.py:65-74);
`predict` = K* build, mean K* alpha, and either the diagonal predictive variance
diag(K**) - rowsum(K* o (K^-1 K*^T)^T) (gpr.py:96-106) or the full covariance (gpr.py:108-120).
All state lives on the GPU in padded buffers (n rounded up to 256, identity in the padding); the
leading expert dimension of the reference's batched models lives in stacked tensors (`_batch`): factorisation, inverse,
weights AND the prediction of all experts are batched calls (round 5: K* of every expert in one launch, mean + diagonal
variance in three, gpr.py:76-106 on x [nc, n, d]; PG_PREDICT_SERIAL=1 walks the experts one by one as rounds 1-4 did).

Differences a caller can observe:
  * the triangular solves against K* use the explicit inverse factor L^-1 (cached per update), so the
    variance is a GEMM with a fused column-sum-of-squares epilogue instead of `cholesky_solve`
  * K** is never built for var="diag": its diagonal is sum sigma_c^2 + sum sigma_n^2 analytically
  * assigning `model.x` / `model.y` marks the model dirty (the reference keeps a stale factor there)
  * `krn`, `krnchd`, `wt` are read-only views materialised on access
  * `append` and `loo_predict` are new: conditioning on further points, and leave-one-out predictions from the cached L^-1
  * `sampler` / `sample` are new: joint draws from the posterior or the prior at a set of test points (`PosteriorSampler`), with
    normals from the library's counter-based generator (`randn`)
"""
import os
from typing import Sequence

import torch
from torch import Tensor

from . import _lib
from ._ops import JITTER, get_ops, pad_to
from .covar import Covar, layout, spec_of, terms

_CHUNK = 8192  # test points per device batch
# Experts of a batched model are factorised in ONE batched call (every launch covers all experts: pg_build_potrf_trtri_batched)
# up to this padded size; above it the per-step launches no longer matter and each expert takes the single-model schedule with
# its flag-coupled chain, one after the other.  PG_BATCH_MAX_N overrides (0: never batch).
_BATCH_MAX_N = int(os.environ.get("PG_BATCH_MAX_N", "12288"))
_FULL_VT_BYTES = 16 << 30   # predict(var="full"): experts whose V^T fit this together share one rank-n update launch (and at most
                            # 40 % of the device memory that is free when the call starts: `_group_budget`)
_APPEND_K = 128         # points per pg_chol_append block (Exact_GP.append)
_BATCH_EAGER_N = 4096   # batched experts up to this size form L^-1 with the factor even when nobody asked for variances: the
                        # batched inverse + three batched mat-vec launches are cheaper than one substitution sweep per expert


class ChainTimeout(torch.linalg.LinAlgError):
    """info = -1: a bounded wait inside the factorisation's flag-coupled chain expired -- kernels of the library's streams did
    not run concurrently (include/pygpr_hip.h).  Not a property of the matrix.  Every caller in this package answers it by
    repeating the evaluation on the classic chain (`HipOps.recover_from_timeout`); the exception only escapes if the repeat
    fails too.  A LinAlgError subclass so that the committee's status-word paths (gr_bcm.py) treat it like any failed expert."""


def _lin_alg_error(info: int, note: str = ""):
    if int(info) < 0:
        err = ChainTimeout("pygpr_amd: the factorisation's coupled chain timed out twice (info = %d): kernels of different "
                           "streams do not run concurrently in this environment%s" % (int(info), note))
        err.pg_info = int(info)
        return err
    err = torch.linalg.LinAlgError(
        "cholesky: The factorization could not be completed because the input is not positive-definite "
        "(the leading minor of order %d is not positive-definite)%s." % (info, note))
    err.pg_info = int(info)
    return err


def _checked(enqueue, infos):
    """Run `enqueue()` (device work that ends in the factorisation status words `infos()` reads after one sync).  info < 0 is
    the coupled chain's time-out: switch the handle to the classic chain and repeat ONCE from the start -- tc.cholesky
    (gpr.py:69) never fails on a positive-definite matrix.  Returns the final status words."""
    enqueue()
    vals = [int(v) for v in infos()]
    if any(v < 0 for v in vals):
        get_ops().recover_from_timeout()
        enqueue()
        vals = [int(v) for v in infos()]
    return vals


def _group_budget(cap, need=None):
    """Bytes a prediction may spend on the per-expert scratch of ONE launch group: `cap`, but never more than 40 % of what the device
    has free right now (torch's cached blocks count as free: they are re-used) -- a fuller or smaller device gets smaller groups,
    down to one expert per launch, instead of an out-of-memory error.  `need`: what the caller wants in all; up to 1 GiB is granted
    without asking (torch's memory statistics cost 0.1 ms per query -- 40 % of a prediction at the reference's test sizes)."""
    if need is not None and need <= (1 << 30):
        return cap
    try:
        free, _ = torch.cuda.mem_get_info()
        free += torch.cuda.memory_reserved() - torch.cuda.memory_allocated()
    except Exception:
        return cap
    return max(1, min(cap, int(0.4 * free)))


def _stacked_rows(ts):
    """ts: per-expert 1-D device tensors.  If they are rows of one buffer at a constant stride, that buffer as a [len(ts), m] view;
    None otherwise (the committee's batched aggregation kernel takes a base pointer and a stride)."""
    if not ts:
        return None
    t0 = ts[0]
    if any(t.dim() != 1 or t.stride(0) != 1 or t.dtype != t0.dtype or t.numel() != t0.numel() for t in ts):
        return None
    base = t0.untyped_storage().data_ptr()
    if any(t.untyped_storage().data_ptr() != base for t in ts):      # views of ONE allocation only
        return None
    item = t0.element_size()
    step = (ts[1].data_ptr() - t0.data_ptr()) // item if len(ts) > 1 else t0.numel()
    if len(ts) > 1 and (step < t0.numel() or any(t.data_ptr() - t0.data_ptr() != i * step * item for i, t in enumerate(ts))):
        return None
    return torch.as_strided(t0, (len(ts), t0.numel()), (step, 1))


def _stacked_pair(a, b):
    """a, b: [nc, m] views of the same shape and strides inside ONE allocation, b behind a: the [2, nc, m] view over both; else None."""
    if a.shape != b.shape or a.stride() != b.stride() or a.dtype != b.dtype:
        return None
    if a.untyped_storage().data_ptr() != b.untyped_storage().data_ptr():
        return None
    step = (b.data_ptr() - a.data_ptr()) // a.element_size()
    if step <= 0 or step < (a.shape[0] - 1) * a.stride(0) + a.shape[1]:
        return None
    return torch.as_strided(a, (2,) + tuple(a.shape), (step,) + tuple(a.stride()))


def _blockdiag_eye(a, n_pad):
    """[n_pad, n_pad] copy of the square a with the identity below and right of it."""
    out = torch.zeros(n_pad, n_pad, dtype=a.dtype, device=a.device)
    m = a.shape[0]
    out[:m, :m] = a
    out[m:, m:].diagonal().fill_(1)
    return out


class GPR:
    """Base class for Gaussian process regression models (PyGPR/gpr.py:13-43)."""

    def __init__(self, x: Tensor, y: Tensor, cov: Covar) -> None:
        self._x: Tensor = x
        self._y: Tensor = y
        self.cov = cov
        self.params: Tensor = NotImplemented
        self.need_upd: bool = True
        return None

    @property
    def x(self) -> Tensor:
        return self._x

    @x.setter
    def x(self, value: Tensor) -> None:
        self._x = value
        self._data_changed()

    @property
    def y(self) -> Tensor:
        return self._y

    @y.setter
    def y(self, value: Tensor) -> None:
        self._y = value
        self._data_changed()

    def _data_changed(self) -> None:
        self.need_upd = True

    def set_params(self, params: Tensor) -> None:
        self.params = torch.clone(params)
        self.need_upd = True
        return None

    def update(self) -> None:
        raise NotImplementedError

    def append(self, x_new: Tensor, y_new: Tensor) -> None:
        raise NotImplementedError("%s has no incremental append; assign x / y and refit" % type(self).__name__)

    def predict(self, xp: Tensor, var: str) -> Sequence[Tensor]:
        raise NotImplementedError

    def loo_predict(self) -> Sequence[Tensor]:
        raise NotImplementedError("%s has no leave-one-out prediction; fit an Exact_GP on the data" % type(self).__name__)

    def sampler(self, xp: Tensor, **kwargs):
        raise NotImplementedError("%s has no joint sampler; draw from an Exact_GP" % type(self).__name__)

    def sample(self, xp: Tensor, n_samples: int = 1, seed: int = 0, **kwargs) -> Tensor:
        raise NotImplementedError("%s has no joint sampler; draw from an Exact_GP" % type(self).__name__)

    def predict_var(self, xp: Tensor, **kwrgs: Tensor) -> Tensor:
        raise NotImplementedError

    def predict_covar(self, xp: Tensor, **kwargs: Tensor) -> Tensor:
        raise NotImplementedError


class _Data:
    """Device copy of one (x, y) pair: x [n, d], y zero-padded to n_pad."""

    __slots__ = ("x", "y", "n", "n_pad")


class _Expert:
    """Device state of one expert (its data may be shared with other experts: batched params on unbatched x)."""

    # u = L^-1 y: held from the first append after a fit on (Exact_GP.append keeps it current), None otherwise
    __slots__ = ("x", "y", "n", "n_pad", "chol", "invd", "alpha", "minv", "minv_valid", "work", "hp", "info", "u")

    def __init__(self, data):
        self.x, self.y, self.n, self.n_pad = data.x, data.y, data.n, data.n_pad
        self.chol = self.invd = self.alpha = self.minv = self.work = self.hp = self.info = self.u = None
        self.minv_valid = False


class Exact_GP(GPR):
    """Exact GP model (PyGPR/gpr.py:46-120); x [(nc), n, d], y [(nc), n], params [(nc), nhp]."""

    def __init__(self, x: Tensor, y: Tensor, cov: Covar, eager_inverse: bool = False) -> None:
        super().__init__(x, y, cov)
        self.params: Tensor = cov.init_params(x)
        self._experts = None
        self._data = None
        self._data_key = None
        self._bat = None
        self._pbuf = None
        self._x_all = self._y_all = None
        self.need_upd: bool = True
        # eager_inverse: form L^-1 inside update() (fused with the Cholesky) and take alpha = L^-T (L^-1 y) from two
        # triangular mat-vecs.  Worth it whenever predictive variances follow (grBCM experts); wasted work otherwise.
        self.eager_inverse = eager_inverse
        self._upd_count = 0     # bumped by every change of the model's state: a backward checks it against its forward (_state_token)
        return None

    # ---- device residency -------------------------------------------------------------------
    @property
    def dtype(self):
        return self._x.dtype if self._x.dtype == torch.float32 else torch.float64

    @property
    def batched(self) -> bool:
        """More than one expert: the reference's kernels squeeze a batch of one away (covar.py:161-165), so x [1, n, d]
        behaves like x [n, d]."""
        return len(self._device_experts()) > 1

    def _data_changed(self) -> None:
        self._experts = None
        self._data = None
        self._pbuf = None
        self.need_upd = True
        self._upd_count = getattr(self, "_upd_count", 0) + 1

    def set_params(self, params: Tensor) -> None:
        super().set_params(params)
        self._upd_count = getattr(self, "_upd_count", 0) + 1

    def _state_token(self):
        """What a prediction's backward needs unchanged since its forward: the update counter and the identity and version of x, y and
        params (in-place edits bump a tensor's version, as torch's own saved-tensor check sees them)."""
        return (self._upd_count, id(self._x), self._x._version, id(self._y), self._y._version, id(self.params), self.params._version)

    def _device_data(self):
        """x / y on the device, one _Data per leading index of x, uploaded once per (tensor identity, version): in-place
        edits of model.x / model.y (`model.y.copy_(new)`) are seen by the next evaluation, as in the reference, which
        re-reads model.x / model.y on every call (loss.py:37,43)."""
        key = (id(self._x), self._x._version, id(self._y), self._y._version)
        if self._data is None or self._data_key != key:
            ops = get_ops()
            xb = self._x.reshape(-1, self._x.shape[-2], self._x.shape[-1])
            yb = self._y.reshape(-1, self._y.shape[-1])
            nbd = max(xb.shape[0], yb.shape[0])
            if xb.shape[0] not in (1, nbd) or yb.shape[0] not in (1, nbd):
                raise RuntimeError("batch dimensions of x and y do not broadcast")
            x_all = ops.to_device(xb, self.dtype)                       # [nbx, n, d]: ONE upload; experts take views
            n_pad = pad_to(xb.shape[1])
            y_all = ops.zeros(nbd, n_pad, dtype=self.dtype)
            y_all[:, : xb.shape[1]] = ops.to_device(yb, self.dtype).expand(nbd, -1) if yb.shape[0] != nbd else ops.to_device(yb, self.dtype)
            data = []
            for b in range(nbd):
                dt = _Data()
                dt.n = xb.shape[1]
                dt.n_pad = n_pad
                dt.x = x_all[b % x_all.shape[0]]
                dt.y = y_all[b]
                data.append(dt)
            self._x_all, self._y_all = x_all, y_all
            self._data, self._data_key = data, key
            self._experts = None
        return self._data

    def _device_experts(self):
        """One _Expert per model of the batch: max(batch of x / y, batch of params) of them, as cov.kernel(params, x)
        broadcasts in the reference (gpr.py:67; params [nc, nhp] on an unbatched x are nc models on the same points)."""
        data = self._device_data()
        nb = max(len(data), self._hp_rows().shape[0])
        if len(data) not in (1, nb) or self._hp_rows().shape[0] not in (1, nb):
            raise RuntimeError("batch dimensions of params and x do not broadcast")
        if self._experts is None or len(self._experts) != nb:
            self._experts = [_Expert(data[b % len(data)]) for b in range(nb)]
            self._bat = None
            self.need_upd = True
        return self._experts

    def _batch(self):
        """Stacked buffers of a batched model whose experts are factorised together: chol / invd / alpha / info (and minv, work
        when the inverse is eager) as [nexp, ...] tensors, the experts holding views.  None when the model is not batched that way
        (one expert, a Compose longer than one pg_covspec, or experts above _BATCH_MAX_N)."""
        experts = self._experts
        n_pad = experts[0].n_pad
        spec, _ = spec_of(self.cov, self._x.shape[-1])
        if len(experts) < 2 or n_pad > _BATCH_MAX_N or isinstance(spec, (list, tuple)) and len(spec) != 1:
            return None
        if self._bat is None:
            ops = get_ops()
            nb = len(experts)
            bat = {
                "chol": ops.empty(nb, n_pad, n_pad, dtype=self.dtype),
                "invd": ops.empty(nb, ops.potrf_worksize(n_pad, self.dtype), dtype=self.dtype),
                "alpha": ops.empty(nb, n_pad, dtype=self.dtype),
                "info": torch.zeros(nb, dtype=torch.int32, device=ops.device),
                "hp": ops.empty(nb, self.params.shape[-1], dtype=torch.float64),
                "minv": None, "u": None, "work": None,
            }
            for b, e in enumerate(experts):
                e.chol, e.invd, e.alpha, e.info, e.hp = bat["chol"][b], bat["invd"][b], bat["alpha"][b], bat["info"][b: b + 1], bat["hp"][b]
            self._bat = bat
        self._bat["eager"] = self.eager_inverse or n_pad <= _BATCH_EAGER_N
        if self._bat["eager"]:
            self._batch_inverse(weights=True)
        return self._bat

    def _batch_inverse(self, weights=False):
        """The stack of the experts' L^-1 in `_bat` and, with `weights`, the scratch of the eager weights (u, work): each is allocated
        when IT is missing, whoever asked first -- a prediction of a lazy model forms the stack long before `eager_inverse` may be
        switched on.  A new stack holds nothing yet: the experts' views of it are marked invalid."""
        ops = get_ops()
        bat, experts = self._bat, self._experts
        nb, n_pad = len(experts), experts[0].n_pad
        if bat["minv"] is None:
            bat["minv"] = ops.empty(nb, n_pad, n_pad, dtype=self.dtype)
            for b, e in enumerate(experts):
                e.minv, e.minv_valid = bat["minv"][b], False
        if weights and bat["u"] is None:
            bat["u"] = ops.empty(nb, n_pad, dtype=self.dtype)
            bat["work"] = ops.empty(nb, (n_pad // 256) * n_pad, dtype=self.dtype)
        return bat["minv"]

    def _expert_inverse(self, e, weights=False):
        """The same for one expert outside a stack: e.minv and, with `weights`, e.work."""
        ops = get_ops()
        if e.minv is None:
            e.minv = ops.empty(e.n_pad, e.n_pad, dtype=self.dtype)
            e.minv_valid = False
        if weights and e.work is None:
            e.work = ops.empty((e.n_pad // 256 + 1) * e.n_pad, dtype=self.dtype)
        return e.minv

    def _hp_rows(self):
        nhp = self.params.shape[-1]
        return self.params.reshape(-1, nhp).to(torch.float64)

    # ---- the path ---------------------------------------------------------------------------
    def update(self) -> None:
        experts = self._device_experts()      # first: an in-place edit of x / y (version bump) marks the model dirty here
        if self.need_upd:
            ops = get_ops()
            hp_rows = self._hp_rows()
            spec, nhp = spec_of(self.cov, self._x.shape[-1])
            assert hp_rows.shape[-1] == nhp

            bat = self._batch()

            def enqueue_batched():
                # all experts in one call: every launch of the blocked factorisation (and of L^-1) covers the whole batch
                bat["hp"].copy_(hp_rows.expand(len(experts), -1) if hp_rows.shape[0] == 1 else hp_rows)
                x_stride = self._x_all.stride(0) if self._x_all.shape[0] > 1 else 0
                ops.build_factor_batched(spec, bat["hp"], self._x_all, x_stride, bat["chol"], bat["invd"], bat["info"],
                                         bat["minv"] if bat["eager"] else None)
                if bat["eager"]:
                    ops.alpha_batched(bat["minv"], self._y_all, bat["u"], bat["alpha"], bat["work"])
                for e in experts:
                    e.minv_valid = bat["eager"]
                    if not bat["eager"]:
                        ops.potrs_vec(e.chol, e.invd, e.y, e.alpha)

            def enqueue_serial():
                for b, e in enumerate(experts):
                    e.u = None
                    e.hp = ops.to_device(hp_rows[b % hp_rows.shape[0]], torch.float64)
                    if e.chol is None:
                        e.chol = ops.empty(e.n_pad, e.n_pad, dtype=self.dtype)
                        e.invd = ops.potrf_workspace(e.n_pad, self.dtype)
                        e.alpha = ops.empty(e.n_pad, dtype=self.dtype)
                        e.info = torch.zeros(1, dtype=torch.int32, device=ops.device)
                    if self.eager_inverse:
                        self._expert_inverse(e, weights=True)
                        ops.build_factor(spec, e.hp, e.x, e.chol, e.invd, e.info, e.minv)
                        u = e.work[: e.n_pad]
                        ops.trmv(e.minv, e.y, u, 0)
                        ops.trmv(e.minv, u, e.alpha, 1, e.work[e.n_pad:])
                        e.minv_valid = True
                    else:
                        e.minv_valid = False
                        ops.build_factor(spec, e.hp, e.x, e.chol, e.invd, e.info)
                        ops.potrs_vec(e.chol, e.invd, e.y, e.alpha)

            enqueue = enqueue_batched if bat is not None else enqueue_serial

            # one sync point after everything is enqueued; a timed-out coupled chain repeats the lot on the classic chain
            for info in _checked(enqueue, lambda: torch.cat([e.info for e in experts]).tolist()):
                if info:
                    raise _lin_alg_error(info)
            self.need_upd = False
            self._upd_count += 1
        return None

    def _minv(self, e):
        if not e.minv_valid:
            get_ops().trtri(e.chol, e.invd, self._expert_inverse(e))
            e.minv_valid = True
        return e.minv

    # ---- conditioning on new observations --------------------------------------------------------
    def append(self, x_new: Tensor, y_new: Tensor) -> None:
        """Condition the model on k new observations in place, hyper-parameters unchanged; returns None.  x_new is [k, d] ([1, k, d] or
        [k, d] when x is [1, n, d]), y_new has y's layout with k in its last dimension; both follow the model's dtype and device.
        Afterwards model.x / model.y are new tensors equal to torch.cat of the old and the new (the x / y setters are not used), and the
        model reads exactly as a fresh fit on them does, to rounding.

        A fitted model extends its factor by blocks of at most 128 points (pg_chol_append: O(n^2 k), three passes over L^-1) instead of
        refitting in O(n^3): L^-1 is formed once if it is not held, and kept from then on.  A model that needs an update anyway (never fitted,
        after set_params or an edit of x / y) only takes the data; the next update() fits the lot.  If a pivot of the new block fails
        (e.g. a NaN in x_new) the call raises torch.linalg.LinAlgError and the model is left exactly as it was.  Batched models (more than
        one expert) raise NotImplementedError, and so does GRBCM, unchanged."""
        x_old, y_old = self._x, self._y
        d = x_old.shape[-1]
        nb_params = self.params.reshape(-1, self.params.shape[-1]).shape[0] if isinstance(self.params, Tensor) else 1
        if (x_old.dim() == 3 and x_old.shape[0] > 1) or (y_old.dim() > 1 and y_old.reshape(-1, y_old.shape[-1]).shape[0] > 1) or nb_params > 1:
            raise NotImplementedError("Exact_GP.append: batched models (more than one expert) are not supported")
        if x_new.dim() == 3 and x_new.shape[0] == 1 and x_old.dim() == 3:
            x_new = x_new[0]
        if x_new.dim() != 2 or x_new.shape[1] != d:
            raise ValueError("Exact_GP.append: x_new must be [k, %d], got %s" % (d, tuple(x_new.shape)))
        k = x_new.shape[0]
        if y_new.numel() != k or y_old.shape[-1] != x_old.shape[-2]:
            raise ValueError("Exact_GP.append: y_new must hold %d values in y's layout, got %s" % (k, tuple(y_new.shape)))
        if k == 0:
            return None
        xh = x_new.detach().to(device=x_old.device, dtype=x_old.dtype)
        yh = y_new.detach().reshape(y_old.shape[:-1] + (k,)).to(device=y_old.device, dtype=y_old.dtype)
        x_cat = torch.cat([x_old, xh[None] if x_old.dim() == 3 else xh], dim=-2)
        y_cat = torch.cat([y_old, yh], dim=-1)
        experts = self._device_experts()
        if self.need_upd:                      # the next update() fits the combined data from scratch
            self._x, self._y = x_cat, y_cat
            self._data_changed()
            return None
        self._append_fitted(experts[0], xh, yh.reshape(k), x_cat, y_cat)
        return None

    def _append_fitted(self, e, xh, yh, x_cat, y_cat):
        ops = get_ops()
        dt = self.dtype
        spec, _ = spec_of(self.cov, self._x.shape[-1])
        k, n0 = xh.shape[0], e.n
        total = n0 + k
        n_pad = pad_to(total)
        xd = torch.cat([e.x, ops.to_device(xh, dt)], dim=0)                     # [n + k, d]: every point on the device
        yd = ops.to_device(yh, dt)
        minv = self._minv(e)
        if e.u is None:
            e.u = ops.zeros(e.n_pad, dtype=dt)
            ops.trmv(minv, e.y, e.u, 0)
        # growth, or more than one block: work on copies (blockdiag(., I) when growing) and swap them in only once every block went in
        copy = n_pad > e.n_pad or k > _APPEND_K
        if copy:
            chol, minv_w = _blockdiag_eye(e.chol, n_pad), _blockdiag_eye(minv, n_pad)
            invd = ops.empty(ops.potrf_worksize(n_pad, dt), dtype=dt)
            invd.zero_()
            blocks = invd[: n_pad * 128].view(n_pad // 128, 128, 128)
            nb0 = e.n_pad // 128
            blocks[:nb0] = e.invd[: e.n_pad * 128].view(nb0, 128, 128)
            blocks[nb0:] = torch.eye(128, dtype=dt, device=ops.device)
            u, alpha = ops.zeros(n_pad, dtype=dt), ops.zeros(n_pad, dtype=dt)
            u[: e.n_pad], alpha[: e.n_pad] = e.u, e.alpha
        else:
            chol, minv_w, invd, u, alpha = e.chol, minv, e.invd, e.u, e.alpha
        kmax = min(k, _APPEND_K)
        kpad = pad_to(kmax, 128)
        kt = ops.empty(kpad, n_pad, dtype=dt)
        knn = ops.empty(kpad, kpad, dtype=dt)
        work = ops.empty(ops.chol_append_worksize(n_pad, kmax, dt), dtype=dt)
        info = torch.zeros(1, dtype=torch.int32, device=ops.device)
        for s in range(0, k, _APPEND_K):
            kc = min(_APPEND_K, k - s)
            xc = xd[n0 + s: n0 + s + kc]
            ops.kernel_build(spec, e.hp, xc, xd[: n0 + s], kt)                   # k(Xn, X): zero past n (cross build, no noise)
            ops.kernel_build(spec, e.hp, xc, None, knn, jitter=JITTER)            # k(Xn, Xn) + noise + jitter I, as update() builds K
            ops.chol_append(n0 + s, kc, chol, invd, minv_w, kt, knn, yd[s: s + kc], u, alpha, work, info)
            bad = int(info.item())
            if bad:
                raise _lin_alg_error(bad)
        # every block is in: publish
        if copy:
            e.chol, e.invd, e.minv, e.u, e.alpha = chol, invd, minv_w, u, alpha
            if e.work is not None:
                e.work = ops.empty((n_pad // 256 + 1) * n_pad, dtype=dt)
            self._pbuf = None
        if n_pad > e.n_pad:
            y_all = ops.zeros(1, n_pad, dtype=dt)
            y_all[0, :n0] = e.y[:n0]
        else:
            y_all = self._y_all[:1]
        y_all[0, n0:total] = yd
        dta = _Data()
        dta.n, dta.n_pad, dta.x, dta.y = total, n_pad, xd, y_all[0]
        e.x, e.y, e.n, e.n_pad = xd, y_all[0], total, n_pad
        self._x_all, self._y_all = xd[None], y_all
        self._x, self._y = x_cat, y_cat
        self._data = [dta]
        self._data_key = (id(self._x), self._x._version, id(self._y), self._y._version)
        self._upd_count += 1

    # ---- leave-one-out cross-validation -----------------------------------------------------------
    def loo_predict(self) -> Sequence[Tensor]:
        """[mean, var] of the leave-one-out predictive distributions p(y_i | x, y_-i) (Rasmussen & Williams 5.4.2), each [n] in the
        model's dtype on x's device: mean_i = y_i - alpha_i / c_i and var_i = 1 / c_i with c = diag(K^-1) -- predictive for y_i, the noise
        and the 1e-7 jitter included (K is the matrix update() factors).  Calls update(); c comes from one pass over the cached L^-1
        (pg_loo_terms), which is formed once if it is not held and kept from then on, as `append` does.  Batched models (more than one
        expert) raise NotImplementedError, and so does GRBCM."""
        x_old, y_old = self._x, self._y
        nb_params = self.params.reshape(-1, self.params.shape[-1]).shape[0] if isinstance(self.params, Tensor) else 1
        if (x_old.dim() == 3 and x_old.shape[0] > 1) or (y_old.dim() > 1 and y_old.reshape(-1, y_old.shape[-1]).shape[0] > 1) or nb_params > 1:
            raise NotImplementedError("Exact_GP.loo_predict: batched models (more than one expert) are not supported")
        self.update()
        ops = get_ops()
        e = self._experts[0]
        dt = self.dtype
        c, mu, var = (ops.empty(e.n, dtype=dt) for _ in range(3))
        out = ops.zeros(1, dtype=torch.float64)
        work = ops.empty(ops.loo_terms_worksize(e.n_pad), dtype=torch.float64)
        ops.loo_terms(self._minv(e), e.alpha, e.y, e.n, c, mu, var, out, work)
        return [mu.to(self._x.device), var.to(self._x.device)]

    # ---- joint draws ------------------------------------------------------------------------------
    def sampler(self, xp: Tensor, noise: bool = False, jitter: float = 1e-7, prior: bool = False) -> "PosteriorSampler":
        """A snapshot of the joint Gaussian at xp ([m, d], or [nc, m, d] for a batched model: the rules of `predict`) to draw from.
        prior=False: mean and covariance of predict(xp, "full"), through the same device path (the mean is predict's, bit for bit).
        prior=True: mean 0 and covariance cov.kernel(params, xp); needs no fit and triggers none.  Both covariances carry
        sum sigma_n^2 on their diagonal (White_noise sees xp = None there): noise=True keeps it -- draws of new observations y* --,
        noise=False (the default) subtracts it -- draws of the latent function.  `jitter` is then added to the diagonal and the matrix is
        factored (pg_potrf, experts of a batched model together); a failed pivot raises torch.linalg.LinAlgError -- the jitter is never
        raised silently.  The sampler owns its buffers: later changes of the model do not reach it, and making it changes nothing a
        later predict returns."""
        ops = get_ops()
        dt = self.dtype
        xpd = self._xp_device(xp)
        m = xpd.shape[-2]
        if m < 1:
            raise ValueError("Exact_GP.sampler: xp holds no points")
        m_pad = pad_to(m)
        d = self._x.shape[-1]
        spec, _ = spec_of(self.cov, d)
        _, _, noise_offs, _ = layout(self.cov, d)
        nexp = len(self._device_experts())
        if xpd.dim() == 3 and xpd.shape[0] not in (1, nexp):
            raise RuntimeError("batch dimension of xp (%d) does not match the %d experts" % (xpd.shape[0], nexp))
        hp_rows = self._hp_rows()
        state = {}

        def enqueue():
            if prior:
                mean_all = ops.zeros(nexp, m_pad, dtype=dt)
                c_all = ops.empty(nexp, m_pad, m_pad, dtype=dt)
                for b in range(nexp):
                    hp = ops.to_device(hp_rows[b % hp_rows.shape[0]], torch.float64)
                    ops.kernel_build(spec, hp, xpd if xpd.dim() == 2 else xpd[b % xpd.shape[0]], None, c_all[b])   # K** + sum sigma_n^2 I, identity padding
            else:
                mean_all, c_all = self._predict_device(xpd, "full", padded=True)
            for b in range(nexp):
                diag = c_all[b].diagonal()[:m]
                if not noise:
                    row = hp_rows[b % hp_rows.shape[0]]
                    diag.sub_(float(sum(row[o] ** 2 for o in noise_offs)))
                diag.add_(float(jitter))
            info = torch.zeros(nexp, dtype=torch.int32, device=ops.device)
            invd = ops.empty(nexp, ops.potrf_worksize(m_pad, dt), dtype=dt)
            if nexp == 1:
                ops.potrf(c_all[0], invd[0], info)
            else:
                ops.potrf_trtri_batched(c_all, invd, info, None)
            state.update(mean=mean_all, chol=c_all, info=info, invd=invd)

        for bad in _checked(enqueue, lambda: state["info"].tolist()):
            if bad:
                raise _lin_alg_error(bad, " -- the %s covariance at xp, with jitter = %g and noise = %s, is not positive definite in %s: raise "
                                          "`jitter` or draw with noise=True" % ("prior" if prior else "posterior", jitter, bool(noise),
                                                                               "float32" if dt == torch.float32 else "float64"))
        for b in range(nexp):      # the product of a draw reads the whole diagonal 128-blocks of the factor: clear what potrf left above it
            ops.tril(state["chol"][b], m_pad)
        return PosteriorSampler(state["mean"], state["chol"], m, xp.device, nexp > 1, bool(noise), float(jitter))

    def sample(self, xp: Tensor, n_samples: int = 1, seed: int = 0, **sampler_kwargs) -> Tensor:
        """sampler(xp, **sampler_kwargs).draw(n_samples, seed): [n_samples, m] ([nc, n_samples, m] for a batched model)."""
        return self.sampler(xp, **sampler_kwargs).draw(n_samples, seed)

    def _kss_diag(self, b: int) -> float:
        """diag of cov.kernel(params, xp): sum sigma_c^2 + sum sigma_n^2 (White_noise sees xp=None,
        gpr.py:98), no jitter.  A Product term contributes the product of its factors' sigma^2 (formed in list order, as the
        batched prediction forms it on the device)."""
        tms, noise, _ = terms(self.cov, self._x.shape[-1])
        hp = self._hp_rows()
        row = hp[b % hp.shape[0]]

        def prior(offs):
            v = row[offs[0]] ** 2
            for o in offs[1:]:
                v = v * row[o] ** 2
            return v

        return float(sum(prior(offs) for _, _, offs in tms) + sum(row[o] ** 2 for o in noise))

    def _predict_expert(self, b, e, xpd, want):
        ops = get_ops()
        spec, _ = spec_of(self.cov, self._x.shape[-1])
        m = xpd.shape[0]
        mean = ops.empty(m, dtype=self.dtype)
        var = ops.empty(m, dtype=self.dtype) if want == "diag" else None
        for s in range(0, m, _CHUNK):
            xq = xpd[s: s + _CHUNK]
            mc = xq.shape[0]
            m_pad = pad_to(mc)
            # K* (test-point-major: k(xp, x); the kernels are symmetric) and the product's scratch are kept per model and shape: all
            # experts of a model and all chunks of a call run one after the other on the stream, so ONE set serves them (round 2
            # allocated 604 MB per expert per batch at config 4 through torch's caching allocator)
            key = (m_pad, e.n_pad, want == "diag")
            if self._pbuf is None or self._pbuf[0] != key:
                self._pbuf = (key, ops.empty(m_pad, e.n_pad, dtype=self.dtype), ops.empty((e.n_pad // 64) * m_pad, dtype=self.dtype))
            kt, work = self._pbuf[1], self._pbuf[2]
            ops.kernel_build(spec, e.hp, xq, e.x, kt)
            mu = ops.empty(m_pad, dtype=self.dtype)
            vq = ops.empty(m_pad, dtype=self.dtype) if want == "diag" else None
            ops.predict_mean_q_kt(kt, self._minv(e) if want == "diag" else None, e.alpha, mu, vq,
                                  self._kss_diag(b), work)
            mean[s: s + mc] = mu[:mc]
            if want == "diag":
                var[s: s + mc] = vq[:mc]
        if want == "diag":
            return mean, var
        return mean, None

    def _predict_full(self, xqs, padded=False):
        """Mean K* alpha and K** - K* K^-1 K*^T = K** - V^T V with V = L^-1 K*^T (gpr.py:80-85,108-120) for every expert (expert b at the
        points xqs[b]): per expert the test-point-major K* -- built ONCE, the mean is taken from it too (round 4 built it a second time
        for the mean) --, Vt = K* L^-T (both operands read along k) and K**; then ONE rank-n update for all experts -- the 136 lower tiles
        of one 2048 x 2048 output leave three quarters of the chip idle, eight experts' tiles fill it.  Returns (means, covariances);
        padded: the fresh stacks they are views of instead, mean [nexp, m_pad] and covariance [nexp, m_pad, m_pad] (identity in the padding)."""
        ops = get_ops()
        spec, _ = spec_of(self.cov, self._x.shape[-1])
        experts = self._experts
        m = xqs[0].shape[0]
        m_pad = pad_to(m)
        item = torch.empty(0, dtype=self.dtype).element_size()
        c_all = ops.empty(len(experts), m_pad, m_pad, dtype=self.dtype)
        mean_all = ops.empty(len(experts), m_pad, dtype=self.dtype)
        dummy = ops.empty(256, dtype=self.dtype)
        budget = _group_budget(_FULL_VT_BYTES, 2 * sum(m_pad * e.n_pad for e in experts) * item)      # per group: Vt and (stacked inverses) K* of every expert in it
        b = 0
        while b < len(experts):
            n_pad = experts[b].n_pad
            # experts of one padded size share a launch, within the budget (never fewer than one)
            cnt = 1
            while (b + cnt < len(experts) and experts[b + cnt].n_pad == n_pad and 2 * (cnt + 1) * m_pad * n_pad * item <= budget):
                cnt += 1
            vt = ops.empty(cnt, m_pad, n_pad, dtype=self.dtype)
            minvs = [self._minv(experts[b + i]) for i in range(cnt)]
            step = (minvs[1].data_ptr() - minvs[0].data_ptr()) if cnt > 1 else 0
            stacked = cnt > 1 and step > 0 and all(mi.data_ptr() - minvs[0].data_ptr() == i * step and mi.stride(0) == minvs[0].stride(0)
                                                   for i, mi in enumerate(minvs))
            kt = ops.empty(cnt if stacked else 1, m_pad, n_pad, dtype=self.dtype)
            for i in range(cnt):
                e = experts[b + i]
                ops.kernel_build(spec, e.hp, xqs[b + i], e.x, kt[i if stacked else 0])
                ops.predict_mean_q_kt(kt[i if stacked else 0], None, e.alpha, mean_all[b + i], None, 0.0, dummy)   # mean = K* alpha
                if not stacked:
                    ops.trmm_lower_kt(minvs[i], kt[0], vt[i])
                ops.kernel_build(spec, e.hp, xqs[b + i], None, c_all[b + i])   # K** incl. sigma_n^2, padding = identity
            if stacked:      # experts factorised together hold their inverses in one stack: one launch for all the products
                ops.trmm_lower_kt(minvs, kt, vt)
            ops.syrk_nt_sub_batched(vt, c_all[b: b + cnt], lower_only=True)     # n m^2 flop per expert, lower tiles
            b += cnt
        out = []
        for i in range(len(experts)):
            ops.symmetrize(c_all[i], m_pad)                 # the upper triangle is the mirror: exactly symmetric
            out.append(c_all[i][:m, :m])
        if padded:
            return mean_all, c_all
        return [mean_all[i, :m] for i in range(len(experts))], out

    def _predict_batched(self, xpd, want):
        """Mean (and diagonal variance) of ALL experts of a model whose experts live in stacked buffers (`_batch`): per chunk of test
        points ONE launch builds every expert's test-point-major K*, three more give every mean and variance (round 5; the reference:
        one batched kernel / bmm / cholesky_solve, gpr.py:76-106).  Per expert the numbers are those of `_predict_expert`, bit for bit."""
        ops = get_ops()
        spec, _ = spec_of(self.cov, self._x.shape[-1])
        bat, experts = self._bat, self._experts
        nb, n_pad = len(experts), experts[0].n_pad
        m = xpd.shape[-2]
        diag = want == "diag"
        if diag:                              # inverses not formed with the factor (lazy model): form them into one stack now
            self._batch_inverse()
            for e in experts:
                self._minv(e)
        # outputs: one fresh buffer per call, rows long enough for the padded last chunk -- the kernels write every chunk's means and
        # variances straight into their place (no staging copies: at the reference's test sizes those were half the call)
        mtot = ((m // _CHUNK) * _CHUNK + pad_to(m % _CHUNK)) if m % _CHUNK else m
        # (means and variances as the two halves of ONE buffer: `predict` then brings both to the host in one transfer and one
        # synchronisation -- at the reference's test sizes a device-to-host copy is a tenth of the call)
        out_all = ops.empty(2 if diag else 1, nb, mtot, dtype=self.dtype)
        mean_all = out_all[0]
        var_all = out_all[1] if diag else None
        item = torch.empty(0, dtype=self.dtype).element_size()
        x_all = self._x_all
        for s in range(0, m, _CHUNK):
            xq = xpd[..., s: s + _CHUNK, :]
            xq = xq if xq.is_contiguous() else xq.contiguous()
            mc = xq.shape[-2]
            m_pad = pad_to(mc)
            # experts per launch group: every expert's K* (m_pad x n_pad) at once, within the memory budget
            per = m_pad * n_pad * item
            grp = max(1, min(nb, _group_budget(64 << 30, nb * per) // per))
            key = ("bat", grp, m_pad, n_pad, diag)
            if self._pbuf is None or self._pbuf[0] != key:
                self._pbuf = None
                self._pbuf = (key, ops.empty(grp, m_pad, n_pad, dtype=self.dtype), ops.empty(grp, (n_pad // 64) * m_pad, dtype=self.dtype))
            _, kt, work = self._pbuf
            for b0 in range(0, nb, grp):
                cnt = min(grp, nb - b0)
                xr = xq if xq.dim() == 2 else (xq[b0: b0 + cnt] if xq.shape[0] > 1 else xq[0])
                xc = x_all[b0: b0 + cnt] if x_all.shape[0] > 1 else x_all
                ops.kernel_build_batched(spec, bat["hp"][b0: b0 + cnt], xr, xc, kt[:cnt])
                ops.predict_mean_q_kt_batched(kt[:cnt], bat["minv"][b0: b0 + cnt] if diag else None, bat["alpha"][b0: b0 + cnt],
                                              mean_all[b0: b0 + cnt, s: s + m_pad], var_all[b0: b0 + cnt, s: s + m_pad] if diag else None,
                                              spec, bat["hp"][b0: b0 + cnt], work[:cnt])
        return [mean_all[b, :m] for b in range(nb)], ([var_all[b, :m] for b in range(nb)] if diag else [None] * nb)

    def _predict_device(self, xpd, want, padded=False):
        """Per-expert device tensors (mean[m], var[m] | cov[m,m] | None) for device-resident test points: xpd [m, d]
        (the same points for every expert) or [nc, m, d] (expert b predicts at xpd[b], as cov.kernel(params, x, xp)
        broadcasts in the reference, gpr.py:79)."""
        self._device_experts()
        self.update()
        if xpd.dim() == 3 and xpd.shape[0] not in (1, len(self._experts)):
            raise RuntimeError("batch dimension of xp (%d) does not match the %d experts" % (xpd.shape[0], len(self._experts)))
        if want == "full":       # K* is built once per expert there: mean, Vt and the update all come from it
            return self._predict_full([xpd if xpd.dim() == 2 else xpd[b % xpd.shape[0]] for b in range(len(self._experts))], padded)
        if self._bat is not None and len(self._experts) > 1 and not os.environ.get("PG_PREDICT_SERIAL"):
            self.last_predict_batched = True
            return self._predict_batched(xpd, want)
        self.last_predict_batched = False
        means, covs = [], []
        for b, e in enumerate(self._experts):
            xq = xpd if xpd.dim() == 2 else xpd[b % xpd.shape[0]]
            mu, cv = self._predict_expert(b, e, xq, want)
            means.append(mu)
            covs.append(cv)
        return means, covs

    def predict(self, xp: Tensor, var: str = "full") -> Sequence[Tensor]:
        """[mean, var | covariance | NotImplemented] at xp (gpr.py:76-120).  With grad mode on and xp.requires_grad the outputs come out of
        a torch.autograd.Function whose forward is this same path (identical values) and whose backward differentiates them in xp
        (`_PredictFn`)."""
        want = var if var in ("full", "diag") else "none"
        if torch.is_grad_enabled() and isinstance(xp, Tensor) and xp.requires_grad:
            out = _PredictFn.apply(self, want, xp, self.params, self._x, self._y)
            return [out, NotImplemented] if want == "none" else list(out)
        return self._predict_plain(xp, var)

    def _predict_plain(self, xp: Tensor, var: str) -> Sequence[Tensor]:
        ops = get_ops()
        want = var if var in ("full", "diag") else "none"
        xpd = ops.to_device(xp if xp.dim() == 2 else xp.reshape(-1, xp.shape[-2], xp.shape[-1]), self.dtype)
        means, covs = self._predict_device(xpd, want)
        # (the batched prediction hands out rows of ONE fresh buffer: the stacked result is a view of it, no stacking kernel)
        mstack = _stacked_rows(means) if len(means) > 1 else None
        if want == "diag" and self.batched and mstack is not None:
            cstack = _stacked_rows(covs)
            both = _stacked_pair(mstack, cstack) if cstack is not None else None
            if both is not None:       # [2, nc, m] view of one buffer: one transfer
                host = both.to(xp.device)
                return [host[0].squeeze(), host[1]]
        ys = (mstack if mstack is not None else torch.stack(means)).squeeze().to(xp.device)   # squeeze_(): drops every size-1 dim (gpr.py:87)
        if want == "none":
            covars = NotImplemented
        elif self.batched:
            cstack = _stacked_rows(covs) if want == "diag" else None
            covars = (cstack if cstack is not None else torch.stack(covs)).to(xp.device)
        else:
            covars = covs[0].contiguous().to(xp.device)
        return [ys, covars]

    # ---- derivatives in the test points ---------------------------------------------------------
    def predict_grad(self, xp: Tensor, var: str = "diag") -> Sequence[Tensor]:
        """[mean, var, dmean, dvar] (var="diag") or [mean, dmean] (var="none") without autograd: dmean[..., p, :] = d mean_p / d xp_p and
        dvar[..., p, :] = d var_p / d xp_p, shape [m, d] ([nc, m, d] for a batched model), in the model's dtype on xp's device.  Mean and
        variance are `predict`'s own (same path, same bits).  Both derivatives come out of one contraction launch (pg_kernel_xgrad:
        u = alpha, B = V = K* K^-1); V is only formed when the variance's derivative is asked for."""
        if var not in ("diag", "none"):
            raise ValueError("predict_grad: var must be 'diag' or 'none', got %r" % (var,))
        with torch.no_grad():
            mean, cov = self._predict_plain(xp, var)
            xpd = self._xp_device(xp)
            dmean, dvar = self._xgrad(xpd, var)
        dmean = self._grad_out(dmean, xp)
        if var == "none":
            return [mean, dmean]
        return [mean, cov, dmean, self._grad_out(-2.0 * dvar, xp)]

    def _xp_device(self, xp):
        return get_ops().to_device(xp if xp.dim() == 2 else xp.reshape(-1, xp.shape[-2], xp.shape[-1]), self.dtype)

    def _grad_out(self, g, xp):
        """[nexp, m, d] per-expert rows -> [m, d] for one expert, [nc, m, d] for a batched model, on xp's device."""
        return (g[0] if not self.batched else g).to(xp.device)

    def _xgrad(self, xpd, want, g_mu=None, g_var=None, g_cov=None):
        """Derivatives in the test points of every expert's prediction at xpd ([m, d] shared, or [nexp, m, d]; device, model dtype).
        Without upstream gradients (predict_grad): (out_u, out_b) [nexp, m, d] with out_u = d mean / dx* and out_b = sum_i V_pi dk_pi
        (want "diag"; -1/2 of d var / dx*).  With them (the autograd backward): the vector-Jacobian product [nexp, m, d] of
        g_mu [nexp, m] and g_var [nexp, m] (want "diag") or g_cov [nexp, m, m] (want "full").  Every expert in one batched contraction per
        chunk of test points; the weights V^T = K^-1 K*^T come from the GEMM core (pg_potrs against the cached L^-1) in buffers of their own
        -- never the forward's shared K* buffer."""
        ops = get_ops()
        self._device_experts()
        self.update()
        spec, _ = spec_of(self.cov, self._x.shape[-1])
        experts = self._experts
        nb = len(experts)
        if xpd.dim() == 3 and xpd.shape[0] not in (1, nb):
            raise RuntimeError("batch dimension of xp (%d) does not match the %d experts" % (xpd.shape[0], nb))
        n_pad = experts[0].n_pad
        m, d = xpd.shape[-2], xpd.shape[-1]
        bat = self._bat if (self._bat is not None and len(experts) > 1) else None
        hp_all = bat["hp"] if bat is not None else torch.stack([e.hp for e in experts])
        alpha_all = bat["alpha"] if bat is not None else torch.stack([e.alpha for e in experts])
        bwd = g_mu is not None
        out_u = ops.empty(nb, m, d, dtype=self.dtype)
        out_b = ops.empty(nb, m, d, dtype=self.dtype) if want != "none" else None
        chunk = m if want == "full" else _CHUNK
        for s in range(0, m, chunk):
            xq = xpd[..., s: s + chunk, :]
            xq = xq if xq.is_contiguous() else xq.contiguous()
            mc = xq.shape[-2]
            m_pad = pad_to(mc)
            ou, ob = out_u[:, s: s + mc], (out_b[:, s: s + mc] if out_b is not None else None)
            if want == "none":
                ops.kernel_xgrad_batched(spec, hp_all, xq, self._x_all, u_all=alpha_all, out_u=ou, nexp=nb)
                continue
            sym = None
            if want == "full":       # S = G + G^T, zero-padded
                sym = ops.zeros(nb, m_pad, m_pad, dtype=self.dtype)
                sym[:, :mc, :mc] = g_cov + g_cov.transpose(-1, -2)
            wt = ops.empty(nb, n_pad, m_pad, dtype=self.dtype)      # V^T (diag) or -K^-1 K*^T S = -(S V)^T (full), train-major
            ks = ops.empty(n_pad, m_pad, dtype=self.dtype)
            for b, e in enumerate(experts):
                ops.kernel_build(spec, e.hp, e.x, xq if xq.dim() == 2 else xq[b % xq.shape[0]], ks)      # K*^T = k(x, xp)
                rhs = ks
                if sym is not None:
                    rhs = ops.zeros(n_pad, m_pad, dtype=self.dtype)
                    ops.gemm_raw(_lib.GEMM_NN, n_pad, m_pad, m_pad, -1.0, ks, sym[b], 0.0, rhs)
                wt[b] = ops.potrs(e.chol, e.invd, rhs, minv=self._minv(e))
            if want == "diag":
                ops.kernel_xgrad_batched(spec, hp_all, xq, self._x_all, u_all=alpha_all, b_all=wt, out_u=ou, out_b=ob, trans_b=True, nexp=nb)
            else:    # the K** term (z = the test points, weights S), then the K* term and the mean's, accumulated onto it
                ops.kernel_xgrad_batched(spec, hp_all, xq, xq if xq.dim() == 3 else xq[None], b_all=sym, out_b=ob, nexp=nb)
                ou.zero_()
                ops.kernel_xgrad_batched(spec, hp_all, xq, self._x_all, u_all=alpha_all, b_all=wt, out_u=ou, out_b=ob, trans_b=True,
                                         accumulate=True, nexp=nb)
        if not bwd:
            return out_u, out_b
        g = out_u * g_mu[..., None]
        if want == "diag":
            g = g - 2.0 * (out_b * g_var[..., None])
        elif want == "full":
            g = g + out_b
        return g

    def _predict_vjp(self, xp, want, grads):
        """The backward of predict(xp, want) for the upstream gradients of its outputs: d<grads, outputs>/dxp in xp's shape, dtype, device.
        Experts that predict at one shared xp [m, d] add up; xp [nc, m, d] gets each expert's rows."""
        ops = get_ops()
        xpd = self._xp_device(xp)
        nb = len(self._device_experts())
        m = xpd.shape[-2]

        def dev(t, shape):
            return ops.zeros(*shape, dtype=self.dtype) if t is None else ops.to_device(t.reshape(shape), self.dtype)

        g_mu = dev(grads[0], (nb, m))
        if want == "none":
            g = self._xgrad(xpd, want, g_mu)
        elif want == "diag":
            g = self._xgrad(xpd, want, g_mu, g_var=dev(grads[1], (nb, m)))
        else:
            g = self._xgrad(xpd, want, g_mu, g_cov=dev(grads[1], (nb, m, m)))
        if xpd.dim() == 2 or xpd.shape[0] == 1:
            g = g.sum(0) if nb > 1 else g[0]
        return g.reshape(xp.shape).to(device=xp.device, dtype=xp.dtype)

    def predict_var(self, xp: Tensor, **kwargs: Tensor) -> Tensor:
        return self.predict(xp, var="diag")[1]

    def predict_covar(self, xp: Tensor, **kwargs: Tensor) -> Tensor:
        return self.predict(xp, var="full")[1]

    # ---- reference attributes, materialised on access ------------------------------------------
    def _stack(self, ts):
        out = torch.stack(ts) if self.batched else ts[0]
        return out.contiguous().to(self._x.device)

    @property
    def krn(self) -> Tensor:
        """K + 1e-7 I as `Exact_GP.krn` holds it after update (gpr.py:67-68); rebuilt on access."""
        self.update()
        ops = get_ops()
        spec, _ = spec_of(self.cov, self._x.shape[-1])
        outs = []
        for e in self._experts:
            k = ops.empty(e.n_pad, e.n_pad, dtype=self.dtype)
            ops.kernel_build(spec, e.hp, e.x, None, k, jitter=JITTER)
            outs.append(k[: e.n, : e.n])
        return self._stack(outs)

    @property
    def krnchd(self) -> Tensor:
        """Lower Cholesky factor with a zero upper triangle, like tc.cholesky (gpr.py:69)."""
        self.update()
        ops = get_ops()
        outs = []
        for e in self._experts:
            c = e.chol.clone()
            ops.tril(c, e.n_pad)
            outs.append(c[: e.n, : e.n])
        return self._stack(outs)

    @property
    def wt(self) -> Tensor:
        """alpha = K^-1 y (gpr.py:70-72): cholesky_solve(y[..., None], L) keeps y's leading dimensions."""
        self.update()
        out = self._stack([e.alpha[: e.n] for e in self._experts])
        return out.reshape(self._y.shape) if (not self.batched and self._y.dim() > 1) else out


class _PredictFn(torch.autograd.Function):
    """Exact_GP.predict as an autograd node in the test points.  forward: the library's prediction, unchanged (no grad: same values as a
    call without autograd).  backward: the vector-Jacobian product in xp through pg_kernel_xgrad (Exact_GP._xgrad):
      mean      d/dx*_p = g_mu_p sum_i alpha_i dk(x*_p, x_i)
      diag var  d/dx*_p = -2 g_var_p sum_i V_pi dk(x*_p, x_i)                       (K** has a constant diagonal)
      full cov  d/dx*_p = sum_q S_pq dk(x*_p, x*_q) - sum_i (S V)_pi dk(x*_p, x_i)   (S = G + G^T)
    Gradients flow to xp only: params / x / y that require grad make the backward raise NotImplementedError, and so does -- as a
    RuntimeError -- any change of the model (set_params, update, edits of x / y) between forward and backward."""

    @staticmethod
    def forward(ctx, model, want, xp, params, x, y):
        with torch.no_grad():
            ys, covars = model._predict_plain(xp, want)
        ctx.model, ctx.want, ctx.token = model, want, model._state_token()
        ctx.save_for_backward(xp)
        return ys if want == "none" else (ys, covars)

    @staticmethod
    def backward(ctx, *grads):
        for i, name in ((3, "params"), (4, "x"), (5, "y")):
            if ctx.needs_input_grad[i]:
                raise NotImplementedError("Exact_GP.predict: gradients flow to the test points xp only, but the model's `%s` requires grad"
                                          % name)
        model = ctx.model
        if model._state_token() != ctx.token:
            raise RuntimeError("Exact_GP.predict: the model changed (set_params / update / an edit of x or y) between the forward and the "
                               "backward of this prediction")
        (xp,) = ctx.saved_tensors
        g = model._predict_vjp(xp, ctx.want, grads) if ctx.needs_input_grad[2] else None
        return None, None, g, None, None, None


_DRAW_BYTES = 1 << 30   # PosteriorSampler.draw: Z and the product of one chunk of samples stay under this together


class PosteriorSampler:
    """A joint Gaussian N(mean, L L^T) at m points, as Exact_GP.sampler snapshots it: `mean` [m] ([nc, m] for a batched model), `chol`
    = L [m, m] ([nc, m, m]; lower, zero upper triangle; materialised on access like Exact_GP.krnchd), `m`, `dtype`, `noise`, `jitter`.
    The buffers are the sampler's own."""

    def __init__(self, mean_all, chol_all, m, device, batched, noise, jitter):
        self._mean, self._chol = mean_all, chol_all         # [nexp, m_pad], [nexp, m_pad, m_pad]: block-diag(L, I), upper triangle zero
        self.m, self.dtype, self.noise, self.jitter = int(m), chol_all.dtype, noise, jitter
        self._device, self._batched = device, batched

    def _shape(self, t):
        return (t if self._batched else t[0]).contiguous().to(self._device)

    @property
    def mean(self) -> Tensor:
        return self._shape(self._mean[:, : self.m])

    @property
    def chol(self) -> Tensor:
        return self._shape(self._chol[:, : self.m, : self.m])

    def draw(self, n_samples: int = 1, seed: int = 0, first: int = 0, z: Tensor = None) -> Tensor:
        """[n_samples, m] ([nc, n_samples, m] for a batched model) on xp's device: sample s is mean + L z_s with
        z_s = normal(seed, stream = expert index, first + s, .) from the library's generator (pygpr_amd.randn gives the same values), so
        draw(n, seed, first = k) continues draw(k, seed) without overlap.  With z given ([n_samples, m] or [nc, n_samples, m]) that array
        is used in place of the generator and n_samples, seed and first are ignored.  The samples are generated in chunks of rows
        (Z and the product of a chunk under 1 GiB); by the generator's construction the chunk size cannot change Z."""
        ops = get_ops()
        nexp, m_pad = self._chol.shape[0], self._chol.shape[1]
        m, dt = self.m, self.dtype
        if z is not None:
            if not isinstance(z, Tensor) or z.dim() not in (2, 3) or z.shape[-1] != m or (z.dim() == 3 and z.shape[0] != nexp) \
                    or (z.dim() == 2 and nexp > 1):
                raise ValueError("PosteriorSampler.draw: z must be [n_samples, %d]%s, got %s"
                                 % (m, " or [1, n_samples, %d]" % m if nexp == 1 else " with %d leading experts" % nexp,
                                    tuple(z.shape) if isinstance(z, Tensor) else type(z).__name__))
            n = z.shape[-2]
            zd = ops.to_device(z.reshape(nexp, n, m), dt)
        else:
            n = int(n_samples)
            if n < 0:
                raise ValueError("PosteriorSampler.draw: n_samples must not be negative, got %d" % n)
            if int(first) < 0:
                raise ValueError("PosteriorSampler.draw: first must not be negative, got %d" % int(first))
        out = ops.empty(nexp, n, m, dtype=dt)
        item = torch.empty(0, dtype=dt).element_size()
        chunk = max(128, (_DRAW_BYTES // (2 * nexp * m_pad * item)) // 128 * 128)
        for s0 in range(0, n, chunk):
            sc = min(chunk, n - s0)
            s_pad = pad_to(sc, 128)
            if z is not None:
                zs = ops.zeros(nexp, s_pad, m_pad, dtype=dt)
                zs[:, :sc, :m] = zd[:, s0: s0 + sc]
            else:
                zs = ops.empty(nexp, s_pad, m_pad, dtype=dt)
                for b in range(nexp):
                    ops.randn(zs[b], sc, m, seed, stream_id=b, row0=int(first) + s0)
            prod = ops.empty(nexp, s_pad, m_pad, dtype=dt)
            ops.trmm_lower_kt(self._chol, zs, prod)             # Z L^T, every expert in one launch
            torch.add(prod[:, :sc, :m], self._mean[:, None, :m], out=out[:, s0: s0 + sc])
        return (out if self._batched else out[0]).to(self._device)


def randn(rows: int, cols: int, seed: int = 0, stream: int = 0, first_row: int = 0, dtype=torch.float64) -> Tensor:
    """Host tensor [rows, cols] of the library's counter-based standard normals (include/pygpr_hip_sample.h: Philox4x32-10 and
    Box-Muller in fp64): element (r, q) = normal(seed, stream, first_row + r, q), whatever the shape asked for; float32 is the rounding of
    the float64 value.  What PosteriorSampler.draw multiplies with its factor (stream = expert index, first_row = first)."""
    rows, cols = int(rows), int(cols)
    if rows < 0 or cols < 0 or int(first_row) < 0:
        raise ValueError("randn: rows, cols and first_row must not be negative")
    if dtype not in (torch.float64, torch.float32):
        raise TypeError("randn computes in float64 or float32, got %s" % dtype)
    if rows == 0 or cols == 0:
        return torch.empty(rows, cols, dtype=dtype)
    ops = get_ops()
    return ops.randn(ops.empty(rows, cols, dtype=dtype), rows, cols, seed, stream_id=stream, row0=first_row).cpu()
