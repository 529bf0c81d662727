"""Nearest-neighbour (Vecchia) GP regression on the MI355X.  New, not in the reference.

Every point is conditioned on its at most m nearest predecessors N(i) in an ordering pi of the training points,

    p(y) ~ prod_i p(y_i | y_N(i)),

so fitting, the loss, its gradient and prediction cost O(n m^3) time and O(n m) memory; with m >= n - 1 the model is the exact GP.
With the block B_i = (N(i), i), the target last, A_B the matrix Exact_GP factors restricted to the block (JITTER on its diagonal),
c = A_B^-1 e_last / (A_B^-1)_last,last, v = 1 / (A_B^-1)_last,last and r = c^T y_B:

    loss  = sum_i 1/2 [log v_i + r_i^2 / v_i + log 2 pi],        conditional mean y_i - r_i, conditional variance v_i
    grad  = 1/2 sum_i sum_{p,q in B_i} W_pq dA_pq/dtheta,   W = (1/v - (r/v)^2) c c^T - (r/v)(a c^T + c a^T),   a = [A_NN^-1 y_N ; 0]

and a prediction at x* conditions on the m nearest training points of x* (no ordering constraint), with the prior variance plus the
noise and no jitter on x*'s own diagonal entry, as Exact_GP._kss_diag.  Everything per block runs inside one wavefront
(include/pygpr_hip_vecchia.h): nothing n x n, or n x m x m, is ever written.

The neighbour sets come from a brute-force search (pg_knn) on the unscaled coordinates at the first update() after the data changed
and are then KEPT while the parameters move, so that the loss is a smooth function of the parameters; `refresh_neighbours` recomputes
them in the metric of the current length scales.  x and y stay in the user's order everywhere: the permutation is internal.
`Vecchia_MLE(model)` follows MLE's protocol, so `CG(Vecchia_MLE(model))` trains the model.  Batched models, float32 and covariances
longer than one pg_covspec are not served; the joint predictive covariance, derivatives in the test points, a maxmin ordering,
grouped blocks and a sub-quadratic search are left out."""
from typing import Sequence

import numpy as np
import torch
from numpy import ndarray
from torch import Tensor

from ._ops import JITTER, get_ops
from .covar import Covar, spec_of, terms
from .gpr import _CHUNK, GPR, _lin_alg_error
from .loss import _MemoLoss

_MAX_NEIGHBOURS = 63        # a block is one wavefront: 63 neighbours and the target
_TARGET_CHUNK = 1 << 18     # targets per pg_vecchia_nlml_grad call; an evaluation is the sum of its chunks in chunk order


class Vecchia_GP(GPR):
    """Nearest-neighbour GP: x [n, d], y [n] float64, params as Exact_GP's.  neighbours: m, 1 .. 63.  order: None (as given), "random"
    (a permutation drawn from `seed`) or an integer tensor holding a permutation of 0 .. n - 1 (position -> point)."""

    _matrix_free = True      # MLE / LOO refuse such a model: there is no factor of the n x n matrix

    def __init__(self, x: Tensor, y: Tensor, cov: Covar, neighbours: int = 30, order=None, seed: int = 0) -> None:
        super().__init__(x, y, cov)
        if not 1 <= int(neighbours) <= _MAX_NEIGHBOURS:
            raise ValueError("Vecchia_GP: neighbours must be 1 .. %d, got %r" % (_MAX_NEIGHBOURS, neighbours))
        self._m = int(neighbours)
        self._order_arg, self._seed = order, int(seed)
        self._check_data()
        passes, _ = spec_of(cov, x.shape[-1])
        if len(passes) != 1:
            raise NotImplementedError("Vecchia_GP: covariances that need more than one pg_covspec pass are not supported")
        self.params: Tensor = cov.init_params(x)
        self._dev = self._dev_key = self._perm = None
        self._nbr = None            # [n, m] int32 on the device, positions in the ordering
        self._nbr_version = 0       # bumped whenever the table is computed again: part of Vecchia_MLE's memo key
        self._scale = None          # the search's per-coordinate scales (None: unscaled), also the prediction's
        self._terms = None          # (cond_mean, cond_var, nlml) of the last update()
        self.need_upd = True

    # ---- data -------------------------------------------------------------------------------
    @property
    def dtype(self):
        return torch.float64

    def _data_changed(self) -> None:
        self._dev = self._nbr = self._terms = None
        self.need_upd = True

    def _check_data(self) -> None:
        x, y = self._x, self._y
        for name, t in (("x", x), ("y", y)):
            if t.dtype != torch.float64:
                raise NotImplementedError("Vecchia_GP computes in float64 only; %s is %s" % (name, t.dtype))
        if x.dim() != 2 or y.dim() != 1:
            raise NotImplementedError("Vecchia_GP: batched models are not supported (x [n, d], y [n])")
        if y.shape[0] != x.shape[0] or x.shape[0] < 1:
            raise ValueError("Vecchia_GP: x holds %d points, y %d values" % (x.shape[0], y.shape[0]))

    def _permutation(self, n) -> Tensor:
        o = self._order_arg
        if o is None:
            return torch.arange(n, dtype=torch.int64)
        if isinstance(o, str):
            if o != "random":
                raise ValueError("Vecchia_GP: order is None, \"random\" or a permutation, got %r" % o)
            return torch.randperm(n, generator=torch.Generator().manual_seed(self._seed))
        p = torch.as_tensor(o).detach().cpu()
        if p.dtype.is_floating_point or p.dtype == torch.bool or p.dim() != 1 or p.numel() != n:
            raise ValueError("Vecchia_GP: order must be an integer permutation of 0 .. %d" % (n - 1))
        p = p.to(torch.int64)
        if not torch.equal(torch.sort(p).values, torch.arange(n, dtype=torch.int64)):
            raise ValueError("Vecchia_GP: order is not a permutation of 0 .. %d" % (n - 1))
        return p

    def _device_data(self):
        """(x, y) in the ORDERING on the device, uploaded once per (tensor identity, version)."""
        key = tuple(v for t in (self._x, self._y) for v in (id(t), t._version))
        if self._dev is None or self._dev_key != key:
            self._check_data()
            ops = get_ops()
            self._perm = self._permutation(self._x.shape[0])
            self._dev = (ops.to_device(self._x[self._perm.to(self._x.device)], torch.float64),
                         ops.to_device(self._y[self._perm.to(self._y.device)], torch.float64))
            self._dev_key = key
            self._nbr = self._terms = None
            self.need_upd = True
        return self._dev

    def _hp_host(self, params=None) -> ndarray:
        p = self.params if params is None else params
        p = p.detach().cpu().numpy() if isinstance(p, Tensor) else np.asarray(p)
        _, nhp = spec_of(self.cov, self._x.shape[-1])
        if p.shape[-1] != nhp or p.reshape(-1, nhp).shape[0] != 1:
            raise NotImplementedError("Vecchia_GP: batched hyper-parameters are not supported (params [%d])" % nhp)
        return np.array(p.reshape(nhp), dtype=np.float64)

    # ---- neighbours -------------------------------------------------------------------------
    def _search(self, scale) -> None:
        xd, _ = self._device_data()
        ops = get_ops()
        self._scale = None if scale is None else ops.to_device(torch.as_tensor(np.asarray(scale, dtype=np.float64)), torch.float64)
        self._nbr = ops.knn(xd, xd, self._m, s=self._scale, causal=True)
        self._nbr_version += 1
        self._terms = None
        self.need_upd = True

    def _table(self) -> Tensor:
        self._device_data()
        if self._nbr is None:
            self._search(None)
        return self._nbr

    def refresh_neighbours(self, scaled: bool = True) -> None:
        """Search the neighbour sets again: scaled=True in the metric of the first stationary component's length scales at the current
        params (l multiplies x here: the distance is sum_k (l_k D_k)^2), scaled=False on the plain coordinates.  The model turns
        dirty and a Vecchia_MLE on it drops its memo."""
        scale = None
        if scaled:
            d = self._x.shape[-1]
            tms, _, _ = terms(self.cov, d)
            if not tms:
                raise ValueError("Vecchia_GP.refresh_neighbours(scaled=True): the covariance has no stationary component")
            off = tms[0][2][0]
            scale = self._hp_host()[off + 1: off + 1 + d]
        self._search(scale)

    @property
    def neighbours(self) -> Tensor:
        """[n, m] int64 on the host: row i holds the points that point i (user order) is conditioned on, nearest first, -1 padding."""
        nb = self._table().cpu().to(torch.int64)
        perm = self._perm
        user = torch.where(nb >= 0, perm[nb.clamp(min=0)], torch.full_like(nb, -1))
        out = torch.empty_like(user)
        out[perm] = user
        return out

    # ---- the conditional terms ------------------------------------------------------------------
    def _evaluate(self, hp: ndarray, want_grad: bool, keep: bool = False):
        """(loss, grad | None) at the host vector hp: the targets in chunks, everything enqueued before the ONE synchronisation that
        reads the status words and the sums; the chunks' sums are added in chunk order."""
        xd, yd = self._device_data()
        nbr = self._table()
        ops = get_ops()
        n, d = xd.shape
        (spec,), nhp = spec_of(self.cov, d)
        hpd = ops.to_device(torch.from_numpy(np.ascontiguousarray(hp)), torch.float64)
        chunks = [(s, min(_TARGET_CHUNK, n - s)) for s in range(0, n, _TARGET_CHUNK)]
        cm, cv = ops.empty(n, dtype=torch.float64), ops.empty(n, dtype=torch.float64)
        sums = ops.zeros(len(chunks), nhp + 1, dtype=torch.float64)
        info = ops.zeros(len(chunks), dtype=torch.int32)
        for i, (s, cnt) in enumerate(chunks):
            ops.vecchia_nlml_grad(spec, hpd, xd, yd, nbr[s: s + cnt], s, cnt, JITTER, want_grad, cm[s: s + cnt], cv[s: s + cnt],
                                  sums[i, nhp:], sums[i, :nhp], info[i: i + 1])
        info_h, sums_h = info.cpu().numpy(), sums.cpu().numpy()
        bad = [int(v) for v in info_h if v > 0]
        if bad:
            point = int(self._perm[min(bad) - 1])
            raise _lin_alg_error(point + 1, " (Vecchia_GP: the conditional block of point %d, position %d of the ordering)" % (point, min(bad) - 1))
        loss, grad = 0.0, np.zeros(nhp)
        for row in sums_h:      # chunk order
            loss = loss + float(row[nhp])
            grad = grad + row[:nhp]
        if keep:
            perm = self._perm.to(cm.device)
            cmu, cvu = torch.empty_like(cm), torch.empty_like(cv)
            cmu[perm], cvu[perm] = cm, cv
            self._terms = (cmu, cvu, loss)
        return np.array(loss), (grad if want_grad else None)

    def update(self) -> None:
        self._device_data()                  # first: an in-place edit of x / y (version bump) marks the model dirty here
        self._table()
        if self.need_upd or self._terms is None:
            self._evaluate(self._hp_host(), want_grad=False, keep=True)
            self.need_upd = False
        return None

    def _term(self, i):
        if self.need_upd or self._terms is None:
            raise RuntimeError("Vecchia_GP: call update() first (the data or the parameters changed)")
        return self._terms[i]

    @property
    def cond_mean(self) -> Tensor:
        """E[y_i | y_N(i)] of every training point, user order (after update())."""
        return self._term(0)

    @property
    def cond_var(self) -> Tensor:
        """var[y_i | y_N(i)] of every training point, user order (after update())."""
        return self._term(1)

    @property
    def nlml(self) -> float:
        """The Vecchia loss at the current params (after update())."""
        return self._term(2)

    # ---- prediction -------------------------------------------------------------------------
    def predict(self, xp: Tensor, var: str = "diag") -> Sequence[Tensor]:
        """[mean, var] (var="diag") or [mean] (var="none") of y* at xp [q, d], each point conditioned on its m nearest training
        points (in the metric of the last neighbour search); the test points are chunked.  var="full": the joint covariance of a
        Vecchia model is not implemented."""
        if var == "full":
            raise NotImplementedError("Vecchia_GP.predict(var=\"full\"): the joint predictive covariance is not implemented; var=\"diag\" "
                                      "gives the marginal variances")
        if var not in ("diag", "none"):
            raise ValueError("Vecchia_GP.predict: var is \"diag\" or \"none\", got %r" % (var,))
        if torch.is_grad_enabled() and isinstance(xp, Tensor) and xp.requires_grad:
            raise NotImplementedError("Vecchia_GP.predict is not differentiable in the test points")
        if xp.dim() != 2 or xp.shape[1] != self._x.shape[1] or xp.dtype != torch.float64:
            raise ValueError("Vecchia_GP.predict: xp must be [q, %d] float64" % self._x.shape[1])
        xd, yd = self._device_data()
        ops = get_ops()
        n, d = xd.shape
        (spec,), _ = spec_of(self.cov, d)
        hpd = ops.to_device(torch.from_numpy(self._hp_host()), torch.float64)
        xq = ops.to_device(xp, torch.float64)
        q = xq.shape[0]
        mean = ops.empty(q, dtype=torch.float64)
        vr = ops.empty(q, dtype=torch.float64) if var == "diag" else None
        starts = list(range(0, q, _CHUNK))
        info = ops.zeros(max(len(starts), 1), dtype=torch.int32)
        for i, s in enumerate(starts):
            e = min(s + _CHUNK, q)
            nb = ops.knn(xq[s:e], xd, self._m, s=self._scale, causal=False)
            ops.vecchia_predict(spec, hpd, xd, yd, xq[s:e], nb, JITTER, mean[s:e], None if vr is None else vr[s:e], info[i: i + 1])
        for i, v in enumerate(info.cpu().numpy()):
            if v > 0:
                at = starts[i] + int(v) - 1
                raise _lin_alg_error(at + 1, " (Vecchia_GP.predict: the conditional block of test point %d)" % at)
        return [mean, vr] if var == "diag" else [mean]

    def predict_grad(self, xp: Tensor, var: str = "diag") -> Sequence[Tensor]:
        raise NotImplementedError("Vecchia_GP has no derivatives in the test points; fit an Exact_GP or a Sparse_GP")


class Vecchia_MLE(_MemoLoss):
    """The Vecchia loss of a Vecchia_GP as a training objective with MLE's protocol (`CG(Vecchia_MLE(model))`): loss, grad and
    loss_and_grad take and return host float64, memoised on (parameters, data, covariance, the neighbour table).  The neighbour sets
    are the model's and stay fixed between calls; model.refresh_neighbours() drops the memo."""

    def __init__(self, model: Vecchia_GP) -> None:
        if not isinstance(model, Vecchia_GP):
            raise TypeError("Vecchia_MLE is the loss of a Vecchia_GP, got %s" % type(model).__name__)
        super().__init__(model)
        self._nbr_seen = None

    def _evaluate(self, params: ndarray, want_grad: bool):
        m = self.model
        table = m._table()      # (the memo's key holds x, y and the covariance: the table is the model's own)
        token = (id(table), m._nbr_version)
        if token != self._nbr_seen:
            self._memo = None
            self._nbr_seen = token
        return super()._evaluate(params, want_grad)

    def _evaluate_device(self, params: ndarray, want_grad: bool, key=None, reuse_factor=False):
        m = self.model
        return m._evaluate(m._hp_host(np.asarray(params, dtype=np.float64)), want_grad)
