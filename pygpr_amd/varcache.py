"""Cached predictive variances for Iterative_GP, with error bounds certified up to a stated rounding model.  New, not in
the reference.

Iterative_GP's variance is one block solve per _RHS_BLOCK test points.  A `VarianceCache` replaces the solves by a Galerkin projection
of A^-1 onto a block-Krylov space that is built ONCE:

    B0 = [L | y | k(X, anchors)]                     the preconditioner's factor, the targets, the anchors' cross-covariance columns
    span(Q) = span[B0, A B0, ..., A^steps B0]        Q orthonormal, n x r, every product A Q_j a wide pg_kernel_matmul
    T = Q^T (A Q) = G G^T,   R = Q G^-T              T from actual products, mirrored; factored by pg_potrf
    var(x*) = k** - |k(x*, X) R|^2                   one cross product, no solve

Two properties of the projection carry the tests and the `bounds`:

  it never under-reports   Q (Q^T A Q)^-1 Q^T <= A^-1 for any orthonormal Q, so the cached variance is an upper bound of the exact one;
                           nested spans give nested bounds (monotone in `steps` and in added anchors); exact once the span is R^n.
  it certifies its error   the excess over the exact variance is r*^T A^-1 r* with r* = k* - A Q c* the Galerkin residual
                           (c* = T^-1 Q^T k*), and lambda_min(A) >= shift, hence 0 <= excess <= |r*|^2 / shift.

|r*|^2 = |k*|^2 - 2 c*^T (A Q)^T k* + c*^T (A Q)^T (A Q) c*.  Its first term, sum_j k(x*, x_j)^2, is not linear in k: it is
pg_kernel_rowsq (include/pygpr_hip_rowsq.h); the other two come from a second r-wide cross product against the kept A Q.

Rounding allowance.  The three terms cancel when the cache is good, so the gap carries a floor, FLOOR_MULT(n, r) 2^-53 |k*|^2 / shift,
FLOOR_MULT = 4 (n + 2 r + 66): the terms enter with weights 1, 2 and 1 and each is of the size of |k*|^2 when they cancel (4 |k*|^2 in
all); each is a sum of at most n + 2 r products taken in some fixed order, whose any-order bound is (n + 2 r + 2) 2^-53 of the sum of
the products' absolute values -- taken at the size of the term itself: exact for the first, whose products are squares, an assumption
for the other two -- and a covariance value carries up to 32 own_K <= 64 units of 2^-53 once it is squared (tests/rowsq_ref.py).  The
floor makes `lower` smaller, never larger: it cannot break the bracket, it only says below which size a certified gap is rounding.
"Certified" therefore means: in exact arithmetic the bracket is a theorem; in floating point it holds up to this rounding model, which
is a bound for the first term and an estimate for the two cross terms (their products are not same-signed, so the sum of their absolute
values can exceed the term) and leaves out the rounding already inside the stored A Q and inside c.  The tests check the bracket
against the dense answer.

Orthonormalisation.  A new block is scaled to unit columns, orthogonalised against everything before it (two products of the GEMM core,
repeated before every round below, so at least twice) and orthonormalised inside the block from the eigen-decomposition of its w x w
Gram matrix (formed by the GEMM core, decomposed on the host: w is a few hundred).  A Gram matrix squares the block's condition
number and its entries carry rounding of some w 2^-53, so one decomposition resolves a direction only while its part outside the span
so far -- its novelty -- is above some 1e-6 of the column it came from.  Three rounds therefore:
  1  W <- W V max(lambda, 1e-10)^-1/2: nothing is dropped, what is small is scaled up by at most 1e5;
  2  the same on the result, whose small eigenvalues are now novelty^2 / 1e-10: a direction with an eigenvalue at or below 1e-6, that is
     with a novelty at or below NOVELTY_TOL = 1e-8, is DROPPED -- never kept at tiny norm -- and counted in info["dropped"];
  3  once more, to polish: every eigenvalue is then 1 to some 1e-10 (a round that divides by sqrt(lambda) amplifies what the projection
     left inside the old span by as much, hence the projection before each).
info["orthogonality"] reports max |Q^T Q - I| of the result.  Whatever directions the rounds keep, the bound properties above hold for
ANY orthonormal Q, because T is formed from actual products A Q and never from a recurrence.
"""
from typing import Optional, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from . import _lib
from ._ops import JITTER, get_ops, pad_to
from .gpr import _checked, _lin_alg_error

NOVELTY_TOL = 1e-8   # a direction is dropped when its part outside the span so far is at most this fraction of its unit column
_FLOOR1 = 1e-10      # round one of the in-block orthonormalisation scales by max(eigenvalue, this)^-1/2 and drops nothing
# (drop at or below, floor) of the three rounds: scale up what is small, decide, polish
_ROUNDS = ((-np.inf, _FLOOR1), (NOVELTY_TOL ** 2 / _FLOOR1, 0.0), (0.5, 0.0))
_PASS = 32           # columns of one pg_kernel_matmul pass over the pairs
_Q_CHUNK = 2048      # test points per cross product: nothing larger than this x r is allocated by variance()
_S_BLOCK = 64        # test points whose n x 64 block S = R (K* R)^T one pg_kernel_xgrad call contracts
_ROW_CHUNK = 8192    # rows of Q turned into R at a time


def floor_multiple(n: int, r: int) -> int:
    """FLOOR_MULT(n, r) of the module docstring: the gap's rounding allowance in units of 2^-53 |k*|^2 / shift."""
    return 4 * (int(n) + 2 * int(r) + 66)


def _tn(m):
    return _lib.GEMM_TN_64 if m <= 2048 else _lib.GEMM_TN


class VarianceCache:
    """A snapshot of an Iterative_GP's posterior variance at the parameters it was built with: `variance`, `covariance`,
    `variance_grad` and `check` at any test points, none of them a solve.  Built by `Iterative_GP.variance_cache`.

    The cache owns R (n x rank) and, with bounds, A Q (n x rank), two rank x rank matrices and references to the fitted state it was
    built from (points, hyper-parameters on the device, shift): `set_params` or a refit of the model does not change a cache that
    exists -- build a new one.  `rank`: columns of the basis; `info`: steps, width (columns of the start block), products (columns
    multiplied by A) and passes (pg_kernel_matmul calls), dropped (directions the rank-revealing orthonormalisation left out),
    floor_multiple, orthogonality (max |Q^T Q - I|), bytes (what the cache itself allocated and holds: R, A Q and the two
    rank x rank matrices) and pinned_bytes (the fitted state's tensors the cache refers to and so keeps alive after the model has
    moved on: the points, the preconditioner's factor and capacitance matrix, alpha, the product's workspace -- `check` solves with
    them).  The points are the model's device tensor, not a copy: the snapshot covers `set_params` and refits, NOT an in-place edit
    of the model's x or y."""

    def __init__(self, model, steps: int = 2, anchors: Optional[Tensor] = None, bounds: bool = True, max_columns: int = 4096) -> None:
        if not (isinstance(steps, (int, np.integer)) and steps >= 0):
            raise ValueError("variance_cache: steps must be a non-negative integer, got %r" % (steps,))
        if not (isinstance(max_columns, (int, np.integer)) and max_columns >= 1):
            raise ValueError("variance_cache: max_columns must be a positive integer, got %r" % (max_columns,))
        if anchors is not None:
            model._check_xp(anchors, "variance_cache")
        ops = get_ops()
        model.update()
        st = model._state
        xd, pre = st["x"], st["pre"]
        n = xd.shape[0]
        m = 0 if pre is None else int(pre["m"])
        na = 0 if anchors is None else int(anchors.shape[0])
        w0 = m + 1 + na
        if (int(steps) + 1) * w0 > max_columns:
            raise ValueError("variance_cache: (steps + 1) x (rank + 1 + anchors) = %d x %d columns exceed max_columns = %d; lower steps or "
                             "the number of anchors, or raise max_columns" % (steps + 1, w0, max_columns))
        self._model, self._st, self._bounds = model, st, bool(bounds)
        self._build(ops, int(steps), anchors, w0)

    # ---- the build ----------------------------------------------------------------------------
    def _times_a(self, ops, v, out, cols):
        """out[:n, :cols] = A v[:n, :cols] on padded buffers, one pg_kernel_matmul per _PASS columns on the model's workspace."""
        st = self._st
        xd, n = st["x"], st["x"].shape[0]
        work = st.get("work")
        need = ops.kernel_matmul_worksize(n, n, _PASS)
        if need > 0 and (work is None or work.numel() < need):
            work = ops.empty(need)
        for c in range(0, cols, _PASS):
            c1 = min(cols, c + _PASS)
            ops.kernel_matmul(st["full_spec"], st["hpd"], xd, None, v[:n, c:c1], out=out[:n, c:c1], jitter=self._jitter, work=work)
            self.info["passes"] += 1
        self.info["products"] += cols

    def _project(self, ops, w, wpad, q, rcap, npad):
        """w -= Q (Q^T w): two products of the GEMM core (the unused columns of Q are zero)."""
        coef = ops.empty(rcap, wpad)
        ops.gemm_raw(_tn(rcap), rcap, wpad, npad, 1.0, q, w, 0.0, coef)
        ops.gemm_raw(_lib.GEMM_NN, npad, wpad, rcap, -1.0, q, coef, 1.0, w)

    def _orthonormal_in_block(self, ops, w, width, wpad, npad, drop, floor):
        """(w V D [npad, wpad], kept) from the eigen-decomposition of the block's Gram matrix, V its eigenvectors with an eigenvalue above
        `drop` and D = diag(max(eigenvalue, floor)^-1/2)."""
        gram = ops.empty(wpad, wpad)
        ops.gemm_raw(_tn(wpad), wpad, wpad, npad, 1.0, w, w, 0.0, gram)
        g = gram[:width, :width].cpu().numpy()                          # (one synchronisation per round)
        lam, vec = np.linalg.eigh(0.5 * (g + g.T))
        keep = lam > drop
        kept = int(keep.sum())
        tm = np.zeros((wpad, wpad))
        tm[:width, :kept] = vec[:, keep][:, ::-1] / np.sqrt(np.maximum(lam[keep][::-1], floor))      # the largest eigenvalue first
        out = ops.empty(npad, wpad)
        ops.gemm_raw(_lib.GEMM_NN, npad, wpad, wpad, 1.0, w, ops.to_device(torch.from_numpy(tm), torch.float64), 0.0, out)
        return out, kept

    def _build(self, ops, steps, anchors, w0):
        st = self._st
        xd, hpd, spec, pre = st["x"], st["hpd"], st["spec"], st["pre"]
        n = xd.shape[0]
        npad = pad_to(n)
        self._jitter = JITTER
        self.info = dict(steps=steps, width=w0, products=0, passes=0, dropped=0)
        rcap = pad_to(min((steps + 1) * w0, n))
        wpad = pad_to(w0)
        q = ops.zeros(npad, rcap)
        aq = ops.zeros(npad, rcap) if self._bounds else None
        t = ops.zeros(rcap, rcap)

        # the start block [L | y | k(X, anchors)]
        w = ops.zeros(npad, wpad)
        m = 0 if pre is None else int(pre["m"])
        if m:
            w[:n, :m] = pre["L"][:n, :m]
        w[:n, m] = self._model._device_data()[1]
        if anchors is not None and anchors.shape[0]:
            ad = ops.to_device(anchors.detach(), torch.float64)
            ka = ops.empty(npad, pad_to(ad.shape[0]))
            ops.kernel_build(spec, hpd, xd, ad, ka)                     # k(x, anchors), zero in the padding
            w[:n, m + 1: w0] = ka[:n, : ad.shape[0]]
            del ka

        r, width = 0, w0
        for j in range(steps + 1):
            width = min(width, n - r)                                   # (no more directions than the complement holds)
            norms = w[:n, :width].norm(dim=0)
            w[:, :width] *= torch.where(norms > 0, 1.0 / norms, torch.zeros_like(norms))
            w[:, width:] = 0.0
            if r:
                self._project(ops, w, wpad, q, rcap, npad)
            blk, kept = w, width
            for drop, floor in _ROUNDS:
                if r:
                    self._project(ops, blk, wpad, q, rcap, npad)
                blk, left = self._orthonormal_in_block(ops, blk, kept, wpad, npad, drop, floor)
                self.info["dropped"] += kept - left
                kept = left
                if kept == 0:
                    break
            if kept == 0:
                break
            q[:, r: r + kept] = blk[:, :kept]
            blk[:, kept:] = 0.0
            w = ops.zeros(npad, wpad)
            self._times_a(ops, blk, w, kept)                            # A Q_j: T's block row, and the next block
            row = ops.empty(wpad, rcap)
            ops.gemm_raw(_tn(wpad), wpad, rcap, npad, 1.0, w, q, 0.0, row)      # (A Q_j)^T [Q_0 .. Q_j]
            t[r: r + kept, : r + kept] = row[:kept, : r + kept]
            dg = t[r: r + kept, r: r + kept]
            dg.copy_(0.5 * (dg + dg.t()))
            if aq is not None:
                aq[:, r: r + kept] = w[:, :kept]
            r += kept
            width = kept
            if r >= n:
                break
        if r == 0:
            raise ValueError("variance_cache: the start block holds no direction (y and every column are zero)")
        self.rank = r

        gram = ops.empty(rcap, rcap)
        ops.gemm_raw(_tn(rcap), rcap, rcap, npad, 1.0, q, q, 0.0, gram)
        eye = torch.eye(r, dtype=torch.float64, device=gram.device)
        self.info["orthogonality"] = float((gram[:r, :r] - eye).abs().max())

        # T = G G^T (lower block rows; the upper triangle is their mirror), the identity in the padding; Li = G^-1
        t.diagonal()[r:].fill_(1.0)
        info = torch.zeros(1, dtype=torch.int32, device=t.device)
        out = {}

        def enqueue():
            g = t.clone()
            invd = ops.empty(ops.potrf_worksize(rcap, torch.float64))
            ops.potrf(g, invd, info)
            li = ops.empty(rcap, rcap)
            ops.trtri(g, invd, li)
            ops.tril(li, rcap)                                          # (pg_trtri leaves scratch above the diagonal: the gap's product reads all of Li)
            out.update(li=li)

        for s in _checked(enqueue, lambda: info.tolist()):
            if s:
                raise _lin_alg_error(s, " -- the variance cache's projected matrix Q^T A Q")
        li = out["li"]
        for s in range(0, npad, _ROW_CHUNK):                            # R = Q G^-T, in place chunk by chunk
            rows = min(_ROW_CHUNK, npad - s)
            tmp = ops.empty(rows, rcap)
            ops.trmm_lower_kt(li, q[s: s + rows], tmp)
            q[s: s + rows] = tmp
        self._r, self._rcap = q, rcap
        self._aq = self._li = self._gram = None
        if self._bounds:
            self._aq, self._li = aq, li
            self._gram = ops.empty(rcap, rcap)
            ops.gemm_raw(_tn(rcap), rcap, rcap, npad, 1.0, aq, aq, 0.0, self._gram)
        self.info["floor_multiple"] = floor_multiple(n, r)
        self.info["bytes"] = sum(8 * v.numel() for v in (self._r, self._aq, self._li, self._gram) if v is not None)
        pinned = [st["x"], st["hpd"], st.get("alpha"), st.get("work")] + ([pre[k] for k in ("L", "C", "invd")] if pre is not None else [])
        self.info["pinned_bytes"] = sum(v.element_size() * v.numel() for v in pinned if v is not None)

    # ---- evaluation -----------------------------------------------------------------------------
    def _device_points(self, xp: Tensor, who: str) -> Tensor:
        self._model._check_xp(xp, who)
        return get_ops().to_device(xp.detach(), torch.float64)

    def _cross(self, ops, xpd, v):
        """k(xpd, X) v[:n, :rank] as the leading block of a zero [pad(q), rcap] buffer."""
        st = self._st
        n, qc = st["x"].shape[0], xpd.shape[0]
        u = ops.zeros(pad_to(qc), self._rcap)
        if qc:
            ops.kernel_matmul(st["spec"], st["hpd"], xpd, st["x"], v[:n, : self.rank], out=u[:qc, : self.rank])
        return u

    def _gap(self, ops, xpd, u):
        """The certified gap at the points xpd whose k* R is u (padded)."""
        st = self._st
        qc, qpad, rcap = xpd.shape[0], u.shape[0], self._rcap
        ksq = ops.kernel_rowsq(st["spec"], st["hpd"], xpd, st["x"])
        z = self._cross(ops, xpd, self._aq)                              # k* (A Q)
        c = ops.empty(qpad, rcap)
        ops.gemm_raw(_lib.GEMM_NN, qpad, rcap, rcap, 1.0, u, self._li, 0.0, c)          # c^T = u^T G^-1
        cm = ops.empty(qpad, rcap)
        ops.gemm_raw(_lib.GEMM_NN, qpad, rcap, rcap, 1.0, c, self._gram, 0.0, cm)
        res = ksq - 2.0 * (c[:qc] * z[:qc]).sum(1) + (cm[:qc] * c[:qc]).sum(1)
        floor = self.info["floor_multiple"] * 2.0 ** -53 * ksq
        return (res.clamp_min(0.0) + floor) / st["shift"]

    def _chunks(self, ops, xpd, bounds):
        """(start, u, var, gap) chunk by chunk: variance, variance_grad and check share this path, so their bits agree."""
        for s in range(0, xpd.shape[0], _Q_CHUNK):
            xc = xpd[s: s + _Q_CHUNK]
            u = self._cross(ops, xc, self._r)
            var = self._st["kss"] - (u[: xc.shape[0]] * u[: xc.shape[0]]).sum(1)
            yield s, xc, u, var, (self._gap(ops, xc, u) if bounds else None)

    def variance(self, xp: Tensor, bounds: bool = False) -> Union[Tensor, Tuple[Tensor, Tensor]]:
        """var [q] of y* at xp [q, d], on xp's device: k** - |k(xp, X) R|^2, an UPPER bound of the exact variance, not clamped.
        bounds=True: (upper, lower) with upper the same figure and lower = upper - gap, gap = max(|r*|^2, 0) / shift + floor (the
        module docstring): exact lies in [lower, upper], certified up to the module docstring's rounding model.  Costs a second r-wide cross
        product and one pg_kernel_rowsq; ValueError on a cache built with bounds=False."""
        if bounds and not self._bounds:
            raise ValueError("VarianceCache.variance: this cache was built with bounds=False; build one with bounds=True")
        xpd = self._device_points(xp, "variance")
        ops = get_ops()
        upper, lower = ops.empty(xpd.shape[0]), (ops.empty(xpd.shape[0]) if bounds else None)
        for s, xc, _, var, gap in self._chunks(ops, xpd, bounds):
            upper[s: s + xc.shape[0]] = var
            if bounds:
                lower[s: s + xc.shape[0]] = var - gap
        return (upper.to(xp.device), lower.to(xp.device)) if bounds else upper.to(xp.device)

    def covariance(self, xp: Tensor) -> Tensor:
        """cov [q, q] of y* at xp: K** - (K* R)(K* R)^T with the noise on the diagonal of K**, the upper triangle the mirror of the
        lower as in Iterative_GP.predict: exactly symmetric.  Minus the exact covariance it is positive semi-definite."""
        xpd = self._device_points(xp, "covariance")
        ops = get_ops()
        st = self._st
        q = xpd.shape[0]
        qp = pad_to(q)
        cov = ops.empty(qp, qp)
        ops.kernel_build(st["full_spec"], st["hpd"], xpd, None, cov)     # K** incl. sigma_n^2, identity in the padding
        u = ops.zeros(qp, self._rcap)
        for s in range(0, q, _Q_CHUNK):
            xc = xpd[s: s + _Q_CHUNK]
            ops.kernel_matmul(st["spec"], st["hpd"], xc, st["x"], self._r[: st["x"].shape[0], : self.rank],
                              out=u[s: s + xc.shape[0], : self.rank])
        ops.gemm_raw(_lib.GEMM_NT, qp, qp, self._rcap, -1.0, u, u, 1.0, cov)
        ops.symmetrize(cov, qp)
        return cov[:q, :q].contiguous().to(xp.device)

    def variance_grad(self, xp: Tensor) -> Tuple[Tensor, Tensor]:
        """(var [q], dvar [q, d]): var has the bits of variance(xp); dvar[p] = d var_p / d xp_p = -2 sum_i S_ip dk(xp_p, x_i)/dxp_p with
        S = R (K* R)^T taken in n x 64 blocks through pg_kernel_xgrad's B form, as Iterative_GP.predict_grad takes its block solves
        (K** has a constant diagonal, so there is no other term)."""
        xpd = self._device_points(xp, "variance_grad")
        ops = get_ops()
        st = self._st
        xd = st["x"]
        n, npad, rcap = xd.shape[0], pad_to(xd.shape[0]), self._rcap
        cols = 128                                                       # the GEMM core's column tile: one block's buffer
        var, dvar = ops.empty(xpd.shape[0]), ops.empty(xpd.shape[0], xd.shape[1])
        for s, xc, u, v, _ in self._chunks(ops, xpd, False):
            var[s: s + xc.shape[0]] = v
            for b in range(0, xc.shape[0], _S_BLOCK):
                qb = min(_S_BLOCK, xc.shape[0] - b)
                ub = ops.zeros(cols, rcap)
                ub[:qb] = u[b: b + qb]
                sb = ops.empty(npad, cols)
                ops.gemm_raw(_lib.GEMM_NT, npad, cols, rcap, 1.0, self._r, ub, 0.0, sb)      # S_b = R (K*_b R)^T
                ops.kernel_xgrad(st["spec"], st["hpd"], xc[b: b + qb], xd, b=sb[:n], out_b=dvar[s + b: s + b + qb], trans_b=True)
        dvar.mul_(-2.0)
        return var.to(xp.device), dvar.to(xp.device)

    def check(self, xp: Tensor) -> dict:
        """The cache against the model's own block solve at up to _RHS_BLOCK points: `excess`, the largest cached-minus-solved
        variance, and `gap`, the largest certified gap there (None without bounds).  One block solve at the snapshot's parameters
        and the model's tol: the price of 64 variances the old way."""
        from . import iterative

        xpd = self._device_points(xp, "check")
        if not 1 <= xpd.shape[0] <= int(iterative._RHS_BLOCK):
            raise ValueError("VarianceCache.check: at least one and at most %d points (one block solve)" % int(iterative._RHS_BLOCK))
        ops = get_ops()
        gap = None
        for _, _, _, upper, g in self._chunks(ops, xpd, self._bounds):
            gap = g
        exact = self._model._diag_variance(ops, self._st, xpd)
        return dict(excess=float((upper - exact).max()), gap=None if gap is None else float(gap.max()))
