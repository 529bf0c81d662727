"""Dense NumPy restatement of pygpr_amd/varcache.py on tests/iterative_ref.py's operator and preconditioner factor: the same start
block, the same block-Krylov span, the same Galerkin projection -- with the n x n matrix, which is the point of a reference.

    B0 = [L | y | k(X, anchors)],  span(Q) = span[B0, A B0, ..., A^steps B0],  T = Q^T A Q,  R = Q chol(T)^-T
    upper = k** - |R^T k*|^2,      lower = upper - (max(|k* - A Q c|^2, 0) / shift + floor),   c = T^-1 Q^T k*

The variance depends on the span alone, not on the basis, so the block is orthonormalised in TWO ways -- eigen-decomposition of the
block's Gram matrix (what the device does) and column-pivoted QR -- and the disagreement of the two is the restatement's own error
(`own_error`).  Both drop a direction whose part outside the span so far is at most NOVELTY_TOL = 1e-8 of its unit column."""
import numpy as np
import scipy.linalg as sla

import iterative_ref as ir
import matmul_ref as mr

NOVELTY_TOL = 1e-8      # a direction is dropped when its part outside the span so far is at most this fraction of its unit column
FLOOR1 = 1e-10          # the eigen-decomposition's first round scales by max(eigenvalue, this)^-1/2


def floor_multiple(n, r):
    """The gap's rounding allowance in units of 2^-53 |k*|^2 / shift (pygpr_amd/varcache.py derives it)."""
    return 4 * (n + 2 * r + 66)


def start_block(terms, hp, x, y, rank, anchors=None):
    l, _ = ir.factor_l(terms, hp, x, rank)
    cols = [l, np.asarray(y)[:, None]]
    if anchors is not None and len(anchors):
        cols.append(mr.stationary_kernel(terms, hp, x, anchors))
    return np.concatenate(cols, 1)


def _project(w, q):
    return w - q @ (q.T @ w)


def _block_eigh(w, q):
    """The device's three rounds on the Gram matrix: scale up what is small, decide, polish -- a projection before each."""
    dropped = 0
    for drop, floor in ((-np.inf, FLOOR1), (NOVELTY_TOL ** 2 / FLOOR1, 0.0), (0.5, 0.0)):
        w = _project(w, q)
        g = w.T @ w
        lam, vec = np.linalg.eigh(0.5 * (g + g.T))
        keep = lam > drop
        dropped += int((~keep).sum())
        w = w @ (vec[:, keep][:, ::-1] / np.sqrt(np.maximum(lam[keep][::-1], floor)))
        if w.shape[1] == 0:
            break
    return w, dropped


def _block_qr(w, q):
    """Column-pivoted QR: |R_ii| is the novelty of the column chosen i-th; then a projection and a plain QR to polish."""
    qm, rm, _ = sla.qr(_project(w, q), mode="economic", pivoting=True)
    keep = np.abs(np.diag(rm)) > NOVELTY_TOL
    blk = qm[:, keep]
    if blk.shape[1]:
        blk = np.linalg.qr(_project(blk, q))[0]
    return blk, int((~keep).sum())


def basis(a, b0, steps, how="eigh"):
    """(Q [n, r], dropped): block by block -- unit columns, a projection, the in-block orthonormalisation of `how`."""
    n = a.shape[0]
    q = np.zeros((n, 0))
    w, dropped = b0, 0
    for _ in range(steps + 1):
        w = w[:, : n - q.shape[1]]
        norms = np.linalg.norm(w, axis=0)
        w = w * np.where(norms > 0, 1.0 / np.where(norms > 0, norms, 1.0), 0.0)
        blk, dr = (_block_eigh if how == "eigh" else _block_qr)(_project(w, q), q)
        dropped += dr
        if blk.shape[1] == 0:
            break
        q = np.concatenate([q, blk], 1)
        if q.shape[1] >= n:
            break
        w = a @ blk
    return q, dropped


class Cache:
    """a, b0: the dense operator and the start block when the caller has them already (they depend on neither steps nor how)."""

    def __init__(self, terms, hp, x, y, rank, steps, anchors=None, how="eigh", a=None, b0=None):
        self.terms, self.hp, self.x = terms, np.asarray(hp), np.asarray(x)
        n, d = self.x.shape
        self.a = ir.operator(terms, hp, self.x) if a is None else a
        self.shift = float(mr.shift_of(terms, hp, d, ir.JITTER))
        b0 = start_block(terms, hp, self.x, y, rank, anchors) if b0 is None else b0
        self.q, self.dropped = basis(self.a, b0, steps, how)
        self.rank = self.q.shape[1]
        self.aq = self.a @ self.q
        t = self.q.T @ self.aq
        self.g = np.linalg.cholesky(0.5 * (t + t.T))
        self.r = sla.solve_triangular(self.g, self.q.T, lower=True).T                # Q G^-T
        self.kss = float(mr.stationary_kernel(terms, hp, self.x[:1], self.x[:1])[0, 0] + mr.shift_of(terms, hp, d, 0.0))
        self.floor_multiple = floor_multiple(n, self.rank)

    def cross(self, xp):
        return mr.stationary_kernel(self.terms, self.hp, np.asarray(xp), self.x)       # [q, n]

    def variance(self, xp, bounds=False):
        ks = self.cross(xp)
        u = ks @ self.r
        upper = self.kss - np.sum(u * u, 1)
        if not bounds:
            return upper
        c = sla.solve_triangular(self.g, u.T, lower=True, trans="T").T               # c^T = u^T G^-1
        ksq = np.sum(ks * ks, 1)
        res = ksq - 2.0 * np.sum(c * (ks @ self.aq), 1) + np.sum((c @ (self.aq.T @ self.aq)) * c, 1)
        gap = (np.maximum(res, 0.0) + self.floor_multiple * 2.0 ** -53 * ksq) / self.shift
        return upper, upper - gap

    def covariance(self, xp):
        xp = np.asarray(xp)
        u = self.cross(xp) @ self.r
        kpp = mr.stationary_kernel(self.terms, self.hp, xp, xp) + float(mr.shift_of(self.terms, self.hp, xp.shape[1], 0.0)) * np.eye(len(xp))
        return kpp - u @ u.T

    def exact(self, xp):
        """The variance the cache bounds: k** - k*^T A^-1 k*, dense."""
        ks = self.cross(xp)
        return self.kss - np.sum(ks * np.linalg.solve(self.a, ks.T).T, 1)


def own_error(terms, hp, x, y, rank, steps, xp, anchors=None, a=None, b0=None):
    """(the eigh cache, the QR cache, err): err is the largest disagreement of the two orthonormalisations over upper and lower at
    xp, relative to k** -- the restatement's own error, what tests/sparse_ref.tol_of takes."""
    ce = Cache(terms, hp, x, y, rank, steps, anchors, "eigh", a, b0)
    cq = Cache(terms, hp, x, y, rank, steps, anchors, "qr", a, b0)
    ue, le = ce.variance(xp, bounds=True)
    uq, lq = cq.variance(xp, bounds=True)
    return ce, cq, float(max(np.max(np.abs(ue - uq)), np.max(np.abs(le - lq)))) / ce.kss
