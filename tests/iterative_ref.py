"""NumPy restatement of Iterative_GP (pygpr_amd/iterative.py) on top of tests/kernel_ref.py, tests/matmul_ref.py and
tests/select_ref.py: the operator, the pivoted-Cholesky preconditioner in its Woodbury form, and block PCG with the model's stopping
rule.  Dense and host only: the n x n matrix exists here, which is the point of a reference.

    A      = k(x, x) + (sum sigma_n^2 + JITTER) I                                  (what Exact_GP factors)
    piv    = greedy pivots (select_ref.greedy, floor JITTER), z = x[piv], Lu = chol(k(z, z) + JITTER I), L = k(x, z) Lu^-T
    P^-1 r = (r - L C^-1 L^T r) / shift,   C = shift I + L^T L                     (P = L L^T + shift I)
"""
import numpy as np
import scipy.linalg as sla

import kernel_ref as kr
import matmul_ref as mr
import select_ref as sel

JITTER = kr.JITTER
CHECK_EVERY = 10


def operator(terms, hp, x):
    """A, dense."""
    n, d = x.shape
    return mr.stationary_kernel(terms, hp, x, x) + float(mr.shift_of(terms, hp, d, JITTER)) * np.eye(n)


def factor_l(terms, hp, x, rank):
    """(L [n, m], piv): the preconditioner's factor at up to `rank` greedy pivots; m = 0 gives an [n, 0] factor."""
    n, d = x.shape
    m = min(rank, n)
    if m == 0:
        return np.zeros((n, 0)), np.zeros(0, np.int64)
    piv = sel.greedy(terms, hp, x, m, JITTER).piv
    z = x[piv]
    kuu = mr.stationary_kernel(terms, hp, z, z) + JITTER * np.eye(len(piv))
    lu = np.linalg.cholesky(kuu)
    kxz = mr.stationary_kernel(terms, hp, x, z)
    return sla.solve_triangular(lu, kxz.T, lower=True).T, piv


class Woodbury:
    """P^-1 of P = L L^T + shift I through the m x m matrix C = shift I + L^T L."""

    def __init__(self, l, shift):
        self.l, self.shift = l, float(shift)
        self.c = sla.cho_factor(self.shift * np.eye(l.shape[1]) + l.T @ l, lower=True) if l.shape[1] else None

    def solve(self, r):
        if self.c is None:
            return r.copy()                      # rank 0: plain CG
        return (r - self.l @ sla.cho_solve(self.c, self.l.T @ r)) / self.shift

    def dense(self):
        return self.l @ self.l.T + self.shift * np.eye(self.l.shape[0])


def pcg(a, b, pre, tol, max_iter, check_every=CHECK_EVERY):
    """Block PCG on A X = B [n, nrhs], every column with its own scalars: (X, iterations, true residual, converged).  A column whose
    p^T A p or r^T z is zero takes a zero step; every `check_every` iterations (and at max_iter) the largest ||r_c|| / ||b_c|| -- a zero
    column counts with ||b_c|| = 1 -- is compared with tol; the residual returned is the true one, ||b - A x|| / ||b|| at the end."""
    b2 = b[:, None] if b.ndim == 1 else b
    x = np.zeros_like(b2)
    r = b2.copy()
    z = pre.solve(r)
    p = z.copy()
    rz = np.sum(r * z, 0)
    bn = np.linalg.norm(b2, axis=0)
    bn = np.where(bn == 0, 1.0, bn)
    it, res = 0, np.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        while it < max_iter:
            ap = a @ p
            pap = np.sum(p * ap, 0)
            step = np.where((pap != 0) & (rz != 0), rz / pap, 0.0)
            x += p * step
            r -= ap * step
            z = pre.solve(r)
            rz_new = np.sum(r * z, 0)
            beta = np.where(rz != 0, rz_new / rz, 0.0)
            p = z + p * beta
            rz = rz_new
            it += 1
            if it % check_every == 0 or it == max_iter:
                res = float(np.max(np.linalg.norm(r, axis=0) / bn))
                if not res > tol:
                    break
    true = float(np.max(np.linalg.norm(b2 - a @ x, axis=0) / bn))
    return (x[:, 0] if b.ndim == 1 else x), it, true, bool(res <= tol)


def fit(terms, hp, x, y, rank, tol, max_iter=1000):
    """(alpha, iterations, true residual) of the model's update()."""
    a = operator(terms, hp, x)
    l, _ = factor_l(terms, hp, x, rank)
    alpha, it, res, ok = pcg(a, y, Woodbury(l, mr.shift_of(terms, hp, x.shape[1], JITTER)), tol, max_iter)
    assert ok
    return alpha, it, res
