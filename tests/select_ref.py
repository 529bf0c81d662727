"""NumPy restatement of greedy inducing-point selection (include/pygpr_hip_select.h) on top of tests/kernel_ref.py: the reference of the
selection tests.  Host only, generic in dtype (float64 and np.longdouble).

With kdiag the prior variance of the stationary terms and r_i = kdiag, step j takes p = argmax_i r_i (strict `>` in index order: a tie
takes the lowest index, a NaN is never a maximum), stops unless r_p > floor, and otherwise

    l_i = (k(x_i, x_p) - sum_{t < j} L[i, t] L[p, t]) / sqrt(r_p),   L[i, j] = l_i,   r_i <- r_i - l_i^2,   r_p <- 0,
    piv[j] = p,   trace[j] = sum_i r_i

-- the partial pivoted Cholesky factorisation of k(x, x).  `greedy` is that loop; `replay` follows a GIVEN pivot sequence and returns
every step's residuals, so that a sequence found elsewhere (the device's) can be judged without asking two runs in different
arithmetic to break near-ties the same way.  Terms and hp are kernel_ref's; a "wn" term holds its slot in hp and adds nothing."""
from typing import NamedTuple

import numpy as np

import kernel_ref as kr


def prior_variance(terms, hp, d, dtype=np.float64):
    """kdiag: the sum over the stationary terms of the product of their factors' sigma^2, accumulated in term order."""
    hp = np.asarray(hp, dtype)
    total = dtype(0)
    for t, blocks in kr._chunks(terms, d):
        if t == "wn":
            continue
        term = dtype(1)
        for _, a, _ in blocks:
            term = term * (hp[a] * hp[a])
        total = total + term
    return total


def argmax(r):
    """The lowest index of the largest entry, NaNs never a maximum; -1 when nothing compares above -inf."""
    rr = np.where(np.isnan(r), -np.inf, r)
    p = int(np.argmax(rr))
    return p if rr[p] > -np.inf else -1


def column(terms, hp, x, p, dtype):
    """k(x_i, x_p) for every i, without noise: a cross build against the one point."""
    return kr.kernel(terms, hp, x, x[p: p + 1], dtype)[0]


class Run(NamedTuple):
    piv: np.ndarray        # [count] the pivots in selection order
    trace: np.ndarray      # [count] sum_i r_i after each step
    resid: np.ndarray      # [n] the final residuals
    hist: np.ndarray       # [count + 1, n] the residuals BEFORE each step; hist[count] = resid
    kdiag: float


def _step(terms, hp, x, fac, r, j, p, dtype):
    l = (column(terms, hp, x, p, dtype) - fac[:, :j] @ fac[p, :j]) / np.sqrt(r[p])
    fac[:, j] = l
    r = r - l * l
    r[p] = 0
    return r


def greedy(terms, hp, x, m_max, floor, dtype=np.float64):
    hp, x = np.asarray(hp, dtype), np.asarray(x, dtype)
    n, d = x.shape
    kd = prior_variance(terms, hp, d, dtype)
    r = np.full(n, kd, dtype)
    fac = np.zeros((n, m_max), dtype)
    piv, trace, hist = [], [], [r]
    for j in range(m_max):
        p = argmax(r)
        if p < 0 or not r[p] > floor:
            break
        r = _step(terms, hp, x, fac, r, j, p, dtype)
        piv.append(p)
        trace.append(np.sum(r))
        hist.append(r)
    return Run(np.array(piv, dtype=np.int64), np.array(trace, dtype), r, np.array(hist, dtype), kd)


def replay(terms, hp, x, piv, dtype=np.longdouble):
    """The same updates along the pivot sequence `piv`, whatever the residuals say: hist[j] holds what the selection saw before step j
    (np.nanmax(hist[j]) is the maximum it had to take, hist[j][piv[j]] what the sequence took), hist[len(piv)] the final residuals."""
    hp, x = np.asarray(hp, dtype), np.asarray(x, dtype)
    n, d = x.shape
    kd = prior_variance(terms, hp, d, dtype)
    r = np.full(n, kd, dtype)
    fac = np.zeros((n, max(len(piv), 1)), dtype)
    trace, hist = [], [r]
    with np.errstate(invalid="ignore", divide="ignore"):
        for j, p in enumerate(piv):
            r = _step(terms, hp, x, fac, r, j, int(p), dtype)
            trace.append(np.sum(r))
            hist.append(r)
    return Run(np.asarray(piv, dtype=np.int64), np.array(trace, dtype), r, np.array(hist, dtype), kd)


def own_error(terms, hp, x, piv):
    """The restatement's own rounding on this input: the largest difference between the float64 and the long-double replay of one pivot
    sequence over every step's residuals, relative to kdiag (NaN residuals, a NaN coordinate's, left out)."""
    a, b = replay(terms, hp, x, piv, np.float64), replay(terms, hp, x, piv, np.longdouble)
    diff = np.abs(a.hist.astype(np.longdouble) - b.hist)
    return float(np.nanmax(diff) / b.kdiag) if diff.size else 0.0


def trace_term(terms, hp, x, z):
    """(T, cond(Kuu)) with T = n kdiag - tr(Kuu^-1 Kuf Kfu) and Kuu = k(z, z) WITHOUT jitter: what trace[-1] restates for z = x[piv]."""
    n, d = x.shape
    kuu = kr.kernel(terms, hp, z, z)
    kuf = kr.kernel(terms, hp, x, z)
    t = n * float(prior_variance(terms, hp, d)) - float(np.trace(np.linalg.solve(kuu, kuf @ kuf.T)))
    return t, float(np.linalg.cond(kuu))
