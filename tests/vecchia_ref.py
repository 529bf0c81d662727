"""NumPy restatement of the nearest-neighbour (Vecchia) GP of include/pygpr_hip_vecchia.h: a per-target loop over the blocks of
tests/kernel_ref.py, written from the formulas.

  block of target i:  B = (valid entries of row i of nbr, i), the target LAST
  A_B   = kernel_ref.kernel on the block's points (noise on the diagonal) + jitter I
  c     = A_B^-1 e_last / (A_B^-1)_last,last,   v = 1 / (A_B^-1)_last,last,   r = c^T y_B,   a = [A_NN^-1 y_N ; 0]
  loss  = sum_i 1/2 [log v_i + r_i^2 / v_i + log 2 pi]
  grad  = 1/2 sum_i sum_pq W_pq dA_pq/dtheta,   W = (1/v - (r/v)^2) c c^T - (r/v)(a c^T + c a^T)

float64 solves are NumPy's (LAPACK's LU); `dtype=np.longdouble` runs the same formulas in extended precision with a Cholesky
factorisation written out below, because LAPACK has no extended type: the yardstick of the float64 restatement's own rounding error."""
import numpy as np

import kernel_ref as kr


def knn(xq, xc, s, m, causal):
    """nbr [q, m] int32: for every query the up to m candidates with the smallest sum_k (s_k (xq_ik - xc_jk))^2 (added in ascending k),
    ordered by (distance, index); candidates of query i are j < i when causal; a NaN distance is never selected; -1 padding."""
    xq, xc = np.asarray(xq, np.float64), np.asarray(xc, np.float64)
    q, d = xq.shape
    n = xc.shape[0]
    s = np.ones(d) if s is None else np.asarray(s, np.float64)
    out = np.full((q, m), -1, np.int32)
    for i in range(q):
        lim = min(i, n) if causal else n
        dist = np.zeros(lim)
        for k in range(d):
            dist = dist + (s[k] * (xq[i, k] - xc[:lim, k])) ** 2
        cand = [j for j in range(lim) if not np.isnan(dist[j])]
        cand.sort(key=lambda j: (dist[j], j))
        out[i, :min(m, len(cand))] = cand[:m]
    return out


def _chol_solve(a, b):
    """a^-1 b for a symmetric positive definite a in its own dtype: Cholesky and two substitutions, written out."""
    n = a.shape[0]
    l = np.zeros_like(a)
    for j in range(n):
        l[j, j] = np.sqrt(a[j, j] - l[j, :j] @ l[j, :j])
        for i in range(j + 1, n):
            l[i, j] = (a[i, j] - l[i, :j] @ l[j, :j]) / l[j, j]
    z = np.array(b, dtype=a.dtype)
    for j in range(n):
        z[j] = (z[j] - l[j, :j] @ z[:j]) / l[j, j]
    for j in range(n - 1, -1, -1):
        z[j] = (z[j] - l[j + 1:, j] @ z[j + 1:]) / l[j, j]
    return z


def solve(a, b, dtype):
    if a.shape[0] == 0:
        return np.zeros(0, dtype)
    return np.linalg.solve(a, b) if dtype == np.float64 else _chol_solve(a, b)


def _terms_of_block(a, yb, dtype):
    """(c, v, r) of one block matrix and its values."""
    b = a.shape[0]
    e = np.zeros(b, dtype)
    e[-1] = 1
    z = solve(a, e, dtype)
    v = 1 / z[-1]
    c = z * v
    return c, v, c @ yb


def nlml_and_grad(terms, hp, x, y, nbr, jitter, dtype=np.float64, first=0):
    """(loss, grad [nhp], cond_mean [count], cond_var [count]) of targets first .. first + len(nbr) - 1 in `dtype`."""
    hp, x, y = (np.asarray(t, dtype) for t in (hp, x, y))
    n = x.shape[0]
    count = nbr.shape[0]
    loss, grad = dtype(0), np.zeros(hp.size, dtype)
    cm, cv = np.zeros(count, dtype), np.zeros(count, dtype)
    log2pi = np.log(2 * kr._pi(dtype))
    for t in range(count):
        idx = [int(j) for j in nbr[t] if 0 <= j < n] + [first + t]
        xb, yb = x[idx], y[idx]
        a, dk = kr.kernel_and_grad(terms, hp, xb, dtype)
        a = a + dtype(jitter) * np.eye(len(idx), dtype=dtype)
        c, v, r = _terms_of_block(a, yb, dtype)
        al = np.zeros(len(idx), dtype)
        al[:-1] = solve(a[:-1, :-1], yb[:-1], dtype)
        w = (1 / v - (r / v) ** 2) * np.outer(c, c) - (r / v) * (np.outer(al, c) + np.outer(c, al))
        loss = loss + (np.log(v) + r * r / v + log2pi) / 2
        grad = grad + np.array([np.sum(w * dk[p]) for p in range(hp.size)], dtype) / 2
        cm[t], cv[t] = yb[-1] - r, v
    return loss, grad, cm, cv


def predict(terms, hp, x, y, xq, nbr, jitter, dtype=np.float64):
    """(mean [q], var [q]): query t conditioned on the valid entries of row t of nbr; the last diagonal entry keeps the noise and takes
    no jitter."""
    hp, x, y, xq = (np.asarray(t, dtype) for t in (hp, x, y, xq))
    n = x.shape[0]
    q = xq.shape[0]
    mean, var = np.zeros(q, dtype), np.zeros(q, dtype)
    for t in range(q):
        idx = [int(j) for j in nbr[t] if 0 <= j < n]
        xb = np.concatenate([x[idx], xq[t: t + 1]])
        yb = np.concatenate([y[idx], np.zeros(1, dtype)])
        a = kr.kernel(terms, hp, xb, dtype=dtype)
        jit = dtype(jitter) * np.eye(len(idx) + 1, dtype=dtype)
        jit[-1, -1] = 0
        c, v, r = _terms_of_block(a + jit, yb, dtype)
        mean[t], var[t] = -r, v
    return mean, var
