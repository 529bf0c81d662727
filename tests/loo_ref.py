"""NumPy / SciPy restatement of leave-one-out cross-validation for an exact GP (Rasmussen & Williams, section 5.4.2), on the kernels of
tests/kernel_ref.py (any model of its grammar): the reference of the LOO tests.  K = k(x, x) + noise + JITTER I is the matrix
Exact_GP.update() factors, so every quantity here is predictive for y_i (noise included).

    closed forms   mu_i = y_i - alpha_i / c_i,  var_i = 1 / c_i,  c = diag(K^-1), alpha = K^-1 y               (5.10 - 5.12)
    brute force    n explicit refits on the other n - 1 points
    loss           -sum_i log p(y_i | x, y_-i) = sum_i [ 1/2 log var_i + (y_i - mu_i)^2 / (2 var_i) ] + n/2 log 2pi
    gradient       eq. 5.13, one hyper-parameter at a time with Z_j = K^-1 dK/dtheta_j from the dense slab:
                   dL/dtheta_j = -sum_i ( alpha_i [Z_j alpha]_i - 1/2 (1 + alpha_i^2 / c_i) [Z_j K^-1]_ii ) / c_i
                   -- NOT the weighted-matrix form the library contracts (`grad_gmatrix` restates that one for the identity test)."""
import numpy as np
import scipy.linalg as sla

import kernel_ref as kr

LOG2PI = float(np.log(2.0 * np.pi))


def _kmat(parts, hp, x):
    k = kr.kernel(parts, np.asarray(hp, dtype=np.float64), x)
    k[np.diag_indices_from(k)] += kr.JITTER
    return k


def _solve(parts, hp, x, y):
    """(K^-1, alpha, c)."""
    k = _kmat(parts, hp, x)
    c = sla.cho_factor(k, lower=True)
    kinv = sla.cho_solve(c, np.eye(k.shape[0]))
    kinv = 0.5 * (kinv + kinv.T)
    return kinv, sla.cho_solve(c, y), np.diag(kinv).copy()


def loo_predict(parts, hp, x, y):
    _, alpha, c = _solve(parts, hp, x, y)
    return y - alpha / c, 1.0 / c


def loo_bruteforce(parts, hp, x, y):
    k = _kmat(parts, hp, x)
    n = y.shape[0]
    mu, var = np.empty(n), np.empty(n)
    for i in range(n):
        m = np.arange(n) != i
        s = np.linalg.solve(k[np.ix_(m, m)], k[m, i])
        mu[i] = s @ y[m]
        var[i] = k[i, i] - s @ k[m, i]
    return mu, var


def loss_from(mu, var, y):
    return float(np.sum(0.5 * np.log(var) + 0.5 * (y - mu) ** 2 / var) + 0.5 * y.shape[0] * LOG2PI)


def loo_loss(parts, hp, x, y):
    mu, var = loo_predict(parts, hp, x, y)
    return loss_from(mu, var, y)


def loo_loss_and_grad(parts, hp, x, y):
    """The loss and its gradient by eq. 5.13, per hyper-parameter from the dense dK slabs."""
    hp = np.asarray(hp, dtype=np.float64)
    kinv, alpha, c = _solve(parts, hp, x, y)
    loss = float(np.sum(-0.5 * np.log(c) + 0.5 * alpha * alpha / c) + 0.5 * y.shape[0] * LOG2PI)
    return loss, grad_from(parts, hp, x, kinv, alpha, c)


def grad_from(parts, hp, x, kinv, alpha, c):
    """Eq. 5.13 on a caller's (K^-1, alpha, c): a test that forms K^-1 its own way keeps that route."""
    g = np.zeros(np.size(hp))
    for j, slab in kr.grad_terms(parts, hp, x):
        z = kinv @ slab
        zk_diag = np.einsum("ij,ji->i", z, kinv)
        g[j] = -float(np.sum((alpha * (z @ alpha) - 0.5 * (1.0 + alpha * alpha / c) * zk_diag) / c))
    return g


def gmatrix(kinv, alpha):
    """G with dL/dtheta = 1/2 sum G o dK: G = 2 K^-1 W K^-1 - b alpha^T - alpha b^T, W = diag(1/(2c) + alpha^2/(2c^2)), b = K^-1 (alpha/c);
    the library forms it as S S^T + q q^T - p p^T."""
    c = np.diag(kinv)
    w = 0.5 / c + 0.5 * alpha * alpha / (c * c)
    b = kinv @ (alpha / c)
    return 2.0 * (kinv * w) @ kinv - np.outer(b, alpha) - np.outer(alpha, b)


def grad_gmatrix(parts, hp, x, y):
    hp = np.asarray(hp, dtype=np.float64)
    kinv, alpha, _ = _solve(parts, hp, x, y)
    g_mat = gmatrix(kinv, alpha)
    g = np.zeros(hp.size)
    for j, slab in kr.grad_terms(parts, hp, x):
        g[j] = 0.5 * float(np.sum(g_mat * slab))
    return g
