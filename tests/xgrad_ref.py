"""Plain torch fp64 restatement of the predictive mean, diagonal variance and full covariance of an Exact_GP for the squared exponential,
Matern-5/2 / -3/2 / -1/2 and white noise in any Compose, written with out-of-place operations only so that torch.autograd differentiates
it in the test points: its gradients are the reference of the library's derivatives in x* (pg_kernel_xgrad, Exact_GP.predict_grad and
the autograd backward of Exact_GP.predict).  Same parameter layout as tests/kernel_ref.py: a model is a list of names ("se", "m52",
"m32", "m12", "wn"), hp their parameters concatenated, [sigma, l_1..l_d] per stationary child (l are inverse length scales).

r = 0 (a test point on a training point, or on itself in K**): the radial distance goes through a double `where`, so that its
derivative there is exactly 0 instead of the 0 * inf of sqrt.  For the smooth kinds nothing changes (dsq/dx* = 2 l^2 D = 0 there
anyway); for Matern-1/2, whose derivative does not exist at r = 0, this IS the library's convention: such a pair contributes 0.
Works on any device (the large-n test runs it on the GPU, where the Cholesky of 16384 points takes a second)."""
import math

import torch

JITTER = 1e-7


def _chunks(parts, d):
    o = 0
    for p in parts:
        w = 1 if p == "wn" else d + 1
        yield p, o, o + w
        o += w


def nhp_of(parts, d):
    return sum(1 if p == "wn" else d + 1 for p in parts)


def _radial(part, s2, sq):
    if part == "se":
        return s2 * torch.exp(-sq)
    pos = sq > 0
    r = torch.where(pos, torch.sqrt(torch.where(pos, sq, torch.ones_like(sq))), torch.zeros_like(sq))   # d r / d sq := 0 at r = 0
    if part == "m52":
        return s2 * (1.0 + math.sqrt(5.0) * r + (5.0 / 3.0) * sq) * torch.exp(-math.sqrt(5.0) * r)
    if part == "m32":
        return s2 * (1.0 + math.sqrt(3.0) * r) * torch.exp(-math.sqrt(3.0) * r)
    if part == "m12":
        return s2 * torch.exp(-r)
    raise ValueError(part)


def kernel(parts, hp, x, xp=None):
    """k(xp, x) [m, n] (test points as rows, as the library stores K*), or K [n, n] with the noise diagonal when xp is None."""
    a = x if xp is None else xp
    out = torch.zeros(a.shape[0], x.shape[0], dtype=x.dtype, device=x.device)
    for p, lo, hi in _chunks(parts, x.shape[1]):
        if p == "wn":
            if xp is None:
                out = out + hp[lo] ** 2 * torch.eye(x.shape[0], dtype=x.dtype, device=x.device)
            continue
        sq = 0.0
        for k in range(x.shape[1]):                # direct differences, one coordinate at a time ([rows, n] temporaries only)
            sq = sq + (hp[lo + 1 + k] * (a[:, k, None] - x[None, :, k])) ** 2
        out = out + _radial(p, hp[lo] ** 2, sq)
    return out


def kss_diag(parts, hp, d):
    """The constant diagonal of K** (every stationary sigma^2 plus every noise sigma_n^2)."""
    return sum(float(hp[lo]) ** 2 for p, lo, hi in _chunks(parts, d))


def factor(parts, hp, x, y):
    k = kernel(parts, hp, x) + JITTER * torch.eye(x.shape[0], dtype=x.dtype, device=x.device)
    chol = torch.linalg.cholesky(k)
    return chol, torch.cholesky_solve(y[:, None], chol)[:, 0]


def predict(parts, hp, x, y, xp, var="diag", fac=None):
    """Exact_GP.predict: (mean [m], var [m]) for var="diag", (mean, covariance [m, m]) for "full", (mean, None) for "none".
    `fac`: (chol, alpha) of factor() to reuse across calls."""
    chol, alpha = fac if fac is not None else factor(parts, hp, x, y)
    ks = kernel(parts, hp, x, xp)
    mean = ks @ alpha
    if var == "none":
        return mean, None
    v = torch.cholesky_solve(ks.t(), chol)        # K^-1 K*^T [n, m]
    if var == "diag":
        return mean, kss_diag(parts, hp, x.shape[1]) - (ks * v.t()).sum(1)
    kss = kernel(parts, hp, xp)
    return mean, kss - ks @ v


def predict_grads(parts, hp, x, y, xp, fac=None):
    """d mean_p / d xp_p and d var_p / d xp_p [m, d] by autograd (each output depends on its own test point only)."""
    xq = xp.detach().clone().requires_grad_(True)
    mean, var = predict(parts, hp, x, y, xq, "diag", fac)
    dmean, = torch.autograd.grad(mean.sum(), xq, retain_graph=True)
    dvar, = torch.autograd.grad(var.sum(), xq)
    return mean.detach(), var.detach(), dmean, dvar


def vjp(parts, hp, x, y, xp, var, g_mu, g_2=None, fac=None):
    """<g_mu, mean> + <g_2, var | covariance> differentiated in xp (the autograd backward of predict)."""
    xq = xp.detach().clone().requires_grad_(True)
    mean, second = predict(parts, hp, x, y, xq, var, fac)
    loss = (g_mu * mean).sum()
    if var != "none":
        loss = loss + (g_2 * second).sum()
    g, = torch.autograd.grad(loss, xq)
    return g


def contraction(parts, hp, xq, z, u=None, b=None):
    """out_u[p][k] = sum_i u_i dk(xq_p, z_i)/dxq_pk, out_b[p][k] = sum_i B_pi dk(xq_p, z_i)/dxq_pk (z is a constant, even when it holds
    the same points as xq): what pg_kernel_xgrad computes."""
    xr = xq.detach().clone().requires_grad_(True)
    kc = kernel(parts, hp, z.detach(), xr)       # [m, n], rows = xq
    outs = []
    for w in (None if u is None else u[None, :], b):
        if w is None:
            outs.append(None)
            continue
        g, = torch.autograd.grad((w * kc).sum(), xr, retain_graph=True)
        outs.append(g)
    return outs
