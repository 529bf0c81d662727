"""NumPy restatement of the Matern family (nu = 1/2, 3/2, 5/2) next to the squared exponential and white noise, with DIRECT
differences: the reference for the kinds the oracle package does not cover.

Every stationary child has hp = [sigma, l_1..l_d] (l are inverse length scales), r = sqrt(sum_k l_k^2 D_k^2), D_k = x_k - x'_k:

    se   K = s^2 exp(-r^2)                          dK/dl_k = -2 K l_k D_k^2
    m52  K = s^2 (1 + sqrt5 r + 5 r^2/3) e^-sqrt5 r  dK/dl_k = -5/3 s^2 (1 + sqrt5 r) e^-sqrt5 r l_k D_k^2
    m32  K = s^2 (1 + sqrt3 r) e^-sqrt3 r            dK/dl_k = -3 s^2 e^-sqrt3 r l_k D_k^2
    m12  K = s^2 e^-r                               dK/dl_k = -s^2 e^-r l_k D_k^2 / r  (0 at r = 0)

and dK/dsigma = 2 K / sigma; white noise ("wn", hp = [sigma_n]) is sigma_n^2 I on a symmetric build and nothing on a cross build.
A model is a list of those names in Compose order; hp is their parameters concatenated.  Cross kernels have the TEST points as
rows ([m, n]), as the library's.  The gradient routines never hold the [nhp, n, n] stack, so N = 4096 fits on the host.
"""
import numpy as np
import scipy.linalg as sla

JITTER = 1e-7
NU = {"m12": 0.5, "m32": 1.5, "m52": 2.5}


def nhp_of(parts, d):
    return sum(1 if p == "wn" else d + 1 for p in parts)


def _chunks(parts, d):
    o = 0
    for p in parts:
        w = 1 if p == "wn" else d + 1
        yield p, o, o + w
        o += w


def _radial(part, s2, sq):
    """(K, base) of one stationary kind from the scaled squared distance; dK/dl_k = coef base l_k D_k^2 with coef = COEF[part]."""
    if part == "se":
        k = s2 * np.exp(-sq)
        return k, k
    r = np.sqrt(sq)
    if part == "m52":
        e = np.exp(-np.sqrt(5.0) * r)
        return s2 * (1.0 + np.sqrt(5.0) * r + (5.0 / 3.0) * sq) * e, s2 * (1.0 + np.sqrt(5.0) * r) * e
    if part == "m32":
        e = s2 * np.exp(-np.sqrt(3.0) * r)
        return (1.0 + np.sqrt(3.0) * r) * e, e
    if part == "m12":
        k = s2 * np.exp(-r)
        with np.errstate(divide="ignore", invalid="ignore"):
            base = np.where(sq > 0.0, k / np.where(sq > 0.0, r, 1.0), 0.0)
        return k, base
    raise ValueError(part)


COEF = {"se": -2.0, "m52": -5.0 / 3.0, "m32": -3.0, "m12": -1.0}


def _diff(x, xp, k):
    """D_k [n, n] or [m, n] (rows = xp), formed when needed: the [d, n, n] stack would not fit at N = 4096."""
    a = x if xp is None else xp
    return a[:, k][:, None] - x[:, k][None, :]


def _sq(hpc, x, xp=None):
    sq = 0.0
    for k in range(x.shape[1]):
        sq = sq + (hpc[1 + k] * _diff(x, xp, k)) ** 2
    return sq


def stationary(part, hpc, x, xp=None):
    """One stationary child: K [n, n] (xp None) or [m, n]."""
    return _radial(part, hpc[0] ** 2, _sq(hpc, x, xp))[0]


def kernel(parts, hp, x, xp=None):
    n, d = x.shape
    out = np.zeros((n if xp is None else xp.shape[0], n))
    for p, a, b in _chunks(parts, d):
        if p == "wn":
            if xp is None:
                out += hp[a] ** 2 * np.eye(n)
        else:
            out += _radial(p, hp[a] ** 2, _sq(hp[a:b], x, xp))[0]
    return out


def _grad_terms(parts, hp, x):
    """Yield (hp index, dK slab) one at a time."""
    n, d = x.shape
    for p, a, b in _chunks(parts, d):
        if p == "wn":
            yield a, 2.0 * hp[a] * np.eye(n)
            continue
        kv, base = _radial(p, hp[a] ** 2, _sq(hp[a:b], x))
        yield a, kv * (2.0 / hp[a])
        for k in range(d):
            df = _diff(x, None, k)
            yield a + 1 + k, COEF[p] * base * hp[a + 1 + k] * df * df


def kernel_and_grad(parts, hp, x):
    """K [n, n] and dK [nhp, n, n] (Compose.kernel_and_grad)."""
    n, d = x.shape
    dk = np.empty((nhp_of(parts, d), n, n))
    for i, slab in _grad_terms(parts, hp, x):
        dk[i] = slab
    return kernel(parts, hp, x), dk


def _factor(parts, hp, x, y):
    k = kernel(parts, hp, x)
    k[np.diag_indices_from(k)] += JITTER
    c = sla.cho_factor(k, lower=True)
    return c, sla.cho_solve(c, y)


def nlml(parts, hp, x, y):
    c, alpha = _factor(parts, hp, x, y)
    return 0.5 * float(alpha @ y) + float(np.sum(np.log(np.diag(c[0])))) + 0.5 * y.shape[0] * np.log(2.0 * np.pi)


def nlml_and_grad(parts, hp, x, y):
    """MLE.loss_and_grad: NLML and g_p = 1/2 sum_ij (K^-1 - a a^T)_ij dK_p,ij."""
    c, alpha = _factor(parts, hp, x, y)
    n = y.shape[0]
    loss = 0.5 * float(alpha @ y) + float(np.sum(np.log(np.diag(c[0])))) + 0.5 * n * np.log(2.0 * np.pi)
    w = sla.cho_solve(c, np.eye(n))
    w -= np.outer(alpha, alpha)
    g = np.zeros(hp.size)
    for i, slab in _grad_terms(parts, hp, x):
        g[i] = 0.5 * float(np.sum(w * slab))
    return loss, g


def predict(parts, hp, x, y, xp, var="diag"):
    """Exact_GP.predict: mean K* alpha and the diagonal / full covariance K** - K* K^-1 K*^T (K** keeps the noise)."""
    c, alpha = _factor(parts, hp, x, y)
    ks = kernel(parts, hp, x, xp)
    kss = kernel(parts, hp, xp)
    v = ks @ sla.cho_solve(c, ks.T)
    mean = ks @ alpha
    return (mean, np.diag(kss) - np.diag(v)) if var == "diag" else (mean, kss - v)


def grbcm_predict(parts, hp_g, hp_l, xl, yl, xg, yg, xs):
    """GRBCM.predict(var="diag"): global expert on (xg, yg), local expert c on (xg U xl[c]), aggregated as the reference's committee."""
    mg, vg = predict(parts, hp_g, xg, yg, xs)
    ml, vl = [], []
    for c in range(xl.shape[0]):
        m, v = predict(parts, hp_l[c], np.concatenate([xg, xl[c]]), np.concatenate([yg, yl[c]]), xs)
        ml.append(m)
        vl.append(v)
    ml, vl = np.stack(ml), np.stack(vl)
    prec = np.concatenate([1.0 / vg[None], 1.0 / vl])
    beta = np.empty_like(prec)
    beta[1:] = 0.5 * (np.log(prec[1:]) - np.log(prec[0]))
    beta[1] = 1.0
    beta[0] = 1.0 - beta[1:].sum(0)
    var = 1.0 / (prec * beta).sum(0)
    mu = (np.concatenate([mg[None], ml]) * prec * beta).sum(0) * var
    return mu, var
