"""NumPy restatement of the rational quadratic next to the kinds of tests/matern_ref.py, with DIRECT differences: the reference of the
rational-quadratic tests.

A part name "rq" has hp = [sigma, l_1..l_d, alpha]: d + 2 values, the shape behind the block every other stationary part has.  With
D_k = x_k - x'_k, l the INVERSE length scales and every parameter entering squared:

    sq = sum_k l_k^2 D_k^2,   a = alpha^2,   t = sq / a
    K         = s^2 (1 + t)^(-a) = s^2 exp(-a log1p(t))
    dK/dsigma = 2 K / sigma
    dK/dl_k   = -2 [K / (1 + t)] l_k D_k^2
    dK/dalpha = 2 alpha K [t / (1 + t) - log1p(t)]
    dK/dx*_k  = -2 [K / (1 + t)] l_k^2 D_k          (x* the first argument: the test point of a cross kernel)

"se", "m52", "m32", "m12" and "wn" are matern_ref's, through its own helpers; the routines here only know the wider block.  A model is a
list of part names in Compose order, hp their parameters concatenated; cross kernels have the TEST points as rows ([m, n])."""
import numpy as np
import scipy.linalg as sla

import matern_ref as mr

JITTER = mr.JITTER
COEF = dict(mr.COEF, rq=-2.0)


def width(part, d):
    return 1 if part == "wn" else (d + 2 if part == "rq" else d + 1)


def nhp_of(parts, d):
    return sum(width(p, d) for p in parts)


def _chunks(parts, d):
    o = 0
    for p in parts:
        yield p, o, o + width(p, d)
        o += width(p, d)


def _radial(part, hpc, sq):
    """(K, base, shape slab or None) of one stationary part from the scaled squared distance; dK/dl_k = COEF base l_k D_k^2."""
    if part != "rq":
        return mr._radial(part, hpc[0] ** 2, sq) + (None,)
    a = hpc[-1] ** 2
    t = sq / a
    lg = np.log1p(t)
    k = hpc[0] ** 2 * np.exp(-a * lg)
    return k, k / (1.0 + t), 2.0 * hpc[-1] * k * (t / (1.0 + t) - lg)


def kernel(parts, hp, x, xp=None):
    n, d = x.shape
    out = np.zeros((n if xp is None else xp.shape[0], n))
    for p, a, b in _chunks(parts, d):
        if p == "wn":
            if xp is None:
                out += hp[a] ** 2 * np.eye(n)
        else:
            out += _radial(p, hp[a:b], mr._sq(hp[a:b], x, xp))[0]
    return out


def _grad_terms(parts, hp, x):
    """Yield (hp index, dK slab) one at a time."""
    n, d = x.shape
    for p, a, b in _chunks(parts, d):
        if p == "wn":
            yield a, 2.0 * hp[a] * np.eye(n)
            continue
        kv, base, shape = _radial(p, hp[a:b], mr._sq(hp[a:b], x))
        yield a, kv * (2.0 / hp[a])
        for k in range(d):
            df = mr._diff(x, None, k)
            yield a + 1 + k, COEF[p] * base * hp[a + 1 + k] * df * df
        if shape is not None:
            yield a + d + 1, shape


def kernel_and_grad(parts, hp, x):
    """K [n, n] and dK [nhp, n, n] (Compose.kernel_and_grad)."""
    n, d = x.shape
    dk = np.empty((nhp_of(parts, d), n, n))
    for i, slab in _grad_terms(parts, hp, x):
        dk[i] = slab
    return kernel(parts, hp, x), dk


def kernel_xgrad(parts, hp, x, xp):
    """dK*[p, i] / dxp_pk as [d, m, n]: the derivative of the cross kernel in its test point."""
    n, d = x.shape
    out = np.zeros((d, xp.shape[0], n))
    for p, a, b in _chunks(parts, d):
        if p == "wn":
            continue
        base = _radial(p, hp[a:b], mr._sq(hp[a:b], x, xp))[1]
        for k in range(d):
            out[k] += COEF[p] * base * hp[a + 1 + k] ** 2 * mr._diff(x, xp, k)
    return out


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


def predict_grads(parts, hp, x, y, xp):
    """d mean_p / d xp_p and d var_p / d xp_p, both [m, d] (the diagonal of K** is constant in xp)."""
    c, alpha = _factor(parts, hp, x, y)
    ks = kernel(parts, hp, x, xp)
    dks = kernel_xgrad(parts, hp, x, xp)
    v = sla.cho_solve(c, ks.T).T                       # (K^-1 K*^T)^T [m, n]
    return np.einsum("kpi,i->pk", dks, alpha), -2.0 * np.einsum("kpi,pi->pk", dks, v)


def predict_vjp(parts, hp, x, y, xp, var, g_mu, g_2=None):
    """<g_mu, mean> + <g_2, var | covariance> differentiated in xp [m, d]: the autograd backward of Exact_GP.predict."""
    c, alpha = _factor(parts, hp, x, y)
    ks = kernel(parts, hp, x, xp)
    dks = kernel_xgrad(parts, hp, x, xp)
    out = np.einsum("kpi,i,p->pk", dks, alpha, g_mu)
    if var == "none":
        return out
    v = sla.cho_solve(c, ks.T).T
    if var == "diag":
        return out - 2.0 * np.einsum("kpi,pi,p->pk", dks, v, g_2)
    gs = g_2 + g_2.T
    out -= np.einsum("kpi,pi->pk", dks, gs @ v)
    # K**[p, q] moves with both of its points: the row derivative against G + G^T (its own diagonal has D = 0)
    return out + np.einsum("kpq,pq->pk", kernel_xgrad(parts, hp, xp, xp), gs)


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
