"""NumPy restatement of the periodic kernel next to the kinds of tests/rq_ref.py and tests/matern_ref.py, with the phase formed from
the coordinate DIFFERENCE: the reference of the periodic tests.

A part name "per" has hp = [sigma, l_1..l_d, p_1..p_d]: 2 d + 1 values, the periods behind the block every other stationary part has.
With D_k = x_k - x'_k, l the INVERSE length scales, w_k = pi / p_k and s_k = sin(w_k D_k):

    sq        = sum_k l_k^2 s_k^2
    K         = sigma^2 exp(-sq)
    dK/dsigma = 2 K / sigma
    dK/dl_k   = -2 K l_k s_k^2
    dK/dp_k   = K l_k^2 sin(2 w_k D_k) w_k D_k / p_k
    dK/dx*_k  = -K l_k^2 sin(2 w_k D_k) w_k          (x* the first argument: the test point of a cross kernel)

Every other part ("se", "m52", "m32", "m12", "rq", "wn") is rq_ref's / matern_ref's, through their own helpers; the routines here only
know the wider block.  A model is a list of part names in Compose order, hp their parameters concatenated; cross kernels have the TEST
points as rows ([m, n]).  `dtype=np.longdouble` evaluates the same formulas in extended precision (the offset-data yardstick); pi is
then 4 atan(1) in that precision."""
import numpy as np
import scipy.linalg as sla

import matern_ref as mr
import rq_ref as rq

JITTER = mr.JITTER


def width(part, d):
    return 2 * d + 1 if part == "per" else rq.width(part, d)


def nhp_of(parts, d):
    return sum(width(p, d) for p in parts)


def _chunks(parts, d):
    o = 0
    for p in parts:
        yield p, o, o + width(p, d)
        o += width(p, d)


def _pi(dtype):
    return 4 * np.arctan(dtype(1))


def _phase(hpc, x, xp, k, dtype):
    """w_k D_k [n, n] or [m, n] of a periodic part (rows = xp)."""
    d = x.shape[1]
    return _pi(dtype) * mr._diff(x, xp, k) / hpc[d + 1 + k]


def _per_sq(hpc, x, xp, dtype):
    sq = 0.0
    for k in range(x.shape[1]):
        sq = sq + (hpc[1 + k] * np.sin(_phase(hpc, x, xp, k, dtype))) ** 2
    return sq


def _value(part, hpc, x, xp, dtype):
    if part == "per":
        return hpc[0] ** 2 * np.exp(-_per_sq(hpc, x, xp, dtype))
    return rq._radial(part, hpc, mr._sq(hpc, x, xp))[0]


def kernel(parts, hp, x, xp=None, dtype=np.float64):
    hp, x = np.asarray(hp, dtype), np.asarray(x, dtype)
    xp = None if xp is None else np.asarray(xp, dtype)
    n, d = x.shape
    out = np.zeros((n if xp is None else xp.shape[0], n), dtype)
    for p, a, b in _chunks(parts, d):
        if p == "wn":
            if xp is None:
                out += hp[a] ** 2 * np.eye(n, dtype=dtype)
        else:
            out += _value(p, hp[a:b], x, xp, dtype)
    return out


def _grad_terms(parts, hp, x, dtype=np.float64):
    """Yield (hp index, dK slab) one at a time."""
    hp, x = np.asarray(hp, dtype), np.asarray(x, dtype)
    n, d = x.shape
    for p, a, b in _chunks(parts, d):
        if p != "per":
            for i, slab in rq._grad_terms([p], hp[a:b], x):
                yield a + i, slab
            continue
        hpc = hp[a:b]
        kv = _value(p, hpc, x, None, dtype)
        yield a, kv * (2 / hpc[0])
        for k in range(d):
            ph = _phase(hpc, x, None, k, dtype)
            yield a + 1 + k, -2 * kv * hpc[1 + k] * np.sin(ph) ** 2
            yield a + d + 1 + k, kv * hpc[1 + k] ** 2 * np.sin(2 * ph) * ph / hpc[d + 1 + k]


def kernel_and_grad(parts, hp, x, dtype=np.float64):
    """K [n, n] and dK [nhp, n, n] (Compose.kernel_and_grad)."""
    n, d = x.shape
    dk = np.empty((nhp_of(parts, d), n, n), dtype)
    for i, slab in _grad_terms(parts, hp, x, dtype):
        dk[i] = slab
    return kernel(parts, hp, x, dtype=dtype), dk


def kernel_xgrad(parts, hp, x, xp):
    """dK*[p, i] / dxp_pk as [d, m, n]: the derivative of the cross kernel in its test point."""
    n, d = x.shape
    out = np.zeros((d, xp.shape[0], n))
    for p, a, b in _chunks(parts, d):
        if p == "wn":
            continue
        hpc = hp[a:b]
        if p != "per":
            out += rq.kernel_xgrad([p], hpc, x, xp)
            continue
        kv = _value(p, hpc, x, xp, np.float64)
        for k in range(d):
            ph = _phase(hpc, x, xp, k, np.float64)
            out[k] -= kv * hpc[1 + k] ** 2 * np.sin(2 * ph) * np.pi / hpc[d + 1 + k]
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
