"""NumPy restatement of sums of PRODUCTS of stationary kernels: the reference of the Product tests, written from the formulas and
composed from the per-kind values and derivatives of tests/periodic_ref.py, rq_ref.py and matern_ref.py.

A covariance is a list of TERMS in Compose order.  A term is a part name ("se", "m52", "m32", "m12", "rq", "per", "wn") or a tuple of
stationary part names, the factors of a product; hp is every part's block concatenated in that order, each factor with its own sigma.
For a product term with factors K_c and K_{-c} = prod_{c' != c} K_c' (formed explicitly, never as K / K_c):

    K               = prod_c K_c
    dK/dtheta_{c,j} = K_{-c} dK_c/dtheta_{c,j}
    dK/dx*          = sum_c K_{-c} dK_c/dx*          (x* the first argument: the test point of a cross kernel)

Cross kernels have the TEST points as rows ([m, n]).  `dtype=np.longdouble` evaluates the same formulas in extended precision: the
yardstick of the restatement's own rounding error (the constants sqrt3, sqrt5 of the Matern parts stay the float64 ones)."""
import numpy as np
import scipy.linalg as sla

import matern_ref as mr
import periodic_ref as per
import rq_ref as rq

JITTER = mr.JITTER
width = per.width


def factors(term):
    return (term,) if isinstance(term, str) else tuple(term)


def flat(terms):
    """The part names of every term in hp order."""
    return [p for t in terms for p in factors(t)]


def nhp_of(terms, d):
    return per.nhp_of(flat(terms), d)


def _chunks(terms, d):
    """(term, [(part, a, b) of each factor]) in order."""
    o = 0
    for t in terms:
        blocks = []
        for p in factors(t):
            blocks.append((p, o, o + width(p, d)))
            o += width(p, d)
        yield t, blocks


def _others(vals, c):
    out = 1.0
    for c2, v in enumerate(vals):
        if c2 != c:
            out = out * v
    return out


def _part_xgrad(part, hpc, x, xp, dtype):
    """dK_c[p, i] / dxp_pk of one stationary part as a list of d arrays [m, n]."""
    d = x.shape[1]
    if part == "per":
        kv = per._value(part, hpc, x, xp, dtype)
        return [-kv * hpc[1 + k] ** 2 * np.sin(2 * per._phase(hpc, x, xp, k, dtype)) * per._pi(dtype) / hpc[d + 1 + k] for k in range(d)]
    base = rq._radial(part, hpc, mr._sq(hpc, x, xp))[1]
    return [rq.COEF[part] * base * hpc[1 + k] ** 2 * mr._diff(x, xp, k) for k in range(d)]


def _cast(dtype, *arrays):
    return [None if a is None else np.asarray(a, dtype) for a in arrays]


def kernel(terms, hp, x, xp=None, dtype=np.float64):
    hp, x, xp = _cast(dtype, hp, x, xp)
    n, d = x.shape
    out = np.zeros((n if xp is None else xp.shape[0], n), dtype)
    for t, blocks in _chunks(terms, d):
        if t == "wn":
            if xp is None:
                out += hp[blocks[0][1]] ** 2 * np.eye(n, dtype=dtype)
            continue
        term = 1.0
        for p, a, b in blocks:
            term = term * per._value(p, hp[a:b], x, xp, dtype)
        out += term
    return out


def _grad_terms(terms, hp, x, dtype=np.float64):
    """Yield (hp index, dK slab) one at a time."""
    hp, x = _cast(dtype, hp, x)
    n, d = x.shape
    for t, blocks in _chunks(terms, d):
        if t == "wn":
            yield blocks[0][1], 2 * hp[blocks[0][1]] * np.eye(n, dtype=dtype)
            continue
        vals = [per._value(p, hp[a:b], x, None, dtype) for p, a, b in blocks]
        for c, (p, a, b) in enumerate(blocks):
            oth = _others(vals, c)
            for j, slab in per._grad_terms([p], hp[a:b], x, dtype):
                yield a + j, oth * slab


def kernel_and_grad(terms, hp, x, dtype=np.float64):
    """K [n, n] and dK [nhp, n, n] (Covar.kernel_and_grad)."""
    n, d = np.shape(x)
    dk = np.empty((nhp_of(terms, d), n, n), dtype)
    for i, slab in _grad_terms(terms, hp, x, dtype):
        dk[i] = slab
    return kernel(terms, hp, x, dtype=dtype), dk


def kernel_xgrad(terms, hp, x, xp, dtype=np.float64):
    """dK*[p, i] / dxp_pk as [d, m, n]: the derivative of the cross kernel in its test point."""
    hp, x, xp = _cast(dtype, hp, x, xp)
    n, d = x.shape
    out = np.zeros((d, xp.shape[0], n), dtype)
    for t, blocks in _chunks(terms, d):
        if t == "wn":
            continue
        vals = [per._value(p, hp[a:b], x, xp, dtype) for p, a, b in blocks]
        for c, (p, a, b) in enumerate(blocks):
            oth = _others(vals, c)
            for k, slab in enumerate(_part_xgrad(p, hp[a:b], x, xp, dtype)):
                out[k] += oth * slab
    return out


def _factor(terms, hp, x, y):
    k = kernel(terms, hp, x)
    k[np.diag_indices_from(k)] += JITTER
    c = sla.cho_factor(k, lower=True)
    return c, sla.cho_solve(c, y)


def nlml(terms, hp, x, y):
    c, alpha = _factor(terms, hp, x, y)
    return 0.5 * float(alpha @ y) + float(np.sum(np.log(np.diag(c[0])))) + 0.5 * y.shape[0] * np.log(2.0 * np.pi)


def nlml_and_grad(terms, hp, x, y):
    """MLE.loss_and_grad: NLML and g_p = 1/2 sum_ij (K^-1 - a a^T)_ij dK_p,ij."""
    c, alpha = _factor(terms, hp, x, y)
    n = y.shape[0]
    loss = 0.5 * float(alpha @ y) + float(np.sum(np.log(np.diag(c[0])))) + 0.5 * n * np.log(2.0 * np.pi)
    w = sla.cho_solve(c, np.eye(n))
    w -= np.outer(alpha, alpha)
    g = np.zeros(np.size(hp))
    for i, slab in _grad_terms(terms, hp, x):
        g[i] = 0.5 * float(np.sum(w * slab))
    return loss, g


def predict(terms, hp, x, y, xp, var="diag"):
    """Exact_GP.predict: mean K* alpha and the diagonal / full covariance K** - K* K^-1 K*^T (K** keeps the noise)."""
    c, alpha = _factor(terms, hp, x, y)
    ks = kernel(terms, hp, x, xp)
    kss = kernel(terms, hp, xp)
    v = ks @ sla.cho_solve(c, ks.T)
    mean = ks @ alpha
    return (mean, np.diag(kss) - np.diag(v)) if var == "diag" else (mean, kss - v)


def predict_grads(terms, hp, x, y, xp):
    """d mean_p / d xp_p and d var_p / d xp_p, both [m, d] (the diagonal of K** is constant in xp)."""
    c, alpha = _factor(terms, hp, x, y)
    ks = kernel(terms, hp, x, xp)
    dks = kernel_xgrad(terms, hp, x, xp)
    v = sla.cho_solve(c, ks.T).T                       # (K^-1 K*^T)^T [m, n]
    return np.einsum("kpi,i->pk", dks, alpha), -2.0 * np.einsum("kpi,pi->pk", dks, v)


def predict_vjp(terms, hp, x, y, xp, var, g_mu, g_2=None):
    """<g_mu, mean> + <g_2, var | covariance> differentiated in xp [m, d]: the autograd backward of Exact_GP.predict."""
    c, alpha = _factor(terms, hp, x, y)
    ks = kernel(terms, hp, x, xp)
    dks = kernel_xgrad(terms, hp, x, xp)
    out = np.einsum("kpi,i,p->pk", dks, alpha, g_mu)
    if var == "none":
        return out
    v = sla.cho_solve(c, ks.T).T
    if var == "diag":
        return out - 2.0 * np.einsum("kpi,pi,p->pk", dks, v, g_2)
    gs = g_2 + g_2.T
    out -= np.einsum("kpi,pi->pk", dks, gs @ v)
    # K**[p, q] moves with both of its points: the row derivative against G + G^T (its own diagonal has D = 0)
    return out + np.einsum("kpq,pq->pk", kernel_xgrad(terms, hp, xp, xp), gs)


def loo(terms, hp, x, y):
    """Leave-one-out mean and variance of every training point (Rasmussen & Williams 5.4.2) from K^-1 of the matrix the model factors."""
    c, alpha = _factor(terms, hp, x, y)
    cd = np.diag(sla.cho_solve(c, np.eye(y.shape[0])))
    return y - alpha / cd, 1.0 / cd


def grbcm_predict(terms, hp_g, hp_l, xl, yl, xg, yg, xs):
    """GRBCM.predict(var="diag"): global expert on (xg, yg), local expert c on (xg U xl[c]), aggregated as the reference's committee."""
    mg, vg = predict(terms, hp_g, xg, yg, xs)
    ml, vl = [], []
    for c in range(xl.shape[0]):
        m, v = predict(terms, hp_l[c], np.concatenate([xg, xl[c]]), np.concatenate([yg, yl[c]]), xs)
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
