"""NumPy / SciPy restatement of every covariance kind and of the exact-GP quantities built on them, with DIRECT differences, written
from the formulas: the reference of the kind tests (Matern family, rational quadratic, periodic, Product) and of everything the oracle
package does not cover.

A covariance is a list of TERMS in Compose order.  A term is a part name ("se", "m52", "m32", "m12", "rq", "per", "wn") or a tuple of
stationary part names, the factors of a product; a list without tuples is a plain sum.  hp is every part's block concatenated in that
order, each factor with its own sigma.  Cross kernels have the TEST points as rows ([m, n]), as the library's.

With D_k = x_k - x'_k, l the INVERSE length scales, sq = sum_k l_k^2 D_k^2, r = sqrt(sq) and dK/dsigma = 2 K / sigma for every
stationary part:

  hp = [sigma, l_1..l_d]
    se   K = s^2 exp(-r^2)                          dK/dl_k = -2 K l_k D_k^2
    m52  K = s^2 (1 + sqrt5 r + 5 r^2/3) e^-sqrt5 r  dK/dl_k = -5/3 s^2 (1 + sqrt5 r) e^-sqrt5 r l_k D_k^2
    m32  K = s^2 (1 + sqrt3 r) e^-sqrt3 r            dK/dl_k = -3 s^2 e^-sqrt3 r l_k D_k^2
    m12  K = s^2 e^-r                               dK/dl_k = -s^2 e^-r l_k D_k^2 / r  (0 at r = 0)
  each dK/dl_k = COEF base l_k D_k^2 and dK/dx*_k = COEF base l_k^2 D_k (x* the first argument: the test point of a cross kernel).

  rq: hp = [sigma, l_1..l_d, alpha], d + 2 values, the shape behind the block; every parameter enters squared:
    a = alpha^2,   t = sq / a
    K         = s^2 (1 + t)^(-a) = s^2 exp(-a log1p(t))
    dK/dl_k   = -2 [K / (1 + t)] l_k D_k^2
    dK/dalpha = 2 alpha K [t / (1 + t) - log1p(t)]
    dK/dx*_k  = -2 [K / (1 + t)] l_k^2 D_k

  per: hp = [sigma, l_1..l_d, p_1..p_d], 2 d + 1 values, the periods behind the block; the phase is formed from the coordinate
  DIFFERENCE.  With w_k = pi / p_k and s_k = sin(w_k D_k):
    sq        = sum_k l_k^2 s_k^2
    K         = sigma^2 exp(-sq)
    dK/dl_k   = -2 K l_k s_k^2
    dK/dp_k   = K l_k^2 sin(2 w_k D_k) w_k D_k / p_k
    dK/dx*_k  = -K l_k^2 sin(2 w_k D_k) w_k

  wn: hp = [sigma_n]; sigma_n^2 I on a symmetric build and nothing on a cross build.

  a product term with factors K_c and K_{-c} = prod_{c' != c} K_c' (formed explicitly, never as K / K_c):
    K               = prod_c K_c
    dK/dtheta_{c,j} = K_{-c} dK_c/dtheta_{c,j}
    dK/dx*          = sum_c K_{-c} dK_c/dx*

`dtype=np.longdouble` evaluates the same formulas in extended precision: the yardstick of the restatement's own rounding error.  The
constants sqrt3, sqrt5 of the Matern parts stay the float64 ones; pi is 4 atan(1) in `dtype`.  The gradient routines never hold the
[nhp, n, n] stack, so N = 4096 fits on the host."""
import numpy as np
import scipy.linalg as sla

JITTER = 1e-7
NU = {"m12": 0.5, "m32": 1.5, "m52": 2.5}
COEF = {"se": -2.0, "m52": -5.0 / 3.0, "m32": -3.0, "m12": -1.0, "rq": -2.0}


# ---- the parts -----------------------------------------------------------------------------------------------------------------------
def width(part, d):
    return 1 if part == "wn" else {"rq": d + 2, "per": 2 * d + 1}.get(part, d + 1)


def factors(term):
    return (term,) if isinstance(term, str) else tuple(term)


def flat(terms):
    """The part names of every term in hp order."""
    return [p for t in terms for p in factors(t)]


def nhp_of(terms, d):
    return sum(width(p, d) for p in flat(terms))


def _chunks(terms, d):
    """(term, [(part, a, b) of each factor]) in order."""
    o = 0
    for t in terms:
        blocks = []
        for p in factors(t):
            blocks.append((p, o, o + width(p, d)))
            o += width(p, d)
        yield t, blocks


def _diff(x, xp, k):
    """D_k [n, n] or [m, n] (rows = xp), formed when needed: the [d, n, n] stack would not fit at N = 4096."""
    a = x if xp is None else xp
    return a[:, k][:, None] - x[:, k][None, :]


def sqdist(hpc, x, xp=None):
    """The scaled squared distance sum_k l_k^2 D_k^2."""
    sq = 0.0
    for k in range(x.shape[1]):
        sq = sq + (hpc[1 + k] * _diff(x, xp, k)) ** 2
    return sq


def radial(part, hpc, sq):
    """(K, base, shape slab or None) of one part that is a function of the scaled squared distance; dK/dl_k = COEF base l_k D_k^2."""
    s2 = hpc[0] ** 2
    if part == "se":
        k = s2 * np.exp(-sq)
        return k, k, None
    if part == "rq":
        a = hpc[-1] ** 2
        t = sq / a
        lg = np.log1p(t)
        k = s2 * np.exp(-a * lg)
        return k, k / (1.0 + t), 2.0 * hpc[-1] * k * (t / (1.0 + t) - lg)
    r = np.sqrt(sq)
    if part == "m52":
        e = np.exp(-np.sqrt(5.0) * r)
        return s2 * (1.0 + np.sqrt(5.0) * r + (5.0 / 3.0) * sq) * e, s2 * (1.0 + np.sqrt(5.0) * r) * e, None
    if part == "m32":
        e = s2 * np.exp(-np.sqrt(3.0) * r)
        return (1.0 + np.sqrt(3.0) * r) * e, e, None
    if part == "m12":
        k = s2 * np.exp(-r)
        with np.errstate(divide="ignore", invalid="ignore"):
            base = np.where(sq > 0.0, k / np.where(sq > 0.0, r, 1.0), 0.0)
        return k, base, None
    raise ValueError(part)


def _pi(dtype):
    return 4 * np.arctan(dtype(1))


def _phase(hpc, x, xp, k, dtype):
    """w_k D_k [n, n] or [m, n] of a periodic part (rows = xp)."""
    d = x.shape[1]
    return _pi(dtype) * _diff(x, xp, k) / hpc[d + 1 + k]


def stationary(part, hpc, x, xp=None, dtype=np.float64):
    """One stationary part: K [n, n] (xp None) or [m, n]."""
    if part == "per":
        sq = 0.0
        for k in range(x.shape[1]):
            sq = sq + (hpc[1 + k] * np.sin(_phase(hpc, x, xp, k, dtype))) ** 2
        return hpc[0] ** 2 * np.exp(-sq)
    return radial(part, hpc, sqdist(hpc, x, xp))[0]


def _part_grad(part, hpc, x, dtype):
    """Yield (index in the part's block, dK_c slab) of one stationary part."""
    d = x.shape[1]
    if part == "per":
        kv = stationary(part, hpc, x, None, dtype)
        yield 0, kv * (2 / hpc[0])
        for k in range(d):
            ph = _phase(hpc, x, None, k, dtype)
            yield 1 + k, -2 * kv * hpc[1 + k] * np.sin(ph) ** 2
            yield d + 1 + k, kv * hpc[1 + k] ** 2 * np.sin(2 * ph) * ph / hpc[d + 1 + k]
        return
    kv, base, shape = radial(part, hpc, sqdist(hpc, x))
    yield 0, kv * (2.0 / hpc[0])
    for k in range(d):
        df = _diff(x, None, k)
        yield 1 + k, COEF[part] * base * hpc[1 + k] * df * df
    if shape is not None:
        yield d + 1, shape


def _part_xgrad(part, hpc, x, xp, dtype):
    """dK_c[p, i] / dxp_pk of one stationary part as a list of d arrays [m, n]."""
    d = x.shape[1]
    if part == "per":
        kv = stationary(part, hpc, x, xp, dtype)
        return [-kv * hpc[1 + k] ** 2 * np.sin(2 * _phase(hpc, x, xp, k, dtype)) * _pi(dtype) / hpc[d + 1 + k] for k in range(d)]
    base = radial(part, hpc, sqdist(hpc, x, xp))[1]
    return [COEF[part] * base * hpc[1 + k] ** 2 * _diff(x, xp, k) for k in range(d)]


# ---- the composition -----------------------------------------------------------------------------------------------------------------
def _others(vals, c):
    out = 1.0
    for c2, v in enumerate(vals):
        if c2 != c:
            out = out * v
    return out


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
            term = term * stationary(p, hp[a:b], x, xp, dtype)
        out += term
    return out


def grad_terms(terms, hp, x, dtype=np.float64):
    """Yield (hp index, dK slab) one at a time."""
    hp, x = _cast(dtype, hp, x)
    n, d = x.shape
    for t, blocks in _chunks(terms, d):
        if t == "wn":
            yield blocks[0][1], 2 * hp[blocks[0][1]] * np.eye(n, dtype=dtype)
            continue
        vals = [stationary(p, hp[a:b], x, None, dtype) for p, a, b in blocks] if len(blocks) > 1 else []      # (a lone part: K_{-c} = 1)
        for c, (p, a, b) in enumerate(blocks):
            oth = _others(vals, c)
            for j, slab in _part_grad(p, hp[a:b], x, dtype):
                yield a + j, oth * slab


def kernel_and_grad(terms, hp, x, dtype=np.float64):
    """K [n, n] and dK [nhp, n, n] (Covar.kernel_and_grad)."""
    n, d = np.shape(x)
    dk = np.empty((nhp_of(terms, d), n, n), dtype)
    for i, slab in grad_terms(terms, hp, x, dtype):
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
        vals = [stationary(p, hp[a:b], x, xp, dtype) for p, a, b in blocks]
        for c, (p, a, b) in enumerate(blocks):
            oth = _others(vals, c)
            for k, slab in enumerate(_part_xgrad(p, hp[a:b], x, xp, dtype)):
                out[k] += oth * slab
    return out


# ---- the exact GP --------------------------------------------------------------------------------------------------------------------
def factor(terms, hp, x, y):
    """The Cholesky factor of K + JITTER I, the matrix Exact_GP.update() factors, and alpha = K^-1 y."""
    k = kernel(terms, hp, x)
    k[np.diag_indices_from(k)] += JITTER
    c = sla.cho_factor(k, lower=True)
    return c, sla.cho_solve(c, y)


def nlml(terms, hp, x, y):
    c, alpha = factor(terms, hp, x, y)
    return 0.5 * float(alpha @ y) + float(np.sum(np.log(np.diag(c[0])))) + 0.5 * y.shape[0] * np.log(2.0 * np.pi)


def nlml_and_grad(terms, hp, x, y):
    """MLE.loss_and_grad: NLML and g_p = 1/2 sum_ij (K^-1 - a a^T)_ij dK_p,ij."""
    c, alpha = factor(terms, hp, x, y)
    n = y.shape[0]
    loss = 0.5 * float(alpha @ y) + float(np.sum(np.log(np.diag(c[0])))) + 0.5 * n * np.log(2.0 * np.pi)
    w = sla.cho_solve(c, np.eye(n))
    w -= np.outer(alpha, alpha)
    g = np.zeros(np.size(hp))
    for i, slab in grad_terms(terms, hp, x):
        g[i] = 0.5 * float(np.sum(w * slab))
    return loss, g


def predict(terms, hp, x, y, xp, var="diag"):
    """Exact_GP.predict: mean K* alpha and the diagonal / full covariance K** - K* K^-1 K*^T (K** keeps the noise)."""
    c, alpha = factor(terms, hp, x, y)
    ks = kernel(terms, hp, x, xp)
    kss = kernel(terms, hp, xp)
    v = ks @ sla.cho_solve(c, ks.T)
    mean = ks @ alpha
    return (mean, np.diag(kss) - np.diag(v)) if var == "diag" else (mean, kss - v)


def predict_grads(terms, hp, x, y, xp):
    """d mean_p / d xp_p and d var_p / d xp_p, both [m, d] (the diagonal of K** is constant in xp)."""
    c, alpha = factor(terms, hp, x, y)
    ks = kernel(terms, hp, x, xp)
    dks = kernel_xgrad(terms, hp, x, xp)
    v = sla.cho_solve(c, ks.T).T                       # (K^-1 K*^T)^T [m, n]
    return np.einsum("kpi,i->pk", dks, alpha), -2.0 * np.einsum("kpi,pi->pk", dks, v)


def predict_vjp(terms, hp, x, y, xp, var, g_mu, g_2=None):
    """<g_mu, mean> + <g_2, var | covariance> differentiated in xp [m, d]: the autograd backward of Exact_GP.predict."""
    c, alpha = factor(terms, hp, x, y)
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
    c, alpha = factor(terms, hp, x, y)
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
