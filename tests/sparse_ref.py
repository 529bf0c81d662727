"""NumPy restatement of the inducing-point GP (Titsias' collapsed bound) on top of tests/kernel_ref.py: the reference of the Sparse_GP
tests.  Host only.

With Kuu = k(z, z) + JITTER I, Kuf = k(z, x) (rows = inducing points), sigma^2 = sum of the squared White_noise parameters,
Q = Kuf^T Kuu^-1 Kuf and kdiag the constant prior variance of the stationary terms, the loss (the negative bound) is given two ways:

  dense      1/2 y^T (Q + sigma^2 I)^-1 y + 1/2 log |Q + sigma^2 I| + n/2 log 2pi + tr(Kff - Q) / (2 sigma^2)      (n x n algebra)
  Woodbury   sum log diag Ls - sum log diag Lu + n/2 log sigma^2 + y^T y / (2 sigma^2) - b^T c / (2 sigma^4) + n/2 log 2pi + T / (2 sigma^2)
             Phi = Kuf Kuf^T, b = Kuf y, Sigma = Kuu + Phi / sigma^2, c = Sigma^-1 b, T = n kdiag - tr(Kuu^-1 Phi)      (m x m algebra)

Their disagreement on an input is the restatement's own error there: the yardstick of the model-level tolerances.  The gradient is the
closed form of the Woodbury expression (module docstring of pygpr_amd/sparse.py), contracted against the cross derivative slabs of
`cross_grad_terms`, the two-point-set variant of kernel_ref.grad_terms."""
import numpy as np
import scipy.linalg as sla

import kernel_ref as kr

JITTER = kr.JITTER


# ---- the cross derivative ------------------------------------------------------------------------------------------------------------
def _part_cross_grad(part, hpc, x, xp, dtype):
    """kernel_ref._part_grad on two point sets: yield (index in the part's block, dK_c [m, n] slab), rows = xp."""
    d = x.shape[1]
    if part == "per":
        kv = kr.stationary(part, hpc, x, xp, dtype)
        yield 0, kv * (2 / hpc[0])
        for k in range(d):
            ph = kr._phase(hpc, x, xp, k, dtype)
            yield 1 + k, -2 * kv * hpc[1 + k] * np.sin(ph) ** 2
            yield d + 1 + k, kv * hpc[1 + k] ** 2 * np.sin(2 * ph) * ph / hpc[d + 1 + k]
        return
    kv, base, shape = kr.radial(part, hpc, kr.sqdist(hpc, x, xp))
    yield 0, kv * (2.0 / hpc[0])
    for k in range(d):
        df = kr._diff(x, xp, k)
        yield 1 + k, kr.COEF[part] * base * hpc[1 + k] * df * df
    if shape is not None:
        yield d + 1, shape


def cross_grad_terms(terms, hp, x, xp, dtype=np.float64):
    """Yield (hp index, dk(xp_i, x_j)/dtheta slab [m, n]) of every stationary parameter; White_noise has no cross derivative."""
    hp, x, xp = kr._cast(dtype, hp, x, xp)
    d = x.shape[1]
    for t, blocks in kr._chunks(terms, d):
        if t == "wn":
            continue
        vals = [kr.stationary(p, hp[a:b], x, xp, dtype) for p, a, b in blocks] if len(blocks) > 1 else []
        for c, (p, a, b) in enumerate(blocks):
            oth = kr._others(vals, c)
            for j, slab in _part_cross_grad(p, hp[a:b], x, xp, dtype):
                yield a + j, oth * slab


def cross_grad(terms, hp, z, x, w, dtype=np.float64, grad=None):
    """pg_kernel_cross_grad: grad[p] = sum_ij w[i][j] dk(z_i, x_j)/dtheta_p, the other entries untouched (zero when grad is None)."""
    out = np.zeros(np.size(hp), dtype) if grad is None else grad
    w = np.asarray(w, dtype)
    for i, slab in cross_grad_terms(terms, hp, x, z, dtype):
        out[i] = np.sum(w * slab)
    return out


# ---- the pieces ----------------------------------------------------------------------------------------------------------------------
def _offsets(terms, d):
    """[(term, [offset of each factor's sigma])], [noise offsets]."""
    stat, noise = [], []
    for t, blocks in kr._chunks(terms, d):
        if t == "wn":
            noise.append(blocks[0][1])
        else:
            stat.append((t, [a for _, a, _ in blocks]))
    return stat, noise


def sigma2(terms, hp, d):
    return float(sum(hp[o] ** 2 for o in _offsets(terms, d)[1]))


def kdiag(terms, hp, d):
    return float(sum(np.prod([hp[o] ** 2 for o in offs]) for _, offs in _offsets(terms, d)[0]))


def kuu_kuf(terms, hp, x, z):
    kuu = kr.kernel(terms, hp, z, z)                     # a cross build of z against itself: no noise
    kuu[np.diag_indices_from(kuu)] += JITTER
    return kuu, kr.kernel(terms, hp, x, z)               # rows = z


# ---- the loss, two ways --------------------------------------------------------------------------------------------------------------
def loss_dense(terms, hp, x, y, z):
    n, d = x.shape
    s2 = sigma2(terms, hp, d)
    kuu, kuf = kuu_kuf(terms, hp, x, z)
    q = kuf.T @ sla.cho_solve(sla.cho_factor(kuu, lower=True), kuf)
    c = sla.cho_factor(q + s2 * np.eye(n), lower=True)
    return (0.5 * float(y @ sla.cho_solve(c, y)) + float(np.sum(np.log(np.diag(c[0])))) + 0.5 * n * np.log(2.0 * np.pi)
            + (n * kdiag(terms, hp, d) - float(np.trace(q))) / (2.0 * s2))


def _woodbury(terms, hp, x, y, z):
    n, d = x.shape
    s2 = sigma2(terms, hp, d)
    kuu, kuf = kuu_kuf(terms, hp, x, z)
    phi = kuf @ kuf.T
    b = kuf @ y
    sg = kuu + phi / s2
    cu, cs = sla.cho_factor(kuu, lower=True), sla.cho_factor(sg, lower=True)
    c = sla.cho_solve(cs, b)
    m = z.shape[0]
    kuui, sgi = sla.cho_solve(cu, np.eye(m)), sla.cho_solve(cs, np.eye(m))
    t = n * kdiag(terms, hp, d) - float(np.sum(kuui * phi))
    return dict(n=n, d=d, s2=s2, kuu=kuu, kuf=kuf, phi=phi, b=b, cu=cu, cs=cs, c=c, kuui=kuui, sgi=sgi, t=t, yy=float(y @ y))


def loss_woodbury(terms, hp, x, y, z, parts=None):
    p = parts or _woodbury(terms, hp, x, y, z)
    n, s2 = p["n"], p["s2"]
    return (float(np.sum(np.log(np.diag(p["cs"][0])))) - float(np.sum(np.log(np.diag(p["cu"][0])))) + 0.5 * n * np.log(s2)
            + p["yy"] / (2 * s2) - float(p["b"] @ p["c"]) / (2 * s2 ** 2) + 0.5 * n * np.log(2 * np.pi) + p["t"] / (2 * s2))


def self_error(terms, hp, x, y, z):
    """|dense - Woodbury| relative to the loss: the restatement's own error on this input."""
    a, b = loss_dense(terms, hp, x, y, z), loss_woodbury(terms, hp, x, y, z)
    return abs(a - b) / abs(a)


def loss_and_grad(terms, hp, x, y, z):
    """The Woodbury loss and its closed-form gradient in every hyper-parameter."""
    p = _woodbury(terms, hp, x, y, z)
    n, d, s2, c, kuf = p["n"], p["d"], p["s2"], p["c"], p["kuf"]
    g_uu = 0.5 * p["sgi"] - 0.5 * p["kuui"] + np.outer(c, c) / (2 * s2 ** 2) + p["kuui"] @ p["phi"] @ p["kuui"] / (2 * s2)
    g_uf = (p["sgi"] - p["kuui"]) @ kuf / s2 - np.outer(c, y - kuf.T @ c / s2) / s2 ** 2
    g = cross_grad(terms, hp, z, z, g_uu)
    g += cross_grad(terms, hp, z, x, g_uf)
    ds2 = (-float(np.sum(p["sgi"] * p["phi"])) / (2 * s2 ** 2) + n / (2 * s2) - p["yy"] / (2 * s2 ** 2) + float(p["b"] @ c) / s2 ** 3
           - float(c @ p["phi"] @ c) / (2 * s2 ** 4) - p["t"] / (2 * s2 ** 2))
    stat, noise = _offsets(terms, d)
    for o in noise:
        g[o] = 2.0 * hp[o] * ds2
    for _, offs in stat:
        for o in offs:
            g[o] += n / (2 * s2) * 2.0 * hp[o] * np.prod([hp[o2] ** 2 for o2 in offs if o2 != o])
    return loss_woodbury(terms, hp, x, y, z, p), g


def predict(terms, hp, x, y, z, xp, var="diag"):
    """Sparse_GP.predict: mean Ksu c / sigma^2 and the diagonal / full covariance Kss - Ksu (Kuu^-1 - Sigma^-1) Kus (Kss keeps the noise)."""
    p = _woodbury(terms, hp, x, y, z)
    ksu = kr.kernel(terms, hp, z, xp)                   # rows = xp
    mean = ksu @ p["c"] / p["s2"]
    v = ksu @ (p["kuui"] - p["sgi"]) @ ksu.T
    kss = kr.kernel(terms, hp, xp)
    return (mean, np.diag(kss) - np.diag(v)) if var == "diag" else (mean, kss - v)


def predict_dense(terms, hp, x, y, z, xp):
    """The same mean and full covariance through the n x n form: Q** - Q*f (Qff + sigma^2 I)^-1 Qf* + (Kss - Q**)."""
    d = x.shape[1]
    s2 = sigma2(terms, hp, d)
    kuu, kuf = kuu_kuf(terms, hp, x, z)
    cu = sla.cho_factor(kuu, lower=True)
    ksu = kr.kernel(terms, hp, z, xp)
    qsf = ksu @ sla.cho_solve(cu, kuf)
    qff = kuf.T @ sla.cho_solve(cu, kuf)
    c = sla.cho_factor(qff + s2 * np.eye(x.shape[0]), lower=True)
    mean = qsf @ sla.cho_solve(c, y)
    return mean, kr.kernel(terms, hp, xp) - qsf @ sla.cho_solve(c, qsf.T)


# ---- inducing points that keep the reference well inside its own tolerance -----------------------------------------------------------
def pick_z(x, scale, m, min_dist=0.3):
    """Indices of a greedy subset of x with pairwise distance >= min_dist in the scaled units `scale` (the inverse length scales), in
    index order; raises when fewer than m points qualify."""
    xs = x * scale
    keep = []
    for i in range(x.shape[0]):
        if all(np.sqrt(np.sum((xs[i] - xs[j]) ** 2)) >= min_dist for j in keep):
            keep.append(i)
            if len(keep) == m:
                return np.array(keep)
    raise ValueError("only %d of %d inducing points at distance >= %g" % (len(keep), m, min_dist))


def problem(terms, n=300, m=40, d=3, seed=3):
    """(hp, x, y, z) of a seeded regression problem on the unit cube: z a subset of x at pairwise distance >= 0.3 in scaled units,
    cond(Kuu) <= 1e6 (asserted) -- the restatement's two forms then agree to 1e-12 and better (tests/test_sparse_cpu.py prints it)."""
    rng = np.random.default_rng(seed)
    x = rng.random((n, d))
    y = np.sin(3.0 * x.sum(1)) + 0.1 * rng.standard_normal(n)
    hp = []
    for part in kr.flat(terms):
        if part == "wn":
            hp += [0.3]
        else:
            hp += [0.9 + 0.2 * rng.random()] + list(2.5 + 0.6 * rng.random(d))
            hp += [1.5] if part == "rq" else (list(0.7 + 0.3 * rng.random(d)) if part == "per" else [])
    hp = np.array(hp)
    scale = min(hp[a + 1: a + 1 + d].min() for t, blocks in kr._chunks(terms, d) if t != "wn" for _, a, _ in blocks)
    z = x[pick_z(x, scale, m)]
    assert np.linalg.cond(kuu_kuf(terms, hp, x, z)[0]) <= 1e6
    return hp, x, y, z


def tol_of(err):
    """The issue's rule: 50 x the restatement's own error on the input, floored at 1e-10 (relative)."""
    return max(50.0 * err, 1e-10)
