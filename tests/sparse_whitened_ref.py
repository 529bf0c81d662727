"""NumPy restatement of the WHITENED inducing-point GP (pygpr_amd/sparse.py, "Whitened evaluation") on top of
tests/kernel_ref.py and tests/sparse_ref.py: loss, gradient in the hyper-parameters and in z, mean, variance, full covariance and the
derivatives of a prediction in the test points.  Host only.

With Lu = chol(Kuu + JITTER I), Li = Lu^-1, V = Li Kuf, Psi = V V^T, b~ = V y, D = I + Psi / sigma^2, Ld = chol(D), c~ = D^-1 b~ (by
substitution against Ld) and E = I - D^-1:

    L     = sum log diag Ld + n/2 log sigma^2 + y^T y / (2 sigma^2) - b~^T c~ / (2 sigma^4) + n/2 log 2pi + (n kdiag - tr Psi) / (2 sigma^2)
    G_uu  = 1/2 Li^T [(D^-1 - I) + c~ c~^T / sigma^4 + Psi / sigma^2] Li
    G_uf  = Li^T (M~ V - c~ y^T / sigma^4),      M~ = (D^-1 - I) / sigma^2 + c~ c~^T / sigma^6
    mean* = w c~ / sigma^2,   cov* = Kss - (w E) w^T,   w = Ksu Li^T

Everything is written ONCE over a dtype and runs in float64 and in np.longdouble: the difference between the two on an input is the
restatement's own error there, the yardstick of the model-level tolerances (`answers`).  LAPACK has no long double, so the Cholesky
factorisation, the triangular inverse and the substitutions are plain loops over rows; every result asserts that its dtype carried
through.

The FOLDED forms (`folded_weights`, `folded_var`) fold the whitened m x m quantities back into one matrix that is applied to the
unwhitened Kuf / Ksu.  They are algebraically the same and numerically worse at small noise: tests/test_sparse_whitened_cpu.py keeps
that measured, because it is the reason the library whitens per chunk."""
import functools

import numpy as np
import scipy.linalg as sla

import kernel_ref as kr
import sparse_ref as sr

JITTER = kr.JITTER
LD = np.longdouble


# ---- linear algebra in any dtype -----------------------------------------------------------------------------------------------------
def chol(a):
    """Lower Cholesky factor, row by row; LinAlgError at a pivot that is not positive (what LAPACK reports)."""
    n = a.shape[0]
    l = np.zeros_like(a)
    for i in range(n):
        for j in range(i):
            l[i, j] = (a[i, j] - l[i, :j] @ l[j, :j]) / l[j, j]
        s = a[i, i] - l[i, :i] @ l[i, :i]
        if not s > 0:
            raise np.linalg.LinAlgError("pivot %d is not positive: %g" % (i, float(s)))
        l[i, i] = np.sqrt(s)
    return l


def tri_inv(l):
    """L^-1 of a lower-triangular L by forward substitution, row by row."""
    n = l.shape[0]
    x = np.zeros_like(l)
    eye = np.eye(n, dtype=l.dtype)
    for i in range(n):
        x[i] = (eye[i] - l[i, :i] @ x[:i]) / l[i, i]
    return x


def chol_solve(l, b):
    """(L L^T)^-1 b for a vector b: forward, then backward substitution."""
    n = l.shape[0]
    u = np.zeros_like(b)
    for i in range(n):
        u[i] = (b[i] - l[i, :i] @ u[:i]) / l[i, i]
    x = np.zeros_like(b)
    for i in range(n - 1, -1, -1):
        x[i] = (u[i] - l[i + 1:, i] @ x[i + 1:]) / l[i, i]
    return x


# ---- the pieces ----------------------------------------------------------------------------------------------------------------------
def parts(terms, hp, x, y, z, dtype=np.float64):
    hp, x, y, z = kr._cast(dtype, hp, x, y, z)
    n, d = x.shape
    m = z.shape[0]
    stat, noise = sr._offsets(terms, d)
    s2 = sum(hp[o] ** 2 for o in noise)
    kd = sum(np.prod([hp[o] ** 2 for o in offs]) for _, offs in stat)
    kuu = kr.kernel(terms, hp, z, z, dtype)                  # a cross build of z against itself: no noise
    kuu[np.diag_indices(m)] += dtype(JITTER)
    kuf = kr.kernel(terms, hp, x, z, dtype)                  # rows = z
    lu = chol(kuu)
    li = tri_inv(lu)
    v = li @ kuf
    psi = v @ v.T
    bt = v @ y
    dm = np.eye(m, dtype=dtype) + psi / s2
    ld = chol(dm)
    ct = chol_solve(ld, bt)
    ldi = tri_inv(ld)
    di = ldi.T @ ldi
    p = dict(n=n, d=d, m=m, s2=s2, kd=kd, kuu=kuu, kuf=kuf, lu=lu, li=li, v=v, psi=psi, bt=bt, dm=dm, ld=ld, ct=ct, di=di, yy=y @ y,
             y=y, stat=stat, noise=noise, hp=hp, eye=np.eye(m, dtype=dtype))
    for k in ("s2", "kuu", "kuf", "li", "v", "psi", "ct", "di", "yy"):
        assert np.asarray(p[k]).dtype == dtype, (k, np.asarray(p[k]).dtype)      # the restatement really ran in that precision
    return p


def loss(terms, hp, x, y, z, dtype=np.float64, p=None):
    p = p or parts(terms, hp, x, y, z, dtype)
    n, s2 = p["n"], p["s2"]
    two_pi = 2 * kr._pi(dtype)
    out = (np.sum(np.log(np.diag(p["ld"]))) + n * np.log(s2) / 2 + p["yy"] / (2 * s2) - (p["bt"] @ p["ct"]) / (2 * s2 ** 2)
           + n * np.log(two_pi) / 2 + (n * p["kd"] - np.trace(p["psi"])) / (2 * s2))
    assert out.dtype == dtype
    return out


def weights(p):
    """(G_uu [m, m], G_uf [m, n]) in original coordinates, whitened per column of Kuf: what the library forms per chunk."""
    s2, ct, li = p["s2"], p["ct"], p["li"]
    xm = (p["di"] - p["eye"]) + np.outer(ct, ct) / s2 ** 2 + p["psi"] / s2
    g_uu = li.T @ xm @ li / 2
    mt = (p["di"] - p["eye"]) / s2 + np.outer(ct, ct) / s2 ** 3
    g_uf = li.T @ (mt @ p["v"] - np.outer(ct, p["y"]) / s2 ** 2)
    return g_uu, g_uf


def folded_weights(p):
    """The same G_uf with the whitened quantities folded into one m x m matrix and applied to the UNWHITENED Kuf (measured to be
    worse: see the module docstring)."""
    s2, ct, li = p["s2"], p["ct"], p["li"]
    mt = (p["di"] - p["eye"]) / s2 + np.outer(ct, ct) / s2 ** 3
    mf = li.T @ mt @ li
    cf = li.T @ ct
    return weights(p)[0], mf @ p["kuf"] - np.outer(cf, p["y"]) / s2 ** 2


def _grad_from(terms, p, g_uu, g_uf, x, z, dtype):
    hp, n, s2, ct, m = p["hp"], p["n"], p["s2"], p["ct"], p["m"]
    g = sr.cross_grad(terms, hp, z, z, g_uu, dtype)
    g = g + sr.cross_grad(terms, hp, z, x, g_uf, dtype)
    t = n * p["kd"] - np.trace(p["psi"])
    ds2 = (-(m - np.trace(p["di"])) / (2 * s2) + n / (2 * s2) - p["yy"] / (2 * s2 ** 2) + (p["bt"] @ ct) / s2 ** 3
           - (ct @ p["psi"] @ ct) / (2 * s2 ** 4) - t / (2 * s2 ** 2))
    for o in p["noise"]:
        g[o] = 2 * hp[o] * ds2
    for _, offs in p["stat"]:
        for o in offs:
            g[o] += n / (2 * s2) * 2 * hp[o] * np.prod([hp[o2] ** 2 for o2 in offs if o2 != o])
    assert g.dtype == dtype
    return g


def loss_and_grad(terms, hp, x, y, z, dtype=np.float64, folded=False):
    """The whitened loss and its closed-form gradient in every hyper-parameter."""
    p = parts(terms, hp, x, y, z, dtype)
    g_uu, g_uf = folded_weights(p) if folded else weights(p)
    return loss(terms, hp, x, y, z, dtype, p), _grad_from(terms, p, g_uu, g_uf, x, z, dtype)


def z_grad(terms, hp, x, y, z, dtype=np.float64):
    """dL/dz [m, d]: 2 sum_j G_uu[i][j] dk(z_i, z_j)/dz_i + sum_j G_uf[i][j] dk(z_i, x_j)/dz_i."""
    g_uu, g_uf = weights(parts(terms, hp, x, y, z, dtype))
    dzz = kr.kernel_xgrad(terms, hp, z, z, dtype)
    dzx = kr.kernel_xgrad(terms, hp, x, z, dtype)
    out = 2 * np.einsum("kij,ij->ik", dzz, g_uu) + np.einsum("kij,ij->ik", dzx, g_uf)
    assert out.dtype == dtype
    return out


def predict(terms, hp, x, y, z, xp, dtype=np.float64, p=None):
    """(mean [q], covariance [q, q], prior variance kss [q]) with the noise on the diagonal of Kss."""
    p = p or parts(terms, hp, x, y, z, dtype)
    ksu = kr.kernel(terms, p["hp"], z, xp, dtype)            # rows = xp
    w = ksu @ p["li"].T
    e = p["eye"] - p["di"]
    kss = kr.kernel(terms, p["hp"], xp, dtype=dtype)
    mean, cov = w @ p["ct"] / p["s2"], kss - (w @ e) @ w.T
    assert mean.dtype == dtype and cov.dtype == dtype
    return mean, cov, np.diag(kss).copy()


def folded_var(terms, hp, x, y, z, xp, dtype=np.float64):
    """The predictive variance with B = Li^T E Li folded and applied to the unwhitened Ksu."""
    p = parts(terms, hp, x, y, z, dtype)
    ksu = kr.kernel(terms, p["hp"], z, xp, dtype)
    bf = p["li"].T @ (p["eye"] - p["di"]) @ p["li"]
    return np.diag(kr.kernel(terms, p["hp"], xp, dtype=dtype)) - np.sum((ksu @ bf) * ksu, axis=1)


def predict_grads(terms, hp, x, y, z, xp, dtype=np.float64):
    """d mean_p / d xp_p and d var_p / d xp_p, both [q, d]: u = Li^T c~ / sigma^2 and V = (w E) Li against dk(xp_p, z_i)/dxp_p."""
    p = parts(terms, hp, x, y, z, dtype)
    ksu = kr.kernel(terms, p["hp"], z, xp, dtype)
    dks = kr.kernel_xgrad(terms, p["hp"], z, xp, dtype)      # [d, q, m]
    w = ksu @ p["li"].T
    vm = (w @ (p["eye"] - p["di"])) @ p["li"]
    u = p["li"].T @ p["ct"] / p["s2"]
    dmean, dvar = np.einsum("kpi,i->pk", dks, u), -2 * np.einsum("kpi,pi->pk", dks, vm)
    assert dmean.dtype == dtype and dvar.dtype == dtype
    return dmean, dvar


# ---- the yardstick -------------------------------------------------------------------------------------------------------------------
def _rel(a, b, scale=None):
    a, b = np.asarray(a, LD), np.asarray(b, LD)
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) if scale is None else scale))


def answers(terms, hp, x, y, z, xp):
    """The float64 restatement's answers and, per quantity, its own error against the same formulas in np.longdouble: loss, gradient,
    z-gradient, mean and the test-point derivatives relative to the largest long-double entry; variance and covariance relative to the
    PRIOR variance kss (the hard input's posterior variances go down to 5e-8: relative to them nothing is held)."""
    ref, own = {}, {}
    both = {}
    for dt in (np.float64, LD):
        l, g = loss_and_grad(terms, hp, x, y, z, dt)
        mu, cov, kss = predict(terms, hp, x, y, z, xp, dt)
        dm, dv = predict_grads(terms, hp, x, y, z, xp, dt)
        both[dt] = dict(loss=l, grad=g, zgrad=z_grad(terms, hp, x, y, z, dt), mean=mu, cov=cov, var=np.diag(cov).copy(), dmean=dm,
                        dvar=dv, kss=kss)
    for k, v in both[np.float64].items():
        ref[k] = np.asarray(v, np.float64)
        if k != "kss":
            own[k] = _rel(v, both[LD][k], float(np.max(both[LD]["kss"])) if k in ("var", "cov") else None)
    return ref, own


def hard_problem(seed=1, n=300, m=60, d=3):
    """(terms, hp, x, y, z): se + wn at sigma_n = 1e-4 (White_noise.init_params) with unit sigma and unit length scale, x uniform on
    the unit cube, z a random subset of x.  The unit length scale is the conventional one, k = exp(-r^2 / 2): the library's
    k = sigma^2 exp(-sum (l_k D_k)^2) takes it as l_k = 1 / sqrt(2).  cond(Kuu) is then about 5e8 and the unwhitened Sigma is not
    numerically positive definite (smallest eigenvalue about -6e-5); the tests assert both on their seed."""
    rng = np.random.default_rng(seed)
    x = rng.random((n, d))
    y = np.sin(3.0 * x.sum(1)) + 0.1 * rng.standard_normal(n)
    z = x[np.sort(rng.choice(n, m, replace=False))].copy()
    return ["se", "wn"], np.array([1.0] + [np.sqrt(0.5)] * d + [1e-4]), x, y, z


def hard_preconditions(terms, hp, x, y, z):
    """What makes the hard input hard, asserted with SciPy so that a changed fixture cannot quietly become easy: cond(Kuu) of 1e8 and
    more, LAPACK fails to factor the unwhitened Sigma = Kuu + Phi / sigma^2 (not numerically positive definite), and D = I + Psi / sigma^2
    has no eigenvalue below 1 (within the rounding of its largest, 1e10).  Returns (cond(Kuu), smallest eigenvalue of Sigma, of D)."""
    kuu, kuf = sr.kuu_kuf(terms, hp, x, z)
    sg = kuu + kuf @ kuf.T / sr.sigma2(terms, hp, x.shape[1])
    cond, lo_s = float(np.linalg.cond(kuu)), float(sla.eigvalsh(sg)[0])
    lo_d = float(sla.eigvalsh(parts(terms, hp, x, y, z)["dm"])[0])
    assert cond >= 1e8, cond
    try:
        sla.cho_factor(sg, lower=True)
    except sla.LinAlgError:
        pass
    else:
        raise AssertionError("LAPACK factors the unwhitened Sigma of the hard input (smallest eigenvalue %.2e)" % lo_s)
    assert lo_d >= 0.99, lo_d
    return cond, lo_s, lo_d


# ---- the inputs of the model-level tests, with their answers ---------------------------------------------------------------------------
TERMS = {"se+wn": ["se", "wn"], "se*per+wn": [("se", "per"), "wn"], "hard": ["se", "wn"], "coincident": ["se", "wn"]}
EASY = ["se+wn", "se*per+wn"]


@functools.lru_cache(maxsize=None)
def case(name):
    """(terms, hp, x, y, z, xp, the float64 restatement's answers, its own errors), computed once per input and shared by the tests:
    the easy inputs are sparse_ref.problem (n = 300, m = 40), "hard" is hard_problem, "coincident" the hard input with z[1] = z[0]."""
    if name in ("hard", "coincident"):
        terms, hp, x, y, z = hard_problem()
        if name == "coincident":
            z[1] = z[0]
    else:
        terms = TERMS[name]
        hp, x, y, z = sr.problem(terms)
    xp = np.random.default_rng(9).random((50, x.shape[1]))
    ref, own = answers(terms, hp, x, y, z, xp)
    print("restatement's own error", name, {k: "%.1e" % v for k, v in own.items()})
    return terms, hp, x, y, z, xp, ref, own


def hold(label, got, ref, own, scale=None, who="device"):
    """The tolerance rule: `got` may miss the float64 restatement by sparse_ref.tol_of(own), relative to the largest reference entry or
    to `scale` (variance and covariance: the prior variance).  Prints what it measured."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = float(np.abs(got - ref).max() / (np.abs(ref).max() if scale is None else scale))
    print("%-44s %s %.2e  restatement %.2e  (bound %.2e)" % (label, who, err, own, sr.tol_of(own)))
    assert np.isfinite(got).all() and err <= sr.tol_of(own), (label, err, own)
