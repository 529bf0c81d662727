"""Backward-error yardsticks of the dense linear algebra (factor, triangular inverse, solves, products): the matrix families, the metrics,
LAPACK's own figures on the same input, and a NumPy restatement of the library's algorithm that takes a hook to plant an error.
NumPy / SciPy only; shared by tests/test_backward_error_cpu.py and tests/test_backward_error_gpu.py ("Backward error of
the dense linear algebra").

Every metric is a componentwise relative residual, so it does not change under a symmetric diagonal scaling of A (up to rounding of the
scaling itself), and every one is evaluated in a higher precision than the data: np.longdouble for float64 data, float64 for float32.
Only the NUMERATOR needs that precision (it cancels to the rounding level); the denominators are sums of non-negative terms and are
formed in float64.  A zero denominator requires a zero numerator.

    factor   max_ij |A - L L^T|_ij / (|L| |L^T|)_ij                     lower triangle
    inverse  max |M L - I| / (|M| |L|)  and  max |L M - I| / (|L| |M|)  lower triangle
    product  max |C - op(A) op(B)| / (|op(A)| |op(B)|)
    solve    omega = max_i |y - A x|_i / (|A| |x| + |y|)_i               Oettli-Prager; the largest over the columns of a matrix y
    trisolve max |B - L X| / (|L| |X| + |B|)
    logdet   |got - ref| / sum_i |log L_ii|   (+ |y^T alpha| / 2 in the denominator for the NLML value)

For float64 data an n x n x n product in np.longdouble is too slow, so those figures are taken on the rows of `sample_rows` (ten fixed
rows at the block and panel edges plus forty drawn from the seed), with a float64 evaluation of ALL rows beside it as a coarse net:
float64 evaluates a residual entry with K terms to about (K + 2) 2^-53 of its denominator, so the net is held at NET times the bound."""
import functools

import numpy as np
from scipy.linalg import lapack

import kernel_ref as kr

NB = 128            # leaf / diagonal block of the library (linalg.hip: NB)
NBO = 512           # outer panel up to n = 10240 (linalg.hip: pg_nbo)
HB = 1024           # block of pg_potrs_vec's sweeps from n = 2 HB on (linalg.hip: HB)
NET = 64            # the float64 evaluation of all rows is held at NET times the bound of the sampled rows
FAMILIES = ("spd", "scaled", "gp")
U = {np.float64: 2.0 ** -53, np.float32: 2.0 ** -24}
# inverse length scale (the SE of kernel_ref is exp(-sum l_k^2 D_k^2): length scale 0.3 is l = 1 / (0.3 sqrt 2)) and sigma_n per dtype
GP_L = 1.0 / (0.3 * np.sqrt(2.0))
GP_NOISE = {np.float64: 1e-2, np.float32: 1e-1}
GP_COND = {np.float64: (1e6, 1e7), np.float32: (1e4, 1e5)}


def have_longdouble():
    return np.finfo(np.longdouble).nmant >= 63


def hp_of(dtype):
    """The evaluation precision for data of `dtype`."""
    return np.longdouble if dtype == np.float64 else np.float64


# ---- families ------------------------------------------------------------------------------------------------------------------------
def spd(n, seed):
    r = np.random.default_rng(seed).standard_normal((n, n))
    return r @ r.T / n + np.eye(n)


def scaled(n, seed, dtype=np.float64):
    rng = np.random.default_rng(seed + 1000)
    e = 6.0 if dtype == np.float64 else 3.0
    d = 10.0 ** rng.uniform(-e, e, n)
    a = spd(n, seed) * d[:, None] * d[None, :]
    return (a + a.T) / 2


def gp(n, seed, dtype=np.float64):
    x = np.random.default_rng(seed + 2000).random((n, 3))
    hp = np.array([1.0, GP_L, GP_L, GP_L, GP_NOISE[dtype]])
    a = kr.kernel(["se", "wn"], hp, x)
    return (a + a.T) / 2


@functools.lru_cache(maxsize=None)
def matrix(family, n, dtype=np.float64, seed=0):
    """The family's matrix as float64 values that are exact in `dtype` (float32 data: rounded first; that matrix is "A" for every figure).
    The gp family asserts the condition number of its unit-diagonal scaling."""
    a = {"spd": lambda: spd(n, seed), "scaled": lambda: scaled(n, seed, dtype), "gp": lambda: gp(n, seed, dtype)}[family]()
    a = a.astype(dtype).astype(np.float64)
    assert np.array_equal(a, a.T)
    if family == "gp":
        s = 1.0 / np.sqrt(np.diag(a))
        ev = np.linalg.eigvalsh(a * s[:, None] * s[None, :])
        c = ev[-1] / ev[0]
        lo, hi = GP_COND[dtype]
        assert lo <= c <= hi, ("gp family: condition number %.3g outside [%g, %g]" % (c, lo, hi))
    a.setflags(write=False)
    return a


def rhs(a, seed=0, ncol=None):
    """Right-hand sides scaled by sqrt(diag A), so that no row of the scaled family is negligible."""
    n = a.shape[0]
    y = np.random.default_rng(seed + 3000).standard_normal(n if ncol is None else (n, ncol))
    s = np.sqrt(np.diag(a))
    return y * (s if ncol is None else s[:, None])


def sample_rows(n, seed=0):
    fixed = [0, 1, 127, 128, 129, 511, 512, n - 129, n - 128, n - 1]
    drawn = np.random.default_rng(seed + 4000).choice(n, 40, replace=False)
    return np.unique(np.concatenate([fixed, drawn]).astype(np.int64))


# ---- metrics -------------------------------------------------------------------------------------------------------------------------
def _ratio(num, den, mask=None):
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    if mask is not None:
        num, den = num[mask], den[mask]
    zero = den == 0
    assert np.all(num[zero] == 0), "a zero denominator with a non-zero numerator"
    return float((num[~zero] / den[~zero]).max()) if (~zero).any() else 0.0


def _rows(n, rows):
    return np.arange(n) if rows is None else np.asarray(rows)


def _lower(rows, ncol):
    return np.arange(ncol)[None, :] <= rows[:, None]


def product_figure(c, a, b, rows=None, hp=np.longdouble, mask=None, minus_eye=False):
    """max |C - A B| / (|A| |B|) on `rows` (all when None); with minus_eye the numerator is |A B - I| and c is ignored."""
    r = _rows(a.shape[0], rows)
    prod = a[r].astype(hp) @ b.astype(hp)
    want = (np.eye(a.shape[0], b.shape[1])[r] if minus_eye else np.asarray(c)[r]).astype(hp)
    den = np.abs(a[r]).astype(np.float64) @ np.abs(b).astype(np.float64)
    return _ratio(np.abs(want - prod), den, mask)


def _lower_product_figure(c, a, b, rows, hp, minus_eye=False):
    """product_figure on the lower triangle when row i of A ends at column i (A lower triangular, or B = A^T and only j <= i is
    wanted): row i of the product needs the leading i + 1 columns of A and rows of B only, a third of the extended-precision work."""
    n = a.shape[0]
    if rows is None:                       # all rows: one product (float64 through the BLAS)
        return product_figure(c, a, b, None, hp, _lower(np.arange(n), n), minus_eye)
    r = np.asarray(rows)
    bh = b.astype(hp)
    num = np.zeros((len(r), n))
    for t, i in enumerate(r):
        want = np.zeros(i + 1, hp)
        if minus_eye:
            want[i] = 1
        else:
            want[:] = np.asarray(c)[i, :i + 1]
        num[t, :i + 1] = np.abs(want - a[i, :i + 1].astype(hp) @ bh[:i + 1, :i + 1])
    den = np.abs(a[r]).astype(np.float64) @ np.abs(b).astype(np.float64)
    return _ratio(num, den, _lower(r, n))


def factor_figure(a, l, rows=None, hp=np.longdouble):
    l = np.tril(l)
    return _lower_product_figure(a, l, l.T, rows, hp)


def inverse_figures(l, m, rows=None, hp=np.longdouble):
    """(left, right) = max |M L - I| / (|M| |L|), max |L M - I| / (|L| |M|) on the lower triangle."""
    l, m = np.tril(l), np.tril(m)
    return _lower_product_figure(None, m, l, rows, hp, True), _lower_product_figure(None, l, m, rows, hp, True)


def omega(a, x, y, hp=np.longdouble):
    """Oettli-Prager componentwise backward error of A x = y; the largest over the columns of a matrix right-hand side."""
    res = np.abs(y.astype(hp) - a.astype(hp) @ x.astype(hp))
    return _ratio(res, np.abs(a) @ np.abs(x).astype(np.float64) + np.abs(y))


def trisolve_figure(l, x, b, hp=np.longdouble):
    return omega(np.tril(l), x, b, hp)


def spd_inverse_figure(a, kinv, rows=None, hp=np.longdouble):
    """max |A Kinv - I| / (|A| |Kinv|) from the lower triangle of Kinv, mirrored."""
    k = np.tril(kinv) + np.tril(kinv, -1).T
    return product_figure(None, a, k, rows, hp, None, True)


def logdet_ref(diag):
    """(2 sum log d_i, sum |log d_i|) of a factor's diagonal, in np.longdouble."""
    logs = np.log(np.asarray(diag).astype(np.longdouble))
    return 2 * logs.sum(), float(np.abs(logs).sum())


def logdet_figure(got, diag):
    ref, den = logdet_ref(diag)
    return float(abs(np.longdouble(got) - ref) / den)


def nlml_figure(got, diag, y, alpha):
    """The value 1/2 y^T alpha + sum log d_i + n/2 log 2 pi against np.longdouble, relative to sum |log d_i| + |y^T alpha| / 2."""
    ld, den = logdet_ref(diag)
    ya = (np.asarray(y).astype(np.longdouble) * np.asarray(alpha).astype(np.longdouble)).sum()
    ref = ya / 2 + ld / 2 + np.longdouble(len(diag)) / 2 * np.log(2 * np.longdouble(np.pi))
    return float(abs(np.longdouble(got) - ref) / (den + abs(ya) / 2))


def logdet_bound(n):
    """The device sums n terms in double whatever the data's type (each log of an exactly converted entry, a few ulp), in some order:
    (n + 3) 2^-53 of the sum of magnitudes."""
    return (n + 3) * 2.0 ** -53


def product_bound(k, dtype):
    """(K + 3) u S componentwise for a sum of K products in any order (Higham, section 3.5), in units of S; the evaluation's own rounding
    (float64 for float32 data) rides on top as in tests/test_gemm_core_gpu.py."""
    return (k + 3) * U[dtype] + (k + 3) * (2.0 ** -53 if dtype == np.float32 else 2.0 ** -64)


def cap(n, dtype, kind):
    """The derived caps LAPACK meets (tests/test_backward_error_cpu.py): (n + 1) u for the factor (Higham, Thm 10.3) and for the inverse
    residuals, (3 n + 1) u for omega."""
    return ((3 * n + 1) if kind == "omega" else (n + 1)) * U[dtype]


# ---- LAPACK's figures on the same input --------------------------------------------------------------------------------------------
def _lp(name, dtype):
    return getattr(lapack, ("d" if dtype == np.float64 else "s") + name)


def lapack_factor(a, dtype):
    l, info = _lp("potrf", dtype)(a.astype(dtype), lower=1)
    assert info == 0
    return np.tril(l)


def lapack_inverse(l, dtype):
    m, info = _lp("trtri", dtype)(l.astype(dtype), lower=1)
    assert info == 0
    return np.tril(m)


def lapack_solve(l, y, dtype):
    x, info = _lp("potrs", dtype)(l.astype(dtype), y.astype(dtype), lower=1)
    assert info == 0
    return x


def lapack_trisolve(l, b, dtype):
    x, info = _lp("trtrs", dtype)(l.astype(dtype), b.astype(dtype), lower=1)
    assert info == 0
    return x


@functools.lru_cache(maxsize=None)
def lapack_parts(family, n, dtype=np.float64, seed=0):
    """(A, L, M, rows) with LAPACK's factor and its triangular inverse."""
    a = matrix(family, n, dtype, seed)
    l = lapack_factor(a, dtype)
    return a, l, lapack_inverse(l, dtype), sample_rows(n, seed)


def _sampled(dtype, rows):
    return rows if dtype == np.float64 else None


@functools.lru_cache(maxsize=None)
def lapack_omega(family, n, dtype=np.float64, seed=0, n_real=None):
    """omega of potrs on one right-hand side; with n_real the family's n_real x n_real matrix padded with the identity to n."""
    a = matrix(family, n, dtype, seed) if n_real is None else padded(family, n_real, n, dtype, seed)
    y = rhs(a, seed).astype(dtype)
    return omega(a, lapack_solve(lapack_factor(a, dtype), y, dtype), y, hp_of(dtype))


@functools.lru_cache(maxsize=None)
def lapack_figures(family, n, dtype=np.float64, seed=0):
    """LAPACK's own figures on (family, n, dtype): factor, left, right, omega (one right-hand side)."""
    a, l, m, rows = lapack_parts(family, n, dtype, seed)
    hp, r = hp_of(dtype), _sampled(dtype, rows)
    out = {"factor": factor_figure(a, l, r, hp)}
    out["left"], out["right"] = inverse_figures(l, m, r, hp)
    out["omega"] = lapack_omega(family, n, dtype, seed)
    return out


@functools.lru_cache(maxsize=None)
def lapack_mat_figures(family, n, nrhs, dtype=np.float64, seed=0):
    """(B, omega of potrs over the nrhs columns of B, residual of trtrs on them)."""
    a, l, _, _ = lapack_parts(family, n, dtype, seed)
    hp = hp_of(dtype)
    b = rhs(a, seed, nrhs).astype(dtype)
    b.setflags(write=False)
    return b, omega(a, lapack_solve(l, b, dtype), b, hp), trisolve_figure(l, lapack_trisolve(l, b, dtype), b, hp)


@functools.lru_cache(maxsize=None)
def padded(family, n_real, n, dtype=np.float64, seed=0):
    a = np.eye(n)
    a[:n_real, :n_real] = matrix(family, n_real, dtype, seed)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def lapack_potri_figure(family, n, dtype=np.float64, seed=0):
    a, l, _, rows = lapack_parts(family, n, dtype, seed)
    k, info = _lp("potri", dtype)(l.astype(dtype), lower=1)
    assert info == 0
    return spd_inverse_figure(a, k, _sampled(dtype, rows), hp_of(dtype))


# ---- the library's algorithm, restated -------------------------------------------------------------------------------------------------
def restated_factor(a, dtype=np.float64, hook=None, nbo=NBO):
    """pg_potrf as linalg.hip runs it: outer panels of `nbo` columns; inside a panel, per 128 columns, U (the block column minus the
    panel's earlier columns), the leaf (factor of the diagonal block AND its explicit inverse), T (the rows below times that inverse,
    transposed); then the trailing update by the whole panel.  Returns (L, inv) with inv [n / 128, 128, 128].  Every product runs in
    `dtype`.  hook(what, k, block) may change in place the leaf's factor ("leaf"), its inverse ("inv") or the solved panel ("panel") of
    block column k."""
    w = np.tril(a).astype(dtype)
    n = w.shape[0]
    inv = np.zeros((n // NB, NB, NB), dtype)
    for o0 in range(0, n, nbo):
        oend = min(n, o0 + nbo)
        for k0 in range(o0, oend, NB):
            k1, kb = k0 + NB, k0 // NB
            if k0 > o0:
                w[k0:, k0:k1] -= w[k0:, o0:k0] @ w[k0:k1, o0:k0].T
            lkk = lapack_factor(np.tril(w[k0:k1, k0:k1]) + np.tril(w[k0:k1, k0:k1], -1).T, dtype)
            if hook:
                hook("leaf", kb, lkk)
            inv[kb] = lapack_inverse(lkk, dtype)
            if hook:
                hook("inv", kb, inv[kb])
            w[k0:k1, k0:k1] = lkk
            if k1 < n:
                panel = w[k1:, k0:k1] @ inv[kb].T
                if hook:
                    hook("panel", kb, panel)
                w[k1:, k0:k1] = panel
        if oend < n:
            w[oend:, oend:] -= w[oend:, o0:oend] @ w[oend:, o0:oend].T
    return np.tril(w), inv


def doubling_levels(n, hmax=0):
    """The pairs pg_trtri_t forms, level by level: (r0, h, h2) = the diagonal block [r0, r0 + h) joined with [r0 + h, r0 + h + h2).  The
    diagonal is tiled by full blocks of h and one smaller remainder; an odd full block merges with the remainder, or becomes it."""
    out, h, rem = [], NB, 0
    while True:
        nfull = (n - rem) // h
        if nfull + (1 if rem else 0) <= 1 or (hmax and h >= hmax):
            return out
        level = [(2 * p * h, h, h) for p in range(nfull // 2)]
        if (nfull & 1) and rem:
            level.append(((nfull - 1) * h, h, rem))
        out.append(level)
        if nfull & 1:
            rem = h + rem if rem else h
        h *= 2


def restated_inverse(l, inv, dtype=np.float64, hook=None, hmax=0):
    """pg_trtri: the block inverses on the diagonal, then recursive doubling, X21 = -X22 (L21 X11).  hook("x21", (level, r0), block)."""
    n = l.shape[0]
    l = l.astype(dtype)
    m = np.zeros((n, n), dtype)
    for b in range(n // NB):
        m[b * NB:(b + 1) * NB, b * NB:(b + 1) * NB] = inv[b]
    for lev, pairs in enumerate(doubling_levels(n, hmax)):
        for r0, h, h2 in pairs:
            c, e = r0 + h, r0 + h + h2
            s = l[c:e, r0:c] @ m[r0:c, r0:c]
            x21 = -(m[c:e, c:e] @ s)
            if hook:
                hook("x21", (lev, r0), x21)
            m[c:e, r0:c] = x21
    return m


def restated_solve(l, inv, y, dtype=np.float64, hook=None):
    """pg_potrs_vec: below n = 2048 block substitution with the 128 x 128 inverses; from there on sweeps over 1024-wide blocks against
    their inverses (the doubling stopped at 1024).  The device keeps its partial sums in double for either dtype; here everything runs
    in `dtype`.  hook("fwd" | "bwd", block, vector)."""
    n = l.shape[0]
    l = l.astype(dtype)
    if n < 2 * HB:
        hb, blocks = NB, [inv[b] for b in range(n // NB)]
    else:
        hb, w = HB, restated_inverse(l, inv, dtype, hmax=HB)
        blocks = [w[o:min(n, o + HB), o:min(n, o + HB)] for o in range(0, n, HB)]
    w, z, x = y.astype(dtype).copy(), np.zeros(n, dtype), np.zeros(n, dtype)
    for b, blk in enumerate(blocks):
        o, e = b * hb, min(n, (b + 1) * hb)
        z[o:e] = blk @ w[o:e]
        if hook:
            hook("fwd", b, z[o:e])
        w[e:] -= l[e:, o:e] @ z[o:e]
    for b in range(len(blocks) - 1, -1, -1):
        o, e = b * hb, min(n, (b + 1) * hb)
        x[o:e] = blocks[b].T @ z[o:e]
        if hook:
            hook("bwd", b, x[o:e])
        z[:o] -= l[o:e, :o].T @ x[o:e]
    return x


def restated_solve_by_inverse(m, y, dtype=np.float64):
    """The alpha calls, pg_potrs and pg_potri's use: x = M^T (M y)."""
    m = np.tril(m).astype(dtype)
    return m.T @ (m @ y.astype(dtype))


@functools.lru_cache(maxsize=None)
def restated_parts(family, n, dtype=np.float64, seed=0):
    a = matrix(family, n, dtype, seed)
    l, inv = restated_factor(a, dtype)
    return a, l, inv, restated_inverse(l, inv, dtype), sample_rows(n, seed)


@functools.lru_cache(maxsize=None)
def restated_omega_inv(family, n, dtype=np.float64, seed=0, n_real=None, nrhs=None):
    """omega of x = M^T (M y) with the restatement's own M: one right-hand side (on the identity-padded matrix with n_real), or the
    nrhs columns of lapack_mat_figures."""
    if n_real is None:
        a, _, _, m, _ = restated_parts(family, n, dtype, seed)
    else:
        a = padded(family, n_real, n, dtype, seed)
        l, inv = restated_factor(a, dtype)
        m = restated_inverse(l, inv, dtype)
    y = rhs(a, seed).astype(dtype) if nrhs is None else lapack_mat_figures(family, n, nrhs, dtype, seed)[0]
    return omega(a, restated_solve_by_inverse(m, y, dtype), y, hp_of(dtype))


@functools.lru_cache(maxsize=None)
def restated_figures(family, n, dtype=np.float64, seed=0):
    """The restatement's figures in the metrics of lapack_figures: what the library's ALGORITHM gives in IEEE arithmetic."""
    a, l, inv, m, rows = restated_parts(family, n, dtype, seed)
    hp, r = hp_of(dtype), _sampled(dtype, rows)
    out = {"factor": factor_figure(a, l, r, hp)}
    out["left"], out["right"] = inverse_figures(l, m, r, hp)
    y = rhs(a, seed).astype(dtype)
    out["omega"] = omega(a, restated_solve(l, inv, y, dtype), y, hp)
    out["omega_inv"] = omega(a, restated_solve_by_inverse(m, y, dtype), y, hp)
    return out
