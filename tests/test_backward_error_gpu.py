"""The dense linear algebra held to LAPACK's backward error ("Backward error of the dense linear algebra"): pg_potrf on all
its routes, pg_trtri, pg_lauum, pg_potri, pg_potrs_vec, pg_potrs, pg_trsm_lower, pg_trmv, the alpha calls and pg_logdet, on the three
families of tests/linalg_ref.py (well conditioned, rows scaled over twelve orders of magnitude, a GP covariance of condition 1e6), in
both dtypes, in the componentwise metrics defined there.

Bounds.  Pure products: (K + 3) u of their componentwise scale, derived (tests/test_gemm_core_gpu.py).  Factor, inverse and solves:
BOTH the derived cap LAPACK meets ((n + 1) u, (3 n + 1) u for omega: tests/test_backward_error_cpu.py) AND R times LAPACK's own
figure on the same input (at least u), with R one power of two per metric and family: the smallest at or above four times the worst
device / LAPACK ratio measured on the MI355X over all cases of that metric and family (the table in DESIGN.md).  R is licensed by the
NumPy restatement of the library's algorithm on the CPU, which sits inside it (tests/test_backward_error_cpu.py), never by the device.

Shapes are the smallest that reach each route (linalg.hip): with the coupled chain armed the outer panels are 384 columns wide, so
n = 768 is two panels (no look-ahead below three) and n = 1280 is four, the last one ragged, all on the flag-coupled chain."""
import numpy as np
import pytest
import torch

import linalg_ref as lr
from kind_tools import dev, host, ops  # noqa: F401  (ops: the fixture)
from pygpr_amd._ops import _code

pytestmark = pytest.mark.gpu

# R[metric][family] against LAPACK's figure, and R_RESTATED[(metric, family)] against the restatement's where the rule would need more than
# 16 on a well-conditioned family: DESIGN.md ("Backward error of the dense linear algebra", the table of measured ratios).
# omega: pg_potrs_vec (substitution); omega_inv: the solves through the explicit inverse (pg_potrs, the alpha calls).
R = {
    "factor":    {"spd": 8, "scaled": 16, "gp": 128},
    "left":      {"spd": 16, "scaled": None, "gp": 64},          # scaled: the rule would need 32 (finding 1)
    "right":     {"spd": 16, "scaled": 16, "gp": 4},
    "omega":     {"spd": 16, "scaled": 16, "gp": 16},
    "omega_inv": {"spd": None, "scaled": None, "gp": 64},        # spd, scaled: the rule would need 32 (finding 2)
    "trisolve":  {"spd": 8, "scaled": 8, "gp": 8},
    "potri":     {"spd": 4, "scaled": 8, "gp": 64},
}
R_RESTATED = {("left", "scaled"): 8, ("omega_inv", "spd"): 8, ("omega_inv", "scaled"): 8}
CAP = {"factor": "factor", "left": "inverse", "right": "inverse", "omega": "omega", "omega_inv": "omega", "trisolve": "omega", "potri": None}
TD = {np.float64: torch.float64, np.float32: torch.float32}
DTYPES = [np.float64, np.float32]
both_dtypes = pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32"])
every_family = pytest.mark.parametrize("family", lr.FAMILIES)


@pytest.fixture(autouse=True)
def _extended_precision():
    if not lr.have_longdouble():
        pytest.skip("np.longdouble has fewer than 63 mantissa bits here: no higher precision to evaluate float64 residuals in")


def hold(label, metric, family, n, dtype, got, ref, net=None, restated=None):
    """Device figure against (a) the derived cap and (b) R x max(LAPACK's figure, u) -- or, for the pairs of R_RESTATED, that R x
    max(the restatement's figure, u), computed by `restated()`; `net`: the float64 evaluation of all rows."""
    u = lr.U[dtype]
    if (metric, family) in R_RESTATED:
        own = restated()
        bound, via = R_RESTATED[(metric, family)] * max(own, u), "  restatement %.3e" % own
    else:
        bound, via = R[metric][family] * max(ref, u), ""
    if CAP[metric]:
        bound = min(bound, lr.cap(n, dtype, CAP[metric]))
    print("BE %-34s %-9s %-6s %s n=%-4d device %.3e  lapack %.3e  ratio %6.2f  (bound %.3e)%s%s"
          % (label, metric, family, "f64" if dtype == np.float64 else "f32", n, got, ref, got / max(ref, u), bound, via,
             "" if net is None else "  all rows in float64 %.3e" % net))
    assert got <= bound, (label, metric, family, got, ref, bound)
    assert net is None or net <= lr.NET * bound, (label, metric, family, "net", net, bound)


def hold_product(label, family, n, dtype, got, k, stages=1):
    b = lr.product_bound(k, dtype)
    bound = b if stages == 1 else stages * b * (1 + b) ** (stages - 1)
    print("BE %-34s %-9s %-6s %s n=%-4d device %.3e  (derived bound %.3e)" % (label, "product", family, "f64" if dtype == np.float64 else "f32", n, got, bound))
    assert got <= bound, (label, family, got, bound)


def up(a, td):
    """A host array on the device, as `td` (a copy first: the cached inputs are read-only)."""
    return dev(np.array(a), td)


def rows_of(n, dtype):
    return lr.sample_rows(n) if dtype == np.float64 else None


def factor_figures(a, l, dtype):
    fig = lr.factor_figure(a, l, rows_of(a.shape[0], dtype), lr.hp_of(dtype))
    return fig, (lr.factor_figure(a, l, None, np.float64) if dtype == np.float64 else None)


def inverse_figures(l, m, dtype):
    left, right = lr.inverse_figures(l, m, rows_of(l.shape[0], dtype), lr.hp_of(dtype))
    net = lr.inverse_figures(l, m, None, np.float64) if dtype == np.float64 else (None, None)
    return left, right, net


def hold_factor_and_inverse(label, family, n, dtype, a, l, m=None):
    ref = lr.lapack_figures(family, n, dtype)
    fig, net = factor_figures(a, l, dtype)
    hold(label, "factor", family, n, dtype, fig, ref["factor"], net)
    if m is not None:
        left, right, nets = inverse_figures(l, m, dtype)
        hold(label, "left", family, n, dtype, left, ref["left"], nets[0], lambda: lr.restated_figures(family, n, dtype)["left"])
        hold(label, "right", family, n, dtype, right, ref["right"], nets[1])


def factorise(ops, a, dtype, inverse=False):
    n = a.shape[0]
    ad = up(a, TD[dtype])
    invd = ops.potrf_workspace(n, TD[dtype])
    info = ops.zeros(1, dtype=torch.int32)
    minv = ops.zeros(n, n, dtype=TD[dtype]) if inverse else None
    if inverse:
        ops.potrf_trtri(ad, invd, info, minv)
    else:
        ops.potrf(ad, invd, info)
    assert int(info.item()) == 0
    return ad, invd, minv


def composite_figure(x, m, b, hp):
    """max |X - M^T (M B)| / (|M^T| (|M| |B|)) over all entries: the two-stage products of the alpha calls and of pg_potrs."""
    m = np.tril(m)
    b2, x2 = (b[:, None], x[:, None]) if b.ndim == 1 else (b, x)
    mh = m.astype(hp)
    want = mh.T @ (mh @ b2.astype(hp))
    return lr._ratio(np.abs(x2.astype(hp) - want), np.abs(m).T @ (np.abs(m) @ np.abs(b2)))


# ---- pg_potrf, every route ---------------------------------------------------------------------------------------------------------
@both_dtypes
@every_family
@pytest.mark.parametrize("route,n", [("one stream", 768), ("look-ahead, coupled chain", 1280), ("look-ahead, classic chain", 1280)])
def test_potrf_routes(ops, route, n, family, dtype):
    a = lr.matrix(family, n, dtype)
    try:
        if "classic" in route:
            ops.set_coupled_chain(-1)
        ad, _, _ = factorise(ops, a, dtype)
        panels = ops.last_coupled_panels()
    finally:
        ops.set_coupled_chain(1)
    assert ops.coupled_chain() == 1
    assert (panels > 0) == ("coupled" in route), (route, panels)      # one stream: fewer than three panels, no look-ahead, no chain
    hold_factor_and_inverse("potrf, " + route, family, n, dtype, a, host(ad))


@both_dtypes
@every_family
@pytest.mark.parametrize("route,n", [("fused", 1280), ("recursive split", 1024)])
def test_potrf_trtri_routes(ops, route, n, family, dtype):
    a = lr.matrix(family, n, dtype)
    try:
        if route == "recursive split":
            ops.set_recursive_split(512)
        ad, _, minv = factorise(ops, a, dtype, inverse=True)
    finally:
        ops.set_recursive_split(16384)
    hold_factor_and_inverse("potrf_trtri, " + route, family, n, dtype, a, host(ad), host(minv))


@both_dtypes
def test_batched_experts_one_family_each(ops, dtype):
    """Three experts, one family each: an expert reading another's block shows as a residual of order one.  Factor and inverse per
    expert, then lauum_batched and alpha_batched on the result."""
    n, td = 768, TD[dtype]
    mats = [lr.matrix(f, n, dtype) for f in lr.FAMILIES]
    a_all = up(np.stack(mats), td)
    invd = ops.empty(3, ops.potrf_worksize(n, td), dtype=td)
    info = ops.zeros(3, dtype=torch.int32)
    minv = ops.zeros(3, n, n, dtype=td)
    ops.potrf_trtri_batched(a_all, invd, info, minv)
    assert info.tolist() == [0, 0, 0]
    kinv = ops.zeros(3, n, n, dtype=td)
    ops.lauum_batched(minv, kinv)
    ys = np.stack([lr.rhs(a).astype(dtype) for a in mats])
    u, alpha, work = ops.empty(3, n, dtype=td), ops.empty(3, n, dtype=td), ops.empty(3, (n // 256) * n, dtype=td)
    ops.alpha_batched(minv, dev(ys, td), u, alpha, work)
    la, lm, lk, lal = host(a_all), host(minv), host(kinv), host(alpha)
    hp = lr.hp_of(dtype)
    for e, family in enumerate(lr.FAMILIES):
        label = "batched expert %d" % e
        hold_factor_and_inverse(label, family, n, dtype, mats[e], la[e], lm[e])
        m = np.tril(lm[e])
        rows = rows_of(n, dtype)
        r = lr._rows(n, rows)
        hold_product(label + " lauum", family, n, dtype, lr.product_figure(lk[e], m.T, m, rows, hp, lr._lower(r, n)), n)
        hold_product(label + " alpha", family, n, dtype, composite_figure(lal[e], m, ys[e], hp), n, stages=2)
        hold(label + " alpha", "omega_inv", family, n, dtype, lr.omega(mats[e], lal[e], ys[e], hp), lr.lapack_omega(family, n, dtype),
             restated=lambda: lr.restated_omega_inv(family, n, dtype))


# ---- pg_trtri, pg_lauum, pg_potri -------------------------------------------------------------------------------------------------------
@both_dtypes
@every_family
@pytest.mark.parametrize("n", [768, 1280])
def test_trtri_alone(ops, n, family, dtype):
    """On the device's own factor and block inverses (pg_potrf, then pg_trtri); n = 1280 is ten blocks: five pairs, then two pairs and an
    odd block that becomes the remainder, one pair, and at the top the 1024 block joined with the 256 remainder."""
    assert [len(level) for level in lr.doubling_levels(1280)] == [5, 2, 1, 1] and lr.doubling_levels(1280)[-1] == [(0, 1024, 256)]
    a = lr.matrix(family, n, dtype)
    ad, invd, _ = factorise(ops, a, dtype)
    minv = ops.zeros(n, n, dtype=TD[dtype])
    ops.trtri(ad, invd, minv)
    ref = lr.lapack_figures(family, n, dtype)
    left, right, nets = inverse_figures(host(ad), host(minv), dtype)
    hold("trtri", "left", family, n, dtype, left, ref["left"], nets[0], lambda: lr.restated_figures(family, n, dtype)["left"])
    hold("trtri", "right", family, n, dtype, right, ref["right"], nets[1])


@both_dtypes
@every_family
def test_lauum_and_potri(ops, family, dtype):
    """pg_lauum against the product of the operand it was given; pg_potri in place over the factor, A Kinv = I next to LAPACK potri's figure
    (no derived cap for that one: it grows with the condition number for LAPACK too)."""
    n, td, hp = 768, TD[dtype], lr.hp_of(dtype)
    a = lr.matrix(family, n, dtype)
    ad, invd, minv = factorise(ops, a, dtype, inverse=True)
    kinv = ops.zeros(n, n, dtype=td)
    ops.lauum(minv, kinv)
    m = np.tril(host(minv))
    rows = rows_of(n, dtype)
    hold_product("lauum", family, n, dtype, lr.product_figure(host(kinv), m.T, m, rows, hp, lr._lower(lr._rows(n, rows), n)), n)
    ops.potri(ad, invd, ad)
    hold("potri in place", "potri", family, n, dtype, lr.spd_inverse_figure(a, host(ad), rows, hp), lr.lapack_potri_figure(family, n, dtype))


# ---- solves ---------------------------------------------------------------------------------------------------------------------------
@both_dtypes
@every_family
@pytest.mark.parametrize("n", [1280, 2304])
def test_potrs_vec_both_regimes(ops, n, family, dtype):
    """Below 2 x 1024 rows one fused step per 128 columns; from there on sweeps over 1024-wide blocks (2304: two and a 256 remainder)."""
    assert (n < 2 * lr.HB) == (n == 1280) and ops.lib.pg_potrs_vec_worksize(_code(TD[dtype]), n) == (2 * n if n == 1280 else n * (lr.HB + 7))
    a = lr.matrix(family, n, dtype)
    y = lr.rhs(a).astype(dtype)
    ad, invd, _ = factorise(ops, a, dtype)
    yd, x = dev(y, TD[dtype]), ops.empty(n, dtype=TD[dtype])
    ops.potrs_vec(ad, invd, yd, x)
    assert torch.equal(yd, dev(y, TD[dtype]))                         # the right-hand side is untouched
    hold("potrs_vec", "omega", family, n, dtype, lr.omega(a, host(x), y, lr.hp_of(dtype)), lr.lapack_omega(family, n, dtype))


@both_dtypes
@every_family
@pytest.mark.parametrize("given", [True, False], ids=["Minv given", "Minv NULL"])
def test_potrs_and_trsm_lower(ops, given, family, dtype):
    n, nrhs, td, hp = 768, 128, TD[dtype], lr.hp_of(dtype)
    a = lr.matrix(family, n, dtype)
    b, ref_omega, ref_tri = lr.lapack_mat_figures(family, n, nrhs, dtype)
    ad, invd, minv = factorise(ops, a, dtype, inverse=True)
    bd = up(b, td)
    x = host(ops.potrs(ad, invd, bd, minv if given else None))
    v = host(ops.potrs(ad, invd, bd, minv if given else None, triangular_only=True))
    assert torch.equal(bd, up(b, td))
    tag = " (Minv given)" if given else " (Minv NULL)"
    hold("potrs" + tag, "omega_inv", family, n, dtype, lr.omega(a, x, b, hp), ref_omega, restated=lambda: lr.restated_omega_inv(family, n, dtype, nrhs=nrhs))
    hold("trsm_lower" + tag, "trisolve", family, n, dtype, lr.trisolve_figure(host(ad), v, b, hp), ref_tri)
    if given:
        m = np.tril(host(minv))
        hold_product("trsm_lower = Minv B", family, n, dtype, lr.product_figure(v, m, b, None, hp), n)
        hold_product("potrs = Minv^T (Minv B)", family, n, dtype, composite_figure(x, m, b, hp), n, stages=2)


@both_dtypes
@every_family
@pytest.mark.parametrize("trans", [0, 1])
def test_trmv(ops, trans, family, dtype):
    n, td, hp = 1280, TD[dtype], lr.hp_of(dtype)
    a = lr.matrix(family, n, dtype)
    _, _, minv = factorise(ops, a, dtype, inverse=True)
    v = lr.rhs(a).astype(dtype)
    out = ops.empty(n, dtype=td)
    ops.trmv(minv, dev(v, td), out, trans, ops.empty((n // 256) * n, dtype=td))
    m = np.tril(host(minv))
    op = m.T if trans else m
    hold_product("trmv trans=%d" % trans, family, n, dtype, lr.product_figure(host(out)[:, None], op, v[:, None], None, hp), n)


@both_dtypes
@every_family
def test_alpha_nlml_async_on_a_padded_factor(ops, family, dtype):
    """1200 points padded to 1280 with the identity: alpha against A, alpha as the product it is, and the NLML value."""
    n, n_real, td, hp = 1280, 1200, TD[dtype], lr.hp_of(dtype)
    a = lr.padded(family, n_real, n, dtype)
    y = lr.rhs(a).astype(dtype)
    y[n_real:] = 0
    ad, _, minv = factorise(ops, a, dtype, inverse=True)
    u, alpha, work = ops.empty(n, dtype=td), ops.empty(n, dtype=td), ops.empty((n // 256) * n, dtype=td)
    out = ops.zeros(2)
    ops.alpha_nlml_async(ad, minv, dev(y, td), u, alpha, work, n_real, out)
    torch.cuda.synchronize()
    m, al = np.tril(host(minv)), host(alpha)
    assert not al[n_real:].any()
    hold_product("alpha = Minv^T (Minv y)", family, n, dtype, composite_figure(al, m, y, hp), n, stages=2)
    hold("alpha_nlml_async", "omega_inv", family, n, dtype, lr.omega(a, al, y, hp), lr.lapack_omega(family, n, dtype, n_real=n_real),
         restated=lambda: lr.restated_omega_inv(family, n, dtype, n_real=n_real))
    fig = lr.nlml_figure(float(out[0]), 1.0 / np.diag(m)[:n_real].astype(np.longdouble), y[:n_real], al[:n_real])
    print("BE %-34s %-9s %-6s %s device %.3e  (derived bound %.3e)" % ("alpha_nlml_async value", "nlml", family, dtype.__name__, fig, lr.logdet_bound(n_real)))
    assert fig <= lr.logdet_bound(n_real)


@both_dtypes
@every_family
@pytest.mark.parametrize("rows", [500, 768])
def test_logdet(ops, rows, family, dtype):
    n = 768
    ad, _, _ = factorise(ops, lr.matrix(family, n, dtype), dtype)
    out = ops.zeros(1)
    ops.logdet(ad, rows, out)
    fig = lr.logdet_figure(float(out[0]), np.diag(host(ad))[:rows])
    print("BE %-34s %-9s %-6s %s device %.3e  (derived bound %.3e)"
          % ("logdet over %d rows" % rows, "logdet", family, dtype.__name__, fig, lr.logdet_bound(rows)))
    assert fig <= lr.logdet_bound(rows)
