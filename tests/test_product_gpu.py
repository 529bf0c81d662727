"""GPU tier of Product: a product spec (PG_SPEC_PRODUCT in pg_covspec.ncomp) through every covariance path -- the C ABI entry points,
the multi-pass plans of a Compose that holds products, and the model layer -- against the restatement of tests/kernel_ref.py.

Shapes: n = 130 (d = 1, 8) or 330 (d = 3, 17: six 64-tiles, a second strip of the gradient's four-tile strips, a ragged edge) against m = 70;
d = 17 is past the d <= 16 boundary of the DMAX instantiations.  Data in [-3, 3]^d, sigmas in [0.7, 1.3].  Allowances are the project's own
for these entry points (tests/test_periodic_gpu.py, tests/test_xgrad_gpu.py, tests/test_framed_gpu.py): K 1e-13 and dK 1e-12 absolute,
pg_kernel_xgrad 1e-12 of the largest entry, NLML 1e-10 relative, its gradient 1e-8 of its largest entry, predictions 1e-10, batched against the
loop 1e-11; fp32: K 4e-6, dK 5e-6 max(1, |dK|), the gradient 3 x 3e-3, pg_kernel_xgrad 1e-4.  The element-wise allowances (K, dK, xgrad) are first
held against the restatement's OWN rounding error, kernel_ref in float64 against itself in long double: where a quarter of the allowance
does not cover it the allowance is four times that error, the rule of test_periodic_gpu.py::test_offset_data_against_long_double.  K and the
cross kernel are compared on the whole of the inputs.  The dK stack, the x*-contraction and the NLML gradient (the long-double dK stack
contracted with the float64 weights W = K^-1 - a a^T) are compared on the pairs among the first 64 points and 32 test points of the same
inputs, a subsample for cost: the long-double stack of 90 slabs at n = 330 takes seconds per case.  The NLML itself and the predictions are
not held against a long-double evaluation: that needs a long-double Cholesky, which NumPy / SciPy do not have; their allowances are the
project's, met with five to seven digits to spare.  Measured values: DESIGN.md 4.9c."""
import ctypes as C

import numpy as np
import pytest
import torch

import pygpr_amd as pg
from pygpr_amd import _lib

import kernel_ref as kr
import loo_ref
from kind_tools import N, T, builds, cov_of, dev, grad_inputs, host, one_spec, ops, rel, specs_of  # noqa: F401  (ops: the fixture)

pytestmark = pytest.mark.gpu

FACTORS = [("se", "per"), ("m52", "per"), ("se", "m32"), ("rq", "m12", "per"), ("se", "m32", "rq", "per")]
N_OF_D = {1: 130, 3: 330, 8: 130, 17: 330}
M = 70


def synth(n, d, seed, m=0):
    """Points in [-3, 3]^d, a smooth periodic signal with a drifting shape plus noise, and m test points."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-3.0, 3.0, (n, d))
    y = np.sin(2.0 * np.pi * x[:, 0] / 1.3) * np.exp(-0.05 * (x ** 2).sum(1)) + 0.5 * np.cos(x.sum(1)) + 0.1 * rng.standard_normal(n)
    return (x, y, rng.uniform(-3.0, 3.0, (m, d))) if m else (x, y)


def block(part, d, rng):
    """sigma in [0.7, 1.3]; periods 0.7 .. 2.5, every third one 7 (longer than the data's extent)."""
    if part == "wn":
        return np.array([0.1])
    p = rng.uniform(0.7, 2.5, d)
    p[2::3] = 7.0
    tail = p if part == "per" else ([0.8] if part == "rq" else [])
    return np.concatenate([[rng.uniform(0.7, 1.3)], (0.5 + rng.random(d)) / np.sqrt(d), tail])


def hp_of(model, d, rng):
    return np.concatenate([block(p, d, rng) for p in kr.flat(model)])


def allowance(tol, ref64, ref_ld, scale=1.0):
    """The allowance of an element-wise check: `tol` (times `scale`) unless the restatement's own float64 error on these inputs, measured
    against its long-double evaluation, is more than a quarter of it -- then four times that error."""
    err = float(np.abs(ref64 - ref_ld).max())
    return max(tol * scale, 4.0 * err), err


# --------------------------------------------------------------------------- 1-3. entry points, symmetry, diagonal, routing
@pytest.mark.parametrize("d", [1, 3, 8, 17])
@pytest.mark.parametrize("factors", FACTORS, ids="x".join)
def test_entry_points_against_the_restatement(ops, monkeypatch, factors, d):
    """pg_kernel_build (mirrored, lower-only, cross, accumulate onto a non-zero matrix), _batched, pg_kernel_grad_build, pg_nlml_grad and
    _batched, pg_kernel_xgrad (trans_b 0 / 1), fp64 and fp32, on ONE product spec with its noise.  K is bit-for-bit symmetric and its
    diagonal exactly prod sigma^2 + (jitter + sigma_n^2).  Routing, pinned by result: a product never takes the matrix pipe or the PRESC /
    FAST bodies, so PG_KB_MFMA = 2 / 0 and PG_GRAD_MFMA = 1 / 0 give the same BITS.
    fp32: the sets of two factors at every d and entry point, at the existing absolute allowances.  Those were set for one kind with
    sigma^2 <= 1.44 (K: 4e-6, i.e. 2.8e-6 of the kind's largest value); a product of four factors with these sigmas reaches 1.3^8 = 8.2, where
    4e-6 is four fp32 ulps (measured on [se, m32, rq, per] at d = 1: 4.5e-6 at a value of 3.2).  The builds of the three- and four-factor sets
    are therefore checked in fp32 against a RELATIVE bound: the relative errors of F factors add to first order, so F x 2.8e-6 of max|K|."""
    from pygpr_amd._ops import pad_to

    n, m = N_OF_D[d], M
    rng = np.random.default_rng(100 * d + len(factors) + 7 * FACTORS.index(factors))
    x, y, xp = synth(n, d, seed=d, m=m)
    model = [factors, "wn"]
    hp = hp_of(model, d, rng)
    spec, npad, mpad = one_spec(model, d, product=True), pad_to(n), pad_to(m)
    assert spec.ncomp == len(factors) | 0x100
    ref = kr.kernel(model, hp, x) + 1e-7 * np.eye(n)
    ref_x = kr.kernel(model, hp, x, xp)
    sub, subq = slice(0, 64), slice(0, 32)                       # the pairs of the long-double yardstick
    tol_k, err_k = allowance(1e-13, ref, kr.kernel(model, hp, x, dtype=np.longdouble) + np.longdouble(1e-7) * np.eye(n))
    tol_x, err_x = allowance(1e-13, ref_x, kr.kernel(model, hp, x, xp, dtype=np.longdouble))
    tol_k = max(tol_k, tol_x)
    sig = [hp[o] for o in spec.off[: len(factors)]]
    f32 = len(factors) == 2

    def dtypes(tol64, tol32):
        return ((torch.float64, tol64), (torch.float32, tol32)) if f32 else ((torch.float64, tol64),)

    tol_k32 = 4e-6 if f32 else len(factors) * (4e-6 / 1.44) * np.abs(ref).max()
    for dtype, tol in ((torch.float64, tol_k), (torch.float32, tol_k32)):
        out = {}
        for mode in ("2", "0"):
            monkeypatch.setenv("PG_KB_MFMA", mode)
            out[mode] = builds(ops, spec, hp, x, xp, dtype)
        monkeypatch.delenv("PG_KB_MFMA")
        full, low, cross = out["2"]
        print("%s d=%d %s: K err %.2e, cross err %.2e (bound %.1e; restatement's own %.1e / %.1e)" % (
            "x".join(factors), d, dtype, np.abs(full[:n, :n] - ref).max(), np.abs(cross[:m, :n] - ref_x).max(), tol, err_k, err_x))
        for a, b in zip(out["2"], out["0"]):
            assert np.array_equal(a, b)                                               # the PROD body either way
        np.testing.assert_allclose(full[:n, :n], ref, atol=tol, rtol=0)
        np.testing.assert_allclose(cross[:m, :n], ref_x, atol=tol, rtol=0)
        assert np.array_equal(full[:n, :n], full[:n, :n].T)                           # exactly symmetric
        pad_ref = np.eye(npad)
        pad_ref[:n, :n] = full[:n, :n]
        assert np.array_equal(full, pad_ref)                                          # identity padding
        assert not cross[m:, :].any() and not cross[:, n:].any()                      # zero padding of a cross build
        tl = np.tril_indices(npad)
        assert np.array_equal(low[tl], full[tl])                                      # lower-only == mirrored on the lower triangle
        ft = np.float64 if dtype == torch.float64 else np.float32
        dgv = ft(sig[0] * sig[0])
        for s in sig[1:]:
            dgv = ft(dgv * ft(s * s))
        dgv = np.float64(ft(dgv + ft(1e-7 + hp[-1] * hp[-1])))
        assert (np.diag(full)[:n] == dgv).all()                                       # exactly prod sigma^2 + (jitter + sigma_n^2)
        # accumulate: the product is ADDED to what is there (symmetric: real rows and columns only; cross)
        hpd, xd, xpd = dev(hp), dev(x, dtype), dev(xp, dtype)
        base_s, base_c = rng.standard_normal((npad, npad)), rng.standard_normal((mpad, npad))
        acc_s, acc_c = dev(base_s, dtype), dev(base_c, dtype)
        code = _lib.PG_F64 if dtype == torch.float64 else _lib.PG_F32
        ops._call("pg_kernel_build", code, C.byref(spec), hpd.data_ptr(), xd.data_ptr(), d, n, None, 0, n, d, 0, 1, 0.0, acc_s.data_ptr(), npad, npad,
                  npad, ops._st())
        ops._call("pg_kernel_build", code, C.byref(spec), hpd.data_ptr(), xpd.data_ptr(), d, m, xd.data_ptr(), d, n, d, 0, 1, 0.0, acc_c.data_ptr(), npad,
                  mpad, npad, ops._st())
        want_s, want_c = host(dev(base_s, dtype)), host(dev(base_c, dtype))
        want_s[:n, :n] += ref - 1e-7 * np.eye(n)
        want_c[:m, :n] += ref_x
        np.testing.assert_allclose(host(acc_s), want_s, atol=tol + 8 * np.finfo(ft).eps, rtol=0)     # (+ the addition's rounding on |base| <= ~5)
        np.testing.assert_allclose(host(acc_c), want_c, atol=tol + 8 * np.finfo(ft).eps, rtol=0)
        # batched: three experts (their own points and hyper-parameters) equal their single builds bit for bit
        xs = np.stack([x, x[::-1], 0.5 * x])
        hps = np.stack([hp, hp * 1.01, hp * 0.99])
        outb = ops.empty(3, npad, npad, dtype=dtype)
        ops.kernel_build_batched(spec, dev(hps), dev(xs, dtype), None, outb, jitter=1e-7)
        for e in range(3):
            one = ops.empty(npad, npad, dtype=dtype)
            ops.kernel_build(spec, dev(hps[e]), dev(xs[e], dtype), None, one, jitter=1e-7)
            assert torch.equal(outb[e], one)
    # ---- the dK stack
    dk_ref = kr.kernel_and_grad(model, hp, x)[1]
    tol_dk, err_dk = allowance(1e-12, kr.kernel_and_grad(model, hp, x[sub])[1], kr.kernel_and_grad(model, hp, x[sub], dtype=np.longdouble)[1])
    for dtype, tol in dtypes(tol_dk, 5e-6 * max(1.0, np.abs(dk_ref).max())):
        dk = ops.kernel_grad_build(spec, dev(hp), dev(x, dtype), ops.empty(hp.size, n, n, dtype=dtype))
        print("%s d=%d %s: dK err %.2e (bound %.1e; restatement's own %.1e)" % ("x".join(factors), d, dtype, np.abs(host(dk) - dk_ref).max(), tol, err_dk))
        np.testing.assert_allclose(host(dk), dk_ref, rtol=0, atol=tol)
    # ---- the fused gradient, single and batched
    _, grad_ref = kr.nlml_and_grad(model, hp, x, y)
    scale = np.abs(grad_ref).max()
    # (the restatement's own error: its float64 and long-double dK stacks on the yardstick's pairs, each contracted with the float64 weights)
    kinv_ref = np.linalg.inv(ref)
    a_ref = kinv_ref @ y
    w_sub = (kinv_ref - np.outer(a_ref, a_ref))[sub, sub]
    g_64 = 0.5 * np.einsum("ij,pij->p", w_sub, kr.kernel_and_grad(model, hp, x[sub])[1])
    g_ld = 0.5 * np.einsum("ij,pij->p", w_sub.astype(np.longdouble), kr.kernel_and_grad(model, hp, x[sub], dtype=np.longdouble)[1])
    err_g = float(np.abs(g_64 - g_ld).max() / np.abs(g_64).max())
    print("%s d=%d: the restatement's own gradient error / max %.1e" % ("x".join(factors), d, err_g))
    for dtype, tol in dtypes(max(1e-8, 4 * err_g), 3 * 3e-3):
        hpd, xd, kinv, alpha_v = grad_inputs(ops, spec, hp, x, y, dtype)
        work = ops.empty(ops.nlml_grad_worksize(n, hp.size))
        got = {}
        for mode in ("1", "0"):
            monkeypatch.setenv("PG_GRAD_MFMA", mode)
            g = ops.zeros(hp.size)
            ops.nlml_grad(spec, hpd, xd, n, kinv, alpha_v, g, work)
            got[mode] = host(g)
        monkeypatch.delenv("PG_GRAD_MFMA")
        print("%s d=%d %s: gradient err / max %.2e (bound %.0e)" % ("x".join(factors), d, dtype, np.abs(got["1"] - grad_ref).max() / scale, tol))
        assert np.array_equal(got["1"], got["0"])                                     # the VALU contraction either way
        np.testing.assert_allclose(got["1"], grad_ref, rtol=tol, atol=tol * scale)
        # two experts in one call: the same inputs twice, each equal to the single call bit for bit
        gb = ops.zeros(2, hp.size)
        ops.nlml_grad_batched(spec, hpd[None].repeat(2, 1), xd[None].repeat(2, 1, 1), n * d, n, kinv[None].repeat(2, 1, 1), alpha_v[None].repeat(2, 1), gb,
                              ops.empty(2 * ops.nlml_grad_worksize(n, hp.size)))
        assert np.array_equal(host(gb[0]), got["1"]) and np.array_equal(host(gb[1]), got["1"])
    # ---- derivatives in the test points
    dks = kr.kernel_xgrad(model, hp, x, xp)                                           # [d, m, n]
    u, b = rng.standard_normal(n), rng.standard_normal((m, n))
    ref_u, ref_b = np.einsum("kpi,i->pk", dks, u), np.einsum("kpi,pi->pk", dks, b)
    # (the restatement's own error in the contraction, on the yardstick's pairs: relative to the largest entry like the check itself)
    sub_64 = np.einsum("kpi,pi->pk", kr.kernel_xgrad(model, hp, x[sub], xp[subq]), b[subq, sub])
    sub_ld = np.einsum("kpi,pi->pk", kr.kernel_xgrad(model, hp, x[sub], xp[subq], dtype=np.longdouble), b[subq, sub].astype(np.longdouble))
    err_xg = float(np.abs(sub_64 - sub_ld).max() / np.abs(sub_64).max())
    for dtype, tol in dtypes(max(1e-12, 4 * err_xg), 1e-4):
        for trans_b in (False, True):
            bd = dev(b.T if trans_b else b, dtype)
            ou, ob = ops.kernel_xgrad(spec, dev(hp), dev(xp, dtype), dev(x, dtype), u=dev(u, dtype), b=bd, trans_b=trans_b)
            print("%s d=%d %s trans_b=%d: xgrad u %.2e, B %.2e (bound %.1e; restatement's own %.1e)" % (
                "x".join(factors), d, dtype, trans_b, rel(host(ou), ref_u), rel(host(ob), ref_b), tol, err_xg))
            assert rel(host(ou), ref_u) <= tol and rel(host(ob), ref_b) <= tol
        ou2, _ = ops.kernel_xgrad(spec, dev(hp), dev(xp, dtype), dev(x, dtype), u=dev(u, dtype), out_u=ou.clone(), accumulate=True)
        assert rel(host(ou2), 2.0 * ref_u) <= tol                                     # accumulate adds to what is there


# --------------------------------------------------------------------------- 4. identity
def test_product_of_two_squared_exponentials_is_one():
    """Product([SE(s1, l1), SE(s2, l2)]) = SE(s1 s2, sqrt(l1^2 + l2^2)); the gradients map by the chain rule."""
    rng = np.random.default_rng(4)
    n, d = 130, 3
    x = rng.uniform(-3.0, 3.0, (n, d))
    s1, s2, l1, l2 = 0.9, 1.2, (0.5 + rng.random(d)) / np.sqrt(d), (0.5 + rng.random(d)) / np.sqrt(d)
    lc = np.sqrt(l1 ** 2 + l2 ** 2)
    k, dk = pg.Product([pg.Squared_exponential(), pg.Squared_exponential()]).kernel_and_grad(T(np.concatenate([[s1], l1, [s2], l2])), T(x))
    k1, dk1 = pg.Squared_exponential().kernel_and_grad(T(np.concatenate([[s1 * s2], lc])), T(x))
    k, dk, k1, dk1 = N(k), N(dk), N(k1), N(dk1)
    print("SE x SE: K err %.2e, dK err %.2e" % (np.abs(k - k1).max(), max(np.abs(dk[0] - dk1[0] * s2).max(), np.abs(dk[1: d + 1] - dk1[1:] * (l1 / lc)[:, None, None]).max())))
    np.testing.assert_allclose(k, k1, rtol=0, atol=1e-13)
    np.testing.assert_allclose(dk[0], dk1[0] * s2, rtol=0, atol=1e-12)                 # d sigma / d sigma_1 = sigma_2
    np.testing.assert_allclose(dk[d + 1], dk1[0] * s1, rtol=0, atol=1e-12)
    np.testing.assert_allclose(dk[1: d + 1], dk1[1:] * (l1 / lc)[:, None, None], rtol=0, atol=1e-12)      # d l / d l_1 = l_1 / l
    np.testing.assert_allclose(dk[d + 2:], dk1[1:] * (l2 / lc)[:, None, None], rtol=0, atol=1e-12)


# --------------------------------------------------------------------------- 5. underflow
def test_underflowing_factor_gives_zero_not_nan(ops):
    """Two clusters 40 apart along the first coordinate with l_1 = 1: the squared exponential factor is exactly 0 between them (its
    exponent is below -1500), the periodic factor is not.  K and every dK entry there are 0 and finite, and the NLML gradient matches."""
    rng = np.random.default_rng(5)
    n, d = 130, 3
    x, y = synth(n, d, seed=5)
    x[65:, 0] += 40.0
    model = [("se", "per"), "wn"]
    hp = hp_of(model, d, rng)
    hp[1] = 1.0
    far = np.zeros((n, n), bool)
    far[:65, 65:] = far[65:, :65] = True
    k, dk = cov_of(model).kernel_and_grad(T(hp), T(x))
    k, dk = N(k), N(dk)
    k_ref, dk_ref = kr.kernel_and_grad(model, hp, x)
    assert not k_ref[far].any() and (kr.kernel([("per",)], hp[d + 1: 3 * d + 2], x)[far] > 0).all()
    assert np.isfinite(k).all() and np.isfinite(dk).all()
    assert not k[far].any() and not dk[:, far].any()
    np.testing.assert_allclose(k, k_ref, rtol=0, atol=1e-13)
    np.testing.assert_allclose(dk, dk_ref, rtol=0, atol=1e-12)
    gp = pg.Exact_GP(T(x), T(y), cov_of(model))
    gp.set_params(T(hp))
    loss, grad = pg.MLE(gp).loss_and_grad(hp.copy())
    loss_ref, grad_ref = kr.nlml_and_grad(model, hp, x, y)
    assert np.isfinite(grad).all()
    np.testing.assert_allclose(loss, loss_ref, rtol=1e-10)
    np.testing.assert_allclose(grad, grad_ref, rtol=1e-8, atol=1e-8 * np.abs(grad_ref).max())
    xp = x[:M] + 0.01
    _, _, dmean, dvar = gp.predict_grad(T(xp), var="diag")
    rdm, rdv = kr.predict_grads(model, hp, x, y, xp)
    assert np.isfinite(N(dmean)).all() and rel(N(dmean), rdm) <= 1e-9 and rel(N(dvar), rdv) <= 1e-9


# --------------------------------------------------------------------------- 6. NaN
def test_nan_coordinate_and_nan_period(ops):
    """A NaN coordinate and a NaN period give NaN where the restatement does and nowhere else; the padding stays the identity."""
    rng = np.random.default_rng(6)
    n, d = 70, 3
    x = rng.uniform(-3.0, 3.0, (n, d))
    xn = x.copy()
    xn[23, 1] = np.nan
    model = [("se", "per"), "wn"]
    hp = hp_of(model, d, rng)
    hp_nan = hp.copy()
    hp_nan[2 * d + 3] = np.nan                                   # a period
    spec = one_spec(model, d, product=True)
    pad = np.eye(128)[n:, :]
    with np.errstate(invalid="ignore"):
        for xx, hh in ((xn, hp), (x, hp_nan)):
            k_ref, dk_ref = kr.kernel_and_grad(model, hh, xx)
            assert np.isnan(k_ref).any() and (np.isfinite(k_ref).any() or hh is hp_nan)
            for dt in (torch.float64, torch.float32):
                k = ops.empty(128, 128, dtype=dt)
                ops.kernel_build(spec, dev(hh), dev(xx, dt), None, k, jitter=1e-7)
                got = host(k)
                assert np.array_equal(np.isnan(got[:n, :n]), np.isnan(k_ref))
                assert np.array_equal(got[n:, :], pad) and np.array_equal(got[:, n:], pad.T)
            dk = N(cov_of(model).kernel_and_grad(T(hh), T(xx))[1])
            assert np.array_equal(np.isnan(dk), np.isnan(dk_ref))
            ok = ~np.isnan(dk_ref)
            np.testing.assert_allclose(dk[ok], dk_ref[ok], rtol=0, atol=1e-12)


# --------------------------------------------------------------------------- 7. multi-pass
@pytest.mark.parametrize("model", [["se", ("m32", "per"), "wn"], [("se", "per"), ("rq", "m12"), "wn"]], ids=str)
def test_products_inside_a_longer_sum(model):
    """A plain child beside a product (two passes, the noise in the first) and two products (a noise pass and one pass each): kernel, cross
    kernel, dK, NLML + gradient and predict against the restatement."""
    rng = np.random.default_rng(7)
    n, m, d = 330, M, 3
    x, y, xp = synth(n, d, seed=7, m=m)
    hp = hp_of(model, d, rng)
    cov = cov_of(model)
    specs = specs_of(model, d)
    assert len(specs) == len([t for t in model if isinstance(t, tuple)]) + 1 and specs[0].nnoise == 1 and not specs[0].ncomp & 0x100
    assert all(sp.ncomp & 0x100 and sp.nnoise == 0 for sp in specs[1:])
    np.testing.assert_allclose(N(cov.kernel(T(hp), T(x))), kr.kernel(model, hp, x), rtol=0, atol=1e-13)
    np.testing.assert_allclose(N(cov.kernel(T(hp), T(x), T(xp))), kr.kernel(model, hp, x, xp), rtol=0, atol=1e-13)
    np.testing.assert_allclose(N(cov.kernel_and_grad(T(hp), T(x))[1]), kr.kernel_and_grad(model, hp, x)[1], rtol=0, atol=1e-12)
    gp = pg.Exact_GP(T(x), T(y), cov)
    gp.set_params(T(hp))
    loss, grad = pg.MLE(gp).loss_and_grad(hp.copy())
    loss_ref, grad_ref = kr.nlml_and_grad(model, hp, x, y)
    np.testing.assert_allclose(loss, loss_ref, rtol=1e-10)
    np.testing.assert_allclose(grad, grad_ref, rtol=1e-8, atol=1e-8 * np.abs(grad_ref).max())
    mu, var = gp.predict(T(xp), var="diag")
    mu_ref, var_ref = kr.predict(model, hp, x, y, xp)
    np.testing.assert_allclose(N(mu), mu_ref, rtol=0, atol=1e-10)
    np.testing.assert_allclose(N(var), var_ref, rtol=0, atol=1e-10)
    _, _, dmean, dvar = gp.predict_grad(T(xp), var="diag")
    rdm, rdv = kr.predict_grads(model, hp, x, y, xp)
    assert rel(N(dmean), rdm) <= 1e-9 and rel(N(dvar), rdv) <= 1e-9


# --------------------------------------------------------------------------- 8. the model layer on the locally periodic kernel
LP = [("se", "per"), "wn"]


@pytest.fixture(scope="module")
def lp():
    """Compose([Product([se, per]), wn]), n = 330, d = 3: data, hyper-parameters, a fitted model."""
    rng = np.random.default_rng(8)
    x, y, xp = synth(330, 3, seed=8, m=M)
    hp = hp_of(LP, 3, rng)
    hp[-1] = 0.3
    gp = pg.Exact_GP(T(x), T(y), cov_of(LP))
    gp.set_params(T(hp))
    gp.update()
    return {"x": x, "y": y, "xp": xp, "hp": hp, "gp": gp, "rng": rng}


def test_exact_gp_and_mle(lp):
    x, y, xp, hp, gp = (lp[k] for k in ("x", "y", "xp", "hp", "gp"))
    mu, var = gp.predict(T(xp), var="diag")
    mu_ref, var_ref = kr.predict(LP, hp, x, y, xp)
    np.testing.assert_allclose(N(mu), mu_ref, rtol=0, atol=1e-10)
    np.testing.assert_allclose(N(var), var_ref, rtol=0, atol=1e-10)
    mu_f, cov_f = gp.predict(T(xp), var="full")
    np.testing.assert_allclose(N(mu_f), mu_ref, rtol=0, atol=1e-10)
    np.testing.assert_allclose(N(cov_f), kr.predict(LP, hp, x, y, xp, var="full")[1], rtol=0, atol=1e-10)
    mle = pg.MLE(gp)
    loss_ref, grad_ref = kr.nlml_and_grad(LP, hp, x, y)
    np.testing.assert_allclose(mle.loss(hp.copy()), loss_ref, rtol=1e-10)
    np.testing.assert_allclose(mle.grad(hp.copy()), grad_ref, rtol=1e-8, atol=1e-8 * np.abs(grad_ref).max())
    loss, grad = pg.MLE(gp).loss_and_grad(hp.copy())
    np.testing.assert_allclose(loss, loss_ref, rtol=1e-10)
    np.testing.assert_allclose(grad, grad_ref, rtol=1e-8, atol=1e-8 * np.abs(grad_ref).max())


def test_predict_grad_and_autograd(lp):
    x, y, xp, hp, gp, rng = (lp[k] for k in ("x", "y", "xp", "hp", "gp", "rng"))
    mean, var, dmean, dvar = gp.predict_grad(T(xp), var="diag")
    rdm, rdv = kr.predict_grads(LP, hp, x, y, xp)
    assert rel(N(dmean), rdm) <= 1e-9 and rel(N(dvar), rdv) <= 1e-9
    g_mu = rng.standard_normal(M)
    for var_kind in ("none", "diag", "full"):
        g_2 = rng.standard_normal((M, M) if var_kind == "full" else M)
        xq = T(xp).to("cuda").requires_grad_(True)
        out = gp.predict(xq, var=var_kind)
        loss = (dev(g_mu) * out[0]).sum() + ((dev(g_2) * out[1]).sum() if var_kind != "none" else 0.0)
        loss.backward()
        assert rel(N(xq.grad), kr.predict_vjp(LP, hp, x, y, xp, var_kind, g_mu, g_2)) <= 1e-9, var_kind


def test_append_equals_fresh_fit(lp):
    """append of 10 points against a fresh fit: 1e-9 (ten times that on derivatives), tests/test_append_gpu.py::compare."""
    x, y, xp, hp = T(lp["x"]), T(lp["y"]), T(lp["xp"]), T(lp["hp"])
    gp = pg.Exact_GP(x[:320].clone(), y[:320].clone(), cov_of(LP))
    gp.set_params(hp)
    gp.update()
    gp.append(x[320:], y[320:])
    assert torch.equal(gp.x, x) and torch.equal(gp.y, y)
    ref = lp["gp"]
    for a, b, tol in zip(gp.predict(xp, var="diag") + [gp.predict(xp, var="full")[1]], ref.predict(xp, var="diag") + [ref.predict(xp, var="full")[1]],
                         (1e-9, 1e-9, 1e-9)):
        assert rel(N(a), N(b)) <= tol
    g, gr = gp.predict_grad(xp), ref.predict_grad(xp)
    assert rel(N(g[2]), N(gr[2])) <= 1e-8 and rel(N(g[3]), N(gr[3])) <= 1e-8
    la, ga = pg.MLE(gp).loss_and_grad(lp["hp"].copy())
    lr, grr = pg.MLE(ref).loss_and_grad(lp["hp"].copy())
    assert abs(la - lr) <= 1e-9 * abs(lr) and rel(ga, grr) <= 1e-8


def test_loo(lp):
    """loo_predict and LOO(model).loss_and_grad against loo_ref's closed forms (R&W 5.10 - 5.13) on kernel_ref's kernel and slabs."""
    x, y, hp, gp = (lp[k] for k in ("x", "y", "hp", "gp"))
    n = x.shape[0]
    kinv = np.linalg.inv(kr.kernel(LP, hp, x) + kr.JITTER * np.eye(n))
    kinv = 0.5 * (kinv + kinv.T)
    alpha, c = kinv @ y, np.diag(kinv).copy()
    mu, var = gp.loo_predict()
    np.testing.assert_allclose(N(mu), y - alpha / c, rtol=0, atol=1e-10)
    np.testing.assert_allclose(N(var), 1.0 / c, rtol=0, atol=1e-10)
    loss_ref = loo_ref.loss_from(y - alpha / c, 1.0 / c, y)
    g_ref = loo_ref.grad_from(LP, hp, x, kinv, alpha, c)
    loss, grad = pg.LOO(gp).loss_and_grad(hp.copy())
    np.testing.assert_allclose(loss, loss_ref, rtol=1e-10)
    np.testing.assert_allclose(grad, g_ref, rtol=1e-8, atol=1e-8 * np.abs(g_ref).max())


def test_sampler_mean_and_factor(lp):
    """Posterior: the sampler's mean is predict's, bit for bit, and its factor reproduces predict's full covariance plus the jitter to the
    Cholesky backward-error bound of tests/test_sample_gpu.py (1e-12 of the largest entry).  Prior: mean 0, the factor of K(xp, xp)."""
    x, y, xp, hp, gp = (lp[k] for k in ("x", "y", "xp", "hp", "gp"))
    smp = gp.sampler(T(xp), noise=True, jitter=1e-7)
    pm, pc = gp.predict(T(xp), var="full")
    assert torch.equal(smp.mean, pm)
    L, c = smp.chol.double().numpy(), N(pc)
    assert np.abs(L @ L.T - (c + 1e-7 * np.eye(M))).max() / np.abs(c).max() <= 1e-12
    np.testing.assert_allclose(c, kr.predict(LP, hp, x, y, xp, var="full")[1], rtol=0, atol=1e-10)
    prior = gp.sampler(T(xp), noise=False, jitter=1e-7, prior=True)
    assert not prior.mean.any()
    L = prior.chol.double().numpy()
    kpp = kr.kernel(LP[:1], hp[:-1], xp) + 1e-7 * np.eye(M)      # noise=False: the latent function
    assert np.abs(L @ L.T - kpp).max() / np.abs(kpp).max() <= 1e-12


def test_batched_experts_match_their_loop():
    """3 x 330, d = 3 (a second strip of the batched contraction's four-tile strips): predictions, NLML and its gradient, predict_grad --
    each expert against its own single model and the restatement."""
    rng = np.random.default_rng(22)
    nc, n, m, d = 3, 330, 33, 3
    x = rng.uniform(-3.0, 3.0, (nc, n, d))
    y = np.sin(2.0 * np.pi * x[..., 0] / 1.3) + 0.1 * rng.standard_normal((nc, n))
    xp = rng.uniform(-3.0, 3.0, (nc, m, d))
    hp = np.stack([hp_of(LP, d, rng) for _ in range(nc)])
    gp = pg.Exact_GP(T(x), T(y), cov_of(LP))
    gp.set_params(T(hp))
    mu, var = gp.predict(T(xp), var="diag")
    _, _, dmean, dvar = gp.predict_grad(T(xp), var="diag")
    loss, grad = pg.MLE(pg.Exact_GP(T(x), T(y), cov_of(LP))).loss_and_grad(hp.copy())
    assert grad.shape == (nc, 3 * d + 3) and dmean.shape == (nc, m, d)
    for c in range(nc):
        one = pg.Exact_GP(T(x[c]), T(y[c]), cov_of(LP))
        one.set_params(T(hp[c]))
        mu1, var1 = one.predict(T(xp[c]), var="diag")
        np.testing.assert_allclose(N(mu[c]), N(mu1), rtol=0, atol=1e-11)
        np.testing.assert_allclose(N(var[c]).ravel(), N(var1).ravel(), rtol=0, atol=1e-11)
        l1, g1 = pg.MLE(one).loss_and_grad(hp[c].copy())
        np.testing.assert_allclose(loss[c], l1, rtol=1e-11)
        np.testing.assert_allclose(grad[c], g1, rtol=1e-9, atol=1e-9 * np.abs(g1).max())
        l_ref, g_ref = kr.nlml_and_grad(LP, hp[c], x[c], y[c])
        np.testing.assert_allclose(l1, l_ref, rtol=1e-10)
        np.testing.assert_allclose(g1, g_ref, rtol=1e-8, atol=1e-8 * np.abs(g_ref).max())
        mu_ref, var_ref = kr.predict(LP, hp[c], x[c], y[c], xp[c])
        np.testing.assert_allclose(N(mu1), mu_ref, rtol=0, atol=1e-10)
        np.testing.assert_allclose(N(var1).ravel(), var_ref, rtol=0, atol=1e-10)      # the device forms prod sigma^2 for the batch
        rdm, rdv = kr.predict_grads(LP, hp[c], x[c], y[c], xp[c])
        assert rel(N(dmean[c]), rdm) <= 1e-9 and rel(N(dvar[c]), rdv) <= 1e-9


def test_grbcm():
    """3 x 120 + 40.  Bounds: tests/test_periodic_gpu.py::test_grbcm."""
    rng = np.random.default_rng(33)
    nc, nsc, ng, m, d = 3, 120, 40, 25, 3
    xl, xg, xs = rng.uniform(-3, 3, (nc, nsc, d)), rng.uniform(-3, 3, (ng, d)), rng.uniform(-3, 3, (m, d))
    yl, yg = np.sin(2.0 * np.pi * xl[..., 0] / 1.3), np.sin(2.0 * np.pi * xg[..., 0] / 1.3)
    hp_g = hp_of(LP, d, rng)
    hp_l = np.stack([hp_of(LP, d, rng) for _ in range(nc)])
    model = pg.GRBCM(T(xl), T(yl), T(xg), T(yg), cov_of(LP))
    model.gpg.set_params(T(hp_g))
    model.gpl.set_params(T(hp_l))
    mu, var = model.predict(T(xs), var="diag")
    mu_ref, var_ref = kr.grbcm_predict(LP, hp_g, hp_l, xl, yl, xg, yg, xs)
    np.testing.assert_allclose(N(mu), mu_ref, rtol=0, atol=1e-9)
    np.testing.assert_allclose(N(var).ravel(), var_ref, rtol=1e-9, atol=1e-11)


def test_sk_wrap(lp):
    x, y, xp, hp = (lp[k] for k in ("x", "y", "xp", "hp"))
    gp = pg.Exact_GP(T(x[:10]), T(y[:10]), cov_of(LP))
    gp.set_params(T(hp))
    sk = pg.SK_WRAP(gp).fit(T(x), T(y))
    np.testing.assert_allclose(N(sk.predict(T(xp))), kr.predict(LP, hp, x, y, xp)[0], rtol=0, atol=1e-10)


# --------------------------------------------------------------------------- 9. refusals
def test_refusals_through_the_c_abi(ops):
    """A flagged count of 0 or 5 and a flagged spec with PG_KIND_SQDIST come back -1 with a message; nothing is launched (the output keeps
    its contents)."""
    from pygpr_amd._ops import make_spec

    d = 2
    x = dev(np.random.default_rng(1).random((10, d)))
    hp = dev(np.ones(16))
    bad0, bad5, badsq = make_spec([], [], [3]), make_spec([0, 0, 0, 0], [0, 3, 6, 9], []), make_spec([0, _lib.PG_KIND_SQDIST], [0, 3], [], product=True)
    bad0.ncomp = _lib.PG_SPEC_PRODUCT
    bad5.ncomp = _lib.PG_SPEC_PRODUCT | 5
    for sp, text in ((bad0, "product spec needs 1..4 factors, got 0"), (bad5, "product spec needs 1..4 factors, got 5"), (badsq, "unknown kernel kind 2")):
        out, dk = ops.zeros(64, 64), ops.zeros(16, 10, 10)
        with pytest.raises(RuntimeError, match=r"rc=-1\): pg_kernel_build: .*" + text):
            ops.kernel_build(sp, hp, x, None, out)
        with pytest.raises(RuntimeError, match=r"rc=-1\): pg_kernel_grad_build: .*" + text):
            ops.kernel_grad_build(sp, hp, x, dk)
        with pytest.raises(RuntimeError, match=r"rc=-1\): pg_kernel_xgrad: .*" + text):
            ops.kernel_xgrad(sp, hp, x, x, u=dev(np.ones(10)))
        with pytest.raises(RuntimeError, match=r"rc=-1\): pg_nlml_grad: .*" + text):
            ops.nlml_grad(sp, hp, x, 10, ops.zeros(64, 64), ops.zeros(64), ops.zeros(16), ops.empty(ops.nlml_grad_worksize(10, 16)))
        torch.cuda.synchronize()
        assert not out.any() and not dk.any()
    # an unflagged spec is checked as it always was, and the unassigned kinds stay unknown inside a product
    with pytest.raises(RuntimeError, match="bad covariance spec"):
        sp = make_spec([0], [0], [])
        sp.ncomp = 5
        ops.kernel_build(sp, hp, x, None, ops.zeros(64, 64))
    for kind in (5, 7):
        with pytest.raises(RuntimeError, match="unknown kernel kind %d" % kind):
            ops.kernel_build(make_spec([0, kind], [0, 3], [], product=True), hp, x, None, ops.zeros(64, 64))
