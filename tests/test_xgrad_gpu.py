"""GPU tier of the derivatives in the test points: pg_kernel_xgrad through the C ABI, Exact_GP.predict_grad and the autograd backward
of Exact_GP.predict / predict_var / predict_covar, against the torch restatement of tests/xgrad_ref.py (whose own derivatives the CPU
tier checks against finite differences).  The errors are printed (pytest -s) next to the bound they are held to."""
import numpy as np
import pytest
import torch

import pygpr_amd as pg
from pygpr_amd._lib import PG_MAX_COMP

import xgrad_ref as xr
from kind_tools import rel

pytestmark = pytest.mark.gpu

CLS = {"m12": pg.Matern12, "m32": pg.Matern32, "m52": pg.Matern52, "se": pg.Squared_exponential, "wn": pg.White_noise}
KINDS = ["se", "m52", "m32", "m12"]
F64 = torch.float64


@pytest.fixture(scope="module")
def ops():
    from pygpr_amd._ops import get_ops

    return get_ops()


def compose(parts):
    return pg.Compose([CLS[p]() for p in parts])


def check(name, a, ref, tol):      # (kind_tools.check with a name column of 48: the printed lines stay what they were)
    e = rel(a, ref)
    print("%-48s rel err %.2e (bound %.0e)" % (name, e, tol))
    assert e <= tol, (name, e)


def hp_for(parts, d, rng, noise=0.3):
    hp = []
    for p in parts:
        hp += [noise] if p == "wn" else [rng.uniform(0.8, 1.3)] + list(rng.uniform(0.5, 1.5, d) / np.sqrt(d))
    return torch.tensor(hp, dtype=F64)


def problem(parts, n, m, d, seed=0, shift=0.0):
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.random((n, d)) + shift)
    y = torch.from_numpy(np.sin(3.0 * (x.numpy() - shift)).sum(1) + 0.1 * rng.standard_normal(n))
    xp = torch.from_numpy(rng.random((m, d)) + shift)
    return x, y, xp, hp_for(parts, d, rng)


def model(parts, x, y, hp, dtype=F64):
    gp = pg.Exact_GP(x.to(dtype), y.to(dtype), compose(parts))
    gp.set_params(hp)
    return gp


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def _abi_case(ops, parts, d, m, n, dtype, seed, forms=("u", "b", "ub"), tol=None):
    from pygpr_amd.covar import spec_of

    rng = np.random.default_rng(seed)
    xq = torch.from_numpy(rng.random((m, d))).to(dtype)
    z = torch.from_numpy(rng.random((n, d))).to(dtype)
    u = torch.from_numpy(rng.standard_normal(n)).to(dtype)
    b = torch.from_numpy(rng.standard_normal((m, n))).to(dtype)
    hp = hp_for(parts, d, rng)
    ref_u, ref_b = xr.contraction(parts, hp, xq.double(), z.double(), u.double(), b.double())
    spec, _ = spec_of(compose(parts), d)
    cu = lambda t: t.to("cuda").contiguous()     # noqa: E731
    tol = tol or (1e-12 if dtype == F64 else 1e-4)
    for form in forms:
        for trans in ((False, True) if "b" in form else (False,)):
            # B with a leading dimension beyond its columns (padding that must never be read: NaN) -- or stored transposed
            if trans:
                bb = torch.full((n + 3, m + 5), float("nan"), dtype=dtype)
                bb[:n, :m] = b.t()
            else:
                bb = torch.full((m + 2, n + 7), float("nan"), dtype=dtype)
                bb[:m, :n] = b
            uu = torch.cat([u, torch.full((9,), float("nan"), dtype=dtype)])
            ou, ob = ops.kernel_xgrad(spec, cu(hp), cu(xq), cu(z), u=cu(uu) if "u" in form else None, b=cu(bb) if "b" in form else None,
                                      trans_b=trans)
            tag = "%s d=%d m=%d n=%d %s %s%s" % ("+".join(parts), d, m, n, str(dtype)[-7:], form, " trans" if trans else "")
            if "u" in form:
                check(tag + " u", ou, ref_u, tol)
            if "b" in form:
                check(tag + " B", ob, ref_b, tol)


@pytest.mark.parametrize("dtype", [F64, torch.float32])
@pytest.mark.parametrize("kind", KINDS)
def test_contraction_every_kind_and_width(ops, kind, dtype):
    for i, (d, m, n) in enumerate([(1, 1, 130), (3, 70, 300), (8, 129, 211), (16, 65, 257), (33, 3, 190)]):
        _abi_case(ops, [kind, "wn"], d, m, n, dtype, seed=10 * i, forms=("u", "b", "ub") if d in (3, 33) else ("ub",))


@pytest.mark.parametrize("dtype", [F64, torch.float32])
def test_contraction_compose_and_accumulate_pass(ops, dtype):
    _abi_case(ops, ["se", "m12", "wn"], 5, 77, 201, dtype, seed=3)
    long = ["se", "m52", "m32", "m12", "se", "wn"]          # five stationary children: a second, accumulating pass
    assert sum(p != "wn" for p in long) > PG_MAX_COMP
    _abi_case(ops, long, 4, 66, 150, dtype, seed=4, forms=("ub",))


def test_contraction_batched_experts_and_shared_operands(ops):
    from pygpr_amd.covar import spec_of

    rng = np.random.default_rng(8)
    ne, m, n, d = 3, 50, 140, 4
    parts = ["m52", "wn"]
    spec, _ = spec_of(compose(parts), d)
    hps = torch.stack([hp_for(parts, d, rng) for _ in range(ne)])
    xq = torch.from_numpy(rng.random((m, d)))                    # shared test points
    z = torch.from_numpy(rng.random((ne, n, d)))
    u = torch.from_numpy(rng.standard_normal((ne, n)))
    b = torch.from_numpy(rng.standard_normal((ne, m, n)))
    ou, ob = ops.kernel_xgrad_batched(spec, hps.cuda(), xq.cuda(), z.cuda(), u.cuda(), b.cuda())
    for e in range(ne):
        ru, rb = xr.contraction(parts, hps[e], xq, z[e], u[e], b[e])
        check("batched expert %d u" % e, ou[e], ru, 1e-12)
        check("batched expert %d B" % e, ob[e], rb, 1e-12)


# ---- predict_grad ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parts", [["se", "wn"], ["m52", "wn"], ["m32", "wn"], ["m12", "wn"], ["se", "m32", "wn"]])
def test_predict_grad_single(parts):
    x, y, xp, hp = problem(parts, 300, 45, 5, seed=1)
    gp = model(parts, x, y, hp)
    mean, var, dmean, dvar = gp.predict_grad(xp, var="diag")
    m0, v0 = gp.predict(xp, var="diag")
    assert torch.equal(mean, m0) and torch.equal(var, v0)
    assert dmean.shape == xp.shape and dvar.shape == xp.shape and dmean.device == xp.device
    _, _, rdm, rdv = xr.predict_grads(parts, hp, x, y, xp)
    check("predict_grad %s dmean" % "+".join(parts), dmean, rdm, 1e-9)
    check("predict_grad %s dvar" % "+".join(parts), dvar, rdv, 1e-9)
    mean1, dmean1 = gp.predict_grad(xp, var="none")
    assert torch.equal(mean1, m0) and torch.equal(dmean1, dmean)


def test_predict_grad_batched():
    parts = ["se", "wn"]
    nc, n, m, d = 3, 200, 33, 3
    rng = np.random.default_rng(2)
    x = torch.from_numpy(rng.random((nc, n, d)))
    y = torch.from_numpy(rng.standard_normal((nc, n)))
    xp = torch.from_numpy(rng.random((m, d)))
    hps = torch.stack([hp_for(parts, d, rng) for _ in range(nc)])
    gp = model(parts, x, y, hps)
    mean, var, dmean, dvar = gp.predict_grad(xp, var="diag")
    m0, v0 = gp.predict(xp, var="diag")
    assert torch.equal(mean, m0) and torch.equal(var, v0)
    assert dmean.shape == (nc, m, d)
    for c in range(nc):
        _, _, rdm, rdv = xr.predict_grads(parts, hps[c], x[c], y[c], xp)
        check("predict_grad batched expert %d dmean" % c, dmean[c], rdm, 1e-9)
        check("predict_grad batched expert %d dvar" % c, dvar[c], rdv, 1e-9)


# ---- autograd ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("var", ["none", "diag", "full"])
@pytest.mark.parametrize("parts", [["m52", "wn"], ["m12", "se", "wn"]])
def test_autograd_against_reference(parts, var):
    x, y, xp, hp = problem(parts, 260, 37, 4, seed=5)
    gp = model(parts, x, y, hp)
    rng = np.random.default_rng(6)
    g_mu = torch.from_numpy(rng.standard_normal(37))
    g_2 = torch.from_numpy(rng.standard_normal((37, 37) if var == "full" else 37))
    for device in ("cuda", "cpu"):
        xq = xp.to(device).requires_grad_(True)
        out = gp.predict(xq, var=var)
        loss = (g_mu.to(device) * out[0]).sum() + ((g_2.to(device) * out[1]).sum() if var != "none" else 0.0)
        loss.backward()
        assert xq.grad.device == xq.device and xq.grad.dtype == F64
        ref = xr.vjp(parts, hp, x, y, xp, var, g_mu, g_2)
        check("autograd %s %s xp on %s" % ("+".join(parts), var, device), xq.grad, ref, 1e-9)
        with torch.no_grad():
            plain = gp.predict(xp.to(device), var=var)
        assert torch.equal(out[0].detach(), plain[0])
        if var != "none":
            assert torch.equal(out[1].detach(), plain[1])


@pytest.mark.parametrize("var", ["none", "diag", "full"])
def test_gradcheck(var):
    parts = ["m32", "wn"]
    x, y, xp, hp = problem(parts, 40, 5, 3, seed=9)
    gp = model(parts, x, y, hp)
    xq = xp.cuda().requires_grad_(True)
    if var == "none":
        fn = lambda a: gp.predict(a, var="none")[0]     # noqa: E731
    else:
        fn = lambda a: tuple(gp.predict(a, var=var))     # noqa: E731
    assert torch.autograd.gradcheck(fn, (xq,), eps=1e-6, atol=1e-6, rtol=1e-5)
    assert torch.autograd.gradcheck(lambda a: gp.predict_var(a), (xq,), eps=1e-6, atol=1e-6, rtol=1e-5) if var == "diag" else True
    assert torch.autograd.gradcheck(lambda a: gp.predict_covar(a), (xq,), eps=1e-6, atol=1e-6, rtol=1e-5) if var == "full" else True


@pytest.mark.parametrize("shared", [True, False])
def test_autograd_batched(shared):
    parts = ["m52", "wn"]
    nc, n, m, d = 3, 180, 21, 3
    rng = np.random.default_rng(12)
    x = torch.from_numpy(rng.random((nc, n, d)))
    y = torch.from_numpy(rng.standard_normal((nc, n)))
    hps = torch.stack([hp_for(parts, d, rng) for _ in range(nc)])
    xp = torch.from_numpy(rng.random((m, d) if shared else (nc, m, d)))
    gp = model(parts, x, y, hps)
    g_mu = torch.from_numpy(rng.standard_normal((nc, m)))
    g_v = torch.from_numpy(rng.standard_normal((nc, m)))
    for var in ("diag", "full"):
        xq = xp.clone().requires_grad_(True)
        mu, v = gp.predict(xq, var=var)
        gv = g_v if var == "diag" else torch.from_numpy(rng.standard_normal((nc, m, m)))
        ((g_mu * mu).sum() + (gv * v).sum()).backward()
        ref = torch.zeros_like(xp)
        for c in range(nc):
            rc = xr.vjp(parts, hps[c], x[c], y[c], xp if shared else xp[c], var, g_mu[c], gv[c])
            if shared:
                ref = ref + rc
            else:
                ref[c] = rc
        check("autograd batched %s %s" % ("shared" if shared else "per-expert", var), xq.grad, ref, 1e-9)


# ---- fp32 models -------------------------------------------------------------------------------------------------------------------
def test_fp32_model():
    parts = ["m52", "wn"]
    x, y, xp, hp = problem(parts, 250, 30, 4, seed=13)
    gp = model(parts, x, y, hp, dtype=torch.float32)
    _, _, dmean, dvar = gp.predict_grad(xp.float(), var="diag")
    _, _, rdm, rdv = xr.predict_grads(parts, hp, x.float().double(), y.float().double(), xp.float().double())
    check("fp32 predict_grad dmean", dmean, rdm, 1e-5)
    check("fp32 predict_grad dvar", dvar, rdv, 1e-4)
    xq = xp.float().requires_grad_(True)
    mu, v = gp.predict(xq, var="diag")
    (mu.sum() + v.sum()).backward()
    assert xq.grad.dtype == torch.float32
    check("fp32 autograd diag", xq.grad, rdm + rdv, 1e-5)


# ---- numerics ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["m52", "m12"])
def test_offset_and_near_duplicate_points(kind):
    parts = [kind, "wn"]
    x, y, xp, hp = problem(parts, 220, 30, 3, seed=14, shift=1000.0)
    xp[:5] = x[:5] + 1e-9                        # near-duplicates of training points
    gp = model(parts, x, y, hp)
    _, _, dmean, dvar = gp.predict_grad(xp, var="diag")
    _, _, rdm, rdv = xr.predict_grads(parts, hp, x, y, xp)
    check("offset +1000 %s dmean" % kind, dmean, rdm, 1e-9)
    check("offset +1000 %s dvar" % kind, dvar, rdv, 1e-9)


@pytest.mark.parametrize("kind", KINDS)
def test_coincident_points(kind):
    parts = [kind, "wn"]
    x, y, xp, hp = problem(parts, 150, 12, 3, seed=15)
    xp[:4] = x[10:14]                             # exactly on training points
    gp = model(parts, x, y, hp)
    _, _, dmean, dvar = gp.predict_grad(xp, var="diag")
    assert torch.isfinite(dmean).all() and torch.isfinite(dvar).all()
    _, _, rdm, rdv = xr.predict_grads(parts, hp, x, y, xp)      # (Matern-1/2: the convention, applied explicitly there)
    check("coincident %s dmean" % kind, dmean, rdm, 1e-9)
    check("coincident %s dvar" % kind, dvar, rdv, 1e-9)


def test_nan_stays_in_its_row(ops):
    parts = ["m12", "wn"]
    x, y, xp, hp = problem(parts, 200, 20, 3, seed=16)
    xp[7, 1] = float("nan")
    gp = model(parts, x, y, hp)
    _, _, dmean, dvar = gp.predict_grad(xp, var="diag")
    for g in (dmean, dvar):
        assert torch.isnan(g[7]).all()
        assert torch.isfinite(torch.cat([g[:7], g[8:]])).all()


# ---- nothing changes without requires_grad; honest limits ------------------------------------------------------------------------
def test_no_requires_grad_no_change():
    parts = ["se", "wn"]
    x, y, xp, hp = problem(parts, 120, 10, 3, seed=17)
    gp = model(parts, x, y, hp)
    for var in ("none", "diag", "full"):
        out = gp.predict(xp, var=var)
        assert out[0].grad_fn is None and (var == "none" and out[1] is NotImplemented or out[1].grad_fn is None)
        xq = xp.clone().requires_grad_(True)
        out2 = gp.predict(xq, var=var)
        assert out2[0].grad_fn is not None
        assert torch.equal(out2[0].detach(), out[0])
    assert gp.predict_var(xp).grad_fn is None and gp.predict_covar(xp).grad_fn is None


def test_params_requiring_grad_raise():
    parts = ["se", "wn"]
    x, y, xp, hp = problem(parts, 120, 10, 3, seed=18)
    gp = model(parts, x, y, hp.clone().requires_grad_(True))
    xq = xp.clone().requires_grad_(True)
    mu, v = gp.predict(xq, var="diag")
    with pytest.raises(NotImplementedError, match="params"):
        (mu.sum() + v.sum()).backward()


def test_model_change_between_forward_and_backward_raises():
    parts = ["se", "wn"]
    x, y, xp, hp = problem(parts, 120, 10, 3, seed=19)
    gp = model(parts, x, y, hp)
    xq = xp.clone().requires_grad_(True)
    mu, v = gp.predict(xq, var="diag")
    gp.set_params(hp * 1.1)
    with pytest.raises(RuntimeError, match="changed"):
        (mu.sum() + v.sum()).backward()
    xq = xp.clone().requires_grad_(True)
    mu, _ = gp.predict(xq, var="none")
    gp.y = gp.y + 1.0
    with pytest.raises(RuntimeError, match="changed"):
        mu.sum().backward()


# ---- size --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["se", "m52"])
def test_size_n16384(kind):
    parts = [kind, "wn"]
    n, m, d = 16384, 512, 8
    x, y, xp, hp = problem(parts, n, m, d, seed=20)
    gp = model(parts, x, y, hp)
    mean, var, dmean, dvar = gp.predict_grad(xp, var="diag")
    rows = torch.from_numpy(np.random.default_rng(21).choice(m, 64, replace=False))
    cu = lambda t: t.to("cuda")     # noqa: E731   (the reference's Cholesky of 16384 points, on the GPU through torch)
    fac = xr.factor(parts, cu(hp), cu(x), cu(y))
    _, _, rdm, rdv = xr.predict_grads(parts, cu(hp), cu(x), cu(y), cu(xp[rows]), fac=fac)
    check("n=16384 %s dmean (64 rows)" % kind, dmean[rows], rdm, 1e-9)
    check("n=16384 %s dvar (64 rows)" % kind, dvar[rows], rdv, 1e-9)
