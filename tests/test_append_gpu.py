"""GPU tier of conditioning on new points: pg_chol_append through the C ABI against the padded NumPy restatement (tests/append_ref.py,
itself checked against numpy.linalg on the CPU), and Exact_GP.append against a fresh fit on the concatenated data.  The errors are
printed (pytest -s) next to the bound they are held to."""
import numpy as np
import pytest
import torch

import pygpr_amd as pg
from pygpr_amd._ops import JITTER

import append_ref as ar
from kind_tools import check

pytestmark = pytest.mark.gpu

CLS = {"m12": pg.Matern12, "m32": pg.Matern32, "m52": pg.Matern52, "se": pg.Squared_exponential, "wn": pg.White_noise}
F64, F32 = torch.float64, torch.float32
# fp32: both sides are fp32 fits whose errors are about eps32 x cond(K + sigma_n^2 I) <= 1e-7 x 1e4 here (sigma_n = 0.3, n ~ 1000);
# measured on an MI355X: 4e-6 (mean), 9e-7 (variance), 6e-6 (krnchd)
TOL32 = 1e-3
TOL64 = 1e-9


@pytest.fixture(scope="module")
def ops():
    from pygpr_amd._ops import get_ops

    return get_ops()


def hp_for(parts, d, rng, noise=0.3):
    hp = []
    for p in parts:
        hp += [noise] if p == "wn" else [rng.uniform(0.8, 1.3)] + list(rng.uniform(0.5, 1.5, d) / np.sqrt(d))
    return torch.tensor(hp, dtype=F64)


def data(n, d, seed=0):
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.random((n, d)))
    y = torch.from_numpy(np.sin(3.0 * x.numpy()).sum(1) + 0.1 * rng.standard_normal(n))
    return x, y, rng


def model(parts, x, y, hp, dtype=F64):
    gp = pg.Exact_GP(x.to(dtype), y.to(dtype), pg.Compose([CLS[p]() for p in parts]))
    gp.set_params(hp)
    return gp


def fresh(gp, parts):
    return model(parts, gp.x.clone(), gp.y.clone(), gp.params, gp.dtype)


def compare(gp, ref, xp, tol, parts, full=True):
    mu, var = gp.predict(xp, var="diag")
    mr, vr = ref.predict(xp, var="diag")
    check("mean", mu, mr, tol)
    check("diag variance", var, vr, tol)
    if full:
        check("full covariance", gp.predict(xp, var="full")[1], ref.predict(xp, var="full")[1], tol)
    g, gr = gp.predict_grad(xp), ref.predict_grad(xp)
    check("predict_grad d mean", g[2], gr[2], tol * 10)
    check("predict_grad d var", g[3], gr[3], tol * 10)
    check("krnchd", gp.krnchd, ref.krnchd, tol)
    check("wt", gp.wt, ref.wt, tol * 10)
    hp = gp.params.numpy().copy()
    la, ga = pg.MLE(gp).loss_and_grad(hp)
    lr, grr = pg.MLE(ref).loss_and_grad(hp)
    check("MLE loss", torch.tensor([float(la)]), torch.tensor([float(lr)]), tol)
    check("MLE grad", torch.from_numpy(ga), torch.from_numpy(grr), tol * 10)


# ---- the C ABI ------------------------------------------------------------------------------------
def _abi_state(n, k, n_pad, seed=1):
    rng = np.random.default_rng(seed)
    X = rng.random((n + k, 3))
    y = np.sin(3 * X).sum(1)
    K = ar.se_kernel(X, X) + (0.05 ** 2 + JITTER) * np.eye(n + k)
    state = ar.padded_fit(K[:n, :n], y[:n], n_pad)
    L, invd, M = state[0].copy(), state[1], state[2].copy()
    # the strictly upper part of every real row is scratch: NaN there, inside the diagonal blocks too
    iu = np.triu_indices(n_pad, 1)
    for A in (L, M):
        mask = np.zeros((n_pad, n_pad), bool)
        mask[iu] = True
        mask[n:, :] = False
        A[mask] = np.nan
    Kt = np.zeros((k, n_pad))
    Kt[:, :n] = K[n:, :n]
    return (L, invd, M, state[3], state[4]), Kt, K[n:, n:], y[n:]


def _dev(ops, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ops.device)


def _run_abi(ops, state, Kt, Knn, yn, n):
    L, invd, M, u, alpha = (_dev(ops, a) for a in state)
    n_pad, k = L.shape[0], Knn.shape[0]
    invd_full = torch.zeros(ops.potrf_worksize(n_pad, F64), dtype=F64, device=ops.device)
    invd_full[: n_pad * 128] = invd.reshape(-1)
    work = ops.empty(ops.chol_append_worksize(n_pad, k, F64), dtype=F64)
    info = torch.full((1,), -7, dtype=torch.int32, device=ops.device)
    ops.chol_append(n, k, L, invd_full, M, _dev(ops, Kt), _dev(ops, Knn), _dev(ops, yn), u, alpha, work, info)
    torch.cuda.synchronize()
    return L, invd_full, M, u, alpha, int(info.item())


@pytest.mark.parametrize("k", [1, 7, 30, 128])
def test_abi_against_restatement(ops, k):
    """n = 1000 in n_pad = 1280: k = 30 and 128 straddle the 128-block boundary at 1024.  Minv's and L's strictly upper parts are NaN."""
    n, n_pad = 1000, 1280
    state, Kt, Knn, yn = _abi_state(n, k, n_pad)
    L, invd, M, u, alpha, info = _run_abi(ops, state, Kt, Knn, yn, n)
    assert info == 0
    Lr, ivr, Mr, ur, ar_, inf_r = ar.append(*state, n, Kt, Knn, yn)
    assert inf_r == 0
    Lg, Mg = L.cpu().numpy(), M.cpu().numpy()
    check("L lower", torch.from_numpy(np.tril(Lg)), torch.from_numpy(np.tril(np.nan_to_num(Lr))), 1e-10)
    check("Minv lower", torch.from_numpy(np.tril(Mg)), torch.from_numpy(np.tril(np.nan_to_num(Mr))), 1e-10)
    check("new rows of L", torch.from_numpy(Lg[n:n + k]), torch.from_numpy(Lr[n:n + k]), 1e-10)
    check("new rows of Minv", torch.from_numpy(Mg[n:n + k]), torch.from_numpy(Mr[n:n + k]), 1e-10)
    check("u", u, torch.from_numpy(ur), 1e-10)
    check("alpha", alpha, torch.from_numpy(ar_), 1e-10)
    blocks = invd[: n_pad * 128].reshape(n_pad // 128, 128, 128).cpu()
    check("inv_diag", blocks, torch.from_numpy(ivr), 1e-10)
    eye = np.eye(n_pad)
    # the pad's lower triangle is the identity, exactly (its upper part is the scratch the state came with)
    assert np.array_equal(np.tril(Lg)[n + k:], eye[n + k:]) and np.array_equal(np.tril(Mg)[n + k:], eye[n + k:]), "the pad is not the identity"
    assert np.array_equal(Lg[n + k:], state[0][n + k:]) and np.array_equal(Mg[n + k:], state[2][n + k:])
    assert np.array_equal(blocks.numpy()[(n + k + 127) // 128:], ivr[(n + k + 127) // 128:])
    assert not u[n + k:].any() and not alpha[n + k:].any()


def test_abi_bad_pivot_leaves_buffers(ops):
    n, k, n_pad = 1000, 7, 1280
    state, Kt, Knn, yn = _abi_state(n, k, n_pad)
    Kt[3, 10] = np.nan
    before = [_dev(ops, a) for a in state]
    L, invd, M, u, alpha, info = _run_abi(ops, state, Kt, Knn, yn, n)
    assert info == n + 4
    for name, a, b in zip(("L", "Minv", "u", "alpha"), (L, M, u, alpha), (before[0], before[2], before[3], before[4])):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64)), name
    assert torch.equal(invd[: n_pad * 128].reshape(-1, 128, 128).view(torch.int64), before[1].view(torch.int64))


def test_abi_preconditions(ops):
    L = ops.zeros(256, 256)
    work = ops.zeros(16)
    info = torch.zeros(1, dtype=torch.int32, device=ops.device)
    v = ops.zeros(256)
    for n, k in ((250, 7), (10, 0), (10, 129)):
        with pytest.raises(RuntimeError):
            ops.chol_append(n, k, L, v, L.clone(), L, L, v, v, v.clone(), work, info)


# ---- Exact_GP.append ------------------------------------------------------------------------------
SPECS = [["se", "wn"], ["m52", "wn"], ["m32", "wn"], ["m12", "wn"], ["se", "se", "wn"], ["se", "m52", "m32", "m12", "se", "wn"]]


@pytest.mark.parametrize("parts", SPECS, ids=lambda p: "+".join(p))
def test_append_equals_fresh_fit(parts):
    """Compose([SE, SE, WN]) and a five-kernel Compose, which the library evaluates in two passes of pg_covspec."""
    d = 4
    x, y, rng = data(900, d)
    hp = hp_for(parts, d, rng)
    gp = model(parts, x[:800], y[:800], hp)
    gp.update()
    gp.append(x[800:837], y[800:837])
    gp.append(x[837:], y[837:])
    assert torch.equal(gp.x, x) and torch.equal(gp.y, y)
    xp = torch.from_numpy(rng.random((60, d)))
    compare(gp, fresh(gp, parts), xp, TOL64, parts)


def test_append_fp32():
    parts = ["se", "wn"]
    x, y, rng = data(1000, 3, seed=4)
    hp = hp_for(parts, 3, rng)
    gp = model(parts, x[:900], y[:900], hp, F32)
    gp.update()
    gp.append(x[900:].float(), y[900:].float())
    assert gp.x.dtype == F32 and gp.x.shape == (1000, 3)
    xp = torch.from_numpy(rng.random((40, 3))).float()
    compare(gp, fresh(gp, parts), xp, TOL32, parts, full=False)


@pytest.mark.parametrize("n,k", [(1000, 30), (700, 200)])
def test_append_growth_and_chunks(n, k):
    """1000 + 30 grows n_pad from 1024 to 1280; 700 + 200 runs as two blocks (128 + 72) and grows from 768 to 1024."""
    parts = ["m52", "wn"]
    x, y, rng = data(n + k, 5, seed=7)
    hp = hp_for(parts, 5, rng)
    gp = model(parts, x[:n], y[:n], hp)
    gp.update()
    gp.predict(x[:5], var="diag")       # L^-1 formed by a prediction, then kept by the append
    gp.append(x[n:], y[n:])
    assert gp._experts[0].n_pad == ((n + k + 255) // 256) * 256
    xp = torch.from_numpy(rng.random((50, 5)))
    compare(gp, fresh(gp, parts), xp, TOL64, parts)


def test_many_single_appends_drift():
    """300 appends of one point each from n = 700 (crossing n_pad 768 -> 1024): the drift against a fresh fit stays below 1e-9 (measured
    on an MI355X: 3e-14)."""
    parts = ["se", "wn"]
    x, y, rng = data(1000, 3, seed=9)
    hp = hp_for(parts, 3, rng)
    gp = model(parts, x[:700], y[:700], hp)
    gp.update()
    for i in range(700, 1000):
        gp.append(x[i:i + 1], y[i:i + 1])
    xp = torch.from_numpy(rng.random((50, 3)))
    compare(gp, fresh(gp, parts), xp, 1e-9, parts, full=False)


def test_nan_point_raises_and_leaves_model():
    parts = ["se", "wn"]
    x, y, rng = data(600, 3, seed=2)
    gp = model(parts, x[:500], y[:500], hp_for(parts, 3, rng))
    gp.update()
    xp = torch.from_numpy(rng.random((30, 3)))
    before = gp.predict(xp, var="diag")
    cov_before = gp.predict(xp, var="full")[1]
    x_obj, y_obj = gp.x, gp.y
    xn = x[500:520].clone()
    xn[4, 1] = float("nan")
    with pytest.raises(torch.linalg.LinAlgError):
        gp.append(xn, y[500:520])
    assert gp.x is x_obj and gp.y is y_obj and gp._experts[0].n == 500
    after = gp.predict(xp, var="diag")
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert torch.equal(cov_before, gp.predict(xp, var="full")[1])
    with pytest.raises(torch.linalg.LinAlgError):       # the two-block path (copies) as well
        gp.append(torch.cat([x[500:600], x[500:530], xn]), torch.cat([y[500:600], y[500:530], y[500:520]]))   # NaN in block 2
    assert torch.equal(before[0], gp.predict(xp, var="diag")[0])


def test_dirty_model_and_set_params():
    parts = ["m32", "wn"]
    x, y, rng = data(700, 3, seed=5)
    hp = hp_for(parts, 3, rng)
    xp = torch.from_numpy(rng.random((30, 3)))
    gp = model(parts, x[:600], y[:600], hp)        # never updated: the data is concatenated, the next update fits it
    gp.append(x[600:650], y[600:650])
    gp.update()
    compare(gp, fresh(gp, parts), xp, TOL64, parts, full=False)
    gp.set_params(hp * 1.1)                        # dirty again
    gp.append(x[650:], y[650:])
    assert gp.need_upd
    compare(gp, fresh(gp, parts), xp, TOL64, parts, full=False)


def test_batched_model_raises():
    parts = ["se", "wn"]
    x, y, rng = data(400, 3)
    gp = model(parts, x[:300].reshape(2, 150, 3), y[:300].reshape(2, 150), hp_for(parts, 3, rng))
    gp.update()
    with pytest.raises(NotImplementedError):
        gp.append(x[300:310], y[300:310])
    assert gp.x.shape == (2, 150, 3)


def test_backward_after_append_raises():
    parts = ["se", "wn"]
    x, y, rng = data(400, 3)
    gp = model(parts, x[:350], y[:350], hp_for(parts, 3, rng))
    xp = torch.from_numpy(rng.random((10, 3))).requires_grad_(True)
    mu, var = gp.predict(xp, var="diag")
    gp.append(x[350:], y[350:])
    with pytest.raises(RuntimeError):
        (mu.sum() + var.sum()).backward()


def test_unbatched_leading_one():
    """x [1, n, d] / y [1, n]: x_new [1, k, d] or [k, d], y_new [1, k]."""
    parts = ["se", "wn"]
    x, y, rng = data(500, 3, seed=8)
    hp = hp_for(parts, 3, rng)
    gp = model(parts, x[None, :450], y[None, :450], hp)
    gp.update()
    gp.append(x[None, 450:470], y[None, 450:470])
    gp.append(x[470:], y[None, 470:])
    assert gp.x.shape == (1, 500, 3) and gp.y.shape == (1, 500)
    xp = torch.from_numpy(rng.random((20, 3)))
    compare(gp, fresh(gp, parts), xp, TOL64, parts, full=False)


def test_size_n16384():
    parts = ["se", "wn"]
    d = 8
    x, y, rng = data(16384 + 32, d, seed=11)
    hp = hp_for(parts, d, rng)
    gp = model(parts, x[:16384], y[:16384], hp)
    gp.update()
    gp.append(x[16384:], y[16384:])
    ref = fresh(gp, parts)
    xp = torch.from_numpy(rng.random((64, d)))
    mu, var = gp.predict(xp, var="diag")
    mr, vr = ref.predict(xp, var="diag")
    check("n=16384 mean", mu, mr, 1e-8)
    check("n=16384 diag variance", var, vr, 1e-8)
    check("n=16384 wt", gp.wt, ref.wt, 1e-8)
