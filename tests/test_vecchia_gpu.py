"""The nearest-neighbour (Vecchia) GP on the device (include/pygpr_hip_vecchia.h, pygpr_amd/vecchia.py) against tests/vecchia_ref.py.

pg_knn is held to the restatement integer for integer: the coordinates lie on the grid k / 64, k < 8, and the scales are powers of
two, so every squared distance is exact in fp64 whatever the order or contraction of its terms, and there are many exact ties.

The block kernels have no fixed tolerance.  For every case the yardstick is the distance of the float64 restatement from the
np.longdouble one; the device is compared with the longdouble result and gets four times the yardstick (a Cholesky and substitutions
in place of NumPy's solves is another, equally valid order of operations), with a floor of 64 eps relative to the value's scale for
cases where the restatement happens to be exact.  The scale of a vector is its largest entry; the scale of the loss, a sum over the
targets, is the sum of the magnitudes of its terms (what n additions of those terms may round by).  Each test prints both figures.
The shapes are the smallest at which the kernels can go wrong: the full 64-point block (and every block size below it) at n = 64,
m = 63; rows with -1 padding in a random ordering at n = 130, m = 5; n = 1; a middle range of targets that is no multiple of the
wavefronts of a workgroup; d = 1, 3, 17 (four, four and two wavefronts a workgroup)."""
import numpy as np
import pytest
import torch

import kernel_ref as kr
import kind_tools as kt
from kind_tools import ops  # noqa: F401  (the fixture)
import vecchia_ref as vr
from test_rowsq_cpu import MODELS, _hp

import pygpr_amd as pg
from pygpr_amd import vecchia as vmod

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
LOG2PI = float(np.log(2 * np.pi))


def dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


# ---- pg_knn ----------------------------------------------------------------------------------------------------------------------------
def _grid(rng, n, d):
    return rng.integers(0, 8, (n, d)) / 64.0


@pytest.mark.parametrize("n", [1, 2, 65, 130])
@pytest.mark.parametrize("m", [1, 5, 63])
def test_knn_is_the_restatement_integer_for_integer(ops, n, m):
    rng = np.random.default_rng(100 * n + m)
    for d in (1, 3, 17):
        x = _grid(rng, n, d)
        s = 2.0 ** rng.integers(-2, 3, d)
        # causal, on strided operands (ldx > d, ldn > m) with a scale
        xbuf = torch.full((n, d + 3), 7.0, dtype=torch.float64, device="cuda")
        xbuf[:, :d] = dev(x)
        out = torch.full((n, m + 2), -9, dtype=torch.int32, device="cuda")
        ops.knn(xbuf[:, :d], xbuf[:, :d], m, s=dev(s), causal=True, out=out[:, :m])
        assert np.array_equal(out[:, :m].cpu().numpy(), vr.knn(x, x, s, m, True)), (n, m, d, "causal")
        assert bool((out[:, m:] == -9).all())
        # cross: every candidate, queries of their own, no scale
        q = 70 if n == 130 else min(n, 3)
        xq = _grid(rng, q, d)
        got = ops.knn(dev(xq), dev(x), m, causal=False)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), vr.knn(xq, x, None, m, False)), (n, m, d, "cross")


def test_knn_never_selects_a_nan_point(ops):
    rng = np.random.default_rng(5)
    x = _grid(rng, 130, 3)
    x[40, 1] = np.nan
    for causal in (True, False):
        got = ops.knn(dev(x), dev(x), 63, causal=causal).cpu().numpy()
        ref = vr.knn(x, x, None, 63, causal)
        assert np.array_equal(got, ref) and not (got[np.arange(130) != 40] == 40).any()
        assert (got[40] == -1).all()      # every distance from the NaN point is NaN


# ---- the block kernels -------------------------------------------------------------------------------------------------------------------
def _data(terms, n, d, seed):
    rng = np.random.default_rng(seed)
    x = rng.random((n, d))
    y = np.sin(3.0 * x.sum(1)) + 0.1 * rng.standard_normal(n)
    return _hp(terms, d, rng), x, y


def _held(name, dev_v, f64, ld, scale=None):
    """The rule of the module docstring for one quantity; returns the ratio error / allowance."""
    dev_v, f64, ld = np.asarray(dev_v, np.longdouble), np.asarray(f64, np.longdouble), np.asarray(ld, np.longdouble)
    scale = float(np.max(np.abs(ld))) if scale is None else float(scale)
    yard = float(np.max(np.abs(f64 - ld)))
    err = float(np.max(np.abs(dev_v - ld)))
    tol = max(4.0 * yard, 64.0 * EPS * scale)
    print("    %-6s device %.2e  restatement %.2e  (scale %.2e, allowance %.2e, ratio %.2f)" % (name, err, yard, scale, tol, err / tol))
    assert np.all(np.isfinite(dev_v)) and err <= tol, (name, err, tol)
    return err / tol


_REF = {}


def _reference(key, fn):
    if key not in _REF:
        _REF[key] = (fn(np.float64), fn(np.longdouble))
    return _REF[key]


def _nlml_device(ops, terms, hp, x, y, nbr, first, count, want_grad=True):
    d = x.shape[1]
    spec = kt.one_spec(terms, d, product=any(isinstance(t, tuple) for t in terms))
    cm, cv = torch.full((count,), 5.0, dtype=torch.float64, device="cuda"), torch.full((count,), 5.0, dtype=torch.float64, device="cuda")
    out, grad = torch.full((1,), 5.0, dtype=torch.float64, device="cuda"), torch.full((hp.size,), 5.0, dtype=torch.float64, device="cuda")
    info = torch.full((1,), -3, dtype=torch.int32, device="cuda")
    ops.vecchia_nlml_grad(spec, dev(hp), dev(x), dev(y), dev(nbr, torch.int32), first, count, kr.JITTER, want_grad, cm, cv, out, grad, info)
    return float(out[0]), grad.cpu().numpy(), cm.cpu().numpy(), cv.cpu().numpy(), int(info[0])


def _check_nlml(ops, tag, terms, hp, x, y, nbr, first=0):
    count = nbr.shape[0]
    f64, ld = _reference(("nlml", tag), lambda dt: vr.nlml_and_grad(terms, hp, x, y, nbr, kr.JITTER, dt, first=first))
    loss, grad, cm, cv, info = _nlml_device(ops, terms, hp, x, y, nbr, first, count)
    assert info == 0
    print("%s" % (tag,))
    lscale = float(np.sum(np.abs(0.5 * (np.log(ld[3]) + (y[first: first + count] - ld[2]) ** 2 / ld[3] + LOG2PI))))
    return max(_held("loss", loss, f64[0], ld[0], lscale), _held("grad", grad, f64[1], ld[1]), _held("cmean", cm, f64[2], ld[2], np.max(np.abs(y))),
               _held("cvar", cv, f64[3], ld[3]))


def _full(n, m):
    nbr = np.full((n, m), -1, np.int32)
    for i in range(n):
        nbr[i, :min(i, m)] = np.arange(min(i, m))
    return nbr


@pytest.mark.parametrize("name", sorted(MODELS))
def test_every_block_size_up_to_the_full_block(ops, name):
    """n = 64, m = 63 with every predecessor: block sizes 1 .. 64 in one call."""
    terms = MODELS[name]
    hp, x, y = _data(terms, 64, 3, 21)
    _check_nlml(ops, (name, 64, 63, 3), terms, hp, x, y, _full(64, 63))


@pytest.mark.parametrize("name,d", [("se+m52", 1), ("se*per", 1), ("se+wn", 17), ("se*per", 17), ("rq", 17)])
def test_the_other_dimensions(ops, name, d):
    terms = MODELS[name]
    hp, x, y = _data(terms, 64, d, 22)
    _check_nlml(ops, (name, 64, 63, d), terms, hp, x, y, _full(64, 63))


def _padded_case(name, d=3):
    """n = 130, m = 5 in a random ordering, with entries knocked out of the middle of rows (-1: skipped, the rest keeps its order)."""
    terms = MODELS[name]
    hp, x, y = _data(terms, 130, d, 23)
    rng = np.random.default_rng(24)
    perm = rng.permutation(130)
    x, y = x[perm], y[perm]
    nbr = vr.knn(x, x, None, 5, True)
    hole = rng.random(nbr.shape) < 0.2
    nbr[hole] = -1
    return terms, hp, x, y, nbr


@pytest.mark.parametrize("name", sorted(MODELS))
def test_rows_with_padding_in_a_random_ordering(ops, name):
    terms, hp, x, y, nbr = _padded_case(name)
    _check_nlml(ops, (name, 130, 5, 3), terms, hp, x, y, nbr)


@pytest.mark.parametrize("d", [1, 3, 17])
def test_a_middle_range_of_targets(ops, d):
    """first = 37, count = 41: no multiple of four or two wavefronts."""
    terms, hp, x, y, nbr = _padded_case("se+wn", d)
    _check_nlml(ops, ("se+wn", 130, 5, d, "37+41"), terms, hp, x, y, nbr[37:78], first=37)


def test_one_point(ops):
    terms = MODELS["se+wn"]
    hp, x, y = _data(terms, 1, 3, 25)
    _check_nlml(ops, ("se+wn", 1, 5, 3), terms, hp, x, y, np.full((1, 5), -1, np.int32))


def test_a_call_is_bit_reproducible_and_chunks_add_up(ops, monkeypatch):
    terms, hp, x, y, nbr = _padded_case("se*per")
    a = _nlml_device(ops, terms, hp, x, y, nbr, 0, 130)
    b = _nlml_device(ops, terms, hp, x, y, nbr, 0, 130)
    assert a[0] == b[0] and all(np.array_equal(u, v) for u, v in zip(a[1:4], b[1:4]))
    # the per-target terms do not depend on how the targets are cut; the sums of a chunked evaluation are the chunks' in chunk order
    cuts = [(0, 50), (50, 43), (93, 37)]
    parts = [_nlml_device(ops, terms, hp, x, y, nbr[s: s + c], s, c) for s, c in cuts]
    assert np.array_equal(np.concatenate([p[2] for p in parts]), a[2]) and np.array_equal(np.concatenate([p[3] for p in parts]), a[3])
    cov = kt.cov_of(terms)
    model = pg.Vecchia_GP(torch.from_numpy(x), torch.from_numpy(y), cov, neighbours=5)
    model._device_data()
    model._nbr = dev(nbr, torch.int32)      # the case's own table, holes included
    monkeypatch.setattr(vmod, "_TARGET_CHUNK", 50)
    cuts50 = [(0, 50), (50, 50), (100, 30)]
    parts = [_nlml_device(ops, terms, hp, x, y, nbr[s: s + c], s, c) for s, c in cuts50]
    want_l, want_g = 0.0, np.zeros(hp.size)
    for p in parts:
        want_l, want_g = want_l + p[0], want_g + p[1]
    loss, grad = pg.Vecchia_MLE(model).loss_and_grad(hp)
    assert float(loss) == want_l and np.array_equal(grad, want_g)
    # without the gradient: the same loss and terms, grad untouched
    c = _nlml_device(ops, terms, hp, x, y, nbr, 0, 130, want_grad=False)
    assert c[0] == a[0] and np.array_equal(c[2], a[2]) and bool((c[1] == 5.0).all())


@pytest.mark.parametrize("name", sorted(MODELS))
def test_predict_against_the_restatement(ops, name):
    terms = MODELS[name]
    hp, x, y = _data(terms, 130, 3, 26)
    rng = np.random.default_rng(27)
    xq = rng.random((70, 3))
    xq[5] = x[17]                                  # a test point on a training point: the cross entry carries no noise
    for m in (5, 63):
        nbr = vr.knn(xq, x, None, m, False)
        if m == 5:
            nbr[rng.random(nbr.shape) < 0.2] = -1
        f64, ld = _reference(("predict", name, m), lambda dt: vr.predict(terms, hp, x, y, xq, nbr, kr.JITTER, dt))
        spec = kt.one_spec(terms, 3, product=any(isinstance(t, tuple) for t in terms))
        mean, var = torch.full((70,), 5.0, dtype=torch.float64, device="cuda"), torch.full((70,), 5.0, dtype=torch.float64, device="cuda")
        info = torch.full((1,), -3, dtype=torch.int32, device="cuda")
        ops.vecchia_predict(spec, dev(hp), dev(x), dev(y), dev(xq), dev(nbr, torch.int32), kr.JITTER, mean, var, info)
        assert int(info[0]) == 0
        print((name, "predict", m))
        _held("mean", mean.cpu().numpy(), f64[0], ld[0], np.max(np.abs(y)))
        _held("var", var.cpu().numpy(), f64[1], ld[1])
        only = torch.full((70,), 5.0, dtype=torch.float64, device="cuda")
        ops.vecchia_predict(spec, dev(hp), dev(x), dev(y), dev(xq), dev(nbr, torch.int32), kr.JITTER, only, None, info)
        assert torch.equal(only, mean)


# ---- exactness through the public classes -------------------------------------------------------------------------------------------------
def test_with_every_predecessor_the_loss_is_mles(ops):
    terms = MODELS["se+wn"]
    hp, x, y = _data(terms, 64, 3, 31)
    cov = kt.cov_of(terms)
    X, Y = torch.from_numpy(x), torch.from_numpy(y)
    model = pg.Vecchia_GP(X, Y, cov, neighbours=63)
    loss, grad = pg.Vecchia_MLE(model).loss_and_grad(hp)
    l_ex, g_ex = pg.MLE(pg.Exact_GP(X, Y, cov)).loss_and_grad(hp.copy())
    # the longdouble truth is the restatement's at m = n - 1; the yardstick is kernel_ref's float64 exact GP
    ld = vr.nlml_and_grad(terms, hp, x, y, _full(64, 63), kr.JITTER, np.longdouble)
    l_kr, g_kr = kr.nlml_and_grad(terms, hp, x, y)
    lscale = float(np.sum(np.abs(0.5 * (np.log(ld[3]) + (y - ld[2]) ** 2 / ld[3] + LOG2PI))))
    print("Vecchia_MLE at m = n - 1 against the exact GP")
    _held("loss", float(loss), l_kr, ld[0], lscale)
    _held("grad", grad, g_kr, ld[1])
    print("    MLE(Exact_GP): loss %.2e grad %.2e from the longdouble result" % (abs(float(l_ex) - float(ld[0])), float(np.max(np.abs(g_ex - ld[1])))))
    assert abs(float(loss) - float(l_ex)) <= 1e-10 * abs(float(l_ex)) and np.max(np.abs(grad - g_ex)) <= 1e-9 * np.max(np.abs(g_ex))


def test_with_every_point_a_neighbour_predict_is_exact_gps(ops):
    terms = MODELS["se+wn"]
    hp, x, y = _data(terms, 63, 3, 32)
    cov = kt.cov_of(terms)
    X, Y = torch.from_numpy(x), torch.from_numpy(y)
    xp = np.random.default_rng(33).random((40, 3))
    model = pg.Vecchia_GP(X, Y, cov, neighbours=63, order="random", seed=3)
    model.set_params(torch.from_numpy(hp))
    mean, var = model.predict(torch.from_numpy(xp), "diag")
    exact = pg.Exact_GP(X, Y, cov)
    exact.set_params(torch.from_numpy(hp))
    m_ex, v_ex = exact.predict(torch.from_numpy(xp), var="diag")
    ld = vr.predict(terms, hp, x, y, xp, np.tile(np.arange(63, dtype=np.int32), (40, 1)), kr.JITTER, np.longdouble)
    m_kr, v_kr = kr.predict(terms, hp, x, y, xp, "diag")
    print("Vecchia_GP.predict with every point a neighbour against the exact GP")
    _held("mean", mean.cpu().numpy(), m_kr, ld[0], np.max(np.abs(y)))
    _held("var", var.cpu().numpy(), v_kr, ld[1])
    assert np.max(np.abs(mean.cpu().numpy() - m_ex.cpu().numpy())) <= 1e-9 * np.max(np.abs(y))
    assert np.max(np.abs(var.cpu().numpy() - v_ex.cpu().numpy())) <= 1e-9 * float(np.max(v_kr))
    model.update()
    assert model.cond_mean.shape == (63,) and bool(torch.isfinite(model.cond_var).all()) and np.isfinite(model.nlml)


def test_cg_trains_the_model(ops, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)                              # the optimiser writes its trace into the working directory
    terms = MODELS["se+wn"]
    _, x, y = _data(terms, 700, 3, 34)
    model = pg.Vecchia_GP(torch.from_numpy(x), torch.from_numpy(y), kt.cov_of(terms), neighbours=16, order="random", seed=1)
    # (not cov.init_params: its noise of 1e-4 leaves blocks with a condition of 1e8, where the loss of 8e6 is rounded more coarsely than
    # a line search's first step changes it)
    model.set_params(torch.tensor([1.0, 1.0, 1.0, 1.0, 0.3], dtype=torch.float64))
    p0 = model.params.numpy().copy()
    loss = pg.Vecchia_MLE(model)
    start = float(loss.loss(p0))
    table = model._nbr
    opt = pg.CG(loss)
    opt.args.update(maxiter=6, disp=False)
    opt.minimize()
    end = float(loss.loss(model.params.numpy().copy()))
    print("CG(Vecchia_MLE): %.4f -> %.4f in %d iterations" % (start, end, opt.res.nit))
    assert np.isfinite(end) and end < start - 1.0 and not np.array_equal(model.params.numpy(), p0)
    assert model._nbr is table                               # the neighbour sets stayed while the parameters moved


# ---- the failure path -------------------------------------------------------------------------------------------------------------------------
def test_two_coincident_points_without_noise(ops):
    terms = MODELS["m12"]
    hp, x, y = _data(terms, 40, 3, 35)
    x[39] = x[11]    # the LAST point: no later block holds both (such a block is singular too, and fails with the same right)
    hp[0] = 1.0      # sigma^2 = 1: the duplicate's pivot is 1 - 1 * 1 - 0 = 0 EXACTLY (point 11 is its nearest neighbour, the block's first)
    nbr = vr.knn(x, x, None, 8, True)
    assert nbr[39, 0] == 11
    # jitter = 0 here: with Exact_GP's JITTER on the diagonal the duplicate's pivot is 2e-7, nine orders above the rounding of the
    # block, and the model factors it -- the class is therefore held to a point that no jitter repairs, a NaN coordinate, below
    spec = kt.one_spec(terms, 3)
    cm, cv = torch.zeros(40, dtype=torch.float64, device="cuda"), torch.zeros(40, dtype=torch.float64, device="cuda")
    out, grad = torch.zeros(1, dtype=torch.float64, device="cuda"), torch.zeros(hp.size, dtype=torch.float64, device="cuda")
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.vecchia_nlml_grad(spec, dev(hp), dev(x), dev(y), dev(nbr, torch.int32), 0, 40, 0.0, True, cm, cv, out, grad, info)
    assert int(info[0]) == 40
    cm, cv = cm.cpu().numpy(), cv.cpu().numpy()
    others = np.arange(40) != 39
    assert np.isnan(cm[39]) and np.isnan(cv[39]) and np.isfinite(cm[others]).all() and np.isfinite(cv[others]).all() and np.isnan(float(out[0]))
    # through the class (its JITTER keeps this block factorable, a NaN point does not)
    x[39] = 0.37
    x[29] = np.nan
    model = pg.Vecchia_GP(torch.from_numpy(x), torch.from_numpy(y), kt.cov_of(terms), neighbours=8)
    model.set_params(torch.from_numpy(hp))
    with pytest.raises(torch.linalg.LinAlgError) as err:
        model.update()
    assert "point 29" in str(err.value) and model.need_upd
