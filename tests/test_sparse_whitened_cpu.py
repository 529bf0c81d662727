"""Sparse_GP(whitened=True) on the host: the whitened restatement (tests/sparse_whitened_ref.py) checked against the unwhitened one,
against central differences in long double and against the folded forms it exists to avoid; then the Python class logic of
pygpr_amd/sparse.py on a test double of the device ops.  No GPU.

Tolerances: the project's rule.  A result may miss the float64 restatement by sparse_ref.tol_of(own) = 50 x the restatement's own
float64-vs-np.longdouble difference on that input, floored at 1e-10; loss, gradients and mean relative to the largest reference
entry, variance and covariance relative to the PRIOR variance kss.  Every comparison prints what it measured."""
import functools

import numpy as np
import pytest
import torch

import gemm_ref as gr
import pygpr_amd as pg
import sparse_ref as sr
import sparse_whitened_ref as wr
import sparse_z_ref as szr
from oracle_ops import _np
from pygpr_amd import _lib, _ops
from pygpr_amd import sparse as sparse_mod
from test_sparse_cpu import MODELS
from test_sparse_z_cpu import SparseZOracleOps

EASY, case = wr.EASY, wr.case
MAKE = dict(MODELS, hard=(["se", "wn"], MODELS["se+wn"][1]))
hold = functools.partial(wr.hold, who="got")


# ------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", EASY)
def test_whitened_and_unwhitened_restatements_agree_on_the_easy_input(name):
    terms, hp, x, y, z, xp, ref, _ = case(name)
    own = sr.self_error(terms, hp, x, y, z)
    loss, grad = sr.loss_and_grad(terms, hp, x, y, z)
    mu, cov = sr.predict(terms, hp, x, y, z, xp, var="full")
    dm, dv = szr.predict_grads(terms, hp, x, y, z, xp)
    hold(name + " loss", ref["loss"], loss, own)
    hold(name + " gradient", ref["grad"], grad, own)
    hold(name + " z gradient", ref["zgrad"], szr.z_grad(terms, hp, x, y, z), own)
    hold(name + " mean", ref["mean"], mu, own)
    hold(name + " covariance", ref["cov"], cov, own, scale=ref["kss"].max())
    hold(name + " d mean / dx*", ref["dmean"], dm, own)
    hold(name + " d var / dx*", ref["dvar"], dv, own)


@pytest.mark.parametrize("name", ["se+wn", "hard"])
def test_gradient_against_central_differences_in_long_double(name):
    """The hyper-parameters and the first three inducing inputs, by quotients of the loss in np.longdouble (64-bit mantissa) at the
    relative step h = 1e-6 |p|: truncation is h^2 = 1e-12 of an entry's own scale, rounding 2^-64 cond(Kuu) |L| / h.  Measured on
    the small hard input (n = 120, m = 30; the sigma_n entry, 2e12, is the largest by four orders): 4e-11 of the largest entry and 3e-6
    of an entry's own size, the quotient's own noise (the closed form in long double sits as far from it).  Held to 1e-9 and 1e-4."""
    terms, hp, x, y, z = wr.hard_problem(n=120, m=30) if name == "hard" else (MODELS[name][0], *sr.problem(MODELS[name][0], n=120, m=20))
    g = np.concatenate([wr.loss_and_grad(terms, hp, x, y, z)[1], wr.z_grad(terms, hp, x, y, z)[:3].reshape(-1)])
    fd = np.zeros(g.size, wr.LD)
    for i in range(g.size):
        up, dn = [np.concatenate([hp, z[:3].reshape(-1)]).astype(wr.LD) for _ in range(2)]
        h = wr.LD(1e-6) * abs(up[i])
        up[i] += h
        dn[i] -= h
        ends = [wr.loss(terms, p[:hp.size], x, y, np.concatenate([p[hp.size:].reshape(3, -1), z[3:].astype(wr.LD)]), wr.LD) for p in (up, dn)]
        fd[i] = (ends[0] - ends[1]) / (2 * h)
    err, each = float(np.abs(g - fd).max() / np.abs(fd).max()), float((np.abs(g - fd) / np.abs(fd)).max())
    print("closed form vs long-double central differences", name, "%.2e of the largest entry, %.2e of its own" % (err, each))
    assert err <= 1e-9 and each <= 1e-4


def test_the_folded_forms_lose_what_the_whitened_ones_keep_on_the_hard_input():
    """The reason the library whitens every chunk: folding Li^T . Li into one m x m weight and applying it to the
    unwhitened Kuf / Ksu costs the gradient four digits and leaves the variance off by a tenth of the smallest variance."""
    terms, hp, x, y, z, xp, ref, own = case("hard")
    print("cond(Kuu) %.2e, smallest eigenvalue of Sigma %.2e, of D %.4f" % wr.hard_preconditions(terms, hp, x, y, z))
    g_ld = wr.loss_and_grad(terms, hp, x, y, z, wr.LD)[1]
    g_fold = wr.loss_and_grad(terms, hp, x, y, z, folded=True)[1]
    v_ld = np.diag(wr.predict(terms, hp, x, y, z, xp, wr.LD)[1])
    e_fold = float(np.abs(g_fold - g_ld).max() / np.abs(g_ld).max())
    v_fold = float(np.abs(wr.folded_var(terms, hp, x, y, z, xp) - v_ld).max())
    v_own = float(np.abs(ref["var"] - v_ld).max())
    print("gradient: folded %.2e whitened %.2e;  variance (absolute): folded %.2e whitened %.2e, smallest variance %.2e"
          % (e_fold, own["grad"], v_fold, v_own, ref["var"].min()))
    assert e_fold >= 1e3 * own["grad"] and v_fold >= 1e3 * v_own
    assert v_fold >= 0.05 * ref["var"].min() and v_own <= 1e-4 * ref["var"].min()
    assert v_fold / ref["kss"].max() > sr.tol_of(own["var"])           # the variance's rule (relative to kss) refuses the folded form


# ------------------------------------------------------------------------------------------- host logic on a test double
RECORDED = ("kernel_build", "symmetrize", "potrf", "trtri", "lauum", "potrs_vec", "kernel_cross_grad", "kernel_xgrad", "trmm_lower",
            "trmm_lower_kt", "trmv")
K_RANGE = {(_lib.GEMM_NN, 0, 1): "GEMM_NN", (_lib.GEMM_NN, 2, 0): "GEMM_NN", (_lib.GEMM_TN, 1, 0): "GEMM_TN"}


class WhitenedOracleOps(SparseZOracleOps):
    """SparseZOracleOps plus the K-range products the whitened evaluation issues (NN with khi = 1 or klo = 2, TN with klo = 1), tile by
    tile as tests/gemm_ref.py states them.  pg_trtri leaves scratch above the diagonal 128-blocks: this double leaves NaN there, so a
    product that reads them shows.  Every device call is recorded by name (products: with variant, tri, klo, khi)."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def gemm_raw(self, variant, m, n, k, alpha, a, b, beta, c, tri=0, klo=0, khi=0):
        self.calls.append(("gemm_raw", variant, tri, klo, khi))
        if klo == khi == 0:
            return super().gemm_raw(variant, m, n, k, alpha, a, b, beta, c, tri=tri)
        name = K_RANGE[(variant, klo, khi)]
        assert not tri and m % 128 == n % 128 == 0 and k % 16 == 0
        op_a = _np(a)[:k, :m].T if variant == _lib.GEMM_TN else _np(a)[:m, :k]
        out, written = gr.expected(name, m, n, k, alpha, op_a, _np(b)[:k, :n], beta, _np(c)[:m, :n].copy(), 0, klo, khi)
        assert written.all()
        _np(c)[:m, :n] = out

    def trtri(self, chol, invd, minv):
        self.calls.append("trtri")
        super().trtri(chol, invd, minv)
        blk = np.arange(minv.shape[0]) // 128
        _np(minv)[blk[None, :] > blk[:, None]] = np.nan


def _recorded(name):
    def call(self, *args, **kwargs):
        self.calls.append(name)
        return getattr(super(WhitenedOracleOps, self), name)(*args, **kwargs)
    return call


for _name in RECORDED:
    if _name != "trtri":
        setattr(WhitenedOracleOps, _name, _recorded(_name))


@pytest.fixture
def w_ops(monkeypatch, tmp_path):
    ops = WhitenedOracleOps()
    monkeypatch.setattr(_ops, "_OPS", ops)
    monkeypatch.chdir(tmp_path)
    return ops


def model_of(name, whitened=True):
    terms, hp, x, y, z, xp, ref, own = case(name)
    gp = pg.Sparse_GP(torch.from_numpy(x), torch.from_numpy(y), MAKE[name][1](), torch.from_numpy(z.copy()), whitened=whitened)
    gp.set_params(torch.from_numpy(hp))
    return gp


@pytest.mark.parametrize("name", EASY + ["hard"])
@pytest.mark.parametrize("chunk", [128, 32768])
def test_class_agrees_with_the_restatement(w_ops, monkeypatch, name, chunk):
    """n = 300: chunk 128 walks chunks of 128, 128 and 44 columns, the default chunk holds all in one."""
    monkeypatch.setattr(sparse_mod, "_SPARSE_CHUNK", chunk)
    terms, hp, x, y, z, xp, ref, own = case(name)
    gp = model_of(name)
    assert gp.whitened is True
    tag = "%s chunk %d " % (name, chunk)
    loss, grad = pg.VFE(gp).loss_and_grad(hp.copy())
    hold(tag + "loss", loss, ref["loss"], own["loss"])
    hold(tag + "gradient", grad, ref["grad"], own["grad"])
    hold(tag + "loss alone", pg.VFE(gp).loss(hp.copy()), ref["loss"], own["loss"])
    vz = pg.VFE(gp, train_z=True)
    lz, gz = vz.loss_and_grad(vz.start_params())
    assert lz == loss and np.array_equal(gz[:hp.size], grad)
    hold(tag + "z gradient", gz[hp.size:].reshape(z.shape), ref["zgrad"], own["zgrad"])
    nch = -(-x.shape[0] // chunk)
    m = z.shape[0]
    cross = [(m, m, False)] + [(m, min(chunk, 300 - s), True) for s in range(0, 300, chunk)]
    assert w_ops.cross_calls == 2 * cross and len(cross) == 1 + nch
    assert w_ops.xgrad_calls == [(m, m, False, True, False)] + [(m, nc, False, True, True) for _, nc, _ in cross[1:]]
    xpt = torch.from_numpy(xp)
    kss = ref["kss"].max()
    m1, vd = gp.predict(xpt, var="diag")
    m2, vf = gp.predict(xpt, var="full")
    m3, none = gp.predict(xpt, var="none")
    for mu in (m1, m2, m3):
        hold(tag + "mean", mu.numpy(), ref["mean"], own["mean"])
    hold(tag + "variance", vd.numpy(), ref["var"], own["var"], scale=kss)
    hold(tag + "covariance", vf.numpy(), ref["cov"], own["cov"], scale=kss)
    assert torch.equal(vf, vf.T) and none is NotImplemented
    mean, var, dmean, dvar = gp.predict_grad(xpt)
    assert torch.equal(mean, m1) and torch.equal(var, vd) and dmean.shape == dvar.shape == xp.shape
    hold(tag + "d mean / dx*", dmean.numpy(), ref["dmean"], own["dmean"])
    hold(tag + "d var / dx*", dvar.numpy(), ref["dvar"], own["dvar"])
    two = gp.predict_grad(xpt, var="none")
    assert len(two) == 2 and torch.equal(two[0], m1)
    hold(tag + "d mean / dx* (var none)", two[1].numpy(), ref["dmean"], own["dmean"])


def test_predict_chunks_the_test_points(w_ops, monkeypatch):
    gp = model_of("se+wn")
    xp = torch.from_numpy(np.random.default_rng(2).random((70, 3)))
    whole = gp.predict_grad(xp)
    monkeypatch.setattr(sparse_mod, "_CHUNK", 32)
    parts = gp.predict_grad(xp)
    for a, b in zip(whole, parts):
        assert torch.allclose(a, b, rtol=0, atol=1e-12)


def test_the_hard_input_fails_unwhitened_and_not_whitened(w_ops):
    terms, hp, x, y, z, *_ = case("hard")
    wr.hard_preconditions(terms, hp, x, y, z)
    plain = model_of("hard", whitened=False)
    with pytest.raises(torch.linalg.LinAlgError):
        plain.update()
    assert plain.need_upd and plain.whitened is False
    gp = model_of("hard")
    gp.update()
    assert not gp.need_upd


def test_state_and_memo_follow_the_data(w_ops):
    terms, hp, x, y, z, *_ = case("se+wn")
    gp = model_of("se+wn")
    assert gp.need_upd
    gp.update()
    assert not gp.need_upd and set(gp._state) >= {"li", "bm", "c"} and "kuui" not in gp._state
    vfe = pg.VFE(gp)
    l0 = float(vfe.loss(hp.copy()))
    n0 = len(w_ops.calls)
    assert float(vfe.loss(hp.copy())) == l0 and len(w_ops.calls) == n0          # served by the memo
    gp.z = torch.from_numpy(z[:30].copy())                     # assigning z marks the model dirty and drops the loss's memo
    assert gp.need_upd
    l1 = float(vfe.loss(hp.copy()))
    assert abs(l1 - float(wr.loss(terms, hp, x, y, z[:30]))) <= 1e-10 * abs(l1) and l1 > l0
    gp.update()
    gp.z[2, 1] += 0.01                                         # an in-place edit: the version counter tells
    l2 = float(vfe.loss(hp.copy()))
    assert l2 != l1 and abs(l2 - float(wr.loss(terms, hp, x, y, gp.z.numpy()))) <= 1e-10 * abs(l2)
    xp = torch.from_numpy(x[:5] + 0.01)
    gp.predict(xp, var="diag")
    assert not gp.need_upd
    gp.y = torch.from_numpy(y + 1.0)
    assert gp.need_upd
    mu = gp.predict(xp, var="diag")[0].numpy()
    assert np.abs(mu - np.asarray(wr.predict(terms, hp, x, y + 1.0, gp.z.numpy(), x[:5] + 0.01)[0])).max() <= 1e-10 * np.abs(mu).max()
    gp.x = torch.from_numpy(x * 1.01)
    assert gp.need_upd
    gp.update()
    gp.set_params(torch.from_numpy(hp * 1.1))
    assert gp.need_upd
    with pytest.raises(AttributeError):
        gp.whitened = False


def test_memo_tells_a_whitened_model_from_an_unwhitened_one(w_ops, monkeypatch):
    """Two models on the same tensors and covariance: the VFE of each evaluates its own model's path, and the part of the memo's key
    that belongs to the model holds `whitened`."""
    terms, hp, x, y, z, *_ = case("se+wn")
    xt, yt, zt, cov = torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(z.copy()), MAKE["se+wn"][1]()
    a, b = pg.Sparse_GP(xt, yt, cov, zt, whitened=True), pg.Sparse_GP(xt, yt, cov, zt)
    va, vb = pg.VFE(a), pg.VFE(b)
    va.loss(hp.copy())
    vb.loss(hp.copy())
    assert va._z_seen != vb._z_seen and va._z_seen[:3] == vb._z_seen[:3] and va._z_seen[3] is True and vb._z_seen[3] is False
    assert va._memo[0] == vb._memo[0]                          # the shared part of the key: same data, covariance and parameters


def test_failed_factorisation_raises_and_leaves_the_model_dirty(w_ops):
    terms, hp, x, y, z, *_ = case("se+wn")
    gp = model_of("se+wn")
    zbad = z.copy()
    zbad[3, 1] = np.nan
    gp.z = torch.from_numpy(zbad)
    with pytest.raises(torch.linalg.LinAlgError):
        gp.update()
    assert gp.need_upd and gp._state is None
    with pytest.raises(torch.linalg.LinAlgError):
        pg.VFE(gp).loss(hp.copy())
    with pytest.raises(torch.linalg.LinAlgError):
        gp.predict(torch.from_numpy(x[:5]), var="diag")
    gp.z = torch.from_numpy(z)
    gp.update()
    assert not gp.need_upd


def test_training_from_init_params_lowers_the_bound_at_m_90(w_ops):
    """sigma_n = 1e-4 and m = 90: where the unwhitened model cannot take a single step (tests/test_sparse_cpu.py trains at m = 20)."""
    terms = MODELS["se+wn"][0]
    hp, x, y, z = sr.problem(terms, n=300, m=90)
    make = lambda whitened: pg.Sparse_GP(torch.from_numpy(x), torch.from_numpy(y), MAKE["se+wn"][1](), torch.from_numpy(z), whitened=whitened)      # noqa: E731
    plain = make(False)
    with pytest.raises(torch.linalg.LinAlgError):
        pg.VFE(plain).loss(plain.params.numpy().copy())
    gp = make(True)
    vfe = pg.VFE(gp)
    start = float(vfe.loss(gp.params.numpy().copy()))
    opt = pg.CG(vfe)
    opt.args.update(maxiter=6, disp=False)
    opt.minimize()
    end = float(vfe.loss(gp.params.numpy().copy()))
    print("CG(VFE), whitened, m = 90: %.4f -> %.4f" % (start, end))
    assert np.isfinite(end) and end < start - 1.0


def test_greedy_hands_whitened_on(w_ops, monkeypatch):
    terms, hp, x, y, z, *_ = case("se+wn")
    pick = sparse_mod.Selection(torch.arange(7), torch.zeros(7), torch.zeros(x.shape[0]))
    monkeypatch.setattr(sparse_mod, "select_inducing", lambda *a, **k: pick)
    xt, yt = torch.from_numpy(x), torch.from_numpy(y)
    assert pg.Sparse_GP.greedy(xt, yt, MAKE["se+wn"][1](), 7, whitened=True).whitened is True
    assert pg.Sparse_GP.greedy(xt, yt, MAKE["se+wn"][1](), 7).whitened is False


# ------------------------------------------------------------------------------------------- the default path is the parent's
def _parent_sequence(nch, want_grad, zgrad=False):
    """The device calls of one unwhitened evaluation as pygpr_amd/sparse.py issued them before `whitened` existed (products: variant,
    tri, klo, khi), written out from that code: pass 1, the m x m algebra, G_uu, pass 2."""
    nt64, nn = _lib.GEMM_NT_64, _lib.GEMM_NN
    seq = ["kernel_build", ("gemm_raw", nt64, 1, 0, 0)] * nch + ["symmetrize", "kernel_build"]
    seq += ["potrf", "trtri", "lauum", "symmetrize"] * 2 + ["potrs_vec", ("gemm_raw", nn, 0, 0, 0)]
    if want_grad:
        seq += [("gemm_raw", nn, 0, 0, 0), "kernel_cross_grad"] + (["kernel_xgrad"] if zgrad else [])
        per = (["kernel_build"] if nch > 1 else []) + [("gemm_raw", nn, 0, 0, 0), "kernel_cross_grad"] + (["kernel_xgrad"] if zgrad else [])
        seq += per * nch
    return seq


@pytest.mark.parametrize("chunk", [128, 32768])
def test_unwhitened_model_issues_the_parents_calls(w_ops, monkeypatch, chunk):
    monkeypatch.setattr(sparse_mod, "_SPARSE_CHUNK", chunk)
    terms, hp, x, y, z, xp, *_ = case("se+wn")
    nch = -(-x.shape[0] // chunk)
    gp = model_of("se+wn", whitened=False)
    pg.VFE(gp).loss(hp.copy())
    assert w_ops.calls == _parent_sequence(nch, False)
    del w_ops.calls[:]
    pg.VFE(gp).loss_and_grad(hp.copy())
    assert w_ops.calls == _parent_sequence(nch, True)
    del w_ops.calls[:]
    vz = pg.VFE(gp, train_z=True)
    vz.loss_and_grad(vz.start_params())
    assert w_ops.calls == _parent_sequence(nch, True, zgrad=True)
    del w_ops.calls[:]
    xpt = torch.from_numpy(xp)
    gp.predict(xpt, var="full")
    nn, nt = _lib.GEMM_NN, _lib.GEMM_NT
    full = ["kernel_build", ("gemm_raw", nn, 0, 0, 0), "kernel_build", ("gemm_raw", nt, 1, 0, 0), "symmetrize"]
    assert w_ops.calls == _parent_sequence(nch, False) + full
    del w_ops.calls[:]
    gp.predict(xpt, var="diag")
    gp.predict_grad(xpt)
    assert w_ops.calls == ["kernel_build", ("gemm_raw", nn, 0, 0, 0)] + ["kernel_build", ("gemm_raw", nn, 0, 0, 0), "kernel_xgrad"]
    # and a whitened model on the same double does use what the parent never did
    del w_ops.calls[:]
    pg.VFE(model_of("se+wn")).loss_and_grad(hp.copy())
    used = {c if isinstance(c, str) else c[1:] for c in w_ops.calls}
    assert {"trmm_lower", (_lib.GEMM_TN, 0, 1, 0), (_lib.GEMM_NN, 0, 2, 0)} <= used
