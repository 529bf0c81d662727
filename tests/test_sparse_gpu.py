"""Sparse_GP on the MI355X: the rectangular contraction pg_kernel_cross_grad alone and on framed operands, then the model -- loss,
gradient and predictions against the NumPy restatement (tests/sparse_ref.py), against Exact_GP, in training and on its failure path.

Tolerances (none is a guess; every test prints what it measured):
  kernel   the device may miss the float64 restatement by 16 x the restatement's own float64-vs-np.longdouble difference.  Both are
           taken per entry relative to S_p = sum_ij |W_ij dk_ij/dtheta_p|, the sum of the magnitudes that are added, and the largest
           over the entries is the figure (an accumulating call: plus the one rounding of grad[p] + sum, `judge`).  The fp32 case: 16 x the difference between the restatement evaluated in np.float32 and in
           float64 on the same fp32-rounded inputs (measured on the CPU), same scale.
  model    per comparison 50 x the disagreement between the restatement's dense (n x n) and Woodbury (m x m) forms on that input,
           floored at 1e-10, relative to the largest reference entry: the loss's disagreement for loss and gradient, the predictive
           mean's for the mean, the predictive covariance's for diagonal and full.  z is a subset of x at pairwise distance >= 0.3 in
           scaled units with cond(Kuu) <= 1e6 (sparse_ref.problem asserts both), which keeps the restatement itself at 1e-12.

z = x against Exact_GP.  The two models are NOT the same function there: Kuu carries JITTER, so Q = K (K + j I)^-1 K, and Exact_GP
factors K + sigma^2 I + j I.  The restatements of the two differ by 9e-7 of the mean at sigma_n = 0.3 (7e-9 even at sigma_n = 40),
far above 1e-10, whatever the implementation.  The test therefore holds the DEVICE difference (Sparse_GP - Exact_GP) to the
RESTATEMENTS' difference (sparse_ref.predict - kernel_ref.predict) within the model tolerance: the jitter's effect is taken out by
the reference, and the comparison against Exact_GP keeps the issue's bound."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import kernel_ref as kr
import pygpr_amd as pg
import sparse_ref as sr
from kind_tools import cov_of, dev, one_spec, ops  # noqa: F401  (ops: the module's fixture)
from pygpr_amd import sparse as sparse_mod
from test_framed_gpu import F32, F64, gaps_odd, ok, p, run

pytestmark = pytest.mark.gpu

KMODELS = {"se+wn": ["se", "wn"], "m12": ["m12"], "rq": ["rq"], "per": ["per"], "se+m52": ["se", "m52"], "se*per": [("se", "per")]}
SHAPES = [(70, 150), (64, 64), (1, 300)]
SENT = 7.25      # what the entries the call must not touch hold before it


def _hp(terms, d, rng):
    hp = []
    for part in kr.flat(terms):
        if part == "wn":
            hp += [0.3]
            continue
        hp += [0.8 + 0.4 * rng.random()] + list((0.8 + 0.8 * rng.random(d)) / np.sqrt(d))
        hp += [1.3] if part == "rq" else (list(0.6 + 0.5 * rng.random(d)) if part == "per" else [])
    return np.array(hp)


def _mine(terms, d):
    """Boolean mask over hp: the entries of the stationary blocks (what the call writes)."""
    mask = np.zeros(kr.nhp_of(terms, d), bool)
    for t, blocks in kr._chunks(terms, d):
        if t != "wn":
            for _, a, b in blocks:
                mask[a:b] = True
    return mask


@functools.lru_cache(maxsize=None)
def kcase(name, m, n, d, symmetric=False, f32=False):
    """Inputs, the float64 restatement, its scale S_p and its own error, computed once per case."""
    terms = KMODELS[name]
    rng = np.random.default_rng(1000 * m + 10 * n + d)
    hp = _hp(terms, d, rng)
    z = rng.random((m, d))
    x = z if symmetric else rng.random((n, d))
    w = rng.standard_normal((m, n))
    if symmetric:
        w = w + w.T
    if f32:
        z, x, w = (a.astype(np.float32).astype(np.float64) for a in (z, x, w))
    ref = sr.cross_grad(terms, hp, z, x, w)
    scale = np.zeros_like(ref)
    for i, slab in sr.cross_grad_terms(terms, hp, x, z):
        scale[i] = np.sum(np.abs(w * slab))
    mine = _mine(terms, d)
    dt = np.float32 if f32 else np.longdouble
    other = np.zeros(hp.size, np.longdouble)
    for i, slab in sr.cross_grad_terms(terms, hp, x, z, dt):
        assert slab.dtype == dt                           # the restatement really ran in that precision
        other[i] = np.sum(np.asarray(w, dt) * slab)
    own = float(np.max(np.abs(other - ref)[mine] / scale[mine]))
    return terms, hp, z, x, w, ref, scale, mine, own


def spec_for(terms, d):
    return one_spec(terms, d, product=any(isinstance(t, tuple) for t in terms))


def call(ops, terms, hp, z, x, w, dtype, accumulate, start):
    d = z.shape[1]
    grad = dev(start)
    out = ops.kernel_cross_grad(spec_for(terms, d), dev(hp), dev(z, dtype), dev(x, dtype), dev(w, dtype), grad, accumulate=accumulate)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def judge(label, got, start, accumulate, ref, scale, mine, own):
    """16 x the restatement's own error, relative to S_p; an accumulating call also rounds grad[p] + sum once, which the restatement's
    error does not hold: half an ulp of the entry it leaves, 2^-53 |grad[p] + sum|, is allowed on top (the start values are larger than
    some S_p here)."""
    want = ref + (start if accumulate else 0.0)
    err = np.abs(got - want)[mine] / scale[mine]
    allowed = 16 * own + (2.0 ** -53 * np.abs(want)[mine] / scale[mine] if accumulate else 0.0)
    print("%-40s device %.2e  restatement %.2e  (bound %.2e)" % (label, float(err.max()), own, float(np.max(allowed))))
    assert np.array_equal(got[~mine], start[~mine]), "entries outside the spec's stationary blocks were touched"
    assert np.all(err <= allowed), (label, float(err.max()), own)


# every model, shape and mode at d = 1, 3, 17 (the kernel's DMAX 4 and 32), then the other instantiations -- d = 5, 9, 33: DMAX 8, 16
# and 64, the last with its opt-in LDS size -- at the one ragged two-by-three-tile shape for a plain, a periodic and a product model
DEEP_D = [5, 9, 33]
DEEP_MODELS = ["se+wn", "per", "se*per"]
GRID = [(m, n, d, name, acc) for acc in (False, True) for name in sorted(KMODELS) for d in (1, 3, 17) for m, n in SHAPES]
GRID += [(70, 150, d, name, False) for d in DEEP_D for name in DEEP_MODELS]


@pytest.mark.parametrize("m,n,d,name,accumulate", GRID, ids=["%d-%d-%d-%s-%s" % (c[:4] + ("acc" if c[4] else "set",)) for c in GRID])
def test_cross_grad_against_the_restatement(ops, m, n, d, name, accumulate):
    terms, hp, z, x, w, ref, scale, mine, own = kcase(name, m, n, d)
    start = np.full(hp.size, SENT) + np.arange(hp.size)
    got = call(ops, terms, hp, z, x, w, F64, accumulate, start)
    judge("%s m=%d n=%d d=%d %s" % (name, m, n, d, "acc" if accumulate else "set"), got, start, accumulate, ref, scale, mine, own)


def test_cross_grad_fp32(ops):
    terms, hp, z, x, w, ref, scale, mine, own = kcase("se+wn", 70, 150, 3, f32=True)
    start = np.full(hp.size, SENT)
    got = call(ops, terms, hp, z, x, w, F32, False, start)
    judge("se+wn fp32", got, start, False, ref, scale, mine, own)


@pytest.mark.parametrize("name", ["se+wn", "se*per"])
def test_cross_grad_on_one_point_set_with_a_symmetric_weight(ops, name):
    """X = Z, W = W^T: the Kuu part of the bound.  Also the sum kernel_ref.grad_terms gives on the one point set."""
    terms, hp, z, x, w, ref, scale, mine, own = kcase(name, 70, 70, 3, symmetric=True)
    sym = np.zeros_like(ref)
    for i, slab in kr.grad_terms(terms, hp, z):
        if mine[i]:
            sym[i] = np.sum(w * slab)
    assert np.max(np.abs(sym - ref)[mine] / scale[mine]) <= 4 * 2.0 ** -52
    start = np.full(hp.size, SENT)
    judge(name + " X = Z", call(ops, terms, hp, z, x, w, F64, False, start), start, False, ref, scale, mine, own)


def test_cross_grad_is_bit_reproducible_and_carries_a_nan(ops):
    terms, hp, z, x, w, ref, scale, mine, own = kcase("se+m52", 70, 150, 3)
    start = np.full(hp.size, SENT)
    a, b = (call(ops, terms, hp, z, x, w, F64, False, start) for _ in range(2))
    assert a.tobytes() == b.tobytes()
    xn = x.copy()
    xn[93, 1] = np.nan                                   # one coordinate of one column point: every entry sums over that column
    got = call(ops, terms, hp, z, xn, w, F64, False, start)
    assert np.isnan(got[mine]).all() and np.array_equal(got[~mine], start[~mine])


def test_cross_grad_refuses_bad_arguments_before_anything_is_enqueued(ops):
    terms, hp, z, x, w, *_ = kcase("se+wn", 70, 150, 3)
    lib, d = ops.lib, 3
    grad = dev(np.full(hp.size, SENT))
    zd, xd, wd, hpd = dev(z), dev(x), dev(w), dev(hp)
    work = torch.zeros(ops.kernel_cross_grad_worksize(70, 150, hp.size), dtype=F64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    q = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    good = spec_for(terms, d)

    def rc(spec=good, d_=d, wp=None, ldw=150, m=70, dtype=0):
        return lib.pg_kernel_cross_grad(ops.h, dtype, C.byref(spec) if spec is not None else None, q(hpd), q(zd), d, m, q(xd), d, 150, d_,
                                        q(wd) if wp is None else wp, ldw, q(grad), 0, q(work), st)

    bad_kind = spec_for(terms, d)
    bad_kind.kind[0] = 5
    too_many = spec_for(terms, d)
    too_many.ncomp = 9
    assert rc(d_=0) == -2 and b"PG_MAX_DIM" in lib.pg_last_error()
    assert rc(d_=65) == -2 and rc(m=-1) == -2
    assert rc(spec=bad_kind) == -1 and b"unknown kernel kind" in lib.pg_last_error()
    assert rc(spec=too_many) == -1 and rc(spec=None) == -1
    assert rc(wp=C.c_void_p(0)) == -1 and rc(ldw=149) == -1 and rc(dtype=3) == -1
    torch.cuda.synchronize()
    assert bool((grad == SENT).all())
    assert rc() == 0
    torch.cuda.synchronize()
    assert not bool((grad[:4] == SENT).any()) and float(grad[4]) == SENT


# ------------------------------------------------------------------------------------------- framed operands
def case_cross_grad(bed, name, m, n, d, accumulate):
    terms, hp, z, x, w, ref, scale, mine, own = kcase(name, m, n, d, f32=bed.dtype == F32)
    start = np.full(hp.size, SENT) + np.arange(hp.size)
    zf, xf, wf = bed.put("Z", z), bed.put("X", x), bed.put("W", w)
    hf = bed.put("hp", hp, dtype=F64)
    gf = bed.put("grad", start, dtype=F64, role="inout", written=mine)
    lw = int(bed.lib.pg_kernel_cross_grad_worksize(m, n, hp.size))
    assert lw == ((m + 63) // 64) * (((n + 63) // 64 + 3) // 4) * hp.size
    work = bed.put("work", shape=(lw,), dtype=F64, role="out", written=np.zeros(lw, bool), scratch=np.ones(lw, bool))
    spec = spec_for(terms, d)
    ok(bed, bed.lib.pg_kernel_cross_grad(bed.h, bed.code, C.byref(spec), p(hf), p(zf), zf.ld, m, p(xf), xf.ld, n, d, p(wf), wf.ld, p(gf),
                                         int(accumulate), p(work), bed.st()))
    want = ref + (start if accumulate else 0.0)
    return [("grad", np.where(mine, want, start), None, float(16 * own * scale[mine].max()), 0.0)]


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@gaps_odd
@pytest.mark.parametrize("name,m,n,d,accumulate", [("se+wn", 70, 150, 3, False), ("se*per", 70, 150, 3, True), ("rq", 1, 300, 17, False)])
def test_cross_grad_framed(ops, dtype, gapset, name, m, n, d, accumulate):
    run(ops, case_cross_grad, dtype, gapset, name=name, m=m, n=n, d=d, accumulate=accumulate)


# ------------------------------------------------------------------------------------------- the model
MODELS = {"se+wn": ["se", "wn"], "m32+rq+wn": ["m32", "rq", "wn"], "se*per+wn": [("se", "per"), "wn"]}


@functools.lru_cache(maxsize=None)
def mcase(name, n=700, m=90):
    """The problem, the restatement's answers and its own errors per quantity, computed once."""
    terms = MODELS[name]
    hp, x, y, z = sr.problem(terms, n=n, m=m)
    xp = np.random.default_rng(9).random((130, x.shape[1]))
    loss, grad = sr.loss_and_grad(terms, hp, x, y, z)
    mu, cov = sr.predict(terms, hp, x, y, z, xp, var="full")
    mu_d, cov_d = sr.predict_dense(terms, hp, x, y, z, xp)
    own = {"loss": sr.self_error(terms, hp, x, y, z), "mean": float(np.abs(mu - mu_d).max() / np.abs(mu_d).max()),
           "cov": float(np.abs(cov - cov_d).max() / np.abs(cov_d).max())}
    print("restatement's own error", name, own, "cond(Kuu) %.2e" % np.linalg.cond(sr.kuu_kuf(terms, hp, x, z)[0]))
    return terms, hp, x, y, z, xp, loss, grad, mu, cov, own


def hold(label, got, ref, own):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = float(np.abs(got - ref).max() / np.abs(ref).max())
    print("%-44s device %.2e  restatement %.2e  (bound %.2e)" % (label, err, own, sr.tol_of(own)))
    assert err <= sr.tol_of(own), (label, err, own)


def fit(name, **kw):
    terms, hp, x, y, z, xp, *_ = mcase(name, **kw)
    gp = pg.Sparse_GP(torch.from_numpy(x), torch.from_numpy(y), cov_of(terms), torch.from_numpy(z))
    gp.set_params(torch.from_numpy(hp))
    return gp


@pytest.mark.parametrize("chunk", [256, None], ids=["chunk256", "default"])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_model_against_the_restatement(ops, monkeypatch, name, chunk):
    """n = 700, m = 90, d = 3; chunk 256 walks three chunks, the last one ragged (188 columns); the default chunk holds all in one."""
    terms, hp, x, y, z, xp, loss, grad, mu, cov, own = mcase(name)
    if chunk is not None:
        monkeypatch.setattr(sparse_mod, "_SPARSE_CHUNK", chunk)
    gp = fit(name)
    got_l, got_g = pg.VFE(gp).loss_and_grad(hp.copy())
    tag = "%s %s " % (name, "chunk %s" % chunk if chunk else "one chunk")
    hold(tag + "loss", got_l, loss, own["loss"])
    hold(tag + "gradient", got_g, grad, own["loss"])
    hold(tag + "loss alone", pg.VFE(gp).loss(hp.copy()), loss, own["loss"])
    xpt = torch.from_numpy(xp)
    m1, vd = gp.predict(xpt, var="diag")
    m2, vf = gp.predict(xpt, var="full")
    hold(tag + "mean (diag call)", m1.numpy(), mu, own["mean"])
    hold(tag + "mean (full call)", m2.numpy(), mu, own["mean"])
    hold(tag + "variance", vd.numpy(), np.diag(cov), own["cov"])
    hold(tag + "covariance", vf.numpy(), cov, own["cov"])
    assert torch.equal(vf, vf.T) and gp.predict(xpt, var="none")[1] is NotImplemented


def test_chunked_and_unchunked_agree_to_rounding(ops, monkeypatch):
    terms, hp, *_ = mcase("se+wn")
    gp = fit("se+wn")
    l1, g1 = pg.VFE(gp).loss_and_grad(hp.copy())
    monkeypatch.setattr(sparse_mod, "_SPARSE_CHUNK", 256)
    l2, g2 = pg.VFE(gp).loss_and_grad(hp.copy())
    print("chunked vs one chunk: loss %.2e gradient %.2e" % (abs(l1 - l2) / abs(l1), np.abs(g1 - g2).max() / np.abs(g1).max()))
    # the same sums in another order: both within the model tolerance of the restatement, so within twice that of each other
    assert abs(l1 - l2) <= 2e-10 * abs(l1) and np.abs(g1 - g2).max() <= 2e-10 * np.abs(g1).max()


def test_bound_lies_above_the_exact_model(ops):
    terms, hp, x, y, z, *_ = mcase("se+wn")
    gp = fit("se+wn")
    exact = pg.Exact_GP(torch.from_numpy(x), torch.from_numpy(y), cov_of(terms))
    exact.set_params(torch.from_numpy(hp))
    vfe, mle = float(pg.VFE(gp).loss(hp.copy())), float(pg.MLE(exact).loss(hp.copy()))
    print("VFE %.6f  MLE %.6f  gap %.3e" % (vfe, mle, vfe - mle))
    assert vfe >= mle


def test_every_point_an_inducing_point_predicts_like_the_exact_model(ops):
    """z = x, n = m = 200 (module docstring): the device difference Sparse_GP - Exact_GP equals the restatements' difference."""
    terms = MODELS["se+wn"]
    rng = np.random.default_rng(5)
    hp = np.array([1.0, 2.6, 2.9, 2.7, 0.3])
    pool = rng.random((4000, 3))
    x = pool[sr.pick_z(pool, hp[1:4].min(), 200)]
    y = np.sin(3.0 * x.sum(1)) + 0.1 * rng.standard_normal(200)
    xp = rng.random((50, 3))
    assert np.linalg.cond(sr.kuu_kuf(terms, hp, x, x)[0]) <= 1e6
    mu_s, _ = sr.predict(terms, hp, x, y, x, xp)
    mu_d, _ = sr.predict_dense(terms, hp, x, y, x, xp)
    mu_e, _ = kr.predict(terms, hp, x, y, xp)
    own = float(np.abs(mu_s - mu_d).max() / np.abs(mu_d).max())
    gp = pg.Sparse_GP(torch.from_numpy(x), torch.from_numpy(y), cov_of(terms), torch.from_numpy(x.copy()))
    exact = pg.Exact_GP(torch.from_numpy(x), torch.from_numpy(y), cov_of(terms))
    for mdl in (gp, exact):
        mdl.set_params(torch.from_numpy(hp))
    got_s = gp.predict(torch.from_numpy(xp), var="diag")[0].numpy()
    got_e = exact.predict(torch.from_numpy(xp), var="diag")[0].numpy()
    scale = np.abs(mu_e).max()
    print("Sparse_GP - Exact_GP: device %.3e, restatements %.3e (the jitter on Kuu)" % (np.abs(got_s - got_e).max() / scale, np.abs(mu_s - mu_e).max() / scale))
    err = float(np.abs((got_s - got_e) - (mu_s - mu_e)).max() / scale)
    print("difference of the differences %.2e  restatement %.2e  (bound %.2e)" % (err, own, sr.tol_of(own)))
    assert err <= sr.tol_of(own)


def test_training_lowers_the_bound(ops, tmp_path, monkeypatch):
    """From init_params, i.e. sigma_n = 1e-4: Sigma = Kuu + Phi / sigma^2 then spans 1e12 and is numerically positive definite only
    while Phi itself is -- with unit length scales on the unit cube at m = 20 (smallest eigenvalue 4e2 against a rounding level of 7e-5),
    no longer at m = 90, where LAPACK's own factorisation of the restatement's Sigma fails too."""
    monkeypatch.chdir(tmp_path)                              # the optimiser writes its trace into the working directory
    gp = fit("se+wn", n=700, m=20)
    gp.set_params(gp.cov.init_params(gp.x))
    vfe = pg.VFE(gp)
    start = float(vfe.loss(gp.params.numpy().copy()))
    opt = pg.CG(vfe)
    opt.args.update(maxiter=6, disp=False)
    opt.minimize()
    end = float(vfe.loss(gp.params.numpy().copy()))
    print("CG(VFE): %.4f -> %.4f in %d iterations" % (start, end, opt.res.nit))
    assert np.isfinite(end) and end < start - 1.0


def test_failed_factorisation_raises_and_leaves_the_model_dirty(ops):
    terms, hp, x, y, z, *_ = mcase("se+wn")
    gp = fit("se+wn")
    zbad = z.copy()
    zbad[17, 2] = np.nan
    gp.z = torch.from_numpy(zbad)
    with pytest.raises(torch.linalg.LinAlgError):
        gp.update()
    assert gp.need_upd
    with pytest.raises(torch.linalg.LinAlgError):
        gp.predict(torch.from_numpy(x[:5]), var="diag")
    gp.z = torch.from_numpy(z)
    gp.update()
    assert not gp.need_upd
