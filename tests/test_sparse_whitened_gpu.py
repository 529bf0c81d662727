"""Sparse_GP(whitened=True) on the MI355X: loss, gradients (hyper-parameters and z), predictions and their derivatives in the test
points against the whitened NumPy restatement (tests/sparse_whitened_ref.py), chunked against unchunked, on the input the unwhitened
model cannot factor, with coincident inducing inputs, in training from init_params at m = 90, and on the failure path.

Tolerances (none is a guess; every comparison prints device, own and bound): the project's rule.  The device may miss the float64
restatement by sparse_ref.tol_of(own) = 50 x the restatement's own float64-vs-np.longdouble difference on that input, floored at
1e-10 -- loss, gradients, mean and the test-point derivatives relative to the largest reference entry, variance and covariance
relative to the PRIOR variance kss: the hard input's posterior variances go down to 5e-8, and the folded form's error of 7e-9 there
(tests/test_sparse_whitened_cpu.py) must not pass.

Inputs (sparse_whitened_ref.case): the easy ones are sparse_ref.problem on se + wn and on the product se * per + wn (n = 300,
m = 40, cond(Kuu) <= 1e6); the hard one is n = 300, m = 60, d = 3 at sigma_n = 1e-4 with cond(Kuu) 5e8, on which LAPACK fails to
factor the unwhitened Sigma (asserted here on the seed, with SciPy)."""
import numpy as np
import pytest
import torch

import pygpr_amd as pg
import sparse_ref as sr
import sparse_whitened_ref as wr
from kind_tools import cov_of, ops  # noqa: F401  (ops: the module's fixture)
from pygpr_amd import sparse as sparse_mod

pytestmark = pytest.mark.gpu

case, hold = wr.case, wr.hold


def model(name, whitened=True, z=None):
    terms, hp, x, y, z0, *_ = case(name)
    gp = pg.Sparse_GP(torch.from_numpy(x), torch.from_numpy(y), cov_of(terms), torch.from_numpy((z0 if z is None else z).copy()),
                      whitened=whitened)
    gp.set_params(torch.from_numpy(hp))
    return gp


def bound_and_gradients(name, tag):
    terms, hp, x, y, z, xp, ref, own = case(name)
    gp = model(name)
    loss, grad = pg.VFE(gp).loss_and_grad(hp.copy())
    hold(tag + "loss", loss, ref["loss"], own["loss"])
    hold(tag + "gradient", grad, ref["grad"], own["grad"])
    hold(tag + "loss alone", pg.VFE(gp).loss(hp.copy()), ref["loss"], own["loss"])
    vz = pg.VFE(gp, train_z=True)
    lz, gz = vz.loss_and_grad(vz.start_params())
    assert lz == loss and np.array_equal(gz[:hp.size], grad)           # the same evaluation with one more contraction
    hold(tag + "z gradient", gz[hp.size:].reshape(z.shape), ref["zgrad"], own["zgrad"])
    return gp


@pytest.mark.parametrize("chunk", [128, None], ids=["chunk128", "default"])
@pytest.mark.parametrize("name", wr.EASY + ["hard"])
def test_model_against_the_restatement(ops, monkeypatch, name, chunk):
    """n = 300: chunk 128 walks chunks of 128, 128 and 44 columns, the default chunk holds all in one."""
    if chunk is not None:
        monkeypatch.setattr(sparse_mod, "_SPARSE_CHUNK", chunk)
    terms, hp, x, y, z, xp, ref, own = case(name)
    tag = "%s %s " % (name, "chunk %s" % chunk if chunk else "one chunk")
    gp = bound_and_gradients(name, tag)
    assert gp.whitened is True
    xpt = torch.from_numpy(xp)
    kss = ref["kss"].max()
    m1, vd = gp.predict(xpt, var="diag")
    m2, vf = gp.predict(xpt, var="full")
    m3, none = gp.predict(xpt, var="none")
    hold(tag + "mean (diag call)", m1.numpy(), ref["mean"], own["mean"])
    hold(tag + "mean (full call)", m2.numpy(), ref["mean"], own["mean"])
    hold(tag + "mean (none call)", m3.numpy(), ref["mean"], own["mean"])
    hold(tag + "variance", vd.numpy(), ref["var"], own["var"], scale=kss)
    hold(tag + "covariance", vf.numpy(), ref["cov"], own["cov"], scale=kss)
    assert torch.equal(vf, vf.T) and none is NotImplemented
    mean, var, dmean, dvar = gp.predict_grad(xpt)
    assert torch.equal(mean, m1) and torch.equal(var, vd)
    for t in (dmean, dvar):
        assert t.shape == xp.shape and t.dtype == torch.float64 and t.device == xpt.device
    hold(tag + "d mean / dx*", dmean.numpy(), ref["dmean"], own["dmean"])
    hold(tag + "d var / dx*", dvar.numpy(), ref["dvar"], own["dvar"])
    two = gp.predict_grad(xpt, var="none")
    assert len(two) == 2 and torch.equal(two[0], m1)
    hold(tag + "d mean / dx* (var none)", two[1].numpy(), ref["dmean"], own["dmean"])


def test_chunked_and_unchunked_agree_to_rounding(ops, monkeypatch):
    terms, hp, x, y, z, *_ = case("se+wn")
    gp = model("se+wn")
    vz = pg.VFE(gp, train_z=True)
    l1, g1 = vz.loss_and_grad(vz.start_params())
    monkeypatch.setattr(sparse_mod, "_SPARSE_CHUNK", 128)
    vz = pg.VFE(gp, train_z=True)
    l2, g2 = vz.loss_and_grad(vz.start_params())
    (h1, z1), (h2, z2) = ((g[:hp.size], g[hp.size:]) for g in (g1, g2))
    print("chunked vs one chunk: loss %.2e gradient %.2e z gradient %.2e"
          % (abs(l1 - l2) / abs(l1), np.abs(h1 - h2).max() / np.abs(h1).max(), np.abs(z1 - z2).max() / np.abs(z1).max()))
    # the same sums in another order: both within the model tolerance (1e-10 here) of the restatement, so within twice that of each other
    assert abs(l1 - l2) <= 2e-10 * abs(l1) and np.abs(h1 - h2).max() <= 2e-10 * np.abs(h1).max()
    assert np.abs(z1 - z2).max() <= 2e-10 * np.abs(z1).max()


def test_the_hard_input_fails_unwhitened_and_not_whitened(ops):
    """cond(Kuu) 5e8 at sigma_n = 1e-4: Sigma = Kuu + Phi / sigma^2 is not numerically positive definite, D = I + Psi / sigma^2 is."""
    terms, hp, x, y, z, xp, ref, own = case("hard")
    print("cond(Kuu) %.2e, smallest eigenvalue of Sigma %.2e, of D %.4f" % wr.hard_preconditions(terms, hp, x, y, z))
    plain = model("hard", whitened=False)
    with pytest.raises(torch.linalg.LinAlgError):
        plain.update()
    assert plain.need_upd and plain.whitened is False
    with pytest.raises(torch.linalg.LinAlgError):
        pg.VFE(plain).loss(hp.copy())
    gp = model("hard")
    gp.update()
    assert not gp.need_upd
    hold("hard: loss where the unwhitened model raises", pg.VFE(gp).loss(hp.copy()), ref["loss"], own["loss"])


def test_two_coincident_inducing_inputs(ops):
    """z[1] = z[0] on the hard input: Kuu is singular but for JITTER, what a train_z line search can reach.  Finite, and within the
    tolerance of the restatement on that input."""
    bound_and_gradients("coincident", "z[1] = z[0] ")


def test_training_from_init_params_lowers_the_bound_at_m_90(ops, tmp_path, monkeypatch):
    """From cov.init_params (sigma_n = 1e-4) at n = 700, m = 90, six CG iterations: tests/test_sparse_gpu.py trains at m = 20 because
    the unwhitened Sigma cannot be factored at m = 90."""
    monkeypatch.chdir(tmp_path)                              # the optimiser writes its trace into the working directory
    terms = wr.TERMS["se+wn"]
    hp, x, y, z = sr.problem(terms, n=700, m=90)
    gp = pg.Sparse_GP(torch.from_numpy(x), torch.from_numpy(y), cov_of(terms), torch.from_numpy(z), whitened=True)
    gp.set_params(gp.cov.init_params(gp.x))
    vfe = pg.VFE(gp)
    start = float(vfe.loss(gp.params.numpy().copy()))
    opt = pg.CG(vfe)
    opt.args.update(maxiter=6, disp=False)
    opt.minimize()
    end = float(vfe.loss(gp.params.numpy().copy()))
    print("CG(VFE), whitened, m = 90: %.4f -> %.4f in %d iterations" % (start, end, opt.res.nit))
    assert np.isfinite(end) and end <= start - 1.0


def test_failed_factorisation_raises_and_leaves_the_model_dirty(ops):
    terms, hp, x, y, z, xp, ref, own = case("se+wn")
    gp = model("se+wn")
    zbad = z.copy()
    zbad[17, 2] = np.nan
    gp.z = torch.from_numpy(zbad)
    with pytest.raises(torch.linalg.LinAlgError):
        gp.update()
    assert gp.need_upd
    with pytest.raises(torch.linalg.LinAlgError):
        gp.predict(torch.from_numpy(x[:5]), var="diag")
    with pytest.raises(torch.linalg.LinAlgError):
        pg.VFE(gp).loss(hp.copy())
    gp.z = torch.from_numpy(z)
    gp.update()
    assert not gp.need_upd
    hold("mean after recovery", gp.predict(torch.from_numpy(xp), var="diag")[0].numpy(), ref["mean"], own["mean"])
