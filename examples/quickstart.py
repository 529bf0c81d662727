"""Drop-in use of the MI355X path behind PyGPR's class surface (needs one GPU and the built library:
`python __graft_entry__.py`).  The only change from a PyGPR script is the import line.

    python examples/quickstart.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pygpr_amd as PyGPR          # instead of: import PyGPR

torch.manual_seed(0)
n, d, m = 2000, 4, 500
x = torch.rand(n, d, dtype=torch.float64)
y = torch.sin(-x.sum(-1)) + 0.05 * torch.randn(n, dtype=torch.float64)
xs = torch.rand(m, d, dtype=torch.float64)

# ---- exact GP: fit, hyper-parameter training with the stock CG driver, prediction
cov = PyGPR.Compose([PyGPR.Squared_exponential(), PyGPR.White_noise()])
gp = PyGPR.Exact_GP(x, y, cov)
gp.set_params(torch.tensor([1.0] + [1.0] * d + [0.1], dtype=torch.float64))
loss = PyGPR.MLE(gp)
print("NLML before training:", float(loss.loss(gp.params.numpy())))
opt = PyGPR.CG(loss)
opt.args.update(maxiter=20, disp=False)
opt.minimize()                       # scipy CG on loss.loss_and_grad; writes the optimum back into gp (prints
                                     # "Optimizer Failed" when it stops at maxiter, as the reference does: opt.py:61-65)
print("NLML after %d evaluations: %.4f" % (opt.res.nfev, float(opt.res.fun)))
mean, var = gp.predict(xs, var="diag")
print("test RMSE %.4f, mean predictive std %.4f" % (float((mean - torch.sin(-xs.sum(-1))).pow(2).mean().sqrt()),
                                                    float(var.sqrt().mean())))
loo_mean, loo_var = gp.loo_predict()   # leave-one-out check of the fit on its own data; PyGPR.LOO(gp) trains on that criterion
print("LOO standardised residuals: std %.3f (1 = calibrated), worst %.1f sigma" % (
    float(((y - loo_mean) / loo_var.sqrt()).std()), float(((y - loo_mean) / loo_var.sqrt()).abs().max())))

# ---- the locally periodic kernel, SE x Periodic (a seasonal shape that drifts), as one term of a sum: hp = the children's blocks in order
lp = PyGPR.Compose([PyGPR.Product([PyGPR.Squared_exponential(), PyGPR.Periodic()]), PyGPR.White_noise()])
gp_lp = PyGPR.Exact_GP(x, y, lp)
gp_lp.set_params(torch.tensor([1.0] + [0.5] * d + [1.0] + [1.0] * d + [2.0] * d + [0.1], dtype=torch.float64))
print("locally periodic kernel: NLML %.4f" % float(PyGPR.MLE(gp_lp).loss(gp_lp.params.numpy())))

# ---- grBCM committee: 4 local experts + a global communication set, shared hyper-parameters
nc, nls, ng = 4, 400, 200
xl, yl = x[: nc * nls].reshape(nc, nls, d), y[: nc * nls].reshape(nc, nls)
xg, yg = x[nc * nls: nc * nls + ng], y[nc * nls: nc * nls + ng]
committee = PyGPR.GRBCM(xl, yl, xg, yg, cov)
committee.set_params(gp.params)
mu_c, var_c = committee.predict(xs, var="diag")
print("committee vs exact GP: max |mean difference| %.4f" % float((mu_c - mean).abs().max()))

# ---- inducing-point regression: 64 inducing inputs chosen greedily among the training points (the point the others explain least,
#      again and again), hyper-parameters trained on the collapsed bound with the same CG driver, then chosen again at the trained ones
sgp = PyGPR.Sparse_GP.greedy(x, y, cov, 64, params=torch.tensor([1.0] + [1.0] * d + [0.1], dtype=torch.float64))
vfe = PyGPR.VFE(sgp)
opt_s = PyGPR.CG(vfe)
opt_s.args.update(maxiter=15, disp=False)
opt_s.minimize()
before = float(vfe.loss(sgp.params.numpy()))
picked = sgp.select_inducing()       # at the trained params; picked.trace is the bound's trace term after 1, 2, ... points: the curve to choose m by
print("sparse GP, m = 64: bound %.4f, %.4f after reselecting; prior variance left unexplained %.3f of %.1f" % (
    before, float(vfe.loss(sgp.params.numpy())), float(picked.trace[-1]), float(n * sgp.params[0] ** 2)))
mu_s, var_s = sgp.predict(xs, var="diag")
print("sparse GP test RMSE %.4f" % float((mu_s - torch.sin(-xs.sum(-1))).pow(2).mean().sqrt()))

# ---- the exact posterior without the n x n matrix: conjugate gradients on the fused covariance product, at the trained parameters
igp = PyGPR.Iterative_GP(x, y, cov, rank=64, tol=1e-10)
igp.set_params(gp.params)
print("iterative vs exact GP: max |mean difference| %.2e after %d CG iterations" % (
    float((igp.predict(xs, var="none")[0] - mean).abs().max()), igp.cg_info["iterations"]))

# ---- ... and trained there as well: the marginal likelihood and its gradient from 15 probe vectors (stochastic Lanczos quadrature on
# the solver's own coefficients), a few CG steps from the untrained start.  The estimate is noisy: slq_info says by how much.
igp.set_params(torch.tensor([1.0] + [1.0] * d + [0.1], dtype=torch.float64))
sloss = PyGPR.Stochastic_MLE(igp, probes=15, seed=0)
sopt = PyGPR.CG(sloss)
sopt.args.update(maxiter=6, disp=False)
sopt.minimize()
print("stochastic NLML after %d evaluations: %.2f +- %.2f (exact at the same parameters: %.2f; MLE's optimum: %.2f)" % (
    sopt.res.nfev, float(sloss.loss(igp.params.numpy())), sloss.slq_info["stderr"] / 2, float(loss.loss(igp.params.numpy())),
    float(opt.res.fun)))

# ---- ... and sampled: posterior functions by pathwise conditioning -- random Fourier features for the prior, ONE block solve for all
# samples, after which an evaluation anywhere is one cross product and one feature product (no further solve, nothing q x q)
igp.set_params(gp.params)
fs = igp.function_samples(n_samples=8, features=1024, seed=0)
draws = fs(xs)                      # [8, q] draws of the latent function: the same eight functions wherever they are evaluated
print("8 function samples (%d features, %d CG iterations): largest |sample mean - posterior mean| %.3f, largest sample sd %.3f" % (
    fs.frequencies.shape[0], fs.cg_info["iterations"], float((draws.mean(0) - mean).abs().max()), float(draws.std(0).max())))
slopes = fs.grad(xs)                # [8, q, d]: the same eight functions' derivatives in the test points (no solve either)
print("largest |d sample / d x*| %.3f; largest |d mean / d x*| %.3f" % (
    float(slopes.abs().max()), float(igp.predict_grad(xs, var="none")[1].abs().max())))

# ---- ... and its variances cached: a projection of A^-1 onto a block-Krylov space started from the preconditioner's factor, y and 64
# anchor points, built once; every variance afterwards is one cross product and no solve -- an upper bound, with a certified lower one
vc = igp.variance_cache(steps=2, anchors=xs[:64])
upper, lower = vc.variance(xs, bounds=True)
print("cached variances (rank %d, %d products): largest excess over the exact GP's %.2e, largest certified gap %.2e" % (
    vc.rank, vc.info["products"], float((upper - var).max()), float((upper - lower).max())))

# ---- scikit-learn facade
sk = PyGPR.SK_WRAP(PyGPR.Exact_GP(x, y, cov))
sk.model.set_params(gp.params)
print("R^2 on the test points: %.4f" % sk.score(xs, torch.sin(-xs.sum(-1))))
if os.path.exists("opt.dat"):       # CG's callback log (opt.py:69-78), as in the reference
    os.remove("opt.dat")
