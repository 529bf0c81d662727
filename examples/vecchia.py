"""Nearest-neighbour (Vecchia) GP regression: linear in n, local detail kept (needs one GPU and the built library:
`python __graft_entry__.py`).

    python examples/vecchia.py
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pygpr_amd as PyGPR

torch.manual_seed(0)
n, d, q = 50000, 3, 2000
f = lambda t: torch.sin(4.0 * t[:, 0]) * torch.cos(3.0 * t[:, 1]) + t[:, 2]      # noqa: E731
x = torch.rand(n, d, dtype=torch.float64)
y = f(x) + 0.05 * torch.randn(n, dtype=torch.float64)
xs = torch.rand(q, d, dtype=torch.float64)

cov = PyGPR.Compose([PyGPR.Squared_exponential(), PyGPR.White_noise()])
# every point is conditioned on its 30 nearest predecessors in a random ordering; x and y stay in their own order
gp = PyGPR.Vecchia_GP(x, y, cov, neighbours=30, order="random", seed=0)
gp.set_params(torch.tensor([1.0] + [1.0] * d + [0.1], dtype=torch.float64))
loss = PyGPR.Vecchia_MLE(gp)
print("Vecchia loss before training: %.2f" % float(loss.loss(gp.params.numpy())))
opt = PyGPR.CG(loss)                 # the neighbour sets stay fixed while the parameters move: the loss is smooth
opt.args.update(maxiter=15, disp=False)
opt.minimize()
print("after %d evaluations: %.2f, params %s" % (opt.res.nfev, float(opt.res.fun), gp.params.numpy().round(3)))
gp.refresh_neighbours()              # search again in the metric of the trained length scales
gp.update()
print("loss with the refreshed neighbours: %.2f; largest conditional variance %.4f" % (gp.nlml, float(gp.cond_var.max())))
mean, var = gp.predict(xs, var="diag")
print("test RMSE %.4f, mean predictive std %.4f" % (float((mean.cpu() - f(xs)).pow(2).mean().sqrt()), float(var.sqrt().mean())))
if os.path.exists("opt.dat"):        # CG's callback log
    os.remove("opt.dat")
