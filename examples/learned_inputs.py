"""Learn a linear input map through the marginal likelihood: x = raw @ M trained with torch.optim.Adam, the gradient dNLML/dx flowing
back into M through pygpr_amd.nlml_of_inputs (MLE.grad_x on an Exact_GP; a Stochastic_MLE on an Iterative_GP works the same way).

    python examples/learned_inputs.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pygpr_amd as pg  # noqa: E402

rng = np.random.default_rng(0)
raw = torch.from_numpy(rng.random((400, 6)))                       # six raw features, of which the target sees one direction
w_true = torch.tensor([1.0, -1.0, 0.5, 0.0, 0.0, 0.0], dtype=torch.float64)
y = torch.sin(4.0 * raw @ w_true) + 0.05 * torch.from_numpy(rng.standard_normal(400))

M = torch.nn.Parameter(torch.from_numpy(0.3 * rng.standard_normal((6, 1))))      # the map to learn: six features -> one input
model = pg.Exact_GP((raw @ M).detach(), y, pg.Compose([pg.Squared_exponential(), pg.White_noise()]))
model.set_params(torch.tensor([1.0, 1.0, 0.2], dtype=torch.float64))
params = model.params.clone().requires_grad_(True)                 # the hyper-parameters train beside the map
loss = pg.MLE(model)

opt = torch.optim.Adam([M, params], lr=0.05)
for step in range(60):
    opt.zero_grad()
    nlml = pg.nlml_of_inputs(loss, raw @ M, params)
    nlml.backward()
    opt.step()
    if step % 10 == 0 or step == 59:
        print("step %2d  NLML %9.3f" % (step, float(nlml.detach())))
direction = (M.detach()[:, 0] / M.detach()[:, 0].norm()).numpy()
print("learned direction", np.round(direction, 2), " true", np.round((w_true / w_true.norm()).numpy(), 2), "(up to sign)")
