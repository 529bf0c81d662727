"""The marginal likelihood as a torch function of the training inputs: `nlml_of_inputs(loss, x, params)` returns the NLML as a scalar
tensor whose backward pass is `grad_x` (and `grad` in the hyper-parameters), so `x = net(raw)` trains through it with any torch optimiser
-- learned input maps (deep kernel learning, input warping), latent-variable models, input-noise corrections, the sensitivity of the fit
to a sensor position.  New, not in the reference; DESIGN 4.27.

Two losses carry a gradient in the training inputs: MLE on an Exact_GP (pg_kernel_xgrad against the dense weight) and Stochastic_MLE on an
Iterative_GP (pg_kernel_lowrank_xgrad against the probes' low-rank weight; an estimator, see pygpr_amd/stochastic.py).  Nothing here is
differentiated by autograd itself: the forward pass is one evaluation of the loss, the backward pass hands out what it computed."""
from typing import Optional

import numpy as np
import torch
from torch import Tensor

from .loss import MLE
from .stochastic import Stochastic_MLE


class _NLMLOfInputs(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, params: Tensor, loss) -> Tensor:
        model = loss.model
        model.x = x.detach()
        p = params.detach().cpu().numpy()
        if isinstance(loss, Stochastic_MLE):
            llhd, ghp, gx = loss.loss_and_grads(p)
        else:
            llhd, ghp = loss.loss_and_grad(p)
            gx = loss.grad_x(p)
        ctx.gx = torch.from_numpy(np.ascontiguousarray(gx)).to(device=x.device, dtype=x.dtype).reshape(x.shape)
        ctx.ghp = torch.from_numpy(np.ascontiguousarray(ghp)).to(device=params.device, dtype=params.dtype).reshape(params.shape)
        return torch.as_tensor(float(llhd), dtype=x.dtype, device=x.device)

    @staticmethod
    def backward(ctx, g: Tensor):
        gx = ctx.gx * g if ctx.needs_input_grad[0] else None
        ghp = ctx.ghp * g.to(device=ctx.ghp.device, dtype=ctx.ghp.dtype) if ctx.needs_input_grad[1] else None
        return gx, ghp, None


def nlml_of_inputs(loss, x: Tensor, params: Optional[Tensor] = None) -> Tensor:
    """The NLML of `loss.model` with its training inputs set to x [n, d], a scalar differentiable in x and -- when `params` is a tensor
    that requires grad -- in the hyper-parameters.  loss: an MLE on an Exact_GP or a Stochastic_MLE on an Iterative_GP; every other loss is
    refused.  The forward pass sets model.x = x.detach(), takes `params` (model.params when None) and evaluates once; the backward pass
    returns grad_x and the hyper-parameter gradient times the upstream scalar, on x's (params') device and dtype."""
    if type(loss) not in (MLE, Stochastic_MLE):
        raise NotImplementedError("nlml_of_inputs: %s has no gradient in the training inputs; use MLE on an Exact_GP or Stochastic_MLE on an "
                                  "Iterative_GP" % type(loss).__name__)
    if not (torch.is_tensor(x) and x.dim() == 2):
        raise NotImplementedError("nlml_of_inputs: x must be a tensor [n, d] (no batches)")
    if params is None:
        params = loss.model.params
    return _NLMLOfInputs.apply(x, params, loss)
