"""pygpr_amd -- MI355X-native dense Gaussian-process hot path behind PyGPR's class surface
(reference export list: PyGPR/__init__.py:1-7; `get_learn_rate`, `Matern52`, `Matern32`, `Matern12`, `Rational_quadratic`, `Periodic`, `Product` and `GRBCM_MLE`
are added, and `LOO`, the leave-one-out loss, `PosteriorSampler` (Exact_GP.sampler), `randn`, the device normal generator,
and `Sparse_GP` with its loss `VFE`, the variational inducing-point model, with `select_inducing`, the greedy choice of its
inducing points, and the `Selection` it returns, and `Iterative_GP`, the matrix-free exact model, with the `NotConverged` its solver
raises, and `Stochastic_MLE`, the loss that trains it from probe vectors, and `FunctionSamples`, the pathwise function samples
`Iterative_GP.function_samples` returns, with `spectral_features`, the random Fourier features they are drawn from, and
`VarianceCache`, the cached variances with certified bounds `Iterative_GP.variance_cache` returns, and `nlml_of_inputs`, the marginal
likelihood as a torch function of the training inputs, and `Vecchia_GP` with its loss `Vecchia_MLE`, the nearest-neighbour model that
scales linearly in n)."""
from .gpr import GPR, Exact_GP, PosteriorSampler, randn
from .covar import Squared_exponential, Matern52, Matern32, Matern12, Rational_quadratic, Periodic, Product, Covar, Compose, White_noise
from .loss import Loss, MLE, LOO
from .sparse import Sparse_GP, VFE, Selection, select_inducing
from .iterative import Iterative_GP, NotConverged
from .stochastic import Stochastic_MLE
from .pathwise import FunctionSamples, spectral_features
from .varcache import VarianceCache
from .inputs import nlml_of_inputs
from .vecchia import Vecchia_GP, Vecchia_MLE
from .opt import Opt, CG, Nelder_Mead, BFGS_Quad, CG_Quad, hessian
from .gr_bcm import GRBCM, GRBCM_MLE, log_likelihood_batched
from .hp_update import get_learn_rate
from .scikit_model import SK_WRAP
from .sampler import UNIFORM, MATERN1, sample_gp, cluster_samples, euclidean_dist

__all__ = [
    "GPR", "Exact_GP", "Squared_exponential", "Matern52", "Matern32", "Matern12", "Rational_quadratic", "Periodic", "Product", "Covar", "Compose", "White_noise", "Loss", "MLE", "LOO", "Opt",
    "CG", "Nelder_Mead", "BFGS_Quad", "CG_Quad", "hessian", "GRBCM", "GRBCM_MLE", "get_learn_rate", "SK_WRAP",
    "UNIFORM", "MATERN1", "cluster_samples", "euclidean_dist", "sample_gp", "log_likelihood_batched", "PosteriorSampler", "randn",
    "Sparse_GP", "VFE", "select_inducing", "Selection", "Iterative_GP", "NotConverged", "Stochastic_MLE", "FunctionSamples", "spectral_features",
    "VarianceCache", "nlml_of_inputs", "Vecchia_GP", "Vecchia_MLE",
]
