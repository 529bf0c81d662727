"""NumPy restatement of the random-feature product (include/pygpr_hip_feature.h): the reference of tests/test_feature_matmul_gpu.py
and the feature matrix of tests/pathwise_ref.py.

    Phi[i][f] = cos(2 pi (x_i . nu_f + u_f)),        out = Phi W

The argument is taken in cycles and reduced as t - rint(t) before the product with 2 pi, as the device reduces it.
`dtype=np.longdouble` evaluates the features and the product in extended precision: the yardstick of the float64 restatement's own
error and the reference the device is held to."""
import numpy as np


def _two_pi(dtype):
    return 8 * np.arctan(dtype(1))


def phi(x, nu, u, dtype=np.float64):
    """The features [nr, nf] (no amplitude)."""
    x, nu, u = (np.asarray(a, dtype) for a in (x, nu, u))
    t = x @ nu.T + u[None, :]
    return np.cos(_two_pi(dtype) * (t - np.rint(t)))


def matmul(x, nu, u, w, dtype=np.float64):
    """(out, S): the product and its scale S_ic = sum_f |W_fc| -- the errors of Phi are absolute (|Phi| <= 1), so the scale of an entry
    is the one-norm of its column of W, the same for every row."""
    w = np.asarray(w, dtype)
    w2 = w[:, None] if w.ndim == 1 else w
    out = phi(x, nu, u, dtype) @ w2
    scale = np.broadcast_to(np.abs(w2).sum(0)[None, :], out.shape)
    return (out[:, 0], scale[:, 0]) if w.ndim == 1 else (out, scale)


def own_phi(x, nu, u):
    """The largest absolute float64-vs-longdouble difference of the restatement's Phi entries, floored at 2^-53."""
    if np.size(x) == 0 or np.size(u) == 0:
        return 2.0 ** -53
    p64, pld = phi(x, nu, u), phi(x, nu, u, np.longdouble)
    assert pld.dtype == np.longdouble
    return max(float(np.max(np.abs(p64 - pld))), 2.0 ** -53)
