"""NumPy restatement of pg_kernel_rowsq (include/pygpr_hip_rowsq.h) on tests/matmul_ref.stationary_kernel:

    out[i] = sum_j k(xr_i, xc_j)^2                        (cross form, no noise term)

`dtype=np.longdouble` evaluates the kernel, the squares and the sum in extended precision: the yardstick of the float64 form's own
error and the reference the device is held to.

Bound, derived and never fitted: with S_i = sum_j k_ij^2 (every term is non-negative, so the sum is its own scale) the device may miss
the longdouble figure by (32 own_K + (nc + 2) 2^-53) S_i -- tests/test_kmatmul_gpu.py's bound with the value's relative error, 16 own_K,
doubled by the square ((k (1 + e))^2 = k^2 (1 + 2 e + e^2)), and the any-order bound of a sum of nc products."""
import numpy as np

import matmul_ref as mr


def rowsq(terms, hp, xr, xc, dtype=np.float64):
    """out [nr] in `dtype`; an empty column range gives zeros."""
    xr, xc = np.asarray(xr), np.asarray(xc)
    if xc.shape[0] == 0:
        return np.zeros(xr.shape[0], dtype)
    k = mr.stationary_kernel(terms, hp, xr, xc, dtype)
    return np.sum(k * k, axis=1)


def bound_of(own, nc):
    """The relative allowance on S_i: own = matmul_ref.own_k of the case."""
    return 32 * own + (nc + 2) * 2.0 ** -53
