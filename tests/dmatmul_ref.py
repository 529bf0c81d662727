"""NumPy restatement of the matrix-free product of the covariance's first-argument derivative (include/pygpr_hip_dmatmul.h) on top of
tests/kernel_ref.kernel_xgrad: the reference of tests/test_dmatmul_gpu.py and of the derivatives of Iterative_GP and FunctionSamples.

    out[i][k][c] = sum_j dk(xr_i, xc_j)/dxr_ik V[j][c]        (no noise term: a cross kernel; xc may hold xr's points)

`dtype=np.longdouble` evaluates the derivative and the product in extended precision: the yardstick of the float64 restatement's own
error and the reference the device is held to."""
import numpy as np

import kernel_ref as kr


def dkernel(terms, hp, xr, xc, dtype=np.float64):
    """dk(xr_i, xc_j)/dxr_ik as [d, nr, nc]."""
    return kr.kernel_xgrad(terms, hp, np.asarray(xc), np.asarray(xr), dtype=dtype)


def matmul_dx(terms, hp, xr, xc, v, dtype=np.float64):
    """(out [nr, d, nrhs], S [nr, d, nrhs]): the product and its scale S_ikc = sum_j |dK_ijk V_jc|.  A one-dimensional v counts as one
    column and both come back [nr, d]."""
    v = np.asarray(v, dtype)
    v2 = v[:, None] if v.ndim == 1 else v
    dk = dkernel(terms, hp, xr, xc, dtype)                     # [d, nr, nc]
    out = np.transpose(dk @ v2, (1, 0, 2))
    scale = np.transpose(np.abs(dk) @ np.abs(v2), (1, 0, 2))
    return (out[:, :, 0], scale[:, :, 0]) if v.ndim == 1 else (out, scale)


def own_dk(terms, hp, xr, xc):
    """The restatement's own error in dK: the largest float64-vs-longdouble difference of an entry RELATIVE TO THE LARGEST |dK| OF ITS ROW
    AND COORDINATE (max over j of |dK_ijk|), floored at 2^-53.  Not per entry: a derivative changes sign -- the periodic kind's
    sin(2 pi D / p) and every D_k pass through zero -- and an entry next to a zero crossing carries the absolute error of its
    neighbours, which a per-entry ratio would turn into an arbitrarily large figure.  The product's scale sum_j |dK_ijk V_jc| is made of
    the row's large entries, so this is the ratio the bound needs."""
    d64 = dkernel(terms, hp, xr, xc)
    dld = dkernel(terms, hp, xr, xc, np.longdouble)
    assert dld.dtype == np.longdouble
    big = np.max(np.abs(dld), axis=2, keepdims=True) if dld.shape[2] else np.zeros(dld.shape[:2] + (1,), np.longdouble)
    nz = np.broadcast_to(big != 0, dld.shape)
    err = float(np.max((np.abs(d64 - dld) / np.where(big != 0, big, 1))[nz])) if nz.any() else 0.0
    return max(err, 2.0 ** -53)
