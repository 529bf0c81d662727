"""NumPy restatement of the matrix-free covariance product (include/pygpr_hip_matmul.h) on top of tests/kernel_ref.py: the reference of
tests/test_kmatmul_gpu.py and the operator of tests/iterative_ref.py.

    cross      out = k(xr, xc) V                          (no noise term: kernel_ref's cross kernel)
    symmetric  out = k(x, x) V + (sum sigma_n^2 + jitter) V

`dtype=np.longdouble` evaluates the kernel and the product in extended precision: the yardstick of the float64 restatement's own error
and the reference the device is held to."""
import numpy as np

import kernel_ref as kr


def noise_offsets(terms, d):
    return [blocks[0][1] for t, blocks in kr._chunks(terms, d) if t == "wn"]


def shift_of(terms, hp, d, jitter=0.0, dtype=np.float64):
    hp = np.asarray(hp, dtype)
    s = dtype(0)
    for o in noise_offsets(terms, d):
        s = s + hp[o] ** 2
    return s + dtype(jitter)


def stationary_kernel(terms, hp, xr, xc, dtype=np.float64):
    """k(xr, xc) [nr, nc] without any noise term, also when xr is xc (the diagonal comes from a zero difference)."""
    return kr.kernel(terms, hp, np.asarray(xc), np.asarray(xr), dtype=dtype)


def matmul(terms, hp, xr, xc, v, jitter=0.0, dtype=np.float64):
    """(out, S): the product and its scale S_ic = sum_j |K_ij V_jc| (+ |shift V_ic|).  xc None: the symmetric form on xr."""
    v = np.asarray(v, dtype)
    v2 = v[:, None] if v.ndim == 1 else v
    sym = xc is None
    k = stationary_kernel(terms, hp, xr, xr if sym else xc, dtype)
    out = k @ v2
    scale = np.abs(k) @ np.abs(v2)
    if sym:
        s = shift_of(terms, hp, np.shape(xr)[1], jitter, dtype)
        out = out + s * v2
        scale = scale + np.abs(s * v2)
    return (out[:, 0], scale[:, 0]) if v.ndim == 1 else (out, scale)


def own_k(terms, hp, xr, xc):
    """The largest relative float64-vs-longdouble difference of the restatement's K entries, floored at 2^-53."""
    k64 = stationary_kernel(terms, hp, xr, xc)
    kld = stationary_kernel(terms, hp, xr, xc, np.longdouble)
    assert kld.dtype == np.longdouble
    nz = kld != 0
    err = float(np.max(np.abs(k64 - kld)[nz] / np.abs(kld)[nz])) if nz.any() else 0.0
    return max(err, 2.0 ** -53)
