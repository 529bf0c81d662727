"""NumPy restatement of pg_kernel_lowrank_grad: the contraction of a rank-r weight W = U V^T against the derivative slabs of
sparse_ref.cross_grad_terms, dense and in any NumPy precision.  Host only.

  cross form       grad[p] = sum_{i < nr, j < nc} W_ij dk(xr_i, xc_j)/dtheta_p
  symmetric form   xc None: the same sum over all ordered pairs of xr, the diagonal once

`scale` is the sum of the magnitudes that are added, S_p = sum_ij (sum_t |U_it| |V_jt|) |dk_ij/dtheta_p|: what an error of the
device is measured against."""
import numpy as np

import kernel_ref as kr
import sparse_ref as sr


def weight(u, v, dtype=np.float64):
    """W = U V^T formed in `dtype` (np.longdouble runs NumPy's own loops, not BLAS)."""
    return np.asarray(u, dtype) @ np.asarray(v, dtype).T


def lowrank_grad(terms, hp, xr, xc, u, v, dtype=np.float64):
    """grad over every stationary parameter (zero elsewhere), computed in `dtype`."""
    x = xr if xc is None else xc
    w = weight(u, v, dtype)
    out = np.zeros(np.size(hp), dtype)
    for i, slab in sr.cross_grad_terms(terms, hp, x, xr, dtype):
        assert slab.dtype == dtype and slab.shape == w.shape
        out[i] = np.sum(w * slab)
    return out


def scale(terms, hp, xr, xc, u, v):
    x = xr if xc is None else xc
    aw = np.abs(u) @ np.abs(v).T
    out = np.zeros(np.size(hp))
    for i, slab in sr.cross_grad_terms(terms, hp, x, xr):
        out[i] = np.sum(aw * np.abs(slab))
    return out


def mine(terms, d):
    """Boolean mask over hp: the entries of the stationary blocks (what the call writes)."""
    mask = np.zeros(kr.nhp_of(terms, d), bool)
    for t, blocks in kr._chunks(terms, d):
        if t != "wn":
            for _, a, b in blocks:
                mask[a:b] = True
    return mask


def component_masks(terms, d):
    """One boolean mask per stationary factor or summand: the entries of its own block."""
    out = []
    for t, blocks in kr._chunks(terms, d):
        if t != "wn":
            for _, a, b in blocks:
                m = np.zeros(kr.nhp_of(terms, d), bool)
                m[a:b] = True
                out.append(m)
    return out


def worksize(nr, nc, r, nhp):
    """The host arithmetic of pg_kernel_lowrank_grad_worksize: one slot row of nhp doubles per column tile, segment of the row tiles
    (at least four tiles, grown so that one pass has at most 32768 workgroups) and pass of 32 factor columns."""
    if min(nr, nc, r, nhp) < 0:
        return -1
    tr, tc, nch = -(-nr // 64), -(-nc // 64), -(-r // 32)
    if tr == 0 or tc == 0 or nch == 0:
        return 0
    tps = min(max(4, -(-(tr * tc) // 32768)), tr)
    return -(-tr // tps) * tc * nch * nhp
