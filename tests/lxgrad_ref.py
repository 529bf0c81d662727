"""NumPy restatement of the training-input contraction against a low-rank weight (include/pygpr_hip_lxgrad.h) on top of
tests/kernel_ref.kernel_xgrad, through tests/dmatmul_ref.dkernel: the reference of tests/test_lxgrad_gpu.py and of Stochastic_MLE.grad_x.

    cross (xc given):      out[i][k] = sum_j (U V^T)_ij dk(xr_i, xc_j)/dxr_ik
    symmetric (xc None):   out[i][k] = sum_j (U V^T + V U^T)_ij dk(xr_i, xr_j)/dxr_ik

`dtype=np.longdouble` evaluates the derivative, the weight and the sum in extended precision, as tests/dmatmul_ref.py does."""
import numpy as np

import dmatmul_ref as dr


def weight(u, v, sym, dtype=np.float64):
    """(Wt, |Wt| bound): U V^T (+ V U^T) and sum_t |U_it V_jt| (+ |V_it U_jt|)."""
    u, v = np.asarray(u, dtype), np.asarray(v, dtype)
    w, a = u @ v.T, np.abs(u) @ np.abs(v).T
    return (w + w.T, a + a.T) if sym else (w, a)


def lowrank_xgrad(terms, hp, xr, xc, u, v, dtype=np.float64):
    """(out [nr, d], S [nr, d]): the contraction and its scale S_ik = sum_j (sum_t |U_it V_jt| [+ |V_it U_jt|]) |dK_ijk|."""
    sym = xc is None
    dk = dr.dkernel(terms, hp, xr, xr if sym else xc, dtype)      # [d, nr, nc]
    w, a = weight(u, v, sym, dtype)
    return np.einsum("ij,kij->ik", w, dk), np.einsum("ij,kij->ik", a, np.abs(dk))


def worksize(nr, nc, d, r):
    """pg_kernel_lowrank_xgrad_worksize: pg_kernel_matmul's column segments at one right-hand side times the passes of 32 factor
    columns, one slab of 64-row tiles by chunks of coordinates (8, or 4 at d <= 4) each; 0 for one slab or none."""
    tiles_r, tiles_c = (nr + 63) // 64, (nc + 63) // 64
    nseg, tps = (1 if tiles_c > 0 else 0), tiles_c
    if 0 < tiles_r < 512 and tiles_c >= 8:
        s = min((512 + tiles_r - 1) // tiles_r, tiles_c // 4)
        tps = (tiles_c + s - 1) // s
        nseg = (tiles_c + tps - 1) // tps
    nslab = nseg * ((r + 31) // 32)
    kc = 4 if d <= 4 else 8
    return nslab * tiles_r * 64 * ((d + kc - 1) // kc) * kc if nslab > 1 and d >= 1 else 0
