"""Device-op layer: torch-ROCm tensors are only buffers + the current stream; every number is
produced by libpygpr_hip through the C ABI (include/pygpr_hip*.h).  No CPU path exists here:
`get_ops()` raises when the library or a GPU is missing."""
import atexit
import ctypes as C
import os

import torch

from . import _lib
from ._lib import PAD, PG_F32, PG_F64, CovSpec

JITTER = 1e-7  # PyGPR/gpr.py:68, loss.py:38,63,96


def pad_to(n, q=PAD):
    return ((int(n) + q - 1) // q) * q


def _code(dtype):
    if dtype == torch.float64:
        return PG_F64
    if dtype == torch.float32:
        return PG_F32
    raise TypeError("pygpr_amd computes in float64 or float32, got %s" % dtype)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class HipOps:
    """One per process (one process per GPU)."""

    def __init__(self):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("pygpr_amd needs a HIP device (MI355X); there is no CPU fallback")
        h = C.c_void_p()
        _lib.check(self.lib.pg_create(C.byref(h)), "pg_create")
        self.h = h
        self.device = torch.device("cuda", torch.cuda.current_device())
        # the library destroys live handles itself at process exit (capi.hip: C atexit registered by pg_create); closing
        # here as well releases the streams while torch's allocator is still up.  PG_NO_PY_ATEXIT=1 leaves it to the library
        # (used once to verify the library-side teardown under rocprofv3).
        if not os.environ.get("PG_NO_PY_ATEXIT"):
            atexit.register(self.close)

    def close(self):
        if getattr(self, "h", None) is not None:
            try:
                torch.cuda.synchronize()
            except Exception:
                pass
            self.lib.pg_destroy(self.h)
            self.h = None

    # -- helpers ------------------------------------------------------------------------------
    def _st(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def _call(self, name, *args):
        """lib.<name>(handle, *args); a non-zero status raises with the library's text under that name."""
        _lib.check(getattr(self.lib, name)(self.h, *args), name)

    def _chk(self, *ts):
        for t in ts:
            if t is None:
                continue
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError("device op needs contiguous CUDA tensors")

    def empty(self, *shape, dtype=torch.float64):
        return torch.empty(*shape, dtype=dtype, device=self.device)

    def zeros(self, *shape, dtype=torch.float64):
        return torch.zeros(*shape, dtype=dtype, device=self.device)

    def to_device(self, t, dtype=None):
        return t.detach().to(device=self.device, dtype=dtype if dtype is not None else t.dtype).contiguous()

    # -- covariance assembly ------------------------------------------------------------------
    def kernel_build(self, spec, hp, xr, xc, out, lower_only=False, jitter=0.0):
        """out[rows_pad, cols_pad] <- k(xr, xc) (xc None: symmetric + noise/jitter diagonal).  `spec` is one pg_covspec
        or the list of passes of a long Compose (make_specs): later passes accumulate."""
        self._chk(hp, xr, xc, out)
        assert hp.dtype == torch.float64
        nr, d = xr.shape
        nc = xc.shape[0] if xc is not None else nr
        for i, sp in enumerate(_passes(spec)):
            if i > 0 and xc is not None and sp.ncomp == 0:
                continue                      # a noise-only pass adds nothing to a cross build (covar.py:243)
            self._call("pg_kernel_build", _code(out.dtype), C.byref(sp), _p(hp), _p(xr), xr.stride(0), nr, _p(xc),
                       xc.stride(0) if xc is not None else 0, nc, d, int(lower_only), int(i > 0), float(jitter) if i == 0 else 0.0, _p(out),
                       out.stride(0), out.shape[0], out.shape[1], self._st())
        return out

    def kernel_build_batched(self, spec, hp_all, xr, xc_all, out_all, lower_only=False, jitter=0.0):
        """out_all[e] [rows_pad, cols_pad] <- k(xr_e, xc_e) for all experts in ONE launch (pg_kernel_build_batched): hp_all [nexp, nhp];
        xr [m, d] (every expert at the same row points) or [nexp, m, d]; xc_all [nexp | 1, n, d] (one leading entry: shared points), or
        None for symmetric builds on xr.  One pg_covspec only (no accumulate passes)."""
        passes = _passes(spec)
        assert len(passes) == 1
        self._chk(hp_all, xr, xc_all, out_all)
        assert hp_all.dtype == torch.float64 and out_all.dim() == 3
        nexp = out_all.shape[0]
        nr, d = xr.shape[-2], xr.shape[-1]
        xr_stride = xr.stride(0) if (xr.dim() == 3 and xr.shape[0] > 1) else 0
        if xc_all is not None:
            nc = xc_all.shape[-2]
            xc_stride = xc_all.stride(0) if (xc_all.dim() == 3 and xc_all.shape[0] > 1) else 0
            ldc = xc_all.stride(-2)
        else:
            nc, xc_stride, ldc = nr, 0, 0
        self._call("pg_kernel_build_batched", _code(out_all.dtype), C.byref(passes[0]), _p(hp_all), hp_all.stride(0) if hp_all.shape[0] > 1 else 0,
                   _p(xr), xr.stride(-2), xr_stride, nr, _p(xc_all), ldc, xc_stride, nc, d, int(lower_only), float(jitter), _p(out_all),
                   out_all.stride(1), out_all.stride(0), out_all.shape[1], out_all.shape[2], nexp, self._st())
        return out_all

    def kernel_grad_build(self, spec, hp, x, out):
        """out[nhp, n, n] <- dK/dtheta stack (public Covar.kernel_and_grad only)."""
        self._chk(hp, x, out)
        n, d = x.shape
        for sp in _passes(spec):              # passes write the slabs of different children
            self._call("pg_kernel_grad_build", _code(out.dtype), C.byref(sp), _p(hp), _p(x), x.stride(0), n, d, _p(out), self._st())
        return out

    def sqdist(self, xr, xc, out):
        """out[rows_pad, cols_pad] <- |xr_i - xc_j|^2 (xc None: xr against itself), direct differences:
        Squared_exponential.distance (covar.py:102-127) through the covariance tile kernel."""
        d = xr.shape[1]
        spec = make_spec([_lib.PG_KIND_SQDIST], [0], [])
        ones = torch.ones(d + 1, dtype=torch.float64, device=self.device)
        return self.kernel_build(spec, ones, xr, xc, out)

    # -- factorisation and solves -------------------------------------------------------------
    def potrf_worksize(self, n_pad, dtype):
        return int(self.lib.pg_potrf_worksize(_code(dtype), n_pad))

    def potrf_workspace(self, n_pad, dtype):
        return self.empty(self.potrf_worksize(n_pad, dtype), dtype=dtype)

    def potrf(self, a, invd, info):
        self._chk(a, invd, info)
        self._call("pg_potrf", _code(a.dtype), a.shape[0], _p(a), a.stride(0), _p(invd), _p(info), self._st())

    def build_factor(self, spec, hp, x, a, invd, info, minv=None, jitter=JITTER):
        """a <- k(x, x) + jitter I (lower tiles), then its Cholesky factor in place (and minv <- L^-1 if given): kernel_build
        folded into potrf / potrf_trtri -- the build of everything right of the first panel overlaps that panel's chain.  A
        Compose longer than one pg_covspec falls back to the separate calls."""
        passes = _passes(spec)
        if len(passes) != 1 or os.environ.get("PG_NO_FOLD"):
            self.kernel_build(spec, hp, x, None, a, lower_only=True, jitter=jitter)
            return self.potrf_trtri(a, invd, info, minv) if minv is not None else self.potrf(a, invd, info)
        self._chk(hp, x, a, invd, info, minv)
        assert hp.dtype == torch.float64
        n, d = x.shape
        self._call("pg_build_potrf_trtri", _code(a.dtype), C.byref(passes[0]), _p(hp), _p(x), x.stride(0), n, d, float(jitter), _p(a), a.stride(0),
                   a.shape[0], _p(invd), _p(info), _p(minv), minv.stride(0) if minv is not None else 0, self._st())

    def build_factor_batched(self, spec, hp_all, x_all, x_stride, a_all, invd_all, info_all, minv_all=None, jitter=JITTER):
        """The same for nexp experts of one size in ONE call (pg_build_potrf_trtri_batched): hp_all [nexp, nhp], x_all [nexp | 1, n, d]
        (x_stride = 0 shares the points), a_all [nexp, n_pad, n_pad], invd_all [nexp, pg_potrf_worksize], info_all [nexp] int32,
        minv_all [nexp, n_pad, n_pad] or None.  Every launch covers all experts; the flag-coupled chain where the batch is still
        latency-bound (experts of at least 2048 points, at most 24576 rows in all), the classic chain otherwise."""
        passes = _passes(spec)
        assert len(passes) == 1
        self._chk(hp_all, x_all, a_all, invd_all, info_all, minv_all)
        assert hp_all.dtype == torch.float64 and info_all.dtype == torch.int32
        nexp, n_pad = a_all.shape[0], a_all.shape[1]
        n, d = x_all.shape[-2], x_all.shape[-1]
        self._call("pg_build_potrf_trtri_batched", _code(a_all.dtype), C.byref(passes[0]), _p(hp_all), hp_all.stride(0), _p(x_all), x_all.stride(-2),
                   int(x_stride), n, d, float(jitter), _p(a_all), a_all.stride(1), a_all.stride(0), n_pad, _p(invd_all), invd_all.stride(0),
                   _p(info_all), _p(minv_all), minv_all.stride(1) if minv_all is not None else 0, minv_all.stride(0) if minv_all is not None else 0,
                   nexp, self._st())

    def potrf_trtri_batched(self, a_all, invd_all, info_all, minv_all=None):
        """Cholesky in place (+ minv_all <- L^-1) of nexp matrices that are already in a_all [nexp, n_pad, n_pad]: the batched call
        without a folded build (X = NULL)."""
        self._chk(a_all, invd_all, info_all, minv_all)
        assert info_all.dtype == torch.int32
        nexp, n_pad = a_all.shape[0], a_all.shape[1]
        self._call("pg_build_potrf_trtri_batched", _code(a_all.dtype), None, None, 0, None, 0, 0, n_pad, 0, 0.0, _p(a_all), a_all.stride(1),
                   a_all.stride(0), n_pad, _p(invd_all), invd_all.stride(0), _p(info_all), _p(minv_all),
                   minv_all.stride(1) if minv_all is not None else 0, minv_all.stride(0) if minv_all is not None else 0, nexp, self._st())

    def alpha_batched(self, minv_all, y_all, u_all, alpha_all, work_all):
        """alpha_e = minv_e^T (minv_e y_e) for all experts in three launches; y_all [nexp | 1, n_pad] (one row: shared targets),
        u_all [nexp, n_pad], work_all [nexp, (n_pad/256) n_pad]."""
        self._chk(minv_all, y_all, u_all, alpha_all, work_all)
        self._call("pg_alpha_batched", _code(minv_all.dtype), minv_all.shape[1], _p(minv_all), minv_all.stride(1), minv_all.stride(0), _p(y_all),
                   y_all.stride(0) if y_all.shape[0] > 1 else 0, _p(u_all), u_all.stride(0), _p(alpha_all), alpha_all.stride(0), _p(work_all),
                   work_all.stride(0), minv_all.shape[0], self._st())

    def alpha_nlml_batched(self, minv_all, y_all, u_all, alpha_all, work_all, n, out_all):
        """alpha_e and NLML_e for all experts (pg_alpha_nlml_batched): out_all [nexp, >= 1] float64 receives NLML_e in column 0."""
        self._chk(minv_all, y_all, u_all, alpha_all, work_all, None)
        assert out_all.dtype == torch.float64 and out_all.is_cuda
        self._call("pg_alpha_nlml_batched", _code(minv_all.dtype), int(n), minv_all.shape[1], _p(minv_all), minv_all.stride(1), minv_all.stride(0),
                   _p(y_all), y_all.stride(0) if y_all.shape[0] > 1 else 0, _p(u_all), u_all.stride(0), _p(alpha_all), alpha_all.stride(0),
                   _p(work_all), work_all.stride(0), _p(out_all), out_all.stride(0), minv_all.shape[0], self._st())

    def lauum_batched(self, minv_all, kinv_all):
        self._chk(minv_all, kinv_all)
        self._call("pg_lauum_batched", _code(minv_all.dtype), minv_all.shape[1], _p(minv_all), minv_all.stride(1), minv_all.stride(0), _p(kinv_all),
                   kinv_all.stride(1), kinv_all.stride(0), minv_all.shape[0], self._st())

    def nlml_grad_batched(self, spec, hp_all, x_all, x_stride, n, kinv_all, alpha_all, grad_all, work):
        """grad_all [nexp, >= nhp] (a view with row stride: e.g. outs[:, 1:]) <- every expert's gradient in two launches."""
        passes = _passes(spec)
        self._chk(hp_all, x_all, kinv_all, alpha_all, work)
        assert grad_all.dtype == torch.float64 and grad_all.is_cuda and grad_all.stride(-1) == 1
        nexp, nhp = kinv_all.shape[0], hp_all.shape[-1]
        for sp in passes:
            self._call("pg_nlml_grad_batched", _code(kinv_all.dtype), C.byref(sp), _p(hp_all), hp_all.stride(0), _p(x_all), x_all.stride(-2),
                       int(x_stride), int(n), x_all.shape[-1], _p(kinv_all), kinv_all.stride(1), kinv_all.stride(0), _p(alpha_all),
                       alpha_all.stride(0), _p(grad_all), grad_all.stride(0), nhp, _p(work), work.numel(), nexp, self._st())

    def potrf_trtri(self, a, invd, info, minv):
        """Cholesky in place + minv = L^-1, fused so that part of the inverse overlaps the factorisation's tail."""
        self._chk(a, invd, info, minv)
        self._call("pg_potrf_trtri", _code(a.dtype), a.shape[0], _p(a), a.stride(0), _p(invd), _p(info), _p(minv), minv.stride(0), self._st())

    def potrs_vec(self, chol, invd, y, x, work=None):
        if work is None:
            work = self.empty(self.lib.pg_potrs_vec_worksize(_code(chol.dtype), chol.shape[0]), dtype=chol.dtype)
        self._chk(chol, invd, y, x, work)
        self._call("pg_potrs_vec", _code(chol.dtype), chol.shape[0], _p(chol), chol.stride(0), _p(invd), _p(y), _p(x), _p(work), self._st())

    def potrs(self, chol, invd, b, minv=None, triangular_only=False):
        """x = K^-1 b (or L^-1 b) for a matrix right-hand side b [n_pad, nrhs_pad] (nrhs_pad a multiple of 128): pg_potrs / pg_trsm_lower."""
        n, nrhs = b.shape
        x = self.empty(n, nrhs, dtype=b.dtype)
        work = self.empty(self.lib.pg_potrs_worksize(_code(b.dtype), n, nrhs, int(minv is not None)), dtype=b.dtype)
        self._chk(chol, invd, b, minv, x, work)
        self._call("pg_trsm_lower" if triangular_only else "pg_potrs", _code(b.dtype), n, nrhs, _p(chol), chol.stride(0) if chol is not None else 0,
                   _p(invd), _p(minv), minv.stride(0) if minv is not None else 0, _p(b), b.stride(0), _p(x), x.stride(0), _p(work), self._st())
        return x

    def potri(self, chol, invd, kinv, work=None):
        """kinv(lower) = K^-1 from the factor (pg_trtri + pg_lauum in one call)."""
        n = chol.shape[0]
        if work is None:
            work = self.empty(n, n, dtype=chol.dtype)
        self._chk(chol, invd, kinv, work)
        self._call("pg_potri", _code(chol.dtype), n, _p(chol), chol.stride(0), _p(invd), _p(kinv), kinv.stride(0), _p(work), self._st())

    def logdet(self, chol, n, out):
        self._chk(chol, out)
        self._call("pg_logdet", _code(chol.dtype), int(n), _p(chol), chol.stride(0), _p(out), self._st())

    def trtri(self, chol, invd, minv):
        self._chk(chol, invd, minv)
        self._call("pg_trtri", _code(chol.dtype), chol.shape[0], _p(chol), chol.stride(0), _p(invd), _p(minv), minv.stride(0), self._st())

    def lauum(self, minv, kinv):
        self._chk(minv, kinv)
        self._call("pg_lauum", _code(minv.dtype), minv.shape[0], _p(minv), minv.stride(0), _p(kinv), kinv.stride(0), self._st())

    def trmv(self, minv, x, y, trans, work=None):
        self._chk(minv, x, y, work)
        self._call("pg_trmv", _code(minv.dtype), minv.shape[0], _p(minv), minv.stride(0), int(trans), _p(x), _p(y), _p(work), self._st())

    def chol_append_worksize(self, n_pad, k, dtype):
        return int(self.lib.pg_chol_append_worksize(_code(dtype), int(n_pad), int(k)))

    def chol_append(self, n, k, chol, invd, minv, kt, knn, y_new, u, alpha, work, info):
        """Condition the factor of n points on k <= 128 more (pg_chol_append): chol, invd, minv, u, alpha [n_pad] are updated in place
        when info[0] comes out 0 and left untouched otherwise; kt [>= k, n_pad] = k(x_new, x) (zero past n), knn [>= k, >= k] =
        k(x_new, x_new) + noise + jitter I, y_new [k]; work: chol_append_worksize elements.  Asynchronous: read info after a sync."""
        self._chk(chol, invd, minv, kt, knn, y_new, u, alpha, work, info)
        assert info.dtype == torch.int32
        n_pad = chol.shape[0]
        self._call("pg_chol_append", _code(chol.dtype), int(n), int(k), n_pad, _p(chol), chol.stride(0), _p(invd), _p(minv), minv.stride(0), _p(kt),
                   kt.stride(0), _p(knn), knn.stride(0), _p(y_new), _p(u), _p(alpha), _p(work), _p(info), self._st())

    def tril(self, a, n):
        self._chk(a)
        self._call("pg_tril", _code(a.dtype), n, _p(a), a.stride(0), self._st())

    # -- NLML ---------------------------------------------------------------------------------
    def nlml_value(self, chol, y, alpha, n, out):
        self._chk(chol, y, alpha, out)
        self._call("pg_nlml_value", _code(chol.dtype), n, _p(chol), chol.stride(0), _p(y), _p(alpha), _p(out), self._st())

    def alpha_nlml_async(self, chol, minv, y, u, alpha, work, n, out):
        """alpha = minv^T (minv y) and out[0] = NLML (out[1]: log det, scratch), overlapped with the next pg_lauum."""
        self._chk(chol, minv, y, u, alpha, work, out)
        assert out.dtype == torch.float64 and out.numel() >= 2
        self._call("pg_alpha_nlml_async", _code(chol.dtype), int(n), chol.shape[0], _p(chol), chol.stride(0), _p(minv), minv.stride(0), _p(y), _p(u),
                   _p(alpha), _p(work), _p(out), self._st())

    def nlml_grad_worksize(self, n, nhp):
        return self.lib.pg_nlml_grad_worksize(n, nhp)

    def nlml_grad(self, spec, hp, x, n, kinv, alpha, grad, work):
        self._chk(hp, x, kinv, alpha, grad, work)
        for sp in _passes(spec):              # each pass fills the gradient entries of its own children
            self._call("pg_nlml_grad", _code(kinv.dtype), C.byref(sp), _p(hp), _p(x), x.stride(0), n, x.shape[1], _p(kinv), kinv.stride(0), _p(alpha),
                       _p(grad), grad.numel(), _p(work), work.numel(), self._st())

    # -- leave-one-out (include/pygpr_hip_loo.h) ----------------------------------------------
    def loo_terms_worksize(self, n_pad):
        return int(self.lib.pg_loo_terms_worksize(int(n_pad)))

    def loo_terms(self, minv, alpha, y, n, c, mu, var, out, work):
        """c = diag(K^-1) from the column sums of squares of minv = L^-1, mu / var = the leave-one-out mean and variance of the n real
        points, out[0] = the LOO loss (fp64); work: loo_terms_worksize(n_pad) doubles."""
        self._chk(minv, alpha, y, c, mu, var, out, work)
        assert out.dtype == torch.float64 and work.dtype == torch.float64 and work.numel() >= self.loo_terms_worksize(minv.shape[0])
        self._call("pg_loo_terms", _code(minv.dtype), int(n), minv.shape[0], _p(minv), minv.stride(0), _p(alpha), _p(y), _p(c), _p(mu), _p(var),
                   _p(out), _p(work), self._st())

    def loo_weights(self, c, alpha, kinv, n, p, q):
        """kinv (full symmetric K^-1) -> S = K^-1 diag(sqrt(2 w)) in place, p / q = (alpha +- K^-1 v) / sqrt2 (pg_loo_weights)."""
        self._chk(c, alpha, kinv, p, q)
        self._call("pg_loo_weights", _code(kinv.dtype), int(n), _p(c), _p(alpha), _p(kinv), kinv.stride(0), _p(p), _p(q), self._st())

    def loo_fold(self, m, q, n):
        """m (lower triangle) += q q^T on the n real points (pg_loo_fold)."""
        self._chk(m, q)
        self._call("pg_loo_fold", _code(m.dtype), int(n), _p(m), m.stride(0), _p(q), self._st())

    # -- the inducing-point GP's contraction (include/pygpr_hip_sparse.h) --------------------------
    def kernel_cross_grad_worksize(self, m, n, nhp):
        return int(self.lib.pg_kernel_cross_grad_worksize(int(m), int(n), int(nhp)))

    def kernel_cross_grad(self, spec, hp, z, x, w, grad, accumulate=False, work=None):
        """grad[p] (+)= sum_ij w[i][j] dk(z_i, x_j)/dtheta_p for the parameters of the spec's stationary components
        (pg_kernel_cross_grad): z [m, d], x [n, d], w a 2-D device tensor or view with at least [m, n] and unit stride along a row, grad
        [nhp] float64; noise entries and entries outside the spec keep their bits.  One pg_covspec only.  work: kernel_cross_grad_worksize
        doubles, allocated when None."""
        (sp,) = _passes(spec)
        self._chk(hp, z, x, grad, work)
        m, d = z.shape
        n = x.shape[0]
        if not (w.is_cuda and w.dim() == 2 and w.stride(1) == 1 and w.shape[0] >= m and w.shape[1] >= n and w.dtype == z.dtype == x.dtype):
            raise ValueError("kernel_cross_grad needs w [>= m, >= n] on the device in the points' dtype, unit stride along a row")
        assert hp.dtype == torch.float64 and grad.dtype == torch.float64 and x.shape[1] == d
        if work is None:
            work = self.empty(max(1, self.kernel_cross_grad_worksize(m, n, grad.numel())), dtype=torch.float64)
        assert work.dtype == torch.float64 and work.numel() >= self.kernel_cross_grad_worksize(m, n, grad.numel())
        self._call("pg_kernel_cross_grad", _code(w.dtype), C.byref(sp), _p(hp), _p(z), z.stride(0), m, _p(x), x.stride(0), n, d, _p(w),
                   w.stride(0), _p(grad), int(bool(accumulate)), _p(work), self._st())
        return grad

    # -- greedy inducing-point selection (include/pygpr_hip_select.h) ----------------------------
    def greedy_select_worksize(self, n, m_max):
        return int(self.lib.pg_greedy_select_worksize(int(n), int(m_max)))

    def greedy_select(self, spec, hp, x, m_max, floor, work=None, out=None):
        """Up to m_max pivots of x [n, d] (float64) by largest residual prior variance under the spec's stationary components
        (pg_greedy_select; the spec's noise entries are ignored).  Returns device tensors (piv [m_max] int32, count [1] int32, trace
        [m_max], resid [n]); piv and trace hold their results in [0, count) and are not touched behind it.  Asynchronous: read count
        after a sync.  One pg_covspec only.  work: greedy_select_worksize doubles (8 n m_max bytes and a little), allocated when None;
        out: the four outputs as contiguous device tensors of at least those lengths, allocated when None."""
        (sp,) = _passes(spec)
        self._chk(hp, work)
        if not (x.is_cuda and x.dim() == 2 and x.stride(1) == 1 and x.dtype == torch.float64):
            raise ValueError("greedy_select needs x [n, d] float64 on the device, unit stride along a row")
        assert hp.dtype == torch.float64
        n, d = x.shape
        m_max = int(m_max)
        size = self.greedy_select_worksize(n, m_max)
        if size < 0:
            raise ValueError("greedy_select: 0 <= m_max <= n, got m_max = %d, n = %d" % (m_max, n))
        if work is None:
            work = self.empty(size, dtype=torch.float64)
        assert work.dtype == torch.float64 and work.numel() >= size
        if out is None:
            out = (torch.empty(max(m_max, 1), dtype=torch.int32, device=self.device), torch.empty(1, dtype=torch.int32, device=self.device),
                   self.empty(max(m_max, 1), dtype=torch.float64), self.empty(max(n, 1), dtype=torch.float64))
        piv, count, trace, resid = out
        self._chk(piv, count, trace, resid)
        assert piv.dtype == count.dtype == torch.int32 and trace.dtype == resid.dtype == torch.float64
        assert piv.numel() >= m_max and count.numel() >= 1 and trace.numel() >= m_max and resid.numel() >= n
        self._call("pg_greedy_select", PG_F64, C.byref(sp), _p(hp), _p(x), x.stride(0), n, d, m_max, float(floor), _p(piv), _p(count),
                   _p(trace), _p(resid), _p(work), self._st())
        return piv[:m_max], count, trace[:m_max], resid[:n]

    # -- the matrix-free covariance product (include/pygpr_hip_matmul.h) --------------------------
    def kernel_matmul_worksize(self, nr, nc, nrhs):
        return int(self.lib.pg_kernel_matmul_worksize(int(nr), int(nc), int(nrhs)))

    def kernel_matmul(self, spec, hp, xr, xc, v, out=None, jitter=0.0, work=None):
        """out[i][c] = sum_j k(xr_i, xc_j) v[j][c] without forming k (pg_kernel_matmul); xc None: the symmetric operator on xr,
        k(xr, xr) v + (sum sigma_n^2 + jitter) v.  xr [nr, d], xc [nc, d] float64 device tensors or views with unit stride along a row;
        v [nc, nrhs] and out [nr, nrhs] likewise (a one-dimensional v counts as one column, and out comes back one-dimensional);
        out is allocated when None.  One pg_covspec only.  work: kernel_matmul_worksize doubles, allocated when None and needed."""
        (sp,) = _passes(spec)
        self._chk(hp, work)
        vec = v.dim() == 1
        v2 = v.unsqueeze(1) if vec else v
        nr, d = xr.shape
        nc = xc.shape[0] if xc is not None else nr
        nrhs = v2.shape[1]
        if out is None:
            out = self.empty(nr, dtype=torch.float64) if vec else self.empty(nr, nrhs, dtype=torch.float64)
        o2 = out.unsqueeze(1) if out.dim() == 1 else out
        for name, t, shape in (("xr", xr, (nr, d)), ("xc", xc, (nc, d)), ("v", v2, (nc, nrhs)), ("out", o2, (nr, nrhs))):
            if t is None:
                continue
            if not (t.is_cuda and t.dim() == 2 and tuple(t.shape) == shape and t.dtype == torch.float64 and (t.stride(1) == 1 or t.shape[1] <= 1)):
                raise ValueError("kernel_matmul needs %s %s float64 on the device, unit stride along a row" % (name, list(shape)))
        assert hp.dtype == torch.float64

        def ld(t, width):      # (a matrix of one row or none has no row stride to speak of)
            return max(int(t.stride(0)), width, 1) if t.shape[0] > 1 else max(width, 1)

        size = self.kernel_matmul_worksize(nr, nc, nrhs)
        if work is None and size > 0:
            work = self.empty(size, dtype=torch.float64)
        assert size == 0 or (work.dtype == torch.float64 and work.numel() >= size)
        xcp = _p(xc) if xc is None or nc > 0 else _p(hp)      # (an empty tensor has a null address, which would read as the symmetric form)
        self._call("pg_kernel_matmul", PG_F64, C.byref(sp), _p(hp), _p(xr), ld(xr, d), nr, xcp, ld(xc, d) if xc is not None else 0, nc, d,
                   _p(v2), ld(v2, nrhs), nrhs, float(jitter), _p(o2), ld(o2, nrhs), _p(work), self._st())
        return out

    # -- the derivative's matrix-free product (include/pygpr_hip_dmatmul.h) ------------------------
    def kernel_matmul_dx_worksize(self, nr, nc, d, nrhs):
        return int(self.lib.pg_kernel_matmul_dx_worksize(int(nr), int(nc), int(d), int(nrhs)))

    def kernel_matmul_dx(self, spec, hp, xr, xc, v, out=None, work=None):
        """out[i][k][c] = sum_j dk(xr_i, xc_j)/dxr_ik v[j][c] without forming dk (pg_kernel_matmul_dx; cross form only: xc may be xr).
        xr [nr, d], xc [nc, d] float64 device tensors or views with unit stride along a row, v [nc, nrhs] likewise; out [nr, d, nrhs]
        with unit stride along its last dimension (a one-dimensional v counts as one column, and out is [nr, d] then); out is
        allocated when None.  One pg_covspec only.  work: kernel_matmul_dx_worksize doubles, allocated when None and needed."""
        (sp,) = _passes(spec)
        self._chk(hp, work)
        if xc is None:
            raise ValueError("kernel_matmul_dx has a cross form only: pass xc (it may be xr)")
        vec = v.dim() == 1
        v2 = v.unsqueeze(1) if vec else v
        nr, d = xr.shape
        nc = xc.shape[0]
        nrhs = v2.shape[1]
        if out is None:
            out = self.empty(nr, d, dtype=torch.float64) if vec else self.empty(nr, d, nrhs, dtype=torch.float64)
        o3 = out.unsqueeze(2) if out.dim() == 2 and vec else out
        for name, t, shape in (("xr", xr, (nr, d)), ("xc", xc, (nc, d)), ("v", v2, (nc, nrhs))):
            if not (t.is_cuda and t.dim() == 2 and tuple(t.shape) == shape and t.dtype == torch.float64 and (t.stride(1) == 1 or t.shape[1] <= 1)):
                raise ValueError("kernel_matmul_dx needs %s %s float64 on the device, unit stride along a row" % (name, list(shape)))
        if not (o3.is_cuda and o3.dim() == 3 and tuple(o3.shape) == (nr, d, nrhs) and o3.dtype == torch.float64
                and (o3.stride(2) == 1 or nrhs <= 1)):
            raise ValueError("kernel_matmul_dx needs out %s float64 on the device, unit stride along its last dimension" % [nr, d, nrhs])
        assert hp.dtype == torch.float64

        def ld(t, width):      # (a matrix of one row or none has no row stride to speak of)
            return max(int(t.stride(0)), width, 1) if t.shape[0] > 1 else max(width, 1)

        ldk = max(int(o3.stride(1)), nrhs, 1) if d > 1 else max(nrhs, 1)
        ldo = max(int(o3.stride(0)), d * ldk) if nr > 1 else d * ldk
        size = self.kernel_matmul_dx_worksize(nr, nc, d, nrhs)
        if work is None and size > 0:
            work = self.empty(size, dtype=torch.float64)
        assert size == 0 or (work.dtype == torch.float64 and work.numel() >= size)
        xcp = _p(xc) if nc > 0 else _p(hp)      # (an empty tensor has a null address, which the library refuses: it has no symmetric form)
        self._call("pg_kernel_matmul_dx", PG_F64, C.byref(sp), _p(hp), _p(xr), ld(xr, d), nr, xcp, ld(xc, d), nc, d, _p(v2), ld(v2, nrhs), nrhs,
                   _p(o3), ldo, ldk, _p(work), self._st())
        return out

    # -- the cross-covariance's squared row norms (include/pygpr_hip_rowsq.h) ----------------------
    def kernel_rowsq_worksize(self, nr, nc):
        return int(self.lib.pg_kernel_rowsq_worksize(int(nr), int(nc)))

    def kernel_rowsq(self, spec, hp, xr, xc, out=None, work=None):
        """out[i] = sum_j k(xr_i, xc_j)^2 without forming k (pg_kernel_rowsq; cross form only: xc may be xr, no noise term).  xr [nr, d],
        xc [nc, d] float64 device tensors or views with unit stride along a row; out [nr] float64 on the device at any stride, allocated
        when None.  One pg_covspec only.  work: kernel_rowsq_worksize doubles, allocated when None and needed."""
        (sp,) = _passes(spec)
        self._chk(hp, work)
        if xc is None:
            raise ValueError("kernel_rowsq has a cross form only: pass xc (it may be xr)")
        nr, d = xr.shape
        nc = xc.shape[0]
        if out is None:
            out = self.empty(nr, dtype=torch.float64)
        for name, t, shape in (("xr", xr, (nr, d)), ("xc", xc, (nc, d))):
            if not (t.is_cuda and t.dim() == 2 and tuple(t.shape) == shape and t.dtype == torch.float64 and (t.stride(1) == 1 or t.shape[1] <= 1)):
                raise ValueError("kernel_rowsq needs %s %s float64 on the device, unit stride along a row" % (name, list(shape)))
        if not (out.is_cuda and out.dim() == 1 and out.shape[0] == nr and out.dtype == torch.float64 and (nr <= 1 or out.stride(0) >= 1)):
            raise ValueError("kernel_rowsq needs out %s float64 on the device" % [nr])
        assert hp.dtype == torch.float64

        def ld(t, width):      # (a matrix of one row or none has no row stride to speak of)
            return max(int(t.stride(0)), width, 1) if t.shape[0] > 1 else max(width, 1)

        size = self.kernel_rowsq_worksize(nr, nc)
        if work is None and size > 0:
            work = self.empty(size, dtype=torch.float64)
        assert size == 0 or (work.dtype == torch.float64 and work.numel() >= size)
        xcp = _p(xc) if nc > 0 else _p(hp)      # (an empty tensor has a null address, which the library refuses: it has no symmetric form)
        self._call("pg_kernel_rowsq", PG_F64, C.byref(sp), _p(hp), _p(xr), ld(xr, d), nr, xcp, ld(xc, d), nc, d, _p(out),
                   int(out.stride(0)) if nr > 1 else 1, _p(work), self._st())
        return out

    # -- the nearest-neighbour GP (include/pygpr_hip_vecchia.h) -------------------------------------
    @staticmethod
    def _rows(name, t, shape, dtype=torch.float64):
        if not (t.is_cuda and t.dim() == 2 and tuple(t.shape) == tuple(shape) and t.dtype == dtype and (t.stride(1) == 1 or t.shape[1] <= 1)):
            raise ValueError("%s must be %s %s on the device, unit stride along a row" % (name, list(shape), dtype))
        return max(int(t.stride(0)), int(shape[1]), 1) if t.shape[0] > 1 else max(int(shape[1]), 1)

    def knn(self, xq, xc, m, s=None, causal=False, out=None):
        """out[i] = the up to m nearest candidates of xc [n, d] for query xq[i] (pg_knn): int32 [q, m], ordered by (scaled squared
        distance, index), -1 in unfilled slots.  s [d]: per-coordinate scales (None: ones).  causal: candidates of query i are j < i
        (xq is then xc or its leading rows)."""
        q, d = xq.shape
        n = xc.shape[0]
        ldq, ldc = self._rows("xq", xq, (q, d)), self._rows("xc", xc, (n, d))
        if out is None:
            out = self.empty(q, int(m), dtype=torch.int32)
        ldn = self._rows("out", out, (q, int(m)), torch.int32)
        if s is not None:
            self._chk(s)
            assert s.dtype == torch.float64 and s.numel() == d
        self._call("pg_knn", PG_F64, _p(xq), ldq, q, _p(xc), ldc, n, d, _p(s), int(m), int(bool(causal)), _p(out), ldn, self._st())
        return out

    def vecchia_nlml_grad_worksize(self, count, d, nhp):
        return int(self.lib.pg_vecchia_nlml_grad_worksize(int(count), int(d), int(nhp)))

    def vecchia_nlml_grad(self, spec, hp, x, y, nbr, first, count, jitter, want_grad, cmean, cvar, out, grad, info, work=None):
        """The conditional terms of targets first .. first + count - 1 (pg_vecchia_nlml_grad): cmean / cvar [count], out [1] the loss
        summed over them, grad [nhp] its gradient (want_grad), info [1] int32.  nbr [count, m] int32: row t holds the neighbours of
        point first + t (indices into x, -1 padding).  One pg_covspec only."""
        (sp,) = _passes(spec)
        self._chk(hp, y, cmean, cvar, out, grad, info, work)
        n, d = x.shape
        m = nbr.shape[1]
        ldx, ldn = self._rows("x", x, (n, d)), self._rows("nbr", nbr, (int(count), m), torch.int32)
        nhp = hp.numel()
        size = self.vecchia_nlml_grad_worksize(count, d, nhp)
        if work is None:
            work = self.empty(max(size, 1), dtype=torch.float64)
        assert work.dtype == torch.float64 and work.numel() >= size and hp.dtype == torch.float64
        self._call("pg_vecchia_nlml_grad", PG_F64, C.byref(sp), _p(hp), nhp, _p(x), ldx, n, d, _p(y), _p(nbr), ldn, m, int(first), int(count),
                   float(jitter), int(bool(want_grad)), _p(cmean), _p(cvar), _p(out), _p(grad), _p(info), _p(work), self._st())

    def vecchia_predict_worksize(self, q, d):
        return int(self.lib.pg_vecchia_predict_worksize(int(q), int(d)))

    def vecchia_predict(self, spec, hp, x, y, xq, nbr, jitter, mean, var, info, work=None):
        """mean / var [q] of the q points xq, each conditioned on row t of nbr [q, m] (indices into x; pg_vecchia_predict).  var may be
        None."""
        (sp,) = _passes(spec)
        self._chk(hp, y, mean, var, info, work)
        n, d = x.shape
        q, m = nbr.shape
        ldx, ldq = self._rows("x", x, (n, d)), self._rows("xq", xq, (q, d))
        ldn = self._rows("nbr", nbr, (q, m), torch.int32)
        size = self.vecchia_predict_worksize(q, d)
        if work is None:
            work = self.empty(max(size, 1), dtype=torch.float64)
        assert work.dtype == torch.float64 and work.numel() >= size and hp.dtype == torch.float64
        self._call("pg_vecchia_predict", PG_F64, C.byref(sp), _p(hp), _p(x), ldx, n, d, _p(y), _p(xq), ldq, q, _p(nbr), ldn, m, float(jitter),
                   _p(mean), _p(var), _p(info), _p(work), self._st())

    # -- the random-feature product (include/pygpr_hip_feature.h) ----------------------------------
    def feature_matmul_worksize(self, nr, nf, nrhs):
        return int(self.lib.pg_feature_matmul_worksize(int(nr), int(nf), int(nrhs)))

    def feature_matmul(self, x, nu, u, w, out=None, work=None):
        """out[i][c] = sum_f cos(2 pi (x_i . nu_f + u_f)) w[f][c] without forming the features (pg_feature_matmul).  x [nr, d],
        nu [nf, d] (cycles per unit), w [nf, nrhs] and out [nr, nrhs] float64 device tensors or views with unit stride along a row,
        u [nf] (cycles) contiguous; a one-dimensional w counts as one column, and out comes back one-dimensional; out is allocated
        when None.  work: feature_matmul_worksize doubles, allocated when None and needed."""
        self._chk(work)
        vec = w.dim() == 1
        w2 = w.unsqueeze(1) if vec else w
        nr, d = x.shape
        nf = nu.shape[0]
        nrhs = w2.shape[1]
        if out is None:
            out = self.empty(nr, dtype=torch.float64) if vec else self.empty(nr, nrhs, dtype=torch.float64)
        o2 = out.unsqueeze(1) if out.dim() == 1 else out
        for name, t, shape in (("x", x, (nr, d)), ("nu", nu, (nf, d)), ("w", w2, (nf, nrhs)), ("out", o2, (nr, nrhs))):
            if not (t.is_cuda and t.dim() == 2 and tuple(t.shape) == shape and t.dtype == torch.float64 and (t.stride(1) == 1 or t.shape[1] <= 1)):
                raise ValueError("feature_matmul needs %s %s float64 on the device, unit stride along a row" % (name, list(shape)))
        if not (u.is_cuda and u.dim() == 1 and u.shape[0] == nf and u.dtype == torch.float64 and (nf <= 1 or u.stride(0) == 1)):
            raise ValueError("feature_matmul needs u [%d] float64 on the device, contiguous" % nf)

        def ld(t, width):      # (a matrix of one row or none has no row stride to speak of)
            return max(int(t.stride(0)), width, 1) if t.shape[0] > 1 else max(width, 1)

        size = self.feature_matmul_worksize(nr, nf, nrhs)
        if work is None and size > 0:
            work = self.empty(size, dtype=torch.float64)
        assert size == 0 or (work.dtype == torch.float64 and work.numel() >= size)
        self._call("pg_feature_matmul", PG_F64, _p(x), ld(x, d), nr, _p(nu), ld(nu, d), nf, d, _p(u), _p(w2), ld(w2, nrhs), nrhs, _p(o2),
                   ld(o2, nrhs), _p(work), self._st())
        return out

    # -- the low-rank gradient contraction (include/pygpr_hip_lowrank.h) --------------------------
    def kernel_lowrank_grad_worksize(self, nr, nc, r, nhp):
        return int(self.lib.pg_kernel_lowrank_grad_worksize(int(nr), int(nc), int(r), int(nhp)))

    def kernel_lowrank_grad(self, spec, hp, xr, xc, u, v, grad=None, accumulate=False, work=None):
        """grad[p] (+)= sum_ij (sum_t u[i][t] v[j][t]) dk(xr_i, xc_j)/dtheta_p for the parameters of the spec's stationary components,
        the weight never formed (pg_kernel_lowrank_grad); xc None: all ordered pairs of xr, the diagonal once.  xr [nr, d], xc [nc, d],
        u [nr, r], v [nc, r] (r <= 64) float64 device tensors or views with unit stride along a row; grad [nhp] float64 (zeros of hp's
        length when None); noise entries and entries outside the spec keep their bits.  One pg_covspec only.  work:
        kernel_lowrank_grad_worksize doubles, allocated when None and needed."""
        (sp,) = _passes(spec)
        self._chk(hp, grad, work)
        nr, d = xr.shape
        nc = xc.shape[0] if xc is not None else nr
        r = u.shape[1] if u.dim() == 2 else -1
        for name, t, shape in (("xr", xr, (nr, d)), ("xc", xc, (nc, d)), ("u", u, (nr, r)), ("v", v, (nc, r))):
            if t is None:
                continue
            if not (t.is_cuda and t.dim() == 2 and tuple(t.shape) == shape and t.dtype == torch.float64
                    and (t.stride(1) == 1 or t.shape[1] <= 1 or t.shape[0] == 0)):
                raise ValueError("kernel_lowrank_grad needs %s %s float64 on the device, unit stride along a row" % (name, list(shape)))
        assert hp.dtype == torch.float64
        if grad is None:
            assert not accumulate
            grad = self.zeros(hp.numel(), dtype=torch.float64)
        assert grad.dtype == torch.float64

        def ld(t, width):      # (a matrix of one row or none has no row stride to speak of)
            return max(int(t.stride(0)), width, 1) if t.shape[0] > 1 else max(width, 1)

        size = self.kernel_lowrank_grad_worksize(nr, nc, r, grad.numel())
        if work is None and size > 0:
            work = self.empty(size, dtype=torch.float64)
        assert size == 0 or (work.dtype == torch.float64 and work.numel() >= size)
        xcp = _p(xc) if xc is None or nc > 0 else _p(hp)      # (an empty tensor has a null address, which would read as the symmetric form)
        self._call("pg_kernel_lowrank_grad", PG_F64, C.byref(sp), _p(hp), _p(xr), ld(xr, d), nr, xcp, ld(xc, d) if xc is not None else 0, nc, d,
                   _p(u), ld(u, r), _p(v), ld(v, r), r, _p(grad), int(bool(accumulate)), _p(work), self._st())
        return grad

    # -- the low-rank training-input gradient (include/pygpr_hip_lxgrad.h) ------------------------
    def kernel_lowrank_xgrad_worksize(self, nr, nc, d, r):
        return int(self.lib.pg_kernel_lowrank_xgrad_worksize(int(nr), int(nc), int(d), int(r)))

    def kernel_lowrank_xgrad(self, spec, hp, xr, xc, u, v, out=None, accumulate=False, work=None):
        """out[i][k] (+)= sum_j (sum_t u[i][t] v[j][t]) dk(xr_i, xc_j)/dxr_ik, the weight never formed (pg_kernel_lowrank_xgrad); xc None:
        the weight is u v^T + v u^T over the one point set xr, the gradient of sum_ij (u v^T)_ij k(xr_i, xr_j) in xr.  xr [nr, d],
        xc [nc, d], u [nr, r], v [nc, r] (r <= 64) float64 device tensors or views with unit stride along a row; out [nr, d] float64 on
        the device, unit stride along a row, allocated when None.  One pg_covspec only.  work: kernel_lowrank_xgrad_worksize doubles,
        allocated when None and needed."""
        (sp,) = _passes(spec)
        self._chk(hp, out, work)
        nr, d = xr.shape
        nc = xc.shape[0] if xc is not None else nr
        r = u.shape[1] if u.dim() == 2 else -1
        if out is None:
            assert not accumulate
            out = self.empty(nr, d, dtype=torch.float64)
        for name, t, shape in (("xr", xr, (nr, d)), ("xc", xc, (nc, d)), ("u", u, (nr, r)), ("v", v, (nc, r)), ("out", out, (nr, d))):
            if t is None:
                continue
            if not (t.is_cuda and t.dim() == 2 and tuple(t.shape) == shape and t.dtype == torch.float64
                    and (t.stride(1) == 1 or t.shape[1] <= 1 or t.shape[0] == 0)):
                raise ValueError("kernel_lowrank_xgrad needs %s %s float64 on the device, unit stride along a row" % (name, list(shape)))
        assert hp.dtype == torch.float64

        def ld(t, width):      # (a matrix of one row or none has no row stride to speak of)
            return max(int(t.stride(0)), width, 1) if t.shape[0] > 1 else max(width, 1)

        size = self.kernel_lowrank_xgrad_worksize(nr, nc, d, r)
        if work is None and size > 0:
            work = self.empty(size, dtype=torch.float64)
        assert size == 0 or (work.dtype == torch.float64 and work.numel() >= size)
        xcp = _p(xc) if xc is None or nc > 0 else _p(hp)      # (an empty tensor has a null address, which would read as the symmetric form)
        self._call("pg_kernel_lowrank_xgrad", PG_F64, C.byref(sp), _p(hp), _p(xr), ld(xr, d), nr, xcp, ld(xc, d) if xc is not None else 0, nc, d,
                   _p(u), ld(u, r), _p(v), ld(v, r), r, _p(out), ld(out, d), int(bool(accumulate)), _p(work), self._st())
        return out

    # -- normal variates (include/pygpr_hip_sample.h) -------------------------------------------
    def randn(self, out, rows, cols, seed, stream_id=0, row0=0):
        """out[r][q] = normal(seed, stream_id, row0 + r, q) for r < rows, q < cols, zero in the rest of out (pg_randn): out is a 2-D
        device tensor or view [rows_pad, cols_pad] with unit stride along a row -- any row stride, any alignment."""
        if not (out.is_cuda and out.dim() == 2 and out.stride(1) == 1):
            raise ValueError("randn needs a 2-D CUDA tensor with unit stride along its rows")
        seed = int(seed)
        if not -(1 << 63) <= seed < (1 << 63):
            raise ValueError("randn: the seed must fit a signed 64-bit integer, got %d" % seed)
        self._call("pg_randn", _code(out.dtype), seed, int(stream_id), int(row0), int(rows), int(cols), _p(out), out.stride(0), out.shape[0],
                   out.shape[1], self._st())
        return out

    # -- derivatives in the test points -------------------------------------------------------
    def kernel_xgrad(self, spec, hp, xq, z, u=None, b=None, out_u=None, out_b=None, trans_b=False, accumulate=False):
        """out_u[p][k] = sum_i u_i dk(xq_p, z_i)/dxq_pk and / or out_b[p][k] = sum_i B_pi dk(xq_p, z_i)/dxq_pk (pg_kernel_xgrad, one pass
        over the pairs for both): xq [m, d], z [n, d], u [>= n], b [m, >= n] (trans_b: [n, >= m], b[i][p]); outputs [m, d] allocated when
        None.  Returns (out_u, out_b)."""
        m, d = xq.shape
        out = self.kernel_xgrad_batched(spec, hp[None], xq, z[None], None if u is None else u[None], None if b is None else b[None],
                                        None if out_u is None else out_u[None], None if out_b is None else out_b[None], trans_b, accumulate,
                                        nexp=1)
        return tuple(None if t is None else t[0] for t in out)

    def kernel_xgrad_batched(self, spec, hp_all, xq, z_all, u_all=None, b_all=None, out_u=None, out_b=None, trans_b=False, accumulate=False,
                             nexp=None):
        """The same for nexp experts in one launch (+ the reduce): hp_all [nexp | 1, nhp]; xq [m, d] (shared) or [nexp, m, d]; z_all
        [nexp | 1, n, d]; u_all [nexp, >= n]; b_all [nexp, m, >= n] (trans_b: [nexp, n, >= m]); outputs [nexp, m, d].  A Compose longer
        than one pg_covspec runs one pass per spec, the later ones accumulating."""
        assert u_all is not None or b_all is not None
        nexp = nexp or max(hp_all.shape[0], z_all.shape[0], xq.shape[0] if xq.dim() == 3 else 1,
                           *(t.shape[0] for t in (u_all, b_all) if t is not None))
        m, d = xq.shape[-2], xq.shape[-1]
        n = z_all.shape[-2]
        dt = xq.dtype
        self._chk(hp_all, xq, z_all, u_all, b_all)
        assert hp_all.dtype == torch.float64 and z_all.dtype == dt
        if u_all is not None and out_u is None:
            out_u = self.empty(nexp, m, d, dtype=dt)
        if b_all is not None and out_b is None:
            out_b = self.empty(nexp, m, d, dtype=dt)
        for t in (out_u, out_b):
            assert t is None or (t.is_cuda and t.dtype == dt and t.dim() == 3 and t.stride(-1) == 1)

        def es(t):    # expert stride; 0 shares the operand
            return t.stride(0) if (t is not None and t.dim() == 3 and t.shape[0] > 1) else 0

        work = self.empty(max(1, int(self.lib.pg_kernel_xgrad_worksize(self.h, m, n, d, nexp))), dtype=torch.float64)
        for i, sp in enumerate(_passes(spec)):
            self._call("pg_kernel_xgrad", _code(dt), C.byref(sp), _p(hp_all), hp_all.stride(0) if hp_all.shape[0] > 1 else 0, _p(xq), xq.stride(-2),
                       es(xq), m, _p(z_all), z_all.stride(-2), es(z_all), n, d, _p(u_all),
                       u_all.stride(0) if (u_all is not None and u_all.shape[0] > 1) else 0, _p(out_u), out_u.stride(1) if out_u is not None else 0,
                       out_u.stride(0) if out_u is not None else 0, _p(b_all), b_all.stride(-2) if b_all is not None else 0, es(b_all),
                       int(bool(trans_b)), _p(out_b), out_b.stride(1) if out_b is not None else 0, out_b.stride(0) if out_b is not None else 0,
                       int(bool(accumulate) or i > 0), _p(work), work.numel(), nexp, self._st())
        return out_u, out_b

    # -- prediction ---------------------------------------------------------------------------
    def predict_mean_q(self, ks, minv, alpha, mean, var, kss, work):
        """mean = Ks^T alpha; var = kss - colsum((Minv Ks)^2) (var None: mean only)."""
        q = var
        self._chk(ks, minv, alpha, mean, q, work)
        self._call("pg_predict_mean_q", _code(ks.dtype), ks.shape[0], ks.shape[1], _p(ks), ks.stride(0), _p(minv),
                   minv.stride(0) if minv is not None else 0, _p(alpha), _p(mean), _p(q), float(kss), _p(work), self._st())

    def predict_mean_q_kt(self, kt, minv, alpha, mean, var, kss, work):
        """The same from kt [m_pad, n_pad] = k(xp, x) (test-point-major): mean = Kt alpha; var = kss - colsum((Minv Kt^T)^2)."""
        q = var
        self._chk(kt, minv, alpha, mean, q, work)
        self._call("pg_predict_mean_q_kt", _code(kt.dtype), kt.shape[1], kt.shape[0], _p(kt), kt.stride(0), _p(minv),
                   minv.stride(0) if minv is not None else 0, _p(alpha), _p(mean), _p(q), float(kss), _p(work), self._st())

    def predict_mean_q_kt_batched(self, kt_all, minv_all, alpha_all, mean_all, var_all, spec, hp_all, work_all):
        """All experts' means (and diagonal variances, var_all not None) in three launches (pg_predict_mean_q_kt_batched): kt_all
        [nexp, m_pad, n_pad], minv_all [nexp, n_pad, n_pad] (any common stride), alpha_all [nexp, n_pad], mean_all / var_all [nexp, m_pad],
        hp_all [nexp | 1, nhp], work_all [nexp, (n_pad/64) m_pad].  kss is formed on the device from hp_all."""
        passes = _passes(spec)
        assert len(passes) == 1
        self._chk(kt_all, alpha_all, hp_all, work_all)
        nexp, m_pad, n_pad = kt_all.shape
        want_var = var_all is not None
        for t in (mean_all, var_all):          # rows may be slices of longer rows (chunks of test points): unit stride inside a row
            assert t is None or (t.is_cuda and t.dim() == 2 and t.stride(1) == 1 and t.shape[1] >= m_pad and (nexp == 1 or t.stride(0) >= m_pad))
        if want_var:
            assert minv_all.is_cuda and minv_all.stride(-1) == 1 and hp_all.dtype == torch.float64
        self._call("pg_predict_mean_q_kt_batched", _code(kt_all.dtype), n_pad, m_pad, _p(kt_all), kt_all.stride(1), kt_all.stride(0),
                   _p(minv_all) if want_var else None, minv_all.stride(-2) if want_var else 0, minv_all.stride(0) if want_var else 0, _p(alpha_all),
                   alpha_all.stride(0), _p(mean_all), mean_all.stride(0), _p(var_all), var_all.stride(0) if want_var else 0, C.byref(passes[0]),
                   _p(hp_all), hp_all.stride(0) if hp_all.shape[0] > 1 else 0, _p(work_all), work_all.stride(0), nexp, self._st())

    def trmm_lower(self, minv, ks, v):
        self._chk(minv, ks, v)
        self._call("pg_trmm_lower", _code(ks.dtype), ks.shape[0], ks.shape[1], _p(minv), minv.stride(0), _p(ks), ks.stride(0), _p(v), v.stride(0),
                   self._st())

    def syrk_tn_sub(self, v, c, lower_only=True):
        self._chk(v, c)
        self._call("pg_syrk_tn_sub", _code(v.dtype), c.shape[0], v.shape[0], _p(v), v.stride(0), _p(c), c.stride(0), int(lower_only), self._st())

    def trmm_lower_kt(self, minv, kt, vt):
        """vt = kt minv^T (= (minv ks)^T) from the test-point-major cross-covariance: kt, vt [m_pad, n_pad] or [nexp, m_pad, n_pad];
        minv [n_pad, n_pad], [nexp, n_pad, n_pad], or a list of nexp matrices that sit at one stride in memory (views of a stack)."""
        if isinstance(minv, (list, tuple)):
            self._chk(kt, vt, *minv)
            m0 = minv[0]
            step = (minv[1].data_ptr() - m0.data_ptr()) // m0.element_size() if len(minv) > 1 else 0
            assert all(mi.data_ptr() - m0.data_ptr() == i * step * m0.element_size() and mi.stride(0) == m0.stride(0)
                       for i, mi in enumerate(minv)), "the experts' inverses do not sit at one stride"
            ldm = m0.stride(0)
        else:
            self._chk(minv, kt, vt)
            m0, ldm, step = minv, minv.stride(-2), (minv.stride(0) if minv.dim() == 3 else 0)
        nexp = kt.shape[0] if kt.dim() == 3 else 1
        self._call("pg_trmm_lower_kt_batched", _code(kt.dtype), kt.shape[-1], kt.shape[-2], _p(m0), ldm, step, _p(kt), kt.stride(-2),
                   kt.stride(0) if kt.dim() == 3 else 0, _p(vt), vt.stride(-2), vt.stride(0) if vt.dim() == 3 else 0, nexp, self._st())

    def syrk_nt_sub_batched(self, vt_all, c_all, lower_only=True):
        """c_all[e] -= vt_all[e] vt_all[e]^T for all experts in one launch: vt_all [nexp, m_pad, n_pad], c_all [nexp, m_pad, m_pad]."""
        self._chk(vt_all, c_all)
        assert vt_all.dim() == 3 and c_all.dim() == 3 and vt_all.shape[0] == c_all.shape[0]
        self._call("pg_syrk_nt_sub_batched", _code(c_all.dtype), c_all.shape[1], vt_all.shape[2], _p(vt_all), vt_all.stride(1), vt_all.stride(0),
                   _p(c_all), c_all.stride(1), c_all.stride(0), c_all.shape[0], int(lower_only), self._st())

    # -- grBCM --------------------------------------------------------------------------------
    def grbcm_local_terms(self, mean_c, var_c, var_g, is_first, accumulate, out, beta=None, prec=None):
        self._chk(mean_c, var_c, var_g, out, beta, prec)
        assert out.dtype == torch.float64 and out.shape[0] == 3
        self._call("pg_grbcm_local_terms", _code(mean_c.dtype), mean_c.numel(), _p(mean_c), _p(var_c), _p(var_g), int(is_first), int(accumulate),
                   _p(out), out.stride(0), _p(beta), _p(prec), self._st())

    def grbcm_local_terms_batched(self, mean_all, var_all, var_g, first, accumulate, out, beta=None, prec=None):
        """The terms of all owned experts in one launch: mean_all / var_all [nexp, >= m] (row stride arbitrary), out [3, m] float64,
        beta / prec [nexp, m] float64 views (common row stride) or None; `first`: index of the committee's first expert among these, -1: none."""
        self._chk(var_g, out)
        assert out.dtype == torch.float64 and out.shape[0] == 3 and mean_all.stride(-1) == 1 and var_all.stride(-1) == 1
        m = var_g.numel()
        nexp = mean_all.shape[0]
        if beta is not None:
            assert beta.stride(-1) == 1 and prec.stride(-1) == 1 and (nexp == 1 or beta.stride(0) == prec.stride(0))
        self._call("pg_grbcm_local_terms_batched", _code(mean_all.dtype), m, _p(mean_all), mean_all.stride(0), _p(var_all), var_all.stride(0),
                   _p(var_g), nexp, int(first), int(accumulate), _p(out), out.stride(0), _p(beta), _p(prec),
                   beta.stride(0) if beta is not None else 0, self._st())

    def grbcm_finish(self, sums, mean_g, var_g, mean, var, beta0=None, prec0=None):
        self._chk(sums, mean_g, var_g, mean, var, beta0, prec0)
        self._call("pg_grbcm_finish", _code(mean_g.dtype), mean_g.numel(), _p(sums), sums.stride(0), _p(mean_g), _p(var_g), _p(mean), _p(var),
                   _p(beta0), _p(prec0), self._st())

    def grbcm_weighted_prec(self, prec, beta, acc, m, accumulate):
        self._chk(prec, beta, acc)
        self._call("pg_grbcm_weighted_prec", _code(acc.dtype), m, acc.shape[0], _p(prec), prec.stride(0), _p(beta), _p(acc), acc.stride(0),
                   int(accumulate), self._st())

    def symmetrize(self, a, n):
        self._chk(a)
        self._call("pg_symmetrize", _code(a.dtype), n, _p(a), a.stride(0), self._st())

    def grbcm_finish_full(self, sums, mean_g, var_g, cov, mean):
        self._chk(sums, mean_g, var_g, cov, mean)
        self._call("pg_grbcm_finish_full", _code(mean_g.dtype), mean_g.numel(), _p(sums), sums.stride(0), _p(mean_g), _p(var_g), _p(cov),
                   cov.stride(0), _p(mean), self._st())

    def spd_inverse_lower(self, a_pad):
        """a_pad (padded SPD, lower triangle valid) -> its inverse's lower triangle in a new buffer; raises on a bad pivot."""
        n = a_pad.shape[0]
        invd = self.potrf_workspace(n, a_pad.dtype)
        info = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.potrf(a_pad, invd, info)
        minv = self.empty(n, n, dtype=a_pad.dtype)
        self.trtri(a_pad, invd, minv)
        out = self.empty(n, n, dtype=a_pad.dtype)
        self.lauum(minv, out)
        return out, info

    def spd_inverse_lower_batched(self, a_all):
        """a_all [nexp, n_pad, n_pad] (padded SPD, lower triangles valid; overwritten) -> (the inverses' lower triangles IN a_all,
        info [nexp]): every step of factor, L^-1 and L^-T L^-1 is one launch over all matrices."""
        nexp, n = a_all.shape[0], a_all.shape[1]
        invd = self.empty(nexp, self.potrf_worksize(n, a_all.dtype), dtype=a_all.dtype)
        info = torch.zeros(nexp, dtype=torch.int32, device=self.device)
        minv = self.empty(nexp, n, n, dtype=a_all.dtype)
        self.potrf_trtri_batched(a_all, invd, info, minv)
        self.lauum_batched(minv, a_all)
        return a_all, info

    def sqdist_argmin(self, x, centres, dist=None, idx=None):
        """dist[n, m] = squared distances, idx[n] (int32) = nearest centre; either output may be None."""
        self._chk(x, centres, dist, idx)
        self._call("pg_sqdist_argmin", _code(x.dtype), _p(x), x.stride(0), x.shape[0], _p(centres), centres.stride(0), centres.shape[0], x.shape[1],
                   _p(dist), dist.stride(0) if dist is not None else 0, _p(idx), self._st())

    # -- raw GEMM core (tests, roofline micro-benchmark) ---------------------------------------
    def gemm_raw(self, variant, m, n, k, alpha, a, b, beta, c, tri=0, klo=0, khi=0):
        self._chk(a, b, c)
        self._call("pg_gemm_raw", _code(c.dtype), variant, m, n, k, float(alpha), _p(a), a.stride(0), _p(b), b.stride(0), float(beta), _p(c),
                   c.stride(0), tri, klo, khi, self._st())

    def set_lookahead(self, on):
        self._call("pg_set_lookahead", int(on))

    def set_outer_panel(self, columns):
        self._call("pg_set_outer_panel", int(columns))

    def set_recursive_split(self, min_n):
        """From min_n points on the fused factor-and-invert call splits the matrix recursively (0: never; default 16384)."""
        self._call("pg_set_recursive_split", int(min_n))

    def set_coupled_chain(self, on):
        self._call("pg_set_coupled_chain", int(on))

    def set_spin_budget(self, microseconds):
        """Wall-time bound of one wait of the coupled chain; 0: scaled to the call (default); < 0: every wait expires at once
        (test hook of the fall-back)."""
        self._call("pg_set_spin_budget", int(microseconds))

    def chain_timeouts(self):
        return int(self.lib.pg_chain_timeouts(self.h))

    def set_rearm_after(self, calls):
        """After a time-out the handle takes the coupled chain back by itself once this many further factorisations have been
        enqueued (default 8; 0: never)."""
        self._call("pg_set_rearm_after", int(calls))

    def chain_rearms(self):
        return int(self.lib.pg_chain_rearms(self.h))

    def wait_budget_us(self, n):
        return int(self.lib.pg_wait_budget_us(self.h, int(n)))

    def spin_probe(self, n):
        """One bounded wait on a flag nobody sets, with the budget of an n x n factorisation: (milliseconds waited, flag came)."""
        scratch = torch.zeros(4, dtype=torch.int64, device=self.device)
        self._call("pg_spin_probe", int(n), _p(scratch), self._st())
        torch.cuda.synchronize()
        v = scratch.tolist()
        return v[2] * 1e-5, bool(v[3])

    def recover_from_timeout(self):
        """A factorisation reported info = -1 (a wait of the coupled chain expired: include/pygpr_hip.h).  The library has
        switched the handle to the classic chain by itself (pinned word polled at every entry point); make sure, count, and
        tell the caller to repeat its sequence from the covariance build."""
        torch.cuda.synchronize()
        self.chain_timeouts()                      # polls the pinned word
        if self.coupled_chain():                   # (-1: off as after a time-out -- the rows stream stays, the handle re-arms itself)
            self._call("pg_set_coupled_chain", -1)
        self.fallbacks = getattr(self, "fallbacks", 0) + 1

    def build_factor_checked(self, spec, hp, x, a, invd, info, minv=None, jitter=JITTER):
        """Blocking build + factor with the fall-back inside the call (pg_build_potrf_trtri_checked); returns info."""
        passes = _passes(spec)
        assert len(passes) == 1
        self._chk(hp, x, a, invd, info, minv)
        n, d = x.shape
        out = C.c_int(0)
        self._call("pg_build_potrf_trtri_checked", _code(a.dtype), C.byref(passes[0]), _p(hp), _p(x), x.stride(0), n, d, float(jitter), _p(a),
                   a.stride(0), a.shape[0], _p(invd), _p(info), _p(minv), minv.stride(0) if minv is not None else 0, self._st(), C.byref(out))
        return out.value

    def coupled_chain(self):
        return int(self.lib.pg_coupled_chain(self.h))

    def last_coupled_panels(self):
        return int(self.lib.pg_last_coupled_panels(self.h))

    def leaf_raw(self, a, inv, info):
        self._chk(a, inv, info)
        self._call("pg_leaf_raw", _code(a.dtype), _p(a), a.stride(0), _p(inv), inv.stride(0) if inv is not None else 0, _p(info), self._st())

    def profile(self, on):
        self._call("pg_profile", int(on))

    def profile_read(self):
        f, ms, n = C.c_double(), C.c_double(), C.c_long()
        self._call("pg_profile_read", C.byref(f), C.byref(ms), C.byref(n))
        return f.value, ms.value, n.value


_OPS = None


def get_ops():
    """The process-wide device-op object; raises (never falls back) without library + GPU."""
    global _OPS
    if _OPS is None:
        _OPS = HipOps()
    return _OPS


def _passes(spec):
    return spec if isinstance(spec, (list, tuple)) else [spec]


def make_specs(kinds, offs, noise_offs):
    """The passes of a Compose of any length: pg_covspec holds PG_MAX_COMP stationary and PG_MAX_COMP noise children, a
    longer sum (the reference's Compose is unlimited, covar.py:28-81) is evaluated PG_MAX_COMP children at a time."""
    q = _lib.PG_MAX_COMP
    npass = max(1, -(-len(kinds) // q), -(-len(noise_offs) // q))
    return [make_spec(kinds[i * q: (i + 1) * q], offs[i * q: (i + 1) * q], noise_offs[i * q: (i + 1) * q]) for i in range(npass)]


def make_spec(kinds, offs, noise_offs, product=False):
    """One pg_covspec; product: the stationary components are the factors of one product term (PG_SPEC_PRODUCT in ncomp)."""
    s = CovSpec()
    if len(kinds) > _lib.PG_MAX_COMP or len(noise_offs) > _lib.PG_MAX_COMP:
        raise ValueError("one pg_covspec holds at most %d stationary and %d noise kernels (make_specs splits a longer Compose)"
                         % (_lib.PG_MAX_COMP, _lib.PG_MAX_COMP))
    if product and not kinds:
        raise ValueError("a product spec needs at least one factor")
    s.ncomp = len(kinds) | (_lib.PG_SPEC_PRODUCT if product else 0)
    for i, (k, o) in enumerate(zip(kinds, offs)):
        s.kind[i], s.off[i] = k, o
    s.nnoise = len(noise_offs)
    for i, o in enumerate(noise_offs):
        s.noise_off[i] = o
    return s
