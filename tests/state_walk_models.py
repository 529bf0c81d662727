"""The walkers of the matrix-free and the sparse models' cached state (helper module: no tests in it).  The pattern is
tests/state_walk.py's: a model under test beside a SHADOW -- plain fp64 NumPy x, y (z), hyper-parameters and the term list in the grammar
of tests/kernel_ref.py -- that never calls pygpr_amd and answers every observation from scratch, through the restatements the fresh-model
tests use (iterative_ref, slq_ref, lowrank_ref, lxgrad_ref, pathwise_ref, varcache_ref; sparse_ref, sparse_z_ref, sparse_whitened_ref,
select_ref).  Every OPERATION (`step`) is applied to both sides and followed by every OBSERVATION (`observe`); `Env`, `Spies` and the
error table are state_walk's.

`IterWalk` drives an Iterative_GP with ONE Stochastic_MLE (4 probes, fixed seed) alive across the walk; `SparseWalk` a Sparse_GP
(whitened or not) with a VFE(model) and a VFE(model, train_z=True) alive across the walk.

Bounds.  None is fitted and none is new: each is the rule of the fresh-model test of that quantity, evaluated on the state at hand.
  Iterative_GP  test_iterative_gpu.held: 2 cond(A) tol relative to the largest reference entry plus that file's dense yardsticks
                (alpha rtol 1e-8, mean atol 1e-10, variance / covariance atol 1e-11; test_iterative_grad_gpu: derivatives rtol 1e-9;
                test_pathwise_gpu: samples atol 1e-10).  cond(A) is recomputed by NumPy for every state.
  loss          test_slq_gpu: sparse_ref.tol_of(the restatement's quadrature-vs-dense-limit difference), against the dense limit.
  gradient      test_slq_gpu: per entry (2 cond(A) tol + 16 own + (2 r + 2) 2^-53) S_p against the dense-solve estimator.
  grad_x        test_input_grad_gpu: (16 own_dK + (n + 2 r + 2) 2^-53) S_ik against the restatement on the device's weight_factors(); the
                factors themselves against the dense solves at `held`'s bound with alpha's yardstick.  Where no solve is kept
                (memoize off) the two are added: (2 cond(A) tol + the kernel's bound) S_ik against the restatement on the dense factors.
  caches        test_varcache_gpu: sparse_ref.tol_of(the disagreement of the restatement's two orthonormalisations) k**; the gradient
                against central differences of the restatement, their truncation estimate plus that.
  Sparse_GP     test_sparse_gpu / test_sparse_z_gpu / test_sparse_whitened_gpu: sparse_ref.tol_of(own), relative to the largest reference
                entry (a whitened model's variances: to the prior variance).  `own` is the restatement's own error ON THAT STATE: the
                disagreement of the two fp64 restatements of the same function (Woodbury, sparse_ref / sparse_z_ref, and whitened,
                sparse_whitened_ref) -- the fresh-model tests measure it against a dense form or np.longdouble, which a walk of twenty
                states cannot afford; two formulations in the same precision differ by at least the smaller of their errors, and the
                rule's floor (1e-10) is what decides at these conditionings.  The reference is the restatement of the model's own form.
"Same bits" is tobytes() equality.  Every figure is printed before it is asserted."""
import collections
import gc
import random

import numpy as np
import pytest
import torch

import dmatmul_ref as dr
import iterative_ref as ir
import kernel_ref as kr
import lowrank_ref as lr
import lxgrad_ref as lx
import matmul_ref as mr
import pathwise_ref as pr
import pygpr_amd as pg
import select_ref as sel
import slq_ref as sq
import sparse_ref as sr
import sparse_whitened_ref as wr
import sparse_z_ref as szr
import state_walk as sw
import varcache_ref as vr
from kind_tools import T, cov_of
from oracle_ops import _np
from pygpr_amd import _lib, _ops
from pygpr_amd import gpr as gpr_mod
from pygpr_amd import iterative as it_mod
from pygpr_amd import sparse as sp_mod
from test_input_grad_cpu import InputOracleOps
from test_iterative_grad_gpu import restated as sample_grad_restated
from test_iterative_gpu import held as iter_held
from test_select_cpu import SelectOracleOps
from test_sparse_whitened_cpu import WhitenedOracleOps
from test_varcache_cpu import VcOracleOps

D = 3
Q = 40                  # test points of an observation: blocks of 16, 16 and 8 right-hand sides, chunks of 32 and 8
TOL = 1e-10             # the solver's (test_iterative_gpu.TOL, which `held` reads)
PROBES, SEED = 4, 3
EPS = 2.0 ** -53
SIGMA_N = 0.3
GATES = ((it_mod, "_RHS_BLOCK", 16), (sp_mod, "_SPARSE_CHUNK", 128), (sp_mod, "_CHUNK", 32), (gpr_mod, "_CHUNK", 32))

KINDS = {"se+wn": ["se", "wn"], "m32+rq+wn": ["m32", "rq", "wn"], "(se*per)+wn": [("se", "per"), "wn"]}
SAME_NHP = dict(sw.SAME_NHP, rq="rq")
SPECTRAL = ("se", "m52", "m32", "m12", "wn")      # parts a FunctionSamples can be drawn from (a product has no spectral law either)

SPIED = ["greedy_select", "potrf", "trtri", "potrs", "potrs_vec", "kernel_matmul", "kernel_build", "kernel_lowrank_grad", "kernel_lowrank_xgrad",
         "kernel_cross_grad", "kernel_xgrad", "kernel_rowsq", "feature_matmul", "gemm_raw", "randn"]


def N(t):
    return t.detach().cpu().numpy()


def swapped(terms):
    return [tuple(SAME_NHP[p] for p in t) if isinstance(t, tuple) else SAME_NHP[t] for t in terms]


# ---- the CPU double ------------------------------------------------------------------------------------------------------------------
class ModelsOracleOps(InputOracleOps, WhitenedOracleOps, SelectOracleOps):
    """The doubles of the matrix-free tests (InputOracleOps) and of the sparse tests (WhitenedOracleOps, SelectOracleOps) in one object.
    Added: only what the parents state twice in forms that exclude each other -- the raw product (the transposed variants are the
    preconditioner's, everything else the sparse double's, K ranges included) and pg_kernel_xgrad in its full contract (both weights,
    given outputs, the transposed B, accumulation)."""

    def __init__(self):
        InputOracleOps.__init__(self)
        WhitenedOracleOps.__init__(self)
        self._kmat = None

    def gemm_raw(self, variant, m, n, k, alpha, a, b, beta, c, tri=0, klo=0, khi=0):
        if variant in (_lib.GEMM_TN, _lib.GEMM_TN_64) and klo == khi == 0:
            return VcOracleOps.gemm_raw(self, variant, m, n, k, alpha, a, b, beta, c, tri, klo, khi)
        return WhitenedOracleOps.gemm_raw(self, variant, m, n, k, alpha, a, b, beta, c, tri, klo, khi)

    def kernel_matmul(self, spec, hp, xr, xc, v, out=None, jitter=0.0, work=None):
        """DxOracleOps' product with the matrix kept between calls: a walk takes some ten thousand conjugate-gradient steps, each of
        which would otherwise restate the same n x n kernel.  The matrix IS the parent's product with the identity (exact: ones and
        zeros), looked up by the bytes of everything it depends on."""
        if xc is not None or v.dim() != 2:
            return InputOracleOps.kernel_matmul(self, spec, hp, xr, xc, v, out, jitter, work)
        (sp,) = spec if isinstance(spec, (list, tuple)) else [spec]
        key = (bytes(sp), _np(hp).tobytes(), _np(xr).tobytes(), float(jitter))
        if self._kmat is None or self._kmat[0] != key:
            n = xr.shape[0]
            self._kmat = (key, _np(InputOracleOps.kernel_matmul(self, spec, hp, xr, None, torch.eye(n, dtype=torch.float64), None, jitter)).copy())
        res = torch.from_numpy(self._kmat[1] @ _np(v))
        return res if out is None else out.copy_(res)

    def kernel_xgrad(self, spec, hp, xq, z, u=None, b=None, out_u=None, out_b=None, trans_b=False, accumulate=False):
        assert u is not None or b is not None
        (sp,) = spec if isinstance(spec, (list, tuple)) else [spec]
        q = _np(xq)
        m, n = q.shape[0], z.shape[0]
        model, h, _ = self._model(sp, _np(hp), q.shape[1])
        dk = dr.dkernel(model, h, q, _np(z))                               # [d, m, n]
        outs = []
        for w, out, sub in ((u, out_u, "kpi,i->pk"), (b, out_b, "kpi,pi->pk")):
            if w is None:
                outs.append(None)
                continue
            wn = _np(w)[:n] if w.dim() == 1 else (_np(w).T[:m, :n] if trans_b else _np(w)[:m, :n])
            val = torch.from_numpy(np.einsum(sub, dk, wn))
            if out is None:
                assert not accumulate
                out = val
            else:
                assert out.shape == val.shape
                out.copy_(out + val if accumulate else val)
            outs.append(out)
        return tuple(outs)


@pytest.fixture
def model_ops(monkeypatch, tmp_path):
    """The double, with the BLAS behind NumPy held to one thread while the test runs: the double issues thousands of products of a few
    hundred rows, which a threaded BLAS beside torch's own pool serves fifteen times slower (measured: 19 s against 1.3 s per sequence)."""
    ops = ModelsOracleOps()
    monkeypatch.setattr(_ops, "_OPS", ops)
    monkeypatch.chdir(tmp_path)
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:                 # (slower, not wrong)
        yield ops
        return
    with threadpool_limits(limits=1):
        yield ops


def make_env(ops, monkeypatch, device=None):
    """state_walk.Env with the models' spies and the issue's size gates: blocks of 16 right-hand sides, chunks of 128 training points
    and of 32 test points (Sparse_GP.predict; Iterative_GP's preconditioner keeps its row chunk, which must stay a multiple of the
    padding unit)."""
    env = sw.Env(ops, monkeypatch, TOL, TOL, spied=SPIED, device=device)
    for mod, name, val in GATES:
        monkeypatch.setattr(mod, name, val)
    return env


# ---- shared pieces -------------------------------------------------------------------------------------------------------------------
def hp_for(terms, rng):
    """Hyper-parameters in sparse_ref.problem's ranges, sigma_n = 0.3."""
    hp = []
    for p in kr.flat(terms):
        if p == "wn":
            hp += [SIGMA_N]
        else:
            hp += [0.9 + 0.2 * rng.random()] + list(2.5 + 0.6 * rng.random(D))
            hp += [1.5] if p == "rq" else (list(0.7 + 0.3 * rng.random(D)) if p == "per" else [])
    return np.array(hp)


def draw(rng, n):
    x = rng.random((n, D))
    return x, np.sin(3.0 * x.sum(1)) + 0.1 * rng.standard_normal(n)


class _Walk:
    """What the two walkers share: the trace, the recording of errors, tensors on the tier's device."""

    def __init__(self, env, terms, seed):
        self.env, self.terms, self.seed = env, list(terms), seed
        self.rng = np.random.default_rng(seed)
        self.trace = []
        self.version = 0            # of the shadow's state: what its cached answers are keyed on
        self._cache = {}
        self.fixed = None           # bits of the predictions at the walk's fixed points, while the model is clean

    def t(self, a):
        t = T(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).clone()            # (never the shadow's memory)
        return t if self.env.device is None else t.to(self.env.device)

    def one_call(self, a, at=()):
        """A tensor made by ONE constructor call, so that the allocator can hand out the address of a tensor dropped before.  at: the
        id()s wanted for it -- tensors are made and kept aside until the allocator hands one of those addresses out again (or 64
        were made: then the last one is taken)."""
        aside = []
        for _ in range(64 if at else 1):
            t = torch.tensor(np.asarray(a, dtype=np.float64), device=self.env.device or "cpu")
            if not at or id(t) in at:
                break
            aside.append(t)
        return t

    def changed(self):
        self.version += 1
        self._cache = {}
        self.fixed = None

    def memo(self, key, fn):
        if key not in self._cache:
            self._cache[key] = fn()
        return self._cache[key]

    def record(self, name, err, bound):
        print("%-40s err %.2e (bound %.2e)" % (name, err, bound))
        old = self.env.errors.get(name)
        if old is None or err / bound >= old[0] / old[1]:
            self.env.errors[name] = (err, bound)
        assert err <= bound, (name, err, bound)

    def same_bits(self, name, a, b):
        assert N(a).tobytes() == N(b).tobytes(), name + ": not the same bits"

    def step(self, name, *args, observe=True):
        self.trace.append("%s%s" % (name, args if args else ""))
        try:
            before = self.fixed if name in self.QUIET else None
            getattr(self, "op_" + name)(*args)
            if before is not None:                      # an evaluation, a snapshot or an update of a clean model: the fit stands, to the bit
                assert not self.gp.need_upd, name + " marked a clean model dirty"
                assert self.fixed_bits() == before, name + " changed the predictions of a fitted model"
            if observe:
                self.observe()
        except BaseException:
            print("walk of seed %d failed; operations so far:\n  %s" % (self.seed, "\n  ".join(self.trace)))
            raise
        return self


# ---- Iterative_GP ----------------------------------------------------------------------------------------------------------------------
ITER_LOSSES = ["sm_" + w for w in ("loss", "grad", "loss_and_grad", "grad_x", "loss_and_grads")]
ITER_CHANGES = {"set_params", "edit_x", "edit_y", "assign_x", "assign_y", "assign_cross", "replace_twice", "cov", "nlml_of_inputs"}
ITER_KINDS = sorted(ITER_CHANGES | set(ITER_LOSSES) | {"update", "variance_cache", "function_samples", "memoize", "weight_factors"})


class IterWalk(_Walk):
    QUIET = set(ITER_LOSSES) | {"update", "variance_cache", "function_samples", "memoize", "weight_factors"}

    def __init__(self, env, terms, n0, rank, seed=0):
        super().__init__(env, terms, seed)
        self.rank = rank
        self.sx, self.sy = draw(self.rng, n0)
        self.shp = hp_for(self.terms, self.rng)
        self.gp = pg.Iterative_GP(self.t(self.sx), self.t(self.sy), cov_of(self.terms), rank=rank, tol=TOL)
        self.gp.set_params(T(self.shp.copy()))
        self.loss = pg.Stochastic_MLE(self.gp, probes=PROBES, seed=SEED)
        self.last_p = None
        self.xq = self.rng.random((7, D))       # the fixed points of the snapshots and of `fixed_bits`
        self.samples, self.caches = [], []
        self.flip = False

    @property
    def n(self):
        return self.sx.shape[0]

    # -- the shadow ------------------------------------------------------------------------------
    def dense(self):
        """A, cond(A), alpha and the rank of the preconditioner at the shadow's state, from scratch."""
        def make():
            a = ir.operator(self.terms, self.shp, self.sx)
            l, piv = ir.factor_l(self.terms, self.shp, self.sx, self.rank)
            chol = np.linalg.cholesky(a)                    # (a LinAlgError here: the walk left the region the cases are drawn from)
            alpha = np.linalg.solve(chol.T, np.linalg.solve(chol, self.sy))
            ok = ir.pcg(a, self.sy, ir.Woodbury(l, mr.shift_of(self.terms, self.shp, D, ir.JITTER)), TOL, 1000)[3]
            assert ok, "the shadow's own solve does not converge at this state"
            return dict(a=a, cond=float(np.linalg.cond(a)), alpha=alpha, rank=len(piv))
        return self.memo("dense", make)

    def estimate(self, p):
        """slq_ref's estimate at p with its dense-solve gradient, the factors, the own errors and cond(A(p))."""
        def make():
            e = sq.estimate(self.terms, p, self.sx, self.sy, self.rank, SEED, PROBES, TOL)
            want, scale, alpha, s, pz = sq.grad_dense(self.terms, p, self.sx, self.sy, e["a"], e["pre"], e["z"])
            u, v = sq.weight_factors(alpha, s, pz)
            mine = lr.mine(self.terms, D)
            f64 = lr.lowrank_grad(self.terms, p, self.sx, None, u, v)
            ld = lr.lowrank_grad(self.terms, p, self.sx, None, u, v, np.longdouble)
            own = max(float(np.max(np.abs(f64 - ld).astype(np.float64)[mine] / scale[mine])), EPS)
            return dict(e, grad=want, scale=scale, u=u, v=v, own=own, cond=float(np.linalg.cond(e["a"])),
                        own_dk=dr.own_dk(self.terms, p, self.sx, self.sx))
        return self.memo(("slq", np.asarray(p).tobytes()), make)

    def held(self, name, got, ref, yard_abs=0.0, yard_rel=0.0, cond=None):
        cond = self.dense()["cond"] if cond is None else cond
        got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        scale = float(np.max(np.abs(ref)))
        self.record(name, float(np.max(np.abs(got - ref))), 2 * cond * TOL * scale + yard_abs + yard_rel * scale)
        iter_held(name, got, ref, cond, yard_abs, yard_rel)            # the imported rule is what asserts

    # -- observations ----------------------------------------------------------------------------
    def fixed_bits(self):
        """(predict_grad's mean and variance are predict's own bits: every observation asserts it)"""
        gp, xq = self.gp, self.t(self.xq)
        out = [gp.predict(xq, "full")[1]] + list(gp.predict_grad(xq, "diag"))
        return b"".join(N(o).tobytes() for o in out)

    def check_cache(self, steps, na):
        xp = self.rng.random((Q, D))
        anchors = self.rng.random((na, D)) if na else None
        vc = self.gp.variance_cache(steps=steps, anchors=None if anchors is None else self.t(anchors))
        ce, _, err = vr.own_error(self.terms, self.shp, self.sx, self.sy, self.rank, steps, xp, anchors, self.dense()["a"])
        tol = sr.tol_of(err) * ce.kss
        assert ce.dropped == 0 and vc.info["dropped"] == 0 and vc.rank == ce.rank, (ce.dropped, vc.info, ce.rank)
        xpt = self.t(xp)
        upper, lower = (N(t) for t in vc.variance(xpt, bounds=True))
        ru, rl = ce.variance(xp, bounds=True)
        self.record("cache: upper", float(np.max(np.abs(upper - ru))), tol)
        self.record("cache: lower", float(np.max(np.abs(lower - rl))), tol)
        var, dvar = vc.variance_grad(xpt)
        self.same_bits("variance_grad's variance", var, vc.variance(xpt))
        h, fd = 1e-5, {}
        for stp in (h, 2 * h):
            fd[stp] = np.stack([(ce.variance(xp + stp * np.eye(D)[k]) - ce.variance(xp - stp * np.eye(D)[k])) / (2 * stp) for k in range(D)], 1)
        trunc = 4.0 / 3.0 * float(np.max(np.abs(fd[2 * h] - fd[h])))
        self.record("cache: variance_grad", float(np.max(np.abs(N(dvar) - fd[h]))), trunc + tol)
        xq = self.t(self.xq)
        self.caches.append((vc, b"".join(N(t).tobytes() for t in vc.variance(xq, bounds=True))))

    def observe(self):
        gp, d = self.gp, self.dense()
        terms, hp, x, y = self.terms, self.shp, self.sx, self.sy
        self.trace.append("    observe")
        xp = self.rng.random((Q, D))
        xpt = self.t(xp)
        self.held("alpha", N(gp.alpha), d["alpha"], yard_rel=1e-8)
        assert gp.cg_info["rank"] == d["rank"] and gp.cg_info["residual"] <= 2 * TOL, gp.cg_info
        mu, cov = kr.predict(terms, hp, x, y, xp, var="full")
        m0, none = gp.predict(xpt, "mean")
        assert none is NotImplemented
        m1, vd = gp.predict(xpt, "diag")
        m2, vf = gp.predict(xpt, "full")
        self.same_bits("mean (none / diag)", m0, m1)
        self.same_bits("mean (none / full)", m0, m2)
        self.held("predict: mean", N(m1), mu, yard_abs=1e-10)
        self.held("predict diag: variance", N(vd), np.diag(cov), yard_abs=1e-11)
        self.held("predict full: covariance", N(vf), cov, yard_abs=1e-11)
        assert np.array_equal(N(vf), N(vf).T)
        g = gp.predict_grad(xpt, "diag")
        self.same_bits("predict_grad: mean", g[0], m1)
        self.same_bits("predict_grad: variance", g[1], vd)
        rdm, rdv = kr.predict_grads(terms, hp, x, y, xp)
        self.held("predict_grad: d mean", N(g[2]), rdm, yard_rel=1e-9)
        self.held("predict_grad: d variance", N(g[3]), rdv, yard_rel=1e-9)
        gn = gp.predict_grad(xpt, "none")
        self.same_bits("predict_grad none: mean", gn[0], m1)
        self.same_bits("predict_grad none: d mean", gn[1], g[2])
        # snapshots: a FunctionSamples clones what it needs and survives everything; a VarianceCache survives what its docstring lists
        xq = self.t(self.xq)
        for fs, vals, grads in self.samples:
            assert N(fs(xq)).tobytes() == vals and N(fs.grad(xq)).tobytes() == grads, "an earlier FunctionSamples changed"
        for vc, bits in self.caches:
            assert b"".join(N(t).tobytes() for t in vc.variance(xq, bounds=True)) == bits, "an earlier VarianceCache changed"
        self.caches = self.caches[:2]
        self.check_cache(len(self.trace) % 2, (0, 8)[(len(self.trace) // 2) % 2])
        assert not gp.need_upd
        self.fixed = self.fixed_bits()

    # -- operations ------------------------------------------------------------------------------
    def op_set_params(self, hp=None):
        self.shp = hp_for(self.terms, self.rng) if hp is None else np.asarray(hp, dtype=np.float64)
        self.gp.set_params(T(self.shp.copy()))
        self.changed()

    def op_edit_x(self):
        c = 0.8 if self.flip else 1.25
        self.flip = not self.flip
        self.gp.x.mul_(c)
        self.sx = self.sx * c                       # (one rounding per entry on both sides)
        self.caches = []                            # VarianceCache's docstring: the snapshot does not cover an in-place edit
        self.changed()
        assert np.array_equal(N(self.gp.x), self.sx)

    def op_edit_y(self):
        self.gp.y.mul_(0.5).add_(0.125)
        self.sy = self.sy * 0.5 + 0.125
        self.caches = []
        self.changed()
        assert np.array_equal(N(self.gp.y), self.sy)

    def op_assign_x(self):
        self.sx = self.rng.random((self.n, D))
        self.gp.x = self.t(self.sx)
        self.changed()

    def op_assign_y(self):
        self.sy = np.sin(3.0 * self.sx.sum(1)) + 0.1 * self.rng.standard_normal(self.n)
        self.gp.y = self.t(self.sy)
        self.changed()

    def op_assign_cross(self):
        """Both with another n, on the other side of the 256 boundary of the padded size."""
        self.sx, self.sy = draw(self.rng, 300 if self.n <= 256 else 200)
        self.gp.x = self.t(self.sx)
        self.gp.y = self.t(self.sy)
        self.changed()

    def op_replace_twice(self):
        """x replaced twice with nothing evaluated in between and no outside reference kept; then gc.collect()."""
        x1, x2 = self.rng.random((self.n, D)), self.rng.random((self.n, D))
        self.gp.x = self.one_call(x1)
        self.gp.x = self.one_call(x2)
        gc.collect()
        self.sx = x2
        self.changed()

    def set_x(self, x, at=()):
        self.gp.x = self.one_call(x, at)
        self.sx = np.array(x)
        self.changed()
        return id(self.gp.x)

    def op_cov(self):
        self.terms = swapped(self.terms)
        self.gp.cov = cov_of(self.terms)
        self.op_set_params()

    def op_update(self):
        self.gp.update()

    def op_variance_cache(self, steps=1, na=8):
        self.check_cache(steps, na)

    def op_function_samples(self, k=3, features=32, seed=5):
        terms, hp = self.terms, self.shp
        if not all(isinstance(t, str) and t in SPECTRAL for t in terms):
            with pytest.raises(NotImplementedError):
                self.gp.function_samples(k, features, seed)
            return
        fs = self.gp.function_samples(k, features, seed)
        nu, u, amp = pr.spectral_features(terms, hp, D, features, seed)
        xp = self.rng.random((Q, D))
        ref = pr.samples(terms, hp, self.sx, self.sy, xp, nu, u, amp, pr.weights(seed, nu.shape[0], k, amp), pr.noise_draws(seed, self.n, k))
        assert fs.cg_info["residual"] <= 2 * TOL and fs.cg_info["solves"] == -(-k // 16)
        self.held("function samples", N(fs(self.t(xp))), ref, yard_abs=1e-10)
        got = N(fs.grad(self.t(xp)))
        gref, bound = sample_grad_restated(fs, terms, hp, self.sx, xp)
        err = np.asarray(np.abs(got - gref), np.float64)
        print("%-40s err / bound %.2e" % ("function samples: grad", float((err / bound).max())))
        assert np.isfinite(got).all() and np.all(err <= bound)
        xq = self.t(self.xq)
        self.samples.append((fs, N(fs(xq)).tobytes(), N(fs.grad(xq)).tobytes()))

    def op_memoize(self):
        self.loss.memoize = not self.loss.memoize

    def point(self, at):
        if at == "last" and self.last_p is not None and self.last_p.shape == self.shp.shape:
            p = self.last_p
        elif at == "new":
            p = hp_for(self.terms, self.rng)
        else:
            p = self.shp
        self.last_p = p.copy()
        return self.last_p

    def check_loss(self, p, got):
        e = self.estimate(p)
        own = abs(e["loss"] - e["loss_limit"]) / abs(e["loss_limit"])
        self.record("Stochastic_MLE loss", abs(float(got) - e["loss_limit"]) / abs(e["loss_limit"]), sr.tol_of(own))

    def check_grad(self, p, got):
        e = self.estimate(p)
        bound = (2 * e["cond"] * TOL + 16 * e["own"] + (2 * (PROBES + 1) + 2) * EPS) * e["scale"]
        err = np.abs(np.asarray(got) - e["grad"])
        worst = int(np.argmax(err / bound))
        self.record("Stochastic_MLE gradient (of S_p)", float(err[worst] / e["scale"][worst]), float(bound[worst] / e["scale"][worst]))
        assert np.all(err <= bound)

    def check_grad_x(self, p, got):
        """Against the restatement on the DENSE factors: the solver's term plus the kernel's (module docstring)."""
        e = self.estimate(p)
        ref, scale = lx.lowrank_xgrad(self.terms, p, self.sx, None, e["u"], e["v"], np.longdouble)
        scale = np.asarray(scale, np.float64)
        rel = 2 * e["cond"] * TOL + 16 * e["own_dk"] + (self.n + 2 * (1 + PROBES) + 2) * EPS
        err = np.asarray(np.abs(np.asarray(got) - ref), np.float64)
        assert got.shape == self.sx.shape and np.isfinite(got).all()
        self.record("Stochastic_MLE grad_x (of S_ik)", float(np.max(err / scale)), rel)

    def check_factors(self, p):
        """weight_factors() against the dense solves, and grad / grad_x as the restatement on them at the kernels' own bounds."""
        e = self.estimate(p)
        u, v = self.loss.weight_factors()
        assert u.shape == v.shape == (self.n, 1 + PROBES) and u.flags.owndata and v.flags.owndata
        self.held("weight_factors: U", u, e["u"], yard_rel=1e-8, cond=e["cond"])
        self.held("weight_factors: V", v, e["v"], yard_rel=1e-8, cond=e["cond"])
        return u, v

    def check_on_factors(self, p, u, v, grad=None, gx=None):
        if gx is not None:
            ref, scale = lx.lowrank_xgrad(self.terms, p, self.sx, None, u, v, np.longdouble)
            bound = 16 * dr.own_dk(self.terms, p, self.sx, self.sx) + (self.n + 2 * (1 + PROBES) + 2) * EPS
            self.record("grad_x on its factors (of S_ik)", float(np.max(np.abs(gx - ref) / scale)), bound)
        if grad is not None:
            mine = lr.mine(self.terms, D)
            ref = lr.lowrank_grad(self.terms, p, self.sx, None, u, v, np.longdouble)
            scale = lr.scale(self.terms, p, self.sx, None, u, v)
            f64 = lr.lowrank_grad(self.terms, p, self.sx, None, u, v)
            own = max(float(np.max(np.abs(f64 - ref).astype(np.float64)[mine] / scale[mine])), EPS)
            err = np.asarray(np.abs(grad - ref), np.float64)[mine] / scale[mine]
            self.record("grad on its factors (of S_p)", float(err.max()), 16 * own + (2 * (PROBES + 1) + 2) * EPS)
            trace = float(np.sum(u * v))
            for t, blocks in kr._chunks(self.terms, D):
                if t == "wn":
                    o = blocks[0][1]
                    assert abs(grad[o] - 2.0 * p[o] * trace) <= 1e-12 * abs(2.0 * p[o] * trace) + 1e-300

    def op_sm(self, what, at="params"):
        p = self.point(at)
        got = getattr(self.loss, what)(p.copy())
        if what == "loss":
            self.check_loss(p, got)
        elif what == "grad":
            self.check_grad(p, got)
        elif what == "grad_x":
            self.check_grad_x(p, got)
        else:
            self.check_loss(p, got[0])
            self.check_grad(p, got[1])
            if what == "loss_and_grads":
                self.check_grad_x(p, got[2])
        assert self.loss.slq_info["rank"] == len(ir.factor_l(self.terms, p, self.sx, self.rank)[1])
        return got

    def op_weight_factors(self):
        p = self.point("params")
        self.loss.grad(p.copy())
        if self.loss.memoize:
            self.check_factors(p)
        else:
            with pytest.raises(RuntimeError, match="no evaluation is kept"):
                self.loss.weight_factors()

    def op_nlml_of_inputs(self):
        """The bridge assigns its x to the model: an assignment of x through another door."""
        x = self.rng.random((self.n, D))
        xt, pt = self.t(x).requires_grad_(True), T(self.shp.copy()).requires_grad_(True)
        val = pg.nlml_of_inputs(self.loss, xt, pt)
        self.sx = x
        self.changed()
        val.backward()
        assert self.gp.x.data_ptr() == xt.data_ptr() and not self.gp.x.requires_grad
        self.check_loss(self.shp, float(val.detach()))
        self.check_grad(self.shp, N(pt.grad))
        self.check_grad_x(self.shp, N(xt.grad))
        self.last_p = self.shp.copy()


for _w in ("loss", "grad", "loss_and_grad", "grad_x", "loss_and_grads"):
    setattr(IterWalk, "op_sm_" + _w, (lambda w: lambda self, at="params": self.op_sm(w, at))(_w))


# ---- Sparse_GP -----------------------------------------------------------------------------------------------------------------------
SPARSE_LOSSES = [o + "_" + w for o in ("vfe", "vfz") for w in ("loss", "grad", "loss_and_grad")]
SPARSE_CHANGES = {"set_params", "edit_x", "edit_y", "edit_z", "assign_x", "assign_y", "assign_z", "assign_z_m", "assign_cross", "select_inducing",
                  "write_back", "replace_z_twice", "replace_x_twice"}
SPARSE_KINDS = sorted(SPARSE_CHANGES | set(SPARSE_LOSSES) | {"update"})


class SparseWalk(_Walk):
    QUIET = set(SPARSE_LOSSES) | {"update"}

    def __init__(self, env, terms, n0, m0, whitened, seed=0):
        super().__init__(env, terms, seed)
        self.whitened = whitened
        self.sx, self.sy = draw(self.rng, n0)
        self.shp = hp_for(self.terms, self.rng)
        self.sz = self.pick(m0)
        self.gp = pg.Sparse_GP(self.t(self.sx), self.t(self.sy), cov_of(self.terms), self.t(self.sz), whitened=whitened)
        self.gp.set_params(T(self.shp.copy()))
        self.vfe, self.vfz = pg.VFE(self.gp), pg.VFE(self.gp, train_z=True)
        self.last = {}
        self.xq = self.rng.random((7, D))
        self.flip = False

    @property
    def n(self):
        return self.sx.shape[0]

    @property
    def m(self):
        return self.sz.shape[0]

    def pick(self, m):
        """m inducing inputs among x at pairwise distance >= 0.3 in scaled units, as sparse_ref.problem chooses them."""
        scale = min(self.shp[a + 1: a + 1 + D].min() for t, blocks in kr._chunks(self.terms, D) if t != "wn" for _, a, _ in blocks)
        return self.sx[sr.pick_z(self.sx, scale, m)].copy()

    # -- the shadow ------------------------------------------------------------------------------
    def both(self, hp, z, xp=None):
        """Every quantity at (hp, z) from the two restatements: (the model's own form, the other form)."""
        terms, x, y = self.terms, self.sx, self.sy
        lu, gu = sr.loss_and_grad(terms, hp, x, y, z)               # (a LinAlgError here: the walk left the region the cases are drawn from)
        lw, gw = wr.loss_and_grad(terms, hp, x, y, z)
        un = dict(loss=np.array(lu), grad=gu, zgrad=szr.z_grad(terms, hp, x, y, z))
        wh = dict(loss=np.array(lw), grad=gw, zgrad=wr.z_grad(terms, hp, x, y, z))
        if xp is not None:
            mu, cov = sr.predict(terms, hp, x, y, z, xp, var="full")
            dm, dv = szr.predict_grads(terms, hp, x, y, z, xp)
            un.update(mean=mu, cov=cov, var=np.diag(cov).copy(), dmean=dm, dvar=dv)
            mu, cov, kss = wr.predict(terms, hp, x, y, z, xp)
            dm, dv = wr.predict_grads(terms, hp, x, y, z, xp)
            wh.update(mean=mu, cov=cov, var=np.diag(cov).copy(), dmean=dm, dvar=dv)
            un["kss"] = wh["kss"] = float(np.max(kss))
        return (wh, un) if self.whitened else (un, wh)

    def hold(self, name, got, mine, other, scale=None):
        got, mine, other = (np.asarray(a, dtype=np.float64) for a in (got, mine, other))
        assert got.shape == mine.shape, (name, got.shape, mine.shape)
        scale = float(np.max(np.abs(mine))) if scale is None else scale
        own = float(np.max(np.abs(mine - other))) / scale
        assert np.isfinite(got).all()
        self.record("Sparse_GP " + name, float(np.max(np.abs(got - mine))) / scale, sr.tol_of(own))

    # -- observations ----------------------------------------------------------------------------
    def fixed_bits(self):
        gp, xq = self.gp, self.t(self.xq)
        out = list(gp.predict(xq, "diag")) + [gp.predict(xq, "full")[1]] + list(gp.predict_grad(xq, "diag"))
        return b"".join(N(o).tobytes() for o in out)

    def observe(self):
        gp = self.gp
        self.trace.append("    observe")
        xp = self.rng.random((Q, D))
        xpt = self.t(xp)
        mine, other = self.both(self.shp, self.sz, xp)
        vscale = mine["kss"] if self.whitened else None         # (test_sparse_whitened_gpu: variances relative to the prior variance)
        m0, none = gp.predict(xpt, "mean")
        assert none is NotImplemented
        m1, vd = gp.predict(xpt, "diag")
        m2, vf = gp.predict(xpt, "full")
        self.same_bits("mean (none / diag)", m0, m1)
        self.hold("predict diag: mean", N(m1), mine["mean"], other["mean"])
        self.hold("predict full: mean", N(m2), mine["mean"], other["mean"])
        self.hold("predict diag: variance", N(vd), mine["var"], other["var"], vscale)
        self.hold("predict full: covariance", N(vf), mine["cov"], other["cov"], vscale)
        assert torch.equal(vf, vf.T)
        g = gp.predict_grad(xpt, "diag")
        self.same_bits("predict_grad: mean", g[0], m1)
        self.same_bits("predict_grad: variance", g[1], vd)
        self.hold("predict_grad: d mean", N(g[2]), mine["dmean"], other["dmean"])
        self.hold("predict_grad: d variance", N(g[3]), mine["dvar"], other["dvar"])
        gn = gp.predict_grad(xpt, "none")
        self.same_bits("predict_grad none: mean", gn[0], m1)
        self.same_bits("predict_grad none: d mean", gn[1], g[2])
        assert not gp.need_upd
        assert np.array_equal(N(gp.z), self.sz) and np.array_equal(N(gp.params).reshape(-1), self.shp)
        self.fixed = self.fixed_bits()

    # -- operations ------------------------------------------------------------------------------
    def op_set_params(self, hp=None):
        self.shp = hp_for(self.terms, self.rng) if hp is None else np.asarray(hp, dtype=np.float64)
        self.gp.set_params(T(self.shp.copy()))
        self.changed()

    def _scale(self):
        c = 0.8 if self.flip else 1.25
        self.flip = not self.flip
        return c

    def op_edit_x(self):
        c = self._scale()
        self.gp.x.mul_(c)
        self.sx = self.sx * c
        self.changed()

    def op_edit_y(self):
        self.gp.y.mul_(0.5).add_(0.125)
        self.sy = self.sy * 0.5 + 0.125
        self.changed()

    def op_edit_z(self):
        self.gp.z.add_(0.015625)
        self.sz = self.sz + 0.015625
        self.changed()

    def op_assign_x(self):
        self.sx = self.rng.random((self.n, D))
        self.gp.x = self.t(self.sx)
        self.changed()

    def op_assign_y(self):
        self.sy = np.sin(3.0 * self.sx.sum(1)) + 0.1 * self.rng.standard_normal(self.n)
        self.gp.y = self.t(self.sy)
        self.changed()

    def op_assign_z(self):
        self.sz = self.pick(self.m)[::-1].copy() + 0.01 * self.rng.standard_normal((self.m, D))
        self.gp.z = self.t(self.sz)
        self.changed()

    def op_assign_z_m(self):
        """A z with another m (20 <-> 37): every m-sized buffer of the pool has the other shape."""
        self.sz = self.pick(37 if self.m == 20 else 20)
        self.gp.z = self.t(self.sz)
        self.changed()

    def op_assign_cross(self):
        self.sx, self.sy = draw(self.rng, 300 if self.n <= 256 else 200)
        self.gp.x = self.t(self.sx)
        self.gp.y = self.t(self.sy)
        self.changed()

    def op_select_inducing(self):
        mark = dict(self.env.spies.n)
        res = self.gp.select_inducing()
        piv = sel.greedy(self.terms, self.shp, self.sx, self.m, ir.JITTER).piv
        assert self.env.spies.since(mark)["greedy_select"] == 1
        assert np.array_equal(N(res.index), piv), "the selection is not the restatement's"
        self.sz = self.sx[piv].copy()
        self.changed()

    def op_update(self):
        self.gp.update()

    def op_replace_z_twice(self):
        z1, z2 = self.pick(self.m) + 0.02, self.pick(self.m) - 0.02
        self.gp.z = self.one_call(z1)
        self.gp.z = self.one_call(z2)
        gc.collect()
        self.sz = z2
        self.changed()

    def op_replace_x_twice(self):
        x1, x2 = self.rng.random((self.n, D)), self.rng.random((self.n, D))
        self.gp.x = self.one_call(x1)
        self.gp.x = self.one_call(x2)
        gc.collect()
        self.sx = x2
        self.changed()

    def set_x(self, x, at=()):
        self.gp.x = self.one_call(x, at)
        self.sx = np.array(x)
        self.changed()
        return id(self.gp.x)

    def set_z(self, z, at=()):
        self.gp.z = self.one_call(z, at)
        self.sz = np.array(z)
        self.changed()
        return id(self.gp.z)

    def point(self, obj, at):
        """(hp, z, the vector the loss takes) at the model's point, the last point of this loss, or a new one."""
        last = self.last.get(obj)
        if at == "last" and last is not None and last[0].shape == self.shp.shape and last[1].shape == self.sz.shape:
            hp, z = last
        elif at == "new":
            hp = hp_for(self.terms, self.rng)
            z = self.sz + 0.01 * self.rng.standard_normal(self.sz.shape)
        else:
            hp, z = self.shp, self.sz
        if obj == "vfe":
            z = self.sz                      # (z is data to VFE(model): it evaluates at the model's own)
        self.last[obj] = (hp.copy(), z.copy())
        return hp, z, (szr.pack(hp, z) if obj == "vfz" else hp.copy())

    def op_eval(self, obj, what, at="params"):
        hp, z, vec = self.point(obj, at)
        got = getattr(getattr(self, obj), what)(vec.copy())
        mine, other = self.both(hp, z)
        if obj == "vfz":
            for d in (mine, other):
                d["grad"] = szr.pack(d["grad"], d["zgrad"])
        name = "VFE" + ("(train_z)" if obj == "vfz" else "")
        if what != "grad":
            self.hold(name + " loss", np.asarray(got if what == "loss" else got[0]), mine["loss"], other["loss"])
        if what != "loss":
            self.hold(name + " gradient", got if what == "grad" else got[1], mine["grad"], other["grad"])

    def op_write_back(self):
        """An optimiser's last act: the packed vector goes into the model."""
        hp = hp_for(self.terms, self.rng)
        z = self.sz + 0.01 * self.rng.standard_normal(self.sz.shape)
        vec = szr.pack(hp, z)
        self.vfz.loss_and_grad(vec.copy())                      # (the memo now holds the very vector that is written back)
        self.vfz.write_back(vec.copy())
        self.shp, self.sz = hp, z
        self.changed()
        assert self.gp.need_upd
        assert np.array_equal(N(self.gp.z), z) and np.array_equal(N(self.gp.params).reshape(-1), hp)
        mark = dict(self.env.spies.n)
        self.last["vfz"] = (hp.copy(), z.copy())
        self.op_eval("vfz", "loss_and_grad", "last")
        assert self.env.spies.since(mark)["potrf"] == 2, "the memo survived write_back"


for _o in ("vfe", "vfz"):
    for _w in ("loss", "grad", "loss_and_grad"):
        setattr(SparseWalk, "op_%s_%s" % (_o, _w), (lambda o, w: lambda self, at="params": self.op_eval(o, w, at))(_o, _w))


# ---- random walks --------------------------------------------------------------------------------------------------------------------
def iter_plan(seed, steps=20):
    rng = random.Random(seed)
    weights = {k: 1 for k in ITER_KINDS}
    weights.update(set_params=2, update=1, memoize=1)
    out = []
    while len(out) < steps:
        name = rng.choices(list(weights), list(weights.values()))[0]
        args = (rng.choice(["params", "last", "new"]),) if name in ITER_LOSSES else ()
        if name == "variance_cache":
            args = (rng.choice([0, 1]), rng.choice([0, 8]))
        out.append((name, args))
    return out


def sparse_plan(seed, steps=20):
    rng = random.Random(seed)
    weights = {k: 1 for k in SPARSE_KINDS}
    weights.update(set_params=2)
    out = []
    while len(out) < steps:
        name = rng.choices(list(weights), list(weights.values()))[0]
        out.append((name, (rng.choice(["params", "last", "new"]),) if name in SPARSE_LOSSES else ()))
    return out


# (seed, kind, n0, rank)
ITER_WALKS = [(200, "se+wn", 150, 20), (201, "m32+rq+wn", 230, 40), (202, "(se*per)+wn", 310, 0), (203, "se+wn", 260, 40)]
# (seed, kind, n0, m0, whitened)
SPARSE_WALKS = [(200, "se+wn", 150, 20, False), (201, "m32+rq+wn", 230, 37, True), (202, "(se*per)+wn", 310, 20, True), (203, "se+wn", 270, 37, False)]


def run_iter_walk(env, seed, kind, n0, rank):
    ops = iter_plan(seed)
    w = IterWalk(env, KINDS[kind], n0, rank, seed)
    for name, args in ops:
        w.step(name, *args)
    env.table()
    return w


def run_sparse_walk(env, seed, kind, n0, m0, whitened):
    ops = sparse_plan(seed)
    w = SparseWalk(env, KINDS[kind], n0, m0, whitened, seed)
    for name, args in ops:
        w.step(name, *args)
    env.table()
    return w


def coverage():
    """{family: (operation kinds over its committed walks, the state changes of each walk)}."""
    out = {}
    for fam, walks, plan, changes in (("iterative", ITER_WALKS, iter_plan, ITER_CHANGES), ("sparse", SPARSE_WALKS, sparse_plan, SPARSE_CHANGES)):
        seen, counts = collections.Counter(), []
        for wk in walks:
            ops = plan(wk[0])
            seen.update(name for name, _ in ops)
            counts.append(sum(name in changes for name, _ in ops))
        out[fam] = (seen, counts)
    return out


# ---- scripted sequences --------------------------------------------------------------------------------------------------------------
need = sw.need


def _bits(*arrays):
    return b"".join(np.asarray(a).tobytes() for a in arrays)


def seq_grad_x_at_a_reused_address(env, tries=12):
    """Sequence 1: x = A, grad_x(p); x = B, loss(p) -- the loss memo now names B, nothing names A; x = C, grad_x(p).  When C lands at A's
    address (version 0 like A's) the memo of grad_x, keyed on id()s, must not serve A's gradient.  A try counts only when id() was in
    fact re-used; none counted is a failure.  Returns (tries that re-used the address, the largest difference from a fresh loss)."""
    w = IterWalk(env, KINDS["se+wn"], 60, 20, seed=21)
    p = w.shp.copy()
    reused, worst = 0, 0.0
    for i in range(tries):
        ida = w.set_x(w.rng.random((60, D)))
        w.loss.grad_x(p.copy())
        w.set_x(w.rng.random((60, D)))
        w.loss.loss(p.copy())
        gc.collect()
        idc = w.set_x(w.rng.random((60, D)), at=(ida,))
        got = w.loss.grad_x(p.copy())
        fresh = pg.Stochastic_MLE(w.gp, probes=PROBES, seed=SEED).grad_x(p.copy())
        diff = float(np.max(np.abs(got - fresh)))
        worst = max(worst, diff)
        reused += idc == ida
        print("try %2d: address %s, grad_x differs from a fresh loss object's by %.3g in max-abs" % (i, "RE-USED" if idc == ida else "new", diff))
        assert got.tobytes() == fresh.tobytes(), "grad_x served the gradient of the data that lay at this address before (max-abs %.3g)" % diff
        w.check_grad_x(p, got)
    assert reused >= 1, "no try re-used an address: the sequence proved nothing"
    env.table()
    return reused, worst


def _replaced(w, evaluate, setter, fresh, tries):
    """evaluate; replace twice through `setter` with no evaluation in between; evaluate: never the old data's value.  Returns how often
    the id() of an earlier tensor of the walk came back (a memo that keeps its keyed tensors alive never meets ITS address again)."""
    seen, reused = set(), 0
    for _ in range(tries):
        evaluate()
        seen.add(setter(fresh()))
        gc.collect()
        now = setter(fresh(), at=frozenset(seen))
        reused += now in seen
        seen.add(now)
        evaluate()
    return reused


def seq_loss_at_a_reused_address(env, tries=12):
    """The same pattern for Stochastic_MLE.loss and grad: each checked against the shadow at the data of the moment."""
    w = IterWalk(env, KINDS["se+wn"], 60, 20, seed=22)

    def evaluate():
        w.step("sm_loss", observe=False).step("sm_grad", observe=False)

    reused = _replaced(w, evaluate, w.set_x, lambda: w.rng.random((60, D)), tries)
    print("ids that came back: %d" % reused)
    assert reused >= 1, "no id() came back: the sequence proved nothing"
    env.table()
    return reused


def seq_vfe_at_a_reused_address(env, which, tries=12):
    """... and for both VFE objects with x (which = "x") or z replaced."""
    w = SparseWalk(env, KINDS["se+wn"], 150, 20, False, seed=23)

    def evaluate():
        w.step("vfe_loss", observe=False).step("vfz_grad", observe=False).step("vfe_grad", observe=False)

    if which == "x":
        reused = _replaced(w, evaluate, w.set_x, lambda: w.rng.random((150, D)), tries)
    else:
        reused = _replaced(w, evaluate, w.set_z, lambda: w.pick(20) + 0.01 * w.rng.standard_normal((20, D)), tries)
    print("ids that came back: %d" % reused)
    assert reused >= 1, "no id() came back: the sequence proved nothing"
    w.observe()
    env.table()
    return reused


def seq_kept_solve(env, kind="se+wn"):
    """Sequence 2: grad_x, loss, grad; loss_and_grads; grad again; weight_factors() after each.  One solve per distinct (params, data)
    point, one gradient kernel of each sort per first request, every value the restatement on the factors, grad after grad_x the bits of
    a grad that never met grad_x (the in-place scaling of the factors happens once).  Then the same with memoize off: every call solves,
    the values are unchanged.  Changing the solver's settings is seen by the key."""
    w = IterWalk(env, KINDS[kind], 170, 20, seed=24)
    loss, p = w.loss, w.shp.copy()
    count = lambda: (loss.solves, loss.grad_calls, loss.xgrad_calls)      # noqa: E731
    gx = loss.grad_x(p.copy())
    assert count() == (1, 0, 1)
    u0, v0 = w.check_factors(p)
    w.check_on_factors(p, u0, v0, gx=gx)
    w.check_grad_x(p, gx)
    w.check_loss(p, loss.loss(p.copy()))
    assert count() == (1, 0, 1)
    g = loss.grad(p.copy())
    assert count() == (1, 1, 1)
    u1, v1 = w.check_factors(p)
    assert _bits(u0, v0) == _bits(u1, v1), "the factors were scaled a second time"
    w.check_on_factors(p, u1, v1, grad=g)
    w.check_grad(p, g)
    plain = pg.Stochastic_MLE(w.gp, probes=PROBES, seed=SEED)             # a loss that never computes grad_x
    assert plain.grad(p.copy()).tobytes() == g.tobytes(), "grad after grad_x is not the grad of a fresh loss"
    l2, g2, gx2 = loss.loss_and_grads(p.copy())
    assert count() == (1, 1, 1) and _bits(g2, gx2) == _bits(g, gx)
    assert loss.grad(p.copy()).tobytes() == g.tobytes() and count() == (1, 1, 1)
    assert _bits(*loss.weight_factors()) == _bits(u0, v0)
    # another point: one more solve, and each kernel once more at its first request
    other = hp_for(w.terms, w.rng)
    lo, go, gxo = loss.loss_and_grads(other.copy())
    assert count() == (2, 2, 2)
    w.check_loss(other, lo), w.check_grad(other, go), w.check_grad_x(other, gxo)
    uo, vo = w.check_factors(other)
    w.check_on_factors(other, uo, vo, grad=go, gx=gxo)
    assert loss.grad(other.copy()).tobytes() == go.tobytes() and count() == (2, 2, 2)
    # back at p: the memo holds one point
    assert loss.grad_x(p.copy()).tobytes() == gx.tobytes() and count() == (3, 2, 3)
    # the solver's settings are part of the key
    w.gp.max_iter = 999
    assert loss.grad_x(p.copy()).tobytes() == gx.tobytes() and count() == (4, 2, 4)
    # memoize off: every call solves, the values are the same bits
    loss.memoize = False
    base = count()
    assert loss.grad_x(p.copy()).tobytes() == gx.tobytes() and np.asarray(loss.loss(p.copy())).tobytes() == np.asarray(l2).tobytes()
    assert loss.grad(p.copy()).tobytes() == g.tobytes()
    l3, g3, gx3 = loss.loss_and_grads(p.copy())
    assert _bits(l3, g3, gx3) == _bits(l2, g, gx)
    assert count() == (base[0] + 5, base[1] + 2, base[2] + 2), count()
    with pytest.raises(RuntimeError, match="no evaluation is kept"):
        loss.weight_factors()
    loss.memoize = True
    assert loss.grad(p.copy()).tobytes() == g.tobytes()
    w.observe()
    env.table()


def seq_evaluation_leaves_the_iterative_fit(env):
    """Sequence 3: update, predict, loss_and_grads at OTHER parameters, predict: same bits, nothing selected or factored for the model."""
    w = IterWalk(env, KINDS["m32+rq+wn"], 200, 20, seed=25)
    w.step("update")
    mark = dict(env.spies.n)
    before = w.fixed_bits()
    since = env.spies.since(mark)
    need(since, greedy_select=0, potrf=0)
    mark = dict(env.spies.n)
    w.step("sm_loss_and_grads", "new", observe=False)
    need(env.spies.since(mark), greedy_select=1, potrf=2, kernel_lowrank_grad=1, kernel_lowrank_xgrad=1)
    mark = dict(env.spies.n)
    assert w.fixed_bits() == before and not w.gp.need_upd
    need(env.spies.since(mark), greedy_select=0, potrf=0)
    w.observe()
    env.table()


def seq_evaluation_leaves_the_sparse_fit(env, whitened):
    """Sequence 3 for Sparse_GP, several chunks with a ragged last one: both VFE objects evaluate at other points through the shared
    scratch pool; predict and predict_grad keep their bits."""
    w = SparseWalk(env, KINDS["se+wn"], 300, 37, whitened, seed=26)
    w.step("update")
    before = w.fixed_bits()
    mark = dict(env.spies.n)
    w.step("vfe_loss_and_grad", "new", observe=False).step("vfz_loss_and_grad", "new", observe=False)
    since = env.spies.since(mark)
    need(since, potrf=4, kernel_cross_grad=2 * (1 + 3))          # each: Kuu once, three chunks of 128, 128 and 44 in pass 2
    assert w.fixed_bits() == before and not w.gp.need_upd
    w.step("vfe_loss", "new", observe=False).step("vfz_loss", "last", observe=False)
    assert w.fixed_bits() == before
    w.observe()
    env.table()


def seq_update_refits_once(env):
    """Sequence 4: update() on a clean model launches nothing; after set_params, an assignment, an in-place edit (a version bump alone)
    and a z assignment it refits exactly once."""
    def launches(since):
        return sum(since.values())

    wi = IterWalk(env, KINDS["se+wn"], 150, 20, seed=27)
    ws = SparseWalk(env, KINDS["se+wn"], 150, 20, False, seed=27)
    for w, changes, fit in ((wi, ("set_params", "assign_x", "assign_y", "edit_x", "edit_y"), "greedy_select"),
                            (ws, ("set_params", "assign_x", "assign_y", "assign_z", "edit_x", "edit_y", "edit_z"), "potrs_vec")):
        w.step("update", observe=False)
        for change in changes:
            w.step(change, observe=False)
            mark = dict(env.spies.n)
            w.gp.update()
            assert env.spies.since(mark)[fit] == 1 and not w.gp.need_upd, "%s: update() did not refit once" % change
            mark = dict(env.spies.n)
            w.gp.update()
            assert launches(env.spies.since(mark)) == 0, "%s: update() on a clean model launched %s" % (change, dict(env.spies.since(mark)))
            w.observe()
    env.table()


def seq_snapshots(env):
    """Sequence 5: caches and function samples; set_params, a refit, assignments: the old snapshots keep their bits (checked by every
    observation), new ones match the shadow at the new state."""
    w = IterWalk(env, KINDS["se+wn"], 180, 20, seed=28)
    w.step("function_samples", 3, 32, 5).step("variance_cache", 1, 8)
    w.step("set_params").step("function_samples", 17, 16, 6).step("variance_cache", 0, 0)
    w.step("assign_y").step("assign_x").step("assign_cross").step("function_samples", 2, 32, 5).step("variance_cache", 1, 0)
    assert len(w.samples) == 3 and len(w.caches) >= 2
    w.step("edit_y").step("edit_x")                  # the FunctionSamples survive these as well
    assert len(w.samples) == 3
    env.table()


def seq_failure_leaves_the_iterative_model_usable(env):
    """Sequence 6: max_iter = 1 raises NotConverged out of update() and out of loss(); with max_iter restored the next predict and loss
    are right and no half-kept solve is reused."""
    w = IterWalk(env, KINDS["se+wn"], 200, 20, seed=29)
    w.step("sm_loss", observe=False)
    w.gp.max_iter = 1
    w.step("set_params", observe=False)
    with pytest.raises(pg.NotConverged):
        w.gp.update()
    assert w.gp.need_upd and w.gp._state is None
    with pytest.raises(pg.NotConverged):
        w.loss.loss(w.shp.copy())
    with pytest.raises(pg.NotConverged):
        w.loss.grad_x(w.shp.copy())
    assert w.loss._kept is None
    w.gp.max_iter = 1000
    solves = w.loss.solves
    w.step("sm_grad_x", observe=False).step("sm_loss", observe=False).step("sm_grad")
    assert w.loss.solves == solves + 1
    env.table()


def seq_failure_leaves_the_sparse_model_usable(env, whitened):
    """... and a Sparse_GP at a parameter point where the shadow's own factorisation fails (a NaN length scale: LAPACK refuses the
    shadow's Kuu as the library's factorisation refuses the model's)."""
    w = SparseWalk(env, KINDS["se+wn"], 200, 20, whitened, seed=30)
    w.step("update")
    good = w.shp.copy()
    bad = good.copy()
    bad[2] = np.nan
    with pytest.raises((np.linalg.LinAlgError, ValueError)):
        sr.loss_and_grad(w.terms, bad, w.sx, w.sy, w.sz)
    w.gp.set_params(T(bad.copy()))
    with pytest.raises(torch.linalg.LinAlgError):
        w.gp.update()
    assert w.gp.need_upd
    with pytest.raises(torch.linalg.LinAlgError):
        w.vfe.loss_and_grad(bad.copy())
    with pytest.raises(torch.linalg.LinAlgError):
        w.gp.predict(w.t(w.xq), "diag")
    w.step("set_params", good).step("vfe_loss_and_grad").step("vfz_loss_and_grad")
    env.table()


def seq_write_back(env, whitened):
    """Sequence 7: write_back of a packed vector, then predict at the new z."""
    w = SparseWalk(env, KINDS["(se*per)+wn"], 230, 37, whitened, seed=31)
    w.step("update").step("write_back").step("vfz_loss", "new").step("write_back")
    env.table()


def flipped(terms, hp):
    """hp with the sign of one sigma, one l_k, the noise and (rq / per) the shape or one period entry flipped; the flipped offsets."""
    hp, offs = hp.copy(), []
    for t, blocks in kr._chunks(terms, D):
        part, a, b = blocks[-1]
        offs += [a] if part == "wn" else [a, a + 2] + ([b - 1] if part in ("rq", "per") else [])
    hp[offs] *= -1.0
    return hp, offs


def seq_signs(env, kind, family, whitened=False):
    """Sequence 8: the hyper-parameters enter squared.  Every observation and the loss at params with flipped signs equal the shadow's at
    those params (which the shadow evaluates itself), and the gradient entries of the flipped parameters change sign."""
    terms = KINDS[kind]
    if family == "iterative":
        w = IterWalk(env, terms, 160, 20, seed=32)
        pos = w.shp.copy()
        neg, offs = flipped(terms, pos)
        lp, gp_, gxp = w.op_sm("loss_and_grads", "params")
        w.step("set_params", neg)
        ln, gn, gxn = w.op_sm("loss_and_grads", "params")
        bound_x = None
    else:
        w = SparseWalk(env, terms, 160, 20, whitened, seed=32)
        pos = w.shp.copy()
        neg, offs = flipped(terms, pos)
        lp, gp_ = w.vfz.loss_and_grad(szr.pack(pos, w.sz))
        w.step("set_params", neg).step("vfe_loss_and_grad").step("vfz_loss_and_grad")
        ln, gn = w.vfz.loss_and_grad(szr.pack(neg, w.sz))
    sign = np.ones(gp_.size)
    sign[offs] = -1.0
    print("flipped entries %s: loss %.12g / %.12g" % (offs, float(lp), float(ln)))
    scale = np.abs(gp_) + 1e-300
    print("gradient entries, |g(-) - sign g(+)| / |g|: %s" % np.array2string(np.abs(gn - sign * gp_) / scale, precision=2))
    assert np.all(np.sign(gn[offs]) == -np.sign(gp_[offs])), "the gradient entries of the flipped parameters did not change sign"
    env.table()
