"""The walker of Exact_GP's cached state (helper module: no tests in it).

A `Walk` holds a model under test and a SHADOW of it: plain fp64 NumPy x, y, hyper-parameters, the term list in the grammar of
tests/kernel_ref.py, and whether a fit is due.  The shadow never calls pygpr_amd; it answers every observation from scratch:

    K = kernel_ref.kernel + (sum sigma_n^2 + 1e-7) I,  numpy.linalg.cholesky / solve,  NLML and gradient by kernel_ref,
    leave-one-out by loo_ref,  derivatives in the test points by xgrad_ref (kernel_ref for the kinds xgrad_ref does not have)

Every OPERATION (`Walk.step`) is applied to the model and to the shadow, and is followed by every OBSERVATION (`Walk.observe`): predict
for "diag", "full" and a third value, predict_grad, loo_predict, wt, krnchd, a new sampler's mean and factor, and bit-identical draws of
the samplers made earlier.  The device ops are wrapped in counting spies (`Spies`: attributes of the ops OBJECT, the library is not
patched), so a scripted sequence can state which ops must have run.  On a failure the seed and the trace of operations are printed.

The sampler is asked for `jitter = SAMPLER_JITTER[dtype]`, not for its default 1e-7: its factor is compared ENTRY BY ENTRY with
numpy.linalg.cholesky of the shadow's covariance (noise removed, jitter added), and the factor of C + J I moves by up to cond(C + J I)
times the relative difference of the two covariances (tests/test_sample_gpu.py holds the default jitter to the backward error L L^T
instead, which does not depend on the conditioning).  The latent posterior covariance has max |C| about 1 and cond(C + J I) <= m / J.
fp64, J = 1e-2: the covariances of the two sides differ by 5e-14 of max |C| (measured, both tiers) and the factors by 4e-13, where
J = 1e-3 gave 2e-12 and J = 1e-4 9e-12: a thousandth of TOL64 and well inside the CPU tier's 1e-11, while a wrong expert, chunk or buffer
moves C by far more than J.  fp32: J = sigma_n^2 = 0.09 puts C + J I at the conditioning TOL32 was derived for
(tests/test_append_gpu.py); at 1e-7 the fp32 latent covariance is not reliably positive definite (tests/test_sample_gpu.py).

The scripted sequences and the plans of the random walks are here, so that the CPU tier (tests/test_state_walk_cpu.py, on the oracle
double `WalkOracleOps`) and the GPU tier (tests/test_state_walk_gpu.py, on the library) run the same ones.  The committee (GRBCM and
GRBCM_MLE) is walked by tests/state_walk_grbcm.py, on this module's `Env`, `Spies`, `Fit` and double."""
import collections
import gc
import random

import numpy as np
import pytest
import scipy.linalg as sla
import torch

import append_ref as ar
import kernel_ref as kr
import loo_ref as lr
import xgrad_ref as xr
import pygpr_amd as pg
from kind_tools import T, cov_of, rel
from oracle_ops import KindOracleOps, _np
from pygpr_amd import _ops
from pygpr_amd import gpr as gpr_mod
from pygpr_amd import loss as loss_mod
from test_loo_cpu import LooOracleOps
from test_sample_cpu import SampleOracleOps

F64, F32 = torch.float64, torch.float32
D = 3
SIGMA_N = 0.3
JITTER = 1e-7
# the append tests' own bounds (tests/test_append_gpu.py): largest error over largest reference entry
TOL64, TOL32 = 1e-9, 1e-3
TOL_DOUBLE = 1e-11      # the CPU tier: oracle against oracle
SAMPLER_JITTER = {F64: 1e-2, F32: SIGMA_N ** 2}
N_PAD_MAX = 768

SE_WN, M52_WN, SEPER_WN = ["se", "wn"], ["m52", "wn"], [("se", "per"), "wn"]
FIVE = ["se", "m52", "m32", "m12", "se", "wn"]         # five stationary children: two passes of pg_covspec
KINDS = {"se+wn": SE_WN, "m52+wn": M52_WN, "(se*per)+wn": SEPER_WN}
SAME_NHP = {"se": "m52", "m52": "se", "m32": "m12", "m12": "m32", "per": "per", "wn": "wn"}     # another cov of the same nhp


def swapped(terms):
    out = []
    for t in terms:
        out.append(tuple(SAME_NHP[p] for p in t) if isinstance(t, tuple) else SAME_NHP[t])
    return out


# ---- the CPU double ------------------------------------------------------------------------------------------------------------------
class WalkOracleOps(LooOracleOps, SampleOracleOps, KindOracleOps):
    """The oracle doubles of the kinds, the leave-one-out ops and the sampler in one object, plus what the walk needs beyond them:
    pg_chol_append by tests/append_ref.py, the matrix solve and the contraction of the test-point derivatives by kernel_ref."""

    def __init__(self):
        LooOracleOps.__init__(self)
        SampleOracleOps.__init__(self)

    def potrs(self, chol, invd, b, minv=None, triangular_only=False):
        assert not triangular_only
        x = sla.cho_solve((np.tril(_np(chol).astype(np.float64)), True), _np(b).astype(np.float64), check_finite=False)
        return torch.from_numpy(x).to(b.dtype)

    def kernel_xgrad_batched(self, spec, hp_all, xq, z_all, u_all=None, b_all=None, out_u=None, out_b=None, trans_b=False, accumulate=False,
                             nexp=None):
        nexp = nexp or max(hp_all.shape[0], z_all.shape[0], xq.shape[0] if xq.dim() == 3 else 1,
                           *(t.shape[0] for t in (u_all, b_all) if t is not None))
        m, d = xq.shape[-2], xq.shape[-1]
        n = z_all.shape[-2]
        if u_all is not None and out_u is None:
            out_u = self.empty(nexp, m, d, dtype=xq.dtype)
        if b_all is not None and out_b is None:
            out_b = self.empty(nexp, m, d, dtype=xq.dtype)

        def put(out, val):
            val = torch.from_numpy(val).to(out.dtype)
            out.copy_(out + val if accumulate else val)

        for e in range(nexp):
            model, h, _ = self._model(spec, _np(hp_all[e % hp_all.shape[0]]), d)
            xe = xq if xq.dim() == 2 else xq[e % xq.shape[0]]
            dks = kr.kernel_xgrad(model, h, _np(z_all[e % z_all.shape[0]]).astype(np.float64), _np(xe).astype(np.float64))    # [d, m, n]
            if u_all is not None:
                put(out_u[e], np.einsum("kpi,i->pk", dks, _np(u_all[e]).astype(np.float64)[:n]))
            if b_all is not None:
                b = _np(b_all[e]).astype(np.float64)
                put(out_b[e], np.einsum("kpi,pi->pk", dks, b[:n, :m].T if trans_b else b[:m, :n]))
        return out_u, out_b

    def chol_append_worksize(self, n_pad, k, dtype):
        return 1

    def chol_append(self, n, k, chol, invd, minv, kt, knn, y_new, u, alpha, work, info):
        n_pad = chol.shape[0]
        f = [_np(t).astype(np.float64) for t in (chol, invd[: n_pad * 128].view(n_pad // 128, 128, 128), minv, u, alpha)]
        out = ar.append(*f, n, _np(kt).astype(np.float64)[:k], _np(knn).astype(np.float64)[:k, :k], _np(y_new).astype(np.float64)[:k])
        info[0] = int(out[5])
        if out[5] == 0:
            for t, a in zip((chol, invd[: n_pad * 128].view(n_pad // 128, 128, 128), minv, u, alpha), out[:5]):
                t.copy_(torch.from_numpy(a))


@pytest.fixture
def walk_ops(monkeypatch, tmp_path):
    ops = WalkOracleOps()
    monkeypatch.setattr(_ops, "_OPS", ops)
    monkeypatch.chdir(tmp_path)
    return ops


# ---- spies ---------------------------------------------------------------------------------------------------------------------------
SPIED = ["build_factor", "build_factor_batched", "potrs_vec", "trtri", "trmv", "alpha_batched", "chol_append", "kernel_build",
         "kernel_build_batched", "predict_mean_q_kt", "predict_mean_q_kt_batched", "trmm_lower_kt", "syrk_nt_sub_batched", "loo_terms",
         "potrf", "potrf_trtri_batched", "alpha_nlml_batched", "nlml_grad", "nlml_grad_batched", "lauum", "kernel_xgrad_batched"]


class Spies:
    """Counting wrappers around the methods of the ops object.  `trmm_lower_kt` is also counted by the form of its first operand: a list
    of views, one matrix, or a stack."""

    def __init__(self, monkeypatch, ops, names=None):
        self.n = collections.Counter()
        for name in (SPIED if names is None else names):
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))

    def _wrap(self, name, real):
        def spy(*args, **kwargs):
            self.n[name] += 1
            if name == "trmm_lower_kt":
                form = "list" if isinstance(args[0], (list, tuple)) else ("stack" if args[0].dim() == 3 else "one")
                self.n[name + ":" + form] += 1
            return real(*args, **kwargs)

        return spy

    def since(self, mark):
        """Calls since `mark = dict(spies.n)`."""
        return collections.Counter({k: v - mark.get(k, 0) for k, v in self.n.items() if v != mark.get(k, 0)})


class Env:
    """What a tier gives the sequences: the ops object with its spies, monkeypatch, and the bounds.  spied: the ops to count (Exact_GP's
    by default); device: where the walks create their tensors (None: on the host, whatever the ops object is)."""

    def __init__(self, ops, monkeypatch, tol64, tol32, deriv=10, spied=None, device=None):
        self.ops, self.monkeypatch, self.deriv = ops, monkeypatch, deriv     # deriv: the factor on the bound of a derivative
        self.device = device
        self.spies = Spies(monkeypatch, ops, spied)
        self.tol = {F64: tol64, F32: tol32}
        self.errors = {}

    def patch(self, **consts):
        """Size gates of the library, set in gpr and (where loss.py imported its own copy) in loss."""
        for name, val in consts.items():
            self.monkeypatch.setattr(gpr_mod, name, val)
            if hasattr(loss_mod, name):
                self.monkeypatch.setattr(loss_mod, name, val)

    def table(self):
        print("largest error of each quantity:")
        for name in sorted(self.errors):
            print("    %-28s %.2e (bound %.0e)" % ((name,) + self.errors[name]))


# ---- the shadow ----------------------------------------------------------------------------------------------------------------------
def hp_for(terms, rng):
    hp = []
    for p in kr.flat(terms):
        if p == "wn":
            hp += [SIGMA_N]
        else:
            hp += [rng.uniform(0.8, 1.3)] + list(rng.uniform(0.5, 1.5, D) / np.sqrt(D)) + (list(rng.uniform(0.7, 2.5, D)) if p == "per" else [])
    return np.array(hp)


def noise_var(terms, hp):
    return float(sum(hp[a] ** 2 for t, blocks in kr._chunks(terms, D) if t == "wn" for _, a, _ in blocks))


class Fit:
    """One expert of the shadow, from scratch."""

    def __init__(self, terms, hp, x, y):
        self.terms, self.hp, self.x, self.y = terms, hp, x, y
        k = kr.kernel(terms, hp, x)
        k[np.diag_indices_from(k)] += JITTER
        self.chol = np.linalg.cholesky(k)
        self.alpha = np.linalg.solve(self.chol.T, np.linalg.solve(self.chol, y))

    def predict(self, xp):
        ks = kr.kernel(self.terms, self.hp, self.x, xp)
        kss = kr.kernel(self.terms, self.hp, xp)
        v = np.linalg.solve(self.chol, ks.T)
        return ks @ self.alpha, np.diag(kss) - (v * v).sum(0), kss - v.T @ v

    def predict_grads(self, xp):
        if all(isinstance(t, str) and t in ("se", "m52", "m32", "m12", "wn") for t in self.terms):
            out = xr.predict_grads(self.terms, T(self.hp), T(self.x), T(self.y), T(xp))
            return out[2].numpy(), out[3].numpy()
        return kr.predict_grads(self.terms, self.hp, self.x, self.y, xp)


# ---- the walk ------------------------------------------------------------------------------------------------------------------------
CHANGES = {"set_params", "set_rows", "edit_x", "edit_y", "replace_twice", "assign_same", "assign_cross", "assign_experts", "append", "append_dirty",
           "toggle_eager", "cov"}
LOSSES = [c + "_" + w for c in ("mle", "loo") for w in ("loss", "grad", "loss_and_grad")]
ALL_KINDS = sorted(CHANGES - {"replace_twice"} | set(LOSSES) | {"update", "append_nan", "illegal_append", "illegal_loo"})


class Walk:
    def __init__(self, env, terms, n0, dtype=F64, seed=0, eager=False, experts=1, m_cycle=(37,)):
        self.env, self.terms, self.dtype, self.seed = env, list(terms), dtype, seed
        self.tol = env.tol[dtype]
        self.rng = np.random.default_rng(seed)
        self.trace = []
        self.m_cycle, self.m_at = tuple(m_cycle), 0
        self.n0 = n0
        self.sx, self.sy = self.draw(n0, experts)
        self.shp = hp_for(self.terms, self.rng)
        self.dirty = True
        self.gp = pg.Exact_GP(self.t(self.sx), self.t(self.sy), cov_of(self.terms), eager_inverse=eager)
        self.gp.set_params(T(self.shp.copy()))
        self.losses = {}
        self.last_p = None
        self.samplers = []          # (sampler, its draws): the first one made and the latest

    # -- data ----------------------------------------------------------------------------------
    def rnd(self, a):
        """Rounded to the model's dtype, as fp64."""
        return T(np.asarray(a, dtype=np.float64)).to(self.dtype).double().numpy()

    def t(self, a):
        t = T(np.ascontiguousarray(a)).to(self.dtype).clone()           # (never the shadow's memory)
        return t if self.env.device is None else t.to(self.env.device)

    def draw(self, n, experts=1):
        shape = (n, D) if experts == 1 else (experts, n, D)
        x = self.rnd(self.rng.random(shape))
        y = self.rnd(np.sin(3.0 * x).sum(-1) + 0.1 * self.rng.standard_normal(shape[:-1]))
        return x, y

    @property
    def n(self):
        return self.sx.shape[-2]

    def experts(self):
        """(hp, x, y) of every expert: the batch of x / y and the batch of hp broadcast."""
        xb, yb, hb = self.sx.reshape(-1, self.n, D), self.sy.reshape(-1, self.n), self.shp.reshape(-1, self.shp.shape[-1])
        nb = max(xb.shape[0], hb.shape[0])
        return [(hb[b % hb.shape[0]], xb[b % xb.shape[0]], yb[b % yb.shape[0]]) for b in range(nb)]

    @property
    def nb(self):
        return max(self.sx.reshape(-1, self.n, D).shape[0], self.shp.reshape(-1, self.shp.shape[-1]).shape[0])

    # -- checks --------------------------------------------------------------------------------
    def check(self, name, a, ref, scale=1):
        ref = np.asarray(ref, dtype=np.float64)
        a = torch.as_tensor(a).detach().cpu().double()
        assert a.numel() == ref.size, (name, tuple(a.shape), ref.shape)
        tol = self.tol * (self.env.deriv if scale > 1 else 1)
        e = rel(a.reshape(ref.shape), ref)
        print("%-28s rel err %.2e (bound %.0e)" % (name, e, tol))
        old = self.env.errors.get(name, (0.0, tol))
        self.env.errors[name] = (max(old[0], e), tol)
        assert e <= tol, (name, e)

    def stack(self, parts):
        return np.stack(parts) if len(parts) > 1 else parts[0]

    def expect_batched(self):
        """Whether the library keeps this model's experts in stacked buffers (`Exact_GP._batch`)."""
        spec, _ = pg.covar.spec_of(self.gp.cov, D)
        return self.nb > 1 and _ops.pad_to(self.n) <= gpr_mod._BATCH_MAX_N and len(spec) == 1

    def observe(self, m=None, per_expert=None):
        gp, nb = self.gp, self.nb
        if m is None:
            m = self.m_cycle[self.m_at % len(self.m_cycle)]
            self.m_at += 1
        if per_expert is None:
            per_expert = nb > 1 and self.m_at % 2 == 0
        self.trace.append("    observe m = %d%s" % (m, ", xp per expert" if per_expert else ""))
        xp = self.rnd(self.rng.random((nb, m, D) if per_expert else (m, D)))
        xpt = self.t(xp)
        fits = [Fit(self.terms, hp, x, y) for hp, x, y in self.experts()]
        xps = [xp[b] if per_expert else xp for b in range(nb)]
        pred = [f.predict(q) for f, q in zip(fits, xps)]
        mean, var, cov = (self.stack([p[i] for p in pred]) for i in range(3))
        mu, v = gp.predict(xpt, "diag")
        assert gp.last_predict_batched == self.expect_batched(), "prediction took the %s path" % ("batched" if gp.last_predict_batched else "serial")
        self.check("predict diag: mean", mu, mean)
        self.check("predict diag: variance", v, var)
        mu, c = gp.predict(xpt, "full")
        self.check("predict full: mean", mu, mean)
        self.check("predict full: covariance", c, cov)
        mu, none = gp.predict(xpt, "mean")
        assert none is NotImplemented
        self.check("predict mean only", mu, mean)
        g = gp.predict_grad(xpt)
        grads = [f.predict_grads(q) for f, q in zip(fits, xps)]
        self.check("predict_grad: mean", g[0], mean)
        self.check("predict_grad: variance", g[1], var)
        self.check("predict_grad: d mean", g[2], self.stack([p[0] for p in grads]), 10)
        self.check("predict_grad: d variance", g[3], self.stack([p[1] for p in grads]), 10)
        if nb > 1:
            with pytest.raises(NotImplementedError):
                gp.loo_predict()
        else:
            lm, lv = gp.loo_predict()
            rm, rv = lr.loo_predict(self.terms, *self.experts()[0])
            self.check("loo_predict: mean", lm, rm)
            self.check("loo_predict: variance", lv, rv)
        self.check("wt", gp.wt, self.stack([f.alpha for f in fits]).reshape(self.sy.shape if nb == 1 else (nb, self.n)), 10)
        self.check("krnchd", gp.krnchd, self.stack([f.chol for f in fits]))
        # samplers made earlier are snapshots: the same bits, whatever happened since
        for smp, args, drawn in self.samplers:
            assert torch.equal(smp.draw(*args), drawn), "an earlier sampler's draw changed"
        jit = SAMPLER_JITTER[self.dtype]
        smp = gp.sampler(xpt, jitter=jit)
        shift = [jit - noise_var(self.terms, f.hp) for f in fits]
        self.check("sampler: mean", smp.mean, mean)
        self.check("sampler: chol", smp.chol, self.stack([np.linalg.cholesky(p[2] + s * np.eye(m)) for p, s in zip(pred, shift)]))
        args = (3, 5 + len(self.trace))
        self.samplers = self.samplers[:1] + [(smp, args, smp.draw(*args))]
        self.dirty = False
        assert not gp.need_upd

    # -- operations ----------------------------------------------------------------------------
    def step(self, name, *args, observe=True):
        self.trace.append("%s%s" % (name, args if args else ""))
        try:
            if name in LOSSES:
                self.op_loss(*name.split("_", 1), *args)
            else:
                getattr(self, "op_" + name)(*args)
            if observe:
                self.observe()
        except BaseException:
            print("walk of seed %d failed; operations so far:\n  %s" % (self.seed, "\n  ".join(self.trace)))
            raise
        return self

    def same_data(self):
        assert torch.equal(self.gp.x, self.t(self.sx)) and torch.equal(self.gp.y, self.t(self.sy)), "model.x / model.y are not the shadow's"

    def op_set_params(self):
        rows = self.shp.reshape(-1, self.shp.shape[-1]).shape[0]
        hp = np.stack([hp_for(self.terms, self.rng) for _ in range(rows)])
        self.shp = hp if self.shp.ndim == 2 else hp[0]
        self.gp.set_params(T(self.shp.copy()))
        self.dirty = True

    def op_set_rows(self):
        """[3, nhp] rows (on shared points when the data is one set), or back to one row."""
        self.shp = np.stack([hp_for(self.terms, self.rng) for _ in range(3)]) if self.shp.ndim == 1 else hp_for(self.terms, self.rng)
        self.gp.set_params(T(self.shp.copy()))
        self.dirty = True

    def op_edit_x(self):
        c = (1.25, 0.75)[len(self.trace) % 2]         # exact in fp32
        self.gp.x.mul_(c)
        self.sx = self.rnd(self.sx * c)         # (the fp64 product of two fp32 numbers is exact: one rounding, as mul_ does)
        self.dirty = True
        self.same_data()

    def op_edit_y(self):
        y = self.rnd(0.5 * self.sy + 0.1)
        self.gp.y.copy_(self.t(y))
        self.sy = y
        self.dirty = True

    def assign(self, n, experts):
        self.sx, self.sy = self.draw(n, experts)
        self.gp.x = self.t(self.sx)
        self.gp.y = self.t(self.sy)
        self.dirty = True

    def op_replace_twice(self):
        """x replaced twice, then y twice, nothing evaluated in between and no outside reference kept; then gc.collect().  Each tensor is made
        by ONE constructor call after its predecessor was dropped, so that the allocator can hand the old address out again."""
        n = self.n
        (x1, y1), (x2, y2) = self.draw(n), self.draw(n)
        npdt = np.float32 if self.dtype == F32 else np.float64
        put = (lambda t: t) if self.env.device is None else (lambda t: t.to(self.env.device))
        self.gp.x = put(torch.from_numpy(np.array(x1, dtype=npdt)))     # (a copy: not the shadow's memory)
        self.gp.x = put(torch.from_numpy(np.array(x2, dtype=npdt)))
        self.gp.y = put(torch.from_numpy(np.array(y1, dtype=npdt)))
        self.gp.y = put(torch.from_numpy(np.array(y2, dtype=npdt)))
        gc.collect()
        self.sx, self.sy = x2, y2
        self.dirty = True

    def op_assign_same(self):
        self.assign(self.n, 1 if self.sx.ndim == 2 else self.sx.shape[0])

    def op_assign_cross(self):
        """n across the 256 boundary of the padded size."""
        self.assign(300 if self.n <= 256 else 200, 1 if self.sx.ndim == 2 else self.sx.shape[0])

    def op_assign_experts(self):
        """Three experts of 100 points, or back to one set of n0."""
        if self.sx.ndim == 2:
            self.assign(100, 3)
        else:
            self.assign(self.n0, 1)

    def op_update(self):
        self.gp.update()
        self.dirty = False

    def op_append(self, k):
        xn, yn = self.draw(k)
        mark = dict(self.env.spies.n)
        if self.nb > 1:
            with pytest.raises(NotImplementedError):
                self.gp.append(self.t(xn), self.t(yn))
            return
        assert self.n + k <= N_PAD_MAX
        self.gp.append(self.t(xn), self.t(yn))
        lead = self.sx.shape[:-2]
        self.sx = np.concatenate([self.sx, xn.reshape(lead + (k, D))], axis=-2)
        self.sy = np.concatenate([self.sy, yn.reshape(self.sy.shape[:-1] + (k,))], axis=-1)
        # a fitted model extends its factor block by block; a dirty one only takes the data
        assert self.env.spies.since(mark)["chol_append"] == (0 if self.dirty else -(-k // 128)), "append took the other branch"
        assert self.gp.need_upd == self.dirty
        self.same_data()

    def op_append_dirty(self, k):
        self.op_set_params()
        self.op_append(k)

    def op_illegal_append(self, k):
        assert self.nb > 1
        self.op_append(k)

    def op_illegal_loo(self):
        assert self.nb > 1
        with pytest.raises(NotImplementedError):
            self.gp.loo_predict()
        with pytest.raises(NotImplementedError):
            self.loss_object("loo").loss(self.shp.copy())         # (the model's own rows: one row on shared points would be legal)

    def op_append_nan(self, k):
        """A NaN among the new points of a fitted model: the refusal of tests/test_append_gpu.py, after which nothing has changed."""
        assert self.nb == 1
        self.gp.update()
        xn, yn = self.draw(k)
        xn[k - 2, 1] = np.nan
        x_obj, y_obj = self.gp.x, self.gp.y
        with pytest.raises(torch.linalg.LinAlgError):
            self.gp.append(self.t(xn), self.t(yn))
        assert self.gp.x is x_obj and self.gp.y is y_obj and not self.gp.need_upd
        self.same_data()

    def op_toggle_eager(self):
        self.gp.eager_inverse = not self.gp.eager_inverse

    def op_cov(self):
        self.terms = swapped(self.terms)
        self.gp.cov = cov_of(self.terms)
        self.op_set_params()

    # -- losses --------------------------------------------------------------------------------
    def loss_object(self, cls):
        if cls not in self.losses:
            self.losses[cls] = {"mle": pg.MLE, "loo": pg.LOO}[cls](self.gp)
            assert self.losses[cls].memoize
        return self.losses[cls]

    def loss_ref(self, cls, p):
        rows = p.reshape(-1, p.shape[-1])
        xb, yb = self.sx.reshape(-1, self.n, D), self.sy.reshape(-1, self.n)
        nb = max(rows.shape[0], xb.shape[0])
        fn = kr.nlml_and_grad if cls == "mle" else lr.loo_loss_and_grad
        out = [fn(self.terms, rows[b % rows.shape[0]], xb[b % xb.shape[0]], yb[b % yb.shape[0]]) for b in range(nb)]
        return self.stack([np.array(o[0]) for o in out]), self.stack([o[1] for o in out])

    def op_loss(self, cls, what, at="params"):
        """cls.what(p) at p = the model's parameters, the p of the last call, or new ones."""
        if at == "last" and self.last_p is not None and self.last_p.shape[-1] == self.shp.shape[-1]:
            p = self.last_p
        elif at == "new":
            p = hp_for(self.terms, self.rng)
        else:
            p = self.shp
        self.last_p = p.copy()
        obj = self.loss_object(cls)
        nb = max(p.reshape(-1, p.shape[-1]).shape[0], self.sx.reshape(-1, self.n, D).shape[0])
        if cls == "loo" and nb > 1:
            with pytest.raises(NotImplementedError):
                getattr(obj, what)(p.copy())
            return
        got = getattr(obj, what)(p.copy())
        loss, grad = self.loss_ref(cls, p)
        name = cls.upper()
        if what != "grad":
            self.check(name + " loss", np.asarray(got if what == "loss" else got[0]), loss)
        if what != "loss":
            self.check(name + " gradient", got if what == "grad" else got[1], grad, 10)
        if cls == "mle" and nb > 1:
            spec, _ = pg.covar.spec_of(self.gp.cov, D)
            n_pad = _ops.pad_to(self.n)
            assert not obj.last_batched or (len(spec) == 1 and n_pad <= loss_mod._BATCH_MAX_N), "MLE took the experts-together path"



# ---- random walks --------------------------------------------------------------------------------------------------------------------
def plan(seed, n0, steps=25):
    """The operations of one random walk, from the seed alone: a light model of the state (points, experts, rows) keeps them legal, or
    knowingly illegal (`illegal_*`: append / loo_predict on a batched model must raise NotImplementedError)."""
    rng = random.Random(seed)
    n, data_experts, rows = n0, 1, 1
    weights = {"set_params": 3, "set_rows": 2, "edit_x": 1, "edit_y": 1, "assign_same": 1, "assign_cross": 1, "assign_experts": 2, "update": 1,
               "append": 4, "append_dirty": 1, "append_nan": 1, "toggle_eager": 3, "cov": 1, "illegal_append": 1, "illegal_loo": 1}
    weights.update({name: 1 for name in LOSSES})
    out = []
    while len(out) < steps:
        name = rng.choices(list(weights), list(weights.values()))[0]
        batched = max(data_experts, rows) > 1
        if name.startswith("illegal") != batched and (name.startswith("illegal") or name.startswith("append")):
            continue
        args = ()
        if name in ("append", "append_dirty", "illegal_append", "append_nan"):
            k = rng.choice([1, 6, 8, 130] if name != "append_nan" else [5, 130])
            if name in ("append", "append_dirty"):
                if n + k > N_PAD_MAX - 130:       # (leaves room for one more long append)
                    continue
                n += k
            args = (k,)
        elif name in LOSSES:
            args = (rng.choice(["params", "last", "new"]),)
        elif name == "set_rows":
            rows = 3 if rows == 1 else 1
        elif name == "assign_cross":
            n = 300 if n <= 256 else 200
        elif name == "assign_experts":
            data_experts, n = (3, 100) if data_experts == 1 else (1, n0)
        out.append((name, args))
    return out


# (seed, kind, n0, dtype, eager at the start, size gates patched for the walk)
WALKS = [
    (101, "se+wn", 120, F64, False, {}),
    (102, "m52+wn", 120, F64, True, {"_CHUNK": 256}),
    (103, "(se*per)+wn", 120, F64, False, {"_BATCH_EAGER_N": 0}),
    (104, "se+wn", 250, F64, False, {"_BATCH_MAX_N": 0}),
    (107, "m52+wn", 120, F64, True, {"_BATCH_EAGER_N": 0, "_CHUNK": 256}),
    (106, "se+wn", 120, F32, False, {}),
]


def run_walk(env, seed, kind, n0, dtype, eager, gates):
    env.patch(**gates)
    ops = plan(seed, n0)
    assert sum(name in CHANGES for name, _ in ops) >= 10, "a walk must change the state at least ten times"
    w = Walk(env, KINDS[kind], n0, dtype, seed, eager, m_cycle=(37, 1, 37, 37, 300, 37, 37))
    for name, args in ops:
        w.step(name, *args)
    env.table()
    return w


def coverage():
    """Operation kinds over all committed walks, and the state changes of each."""
    seen = collections.Counter()
    changes = []
    for seed, _, n0, _, _, _ in WALKS:
        ops = plan(seed, n0)
        seen.update(name for name, _ in ops)
        changes.append(sum(name in CHANGES for name, _ in ops))
    return seen, changes


# ---- scripted sequences --------------------------------------------------------------------------------------------------------------
def need(counts, **at_least):
    """The branch witnesses of a sequence: every named op ran at least that often (0: not at all)."""
    for name, k in at_least.items():
        name = name.replace("__", ":")
        assert (counts[name] == 0) if k == 0 else (counts[name] >= k), "%s ran %d times, expected %s" % (name, counts[name], k or "none")


def seq_eager_after_lazy_single(env, dtype=F64):
    """Defect 1: eager_inverse switched on after a prediction formed L^-1 lazily; the next update needs the eager scratch too."""
    w = Walk(env, SE_WN, 120, dtype, seed=1)
    w.step("update", observe=False)
    assert w.gp._experts[0].minv is None
    w.step("update")                               # the observation's predict(xp, "diag") forms L^-1 lazily
    need(env.spies.n, potrs_vec=1, trtri=1)
    mark = dict(env.spies.n)
    w.step("toggle_eager", observe=False).step("set_params", observe=False).step("update")
    need(env.spies.since(mark), trmv=2, potrs_vec=0)
    w.step("toggle_eager", observe=False).step("set_params")      # and back to the lazy inverse
    env.table()


def seq_eager_after_lazy_batched(env):
    """Defect 2: the same switch on a model whose experts live in stacked buffers (reachable at small n with _BATCH_EAGER_N = 0)."""
    env.patch(_BATCH_EAGER_N=0)
    w = Walk(env, SE_WN, 100, seed=2, experts=3)
    w.step("update")
    assert w.gp.last_predict_batched and not w.gp._bat["eager"]
    need(env.spies.n, potrs_vec=3, predict_mean_q_kt_batched=1, alpha_batched=0)
    mark = dict(env.spies.n)
    w.step("toggle_eager", observe=False).step("set_params")
    assert w.gp._bat["eager"]
    need(env.spies.since(mark), alpha_batched=1, potrs_vec=0)
    w.step("toggle_eager", observe=False).step("set_params")
    env.table()


def seq_appends(env, kind, dtype=F64):
    """Appends of 1, 6 and 8 points inside one padded size and 130 points in two blocks (120 -> 265, n_pad 256 -> 512); the refusal of a NaN
    on both paths; an append to a dirty model."""
    w = Walk(env, KINDS[kind], 120, dtype, seed=3, m_cycle=(37, 1, 300))
    w.step("update").step("append", 1).step("append", 6).step("append", 8)
    assert w.gp._experts[0].n_pad == 256 and w.n == 135
    w.step("append_nan", 5).step("append_nan", 130)
    w.step("append", 130)                                         # two blocks and growth: the copy path
    assert w.gp._experts[0].n_pad == 512
    w.step("append_dirty", 6)
    need(env.spies.n, chol_append=8)
    env.table()


def seq_append_growth(env, kind, dtype=F64):
    """250 + 8 crosses n_pad 256 -> 512 with one short block (the copy path); 250 + 6 fills n_pad = 256 to the last row (no padding left);
    the eager scratch follows the growth."""
    w = Walk(env, KINDS[kind], 250, dtype, seed=4, eager=True)
    w.step("update").step("append", 8)
    assert w.gp._experts[0].n_pad == 512 and w.n == 258
    w.step("set_params").step("toggle_eager").step("append", 1).step("toggle_eager").step("set_params")
    w = Walk(env, KINDS[kind], 250, dtype, seed=5)
    w.step("update").step("append", 6)
    assert w.gp._experts[0].n_pad == 256 and w.n == 256
    w.step("append", 1)
    assert w.gp._experts[0].n_pad == 512
    need(env.spies.n, chol_append=4)
    env.table()


def seq_chunks(env, experts):
    """_CHUNK = 256 with m on both sides of one and of two chunks, on the serial (experts = 1) and the batched prediction."""
    env.patch(_CHUNK=256)
    w = Walk(env, M52_WN, 100 if experts > 1 else 120, seed=5, experts=experts)
    op = "predict_mean_q_kt_batched" if experts > 1 else "predict_mean_q_kt"
    for i, m in enumerate((255, 256, 257, 513)):
        w.observe(m, per_expert=experts > 1 and i % 2 == 1)
        mark = dict(env.spies.n)
        w.gp.predict(w.t(w.rng.random((m, D))), "diag")
        assert env.spies.since(mark)[op] == -(-m // 256), "m = %d did not run in %d chunks" % (m, -(-m // 256))
    assert w.gp.last_predict_batched == (experts > 1)
    env.table()


def seq_lazy_batched(env):
    """_BATCH_EAGER_N = 0: the experts are factorised together without their inverses."""
    env.patch(_BATCH_EAGER_N=0)
    w = Walk(env, SEPER_WN, 100, seed=6, experts=3)
    w.step("update")
    assert w.gp._bat is not None and not w.gp._bat["eager"]
    need(env.spies.n, build_factor_batched=1, potrs_vec=3, alpha_batched=0)
    w.step("mle_loss", observe=False)
    assert not w.losses["mle"].last_batched                       # a loss-only evaluation of lazy experts walks them one by one
    w.step("mle_grad", observe=False)
    assert w.losses["mle"].last_batched
    w.step("set_rows").step("mle_loss_and_grad").step("edit_y").step("set_rows")
    env.table()


def seq_one_by_one(env):
    """_BATCH_MAX_N = 0: no stacked buffers, every expert on the single-model schedule."""
    env.patch(_BATCH_MAX_N=0)
    w = Walk(env, SE_WN, 100, seed=7, experts=3)
    w.step("update")
    assert w.gp._bat is None and not w.gp.last_predict_batched
    need(env.spies.n, build_factor=3, build_factor_batched=0, predict_mean_q_kt_batched=0, trmm_lower_kt=1)
    w.step("mle_loss_and_grad", observe=False)
    assert not w.losses["mle"].last_batched
    w.step("toggle_eager").step("set_params").step("toggle_eager").step("set_rows").step("set_rows")
    env.table()


def seq_group_budget(env):
    """_group_budget as a constant: with 3 experts, launch groups of 2 and 1 in the batched prediction and of 1 in the full covariance
    (the product with ONE inverse); twice the constant: the full covariance takes 2 + 1 (a LIST of views of the stack, then one)."""
    w = Walk(env, SE_WN, 100, seed=8, experts=3)
    per = 256 * 256 * torch.empty(0, dtype=w.dtype).element_size()         # one expert's K* at m_pad = n_pad = 256
    w.step("update")
    xp = w.t(w.rng.random((37, D)))
    env.monkeypatch.setattr(gpr_mod, "_group_budget", lambda cap, need=None: 2 * per)
    mark = dict(env.spies.n)
    w.gp.predict(xp, "diag")
    w.gp.predict(xp, "full")
    got = env.spies.since(mark)
    assert got["predict_mean_q_kt_batched"] == 2 and got["kernel_build_batched"] == 2, "the batched prediction did not run in groups of 2 + 1"
    assert got["trmm_lower_kt:one"] == 3 and got["trmm_lower_kt:list"] == 0 and got["syrk_nt_sub_batched"] == 3
    w.observe()
    w.observe(per_expert=True)
    env.monkeypatch.setattr(gpr_mod, "_group_budget", lambda cap, need=None: 4 * per)
    mark = dict(env.spies.n)
    w.gp.predict(xp, "full")
    got = env.spies.since(mark)
    # (the CPU double serves a list by calling itself once per expert: those count as "one" too)
    assert got["trmm_lower_kt:list"] == 1 and got["trmm_lower_kt:one"] >= 1 and got["syrk_nt_sub_batched"] == 2, dict(got)
    w.step("set_params")
    env.table()


def seq_five_children(env):
    """A Compose of five stationary children is two passes of pg_covspec: no stacked buffers, MLE on the serial loop."""
    w = Walk(env, FIVE, 100, seed=9, experts=3)
    assert len(pg.covar.spec_of(w.gp.cov, D)[0]) == 2
    w.step("update")
    assert w.gp._bat is None and not w.gp.last_predict_batched
    w.step("mle_loss_and_grad", observe=False)
    assert not w.losses["mle"].last_batched
    need(env.spies.n, build_factor=6, build_factor_batched=0, nlml_grad=3, nlml_grad_batched=0)
    w.step("cov").step("set_rows")
    env.table()


def seq_rows_and_data(env, dtype=F64):
    """[3, nhp] rows on shared points and back; in-place edits; new x / y of the same n, across n_pad 256, with another expert count."""
    w = Walk(env, SE_WN, 250, dtype, seed=10, m_cycle=(37, 1, 300))
    w.step("update").step("set_rows")
    assert w.gp.last_predict_batched
    w.step("edit_y").step("set_rows").step("edit_x").step("assign_same").step("assign_cross")
    assert w.gp._experts[0].n_pad == 512
    w.step("assign_experts").step("append", 6).step("illegal_loo").step("set_rows").step("assign_experts").step("set_rows")
    w.step("cov").step("assign_cross")
    env.table()


def seq_memo(env):
    """MLE and LOO on one model, memoize on: loss, grad and loss_and_grad at one p in every order.  The factor of a loss-only evaluation
    is re-used by the gradient at the same p (no second factorisation) unless the model changed in between."""
    w = Walk(env, M52_WN, 120, seed=11)
    spies = env.spies
    for cls in ("mle", "loo"):
        for first, second, builds in (("loss", "grad", 0), ("loss", "loss_and_grad", 0), ("grad", "loss", 0), ("loss_and_grad", "grad", 0),
                                      ("loss_and_grad", "loss", 0), ("grad", "loss_and_grad", 0), ("loss", "loss", 0)):
            w.step("%s_%s" % (cls, first), "new", observe=False)
            mark = dict(spies.n)
            w.step("%s_%s" % (cls, second), "last", observe=False)
            assert spies.since(mark)["build_factor"] == builds, "%s after %s factorised again" % (second, first)
        for change in ("edit_y", "edit_x", "assign_same", "append"):
            w.step("%s_loss" % cls, "new", observe=False)
            w.step(change, *((6,) if change == "append" else ()), observe=change == "append")
            mark = dict(spies.n)
            w.step("%s_grad" % cls, "last", observe=False)           # checked against the shadow's CHANGED data
            assert spies.since(mark)["build_factor"] >= 1, "the factor of the old model was re-used after %s" % change
    # the two objects side by side, each with its own buffers
    w.step("mle_loss", "new", observe=False).step("loo_loss", "last", observe=False)
    w.step("mle_grad", "last", observe=False).step("loo_grad", "last")
    env.table()


def seq_address_reuse(env, tries=12):
    """x and y replaced twice without an evaluation in between and without an outside reference, then gc.collect(): the memo key holds
    id()s, and a tensor at a re-used address must not be served the old result.  Returns how often both addresses came back (a memo
    that keeps its keyed tensors alive never sees one)."""
    w = Walk(env, SE_WN, 120, seed=12)
    reused = 0
    for _ in range(tries):
        w.step("mle_loss", observe=False).step("loo_loss", observe=False)
        ids = (id(w.gp.x), id(w.gp.y))
        w.step("replace_twice", observe=False)
        reused += (id(w.gp.x), id(w.gp.y)) == ids
        w.trace.append("    both addresses re-used %d times so far" % reused)
        w.step("mle_loss", observe=False).step("loo_loss", observe=False)
    w.step("mle_grad")
    env.table()
    return reused
