"""The walker of the committee's cached state (helper module: no tests in it).  The pattern is tests/state_walk.py's, whose `Env`,
`Spies`, `Fit`, `hp_for`, `WalkOracleOps` and `walk_ops` are used as they are: a `CommitteeWalk` holds a pg.GRBCM and a SHADOW of it that
never calls pygpr_amd -- fp64 NumPy data of the global expert and of every local expert (the rows of global set U shard, as the model's
own gpg.x / .y and gpl.x / .y hold them), one hyper-parameter row for the global and one per local expert, the term list in the grammar of
tests/kernel_ref.py.  Per-expert answers come from `Fit` (kernel_ref kernel + (noise + 1e-7) I, NumPy Cholesky); the aggregation is
restated here from the module docstring of pygpr_amd/gr_bcm.py in np.longdouble (`aggregate`, `aggregate_full`):

    prec_c = 1 / var_c,  beta_1 = 1,  beta_c = 1/2 (log prec_c - log prec_0) (c >= 2),  beta_0 = 1 - sum_c beta_c,
    var = 1 / sum beta prec,  mu = var sum beta prec mu;   full: (sum_c 1/2 (beta_i + beta_j) o C_c^-1)^-1, weights from the diagonals

(NumPy has no long-double LAPACK: an inverse is the fp64 one after one Newton step X + X (I - A X) with the residual formed in long
double, which leaves (cond eps64)^2 of the fp64 error; that residual's product runs through fp64 BLAS on exact slices, `_product`.)

Every OPERATION (`step`) is applied to the model and to the shadow and is followed by an OBSERVATION (`observe`), which calls
GRBCM.predict FIRST -- a direct call of gpg / gpl would refresh a stale expert and hide the defect --, alternates var = "diag" / "full"
and cycles m.  It checks three layers:

  (a) end to end against the from-scratch shadow: mean, variance or covariance, beta and prec ([nloc + 1, m], row 0 the global expert, on
      xs.device).  diag: state_walk's TOL64 / TOL32 as `rel`; full: rtol 1e-6, atol 1e-10 (mean: atol 1e-9) of test_grbcm_golden (an
      fp32 committee: TOL32).  The staleness check: a stale expert, row or buffer moves the answer by O(1).
  (b) gpg.predict and gpl.predict against the `Fit`s at TOL64 / TOL32, for the same var.
  (c) the aggregation alone, tight: the library's own per-expert outputs of (b), widened to fp64, aggregated in np.longdouble, against
      what GRBCM.predict returned.  diag: the bounds tests/test_framed_gpu.py holds these kernels to -- 1e-12 on mean and variance
      (+ 2^-23 where the output is fp32; both entry by entry, the mean relative to var sum_c |beta_c prec_c mu_c|, the size of the terms
      the kernel adds: a mean that crosses zero has no relative accuracy of its own), 1e-9 absolute on beta and 1e-9 relative on prec as in the golden test.  full: the same
      inputs are aggregated once more in plain fp64 NumPy (LU inverses); with d_ref = |agg64 - agg80|_max / |agg80|_max the library is
      allowed FULL_FACTOR[dtype] max(d_ref, eps) -- a Cholesky-based inverse and NumPy's LU-based one round differently.  Every
      observation prints d_ref, the library's error and the ratio.

      FULL_FACTOR: one figure per precision, each at most four times the largest ratio that a run of the GPU tier on the MI355X
      printed (every test of tests/test_state_walk_grbcm_gpu.py, 296 fp64 and 60 fp32 full-covariance checks): fp64 largest ratio
      2.40 -> F = 9; fp32 (eps = 2^-23, full covariance at m <= 38) largest ratio 3.85 -> F = 15.  The CPU tier's double (LAPACK
      potrf, triangular inverse, L^-T L^-1) has a largest ratio of 3.92.  beta[c] in place of beta[c + 1] in the weighted sum moves
      the covariance by O(1): ratios of 1e6 (fp32) to 1e15 (fp64).

Also asserted by every observation: cov == cov.T to the bit, not model.need_upd, model.params is gpg.params and the shadow's,
model.aggregate(...) fed the host outputs of (b) reproduces predict to (c)'s bounds, and the spied op counts the state calls for: which
expert refits, which terms kernel ran, how the m x m inversions were issued.  On a failure the seed and the trace are printed.

The scripted sequences and the plans of the random walks are here, so that the CPU tier (tests/test_state_walk_grbcm_cpu.py, on
`WalkOracleOps`) and the GPU tier (tests/test_state_walk_grbcm_gpu.py, on the library) run the same ones."""
import collections
import gc
import os
import random

import numpy as np
import pytest
import torch

import kernel_ref as kr
import pygpr_amd as pg
import state_walk as sw
from kind_tools import T, N, cov_of, rel
from pygpr_amd import _ops
from pygpr_amd import gpr as gpr_mod
from pygpr_amd import gr_bcm as grb_mod
from state_walk import D, F32, F64, Fit, hp_for, need

NG = 24
# (shards of 60, 100 and 250 points: n = 84, 124, 274 and n_pad = 256, 256, 512)
EPS = {F64: 2.0 ** -52, F32: 2.0 ** -23}
FULL_FACTOR = {F64: 9.0, F32: 15.0}
SPIED = ["build_factor", "build_factor_batched", "grbcm_local_terms", "grbcm_local_terms_batched", "grbcm_finish", "grbcm_finish_full",
         "grbcm_weighted_prec", "spd_inverse_lower", "spd_inverse_lower_batched", "syrk_nt_sub_batched", "predict_mean_q_kt",
         "predict_mean_q_kt_batched"]
M_SHAPES = (1, 37, 255, 256, 257, 300, 513)
M_FULL = (1, 37, 255, 256, 257, 300, 513)         # ... and of its full-covariance cases


def make_env(ops, monkeypatch, tol64, tol32, deriv=10):
    return sw.Env(ops, monkeypatch, tol64, tol32, deriv=deriv, spied=SPIED)


def patch(env, **gates):
    """Size gates, each in the module that reads it."""
    for name, val in gates.items():
        if hasattr(grb_mod, name) and not hasattr(gpr_mod, name):
            env.monkeypatch.setattr(grb_mod, name, val)
        else:
            env.patch(**{name: val})


# ---- the aggregation, restated -------------------------------------------------------------------------------------------------------
def _slices(a, axis, bits=21, parts=3):
    """a (long double) as a sum of `parts` fp64 arrays whose entries are whole multiples, of at most `bits` + 1 bits, of a power of two
    common to each line along `axis`; what is left over is 2^-63 of the line's largest entry."""
    r, out = np.asarray(a), []
    low = r.astype(np.float64)
    if np.array_equal(low, r):          # fp64 numbers are cut in fp64 (every step below is exact there too), ten times faster
        r = low
    one = r.dtype.type(1.0)
    for _ in range(parts):
        _, ex = np.frexp(np.max(np.abs(r), axis=axis, keepdims=True))
        unit = np.ldexp(one, ex - bits)
        piece = np.rint(r / unit) * unit
        out.append(piece.astype(np.float64))
        r = r - piece
    return out


def _product(a, x):
    """a @ x in long double through fp64 BLAS: every slice product is a sum of at most 2^10 whole numbers below 2^42, exact in fp64
    (NumPy's own long-double product takes half a second at m = 513); only the nine results are added in long double."""
    assert a.shape[1] <= 1024
    out = np.zeros((a.shape[0], x.shape[1]), dtype=np.longdouble)
    sxs = _slices(x, 0)
    for sa in _slices(a, 1):
        for sx in sxs:
            out += sa @ sx
    return out


def _inverse(a, dtype):
    if dtype != np.longdouble:
        return np.linalg.inv(a)
    x = np.linalg.inv(a.astype(np.float64)).astype(np.longdouble)
    r = np.eye(a.shape[0], dtype=np.longdouble) - _product(a, x)
    x = x + (x.astype(np.float64) @ r.astype(np.float64)).astype(np.longdouble)      # (the correction is 1e-12 of x: fp64 carries it)
    return 0.5 * (x + x.T)


def aggregate(mean_g, var_g, mean_l, var_l, dtype=np.longdouble):
    """(mu [m], var [m], beta [nc + 1, m], prec [nc + 1, m]) of the committee from the experts' means and variances ([m]; [nc, m])."""
    mg, vg, ml, vl = (np.asarray(a, dtype=np.float64).astype(dtype) for a in (mean_g, var_g, mean_l, var_l))
    prec = np.concatenate([1.0 / vg[None], 1.0 / vl])
    beta = np.empty_like(prec)
    beta[1:] = 0.5 * (np.log(prec[1:]) - np.log(prec[0]))
    beta[1] = 1.0
    beta[0] = 1.0 - beta[1:].sum(0)
    w = beta * prec
    var = 1.0 / w.sum(0)
    mu = var * (w * np.concatenate([mg[None], ml])).sum(0)
    return mu, var, beta, prec


def aggregate_full(mean_g, cov_g, mean_l, cov_l, dtype=np.longdouble):
    """(mu [m], cov [m, m], beta, prec): the weights from the diagonals, every covariance inverted, combined and inverted back."""
    cg, cl = (np.asarray(a, dtype=np.float64).astype(dtype) for a in (cov_g, cov_l))
    _, _, beta, prec = aggregate(mean_g, np.diagonal(cg), mean_l, np.diagonal(cl, axis1=1, axis2=2), dtype)
    p = np.zeros_like(cg)
    for c, cov_c in enumerate([cg] + list(cl)):
        p += 0.5 * (beta[c][:, None] + beta[c][None, :]) * _inverse(cov_c, dtype)
    cov = _inverse(p, dtype)
    ys = np.concatenate([np.asarray(mean_g, dtype=np.float64)[None], np.asarray(mean_l, dtype=np.float64)]).astype(dtype)
    mu = np.diagonal(cov) * (beta * prec * ys).sum(0)
    return mu, cov, beta, prec


def f64(*arrays):
    return tuple(np.asarray(a, dtype=np.float64) for a in arrays)


# ---- the walk ------------------------------------------------------------------------------------------------------------------------
LOSSES = ["mle_" + w for w in ("loss", "grad", "loss_and_grad")]
CHANGES = {"set_params", "set_local_vec", "set_local_rows", "gpg_set_params", "gpl_set_params", "edit_gpl_y", "edit_gpg_y", "replace_same",
           "replace_cross", "write_back", "nan_row"}
ASSIGNS = CHANGES - {"edit_gpl_y", "edit_gpg_y", "nan_row"}          # after these model.need_upd reads True at once
QUIET = set(LOSSES) | {"update_gpg", "update_gpl", "memoize"}
ALL_KINDS = sorted(CHANGES | QUIET)


class CommitteeWalk:
    def __init__(self, env, terms, nc, shard, dtype=F64, seed=0, m_cycle=(37,)):
        self.env, self.terms, self.dtype, self.seed, self.nc = env, list(terms), dtype, seed, nc
        self.tol = env.tol[dtype]
        self.rng = np.random.default_rng(seed)
        self.trace = []
        self.m_cycle, self.obs = tuple(m_cycle), 0
        self.shards = (shard, 250 if shard <= 100 else 100)             # replace_cross: the other side of n_pad = 256
        self.sxg, self.syg = self.draw((NG,))
        xl, yl = self.draw((nc, shard))
        self.sxl = np.concatenate([np.broadcast_to(self.sxg, (nc, NG, D)), xl], axis=1)
        self.syl = np.concatenate([np.broadcast_to(self.syg, (nc, NG)), yl], axis=1)
        self.hg = hp_for(self.terms, self.rng)
        self.hl = np.tile(self.hg, (nc, 1))
        self.model = pg.GRBCM(self.t(xl), self.t(yl), self.t(self.sxg), self.t(self.syg), cov_of(self.terms))
        assert (self.model.nc, self.model.nsc, self.model.ng, self.model.dim) == (nc, shard, NG, D)
        assert np.array_equal(N(self.model.gpl.x).astype(np.float64), self.sxl) and np.array_equal(N(self.model.gpl.y).astype(np.float64), self.syl)
        self.model.set_params(T(self.hg.copy()))
        self.dirty_g = self.dirty_l = True
        self.loss = pg.GRBCM_MLE(self.model)
        assert self.loss.memoize
        self.last_p = None
        self.xq = self.rnd(self.rng.random((7, D)))
        self.fixed = None           # bits of the predictions at the fixed points, while the model is clean

    # -- data ----------------------------------------------------------------------------------
    def rnd(self, a):
        return T(np.asarray(a, dtype=np.float64)).to(self.dtype).double().numpy()

    def t(self, a):
        t = T(np.ascontiguousarray(a)).to(self.dtype).clone()           # (never the shadow's memory)
        return t if self.env.device is None else t.to(self.env.device)

    def draw(self, lead):
        x = self.rnd(self.rng.random(tuple(lead) + (D,)))
        return x, self.rnd(np.sin(3.0 * x).sum(-1) + 0.1 * self.rng.standard_normal(tuple(lead)))

    @property
    def n(self):
        return self.sxl.shape[1]

    def batched_l(self):
        """Whether the library keeps the local experts in stacked buffers."""
        spec, _ = pg.covar.spec_of(self.model.cov, D)
        return self.nc > 1 and _ops.pad_to(self.n) <= gpr_mod._BATCH_MAX_N and len(spec) == 1

    def fits(self):
        return Fit(self.terms, self.hg, self.sxg, self.syg), [Fit(self.terms, self.hl[c], self.sxl[c], self.syl[c]) for c in range(self.nc)]

    # -- checks --------------------------------------------------------------------------------
    def record(self, name, err, bound):
        print("%-44s err %.2e (bound %.0e)" % (name, err, bound))
        old = self.env.errors.get(name)
        if old is None or err / bound >= old[0] / old[1]:
            self.env.errors[name] = (err, bound)
        assert err <= bound, (name, err, bound)

    def check(self, name, a, ref, tol=None):
        ref = np.asarray(ref, dtype=np.float64)
        a = torch.as_tensor(a).detach().cpu().double()
        assert a.numel() == ref.size, (name, tuple(a.shape), ref.shape)
        self.record(name, rel(a.reshape(ref.shape), ref), self.tol if tol is None else tol)

    def close(self, name, a, ref, rtol, atol):
        """numpy's allclose rule, as the largest |a - ref| / (atol + rtol |ref|) against 1."""
        a, ref = np.asarray(N(a), dtype=np.float64).reshape(np.shape(ref)), np.asarray(ref, dtype=np.float64)
        self.record("%s (rtol %.0e, atol %.0e)" % (name, rtol, atol), float(np.max(np.abs(a - ref) / (atol + rtol * np.abs(ref)))), 1.0)

    def entrywise(self, name, a, ref, rtol):
        a, ref = np.asarray(N(a), dtype=np.float64).reshape(np.shape(ref)), np.asarray(ref, dtype=np.float64)
        self.record(name, float(np.max(np.abs(a - ref) / np.abs(ref))), rtol)

    def tight(self, tag, got, ref80, ref64=None, size_of=None):
        """Layer (c) on (mean, var | cov, beta, prec) of the library against the long-double aggregation of the same inputs."""
        r32 = 2.0 ** -23 if self.dtype == F32 else 0.0
        mu, out, beta, prec = got
        rmu, rout, rbeta, rprec = f64(*ref80)
        if ref64 is None:
            # entry by entry, relative to var sum_c |beta_c prec_c mu_c|: the size of the terms the kernel adds, which a mean near
            # zero does not have (test_framed_gpu's rtol on the entry itself holds for its one fixed draw, not for every draw of a walk)
            size = np.asarray(ref80[1] * np.abs(ref80[2] * ref80[3] * size_of).sum(0), dtype=np.float64)
            self.record(tag + " diag: mean (of its terms)", float(np.max(np.abs(N(mu).astype(np.float64).reshape(-1) - rmu) / size)), 1e-12 + r32)
            self.entrywise(tag + " diag: variance", out, rout, 1e-12 + r32)
        else:
            for name, a, r80, r64 in (("mean", mu, ref80[0], ref64[0]), ("covariance", out, ref80[1], ref64[1])):
                scale = float(np.max(np.abs(r80)))
                d_ref = float(np.max(np.abs(np.asarray(r64, dtype=np.longdouble) - r80))) / scale
                err = float(np.max(np.abs(N(a).astype(np.longdouble).reshape(np.shape(r80)) - r80))) / scale
                floor = max(d_ref, EPS[self.dtype])
                print("%-44s d_ref %.2e  library %.2e  ratio %.2f" % (tag + " full: " + name, d_ref, err, err / floor))
                self.record(tag + " full: " + name + " / max(d_ref, eps)", err / floor, FULL_FACTOR[self.dtype])
        self.record(tag + ": beta (abs)", float(np.max(np.abs(N(beta) - rbeta))), 1e-9)
        self.entrywise(tag + ": prec", prec, rprec, 1e-9)

    def since(self, mark):
        """The spies' calls since `mark`, without those the CPU double makes of its own single-expert methods while it serves a batched
        one (per expert of build_factor_batched and grbcm_local_terms_batched, per matrix of spd_inverse_lower_batched)."""
        got = self.env.spies.since(mark)
        if isinstance(self.env.ops, sw.WalkOracleOps):
            got["build_factor"] -= self.nc * got["build_factor_batched"]
            got["grbcm_local_terms"] -= self.nc * got["grbcm_local_terms_batched"]
            got["spd_inverse_lower"] -= (self.nc + 1) * got["spd_inverse_lower_batched"]
        return got

    def fixed_bits(self):
        xq = self.t(self.xq)
        out = list(self.model.predict(xq, "diag")) + list(self.model.predict(xq, "full"))
        return b"".join(N(o).tobytes() for o in out)

    def expected_builds(self):
        """(build_factor, build_factor_batched) calls the next prediction owes, from the shadow's flags."""
        bat = self.batched_l()
        return int(self.dirty_g) + (self.nc if self.dirty_l and not bat else 0), int(self.dirty_l and bat)

    def observe(self, m=None, var=None, shape3=None):
        model, nc, spies = self.model, self.nc, self.env.spies
        i = self.obs
        self.obs += 1
        m = self.m_cycle[i % len(self.m_cycle)] if m is None else m
        var = ("diag", "full")[i % 2] if var is None else var
        shape3 = (m % 2 == 0 and i % 3 == 0) if shape3 is None else shape3
        self.trace.append("    observe m = %d, %s%s" % (m, var, ", xs [2, m / 2, d]" if shape3 else ""))
        xs = self.rnd(self.rng.random((m, D)))
        xst = self.t(xs)
        full = var == "full"
        fg, fl = self.fits()
        pg_, pl = fg.predict(xs), [f.predict(xs) for f in fl]
        k = 2 if full else 1
        ref_l = (np.stack([p[0] for p in pl]), np.stack([p[k] for p in pl]))
        ref = (aggregate_full if full else aggregate)(pg_[0], pg_[k], *ref_l)

        # (a) the committee first
        builds = self.expected_builds()
        mark = dict(spies.n)
        mu, out = model.predict(xst.reshape(2, m // 2, D) if shape3 else xst, var)
        got = self.counts = self.since(mark)
        beta, prec = model.beta, model.prec
        assert (got["build_factor"], got["build_factor_batched"]) == builds, "refits: build_factor %d, batched %d; the state calls for %s" % (
            got["build_factor"], got["build_factor_batched"], builds)
        self.dirty_g = self.dirty_l = False
        stacked = (not full and nc > 1 and self.batched_l() and not os.environ.get("PG_PREDICT_SERIAL"))
        assert (got["grbcm_local_terms_batched"], got["grbcm_local_terms"]) == ((1, 0) if stacked else (0, nc)), dict(got)
        if full:
            together = _ops.pad_to(m) <= grb_mod._AGG_BATCH_MAX
            assert (got["spd_inverse_lower_batched"], got["spd_inverse_lower"]) == ((1, 1) if together else (0, nc + 2)), dict(got)
            assert got["grbcm_weighted_prec"] == nc + 1 and got["grbcm_finish_full"] == 1
        else:
            assert got["spd_inverse_lower_batched"] == got["spd_inverse_lower"] == got["grbcm_weighted_prec"] == 0 and got["grbcm_finish"] == 1
        assert mu.shape == (m,) and out.shape == ((m, m) if full else (m,)) and mu.dtype == out.dtype == self.dtype
        assert beta.shape == prec.shape == (nc + 1, m) and beta.device == prec.device == mu.device == out.device == xst.device
        assert beta.dtype == prec.dtype == F64
        assert not model.need_upd and not model.gpg.need_upd and not model.gpl.need_upd
        assert model.params is model.gpg.params and np.array_equal(N(model.params), self.hg)
        assert np.array_equal(N(model.gpl.params).reshape(nc, -1), self.hl)
        if full:
            assert torch.equal(out, out.T), "the covariance is not symmetric to the bit"
        rmu, rout, rbeta, rprec = f64(*ref)
        if full and self.dtype == F64:
            self.close("committee full: mean", mu, rmu, 1e-6, 1e-9)
            self.close("committee full: covariance", out, rout, 1e-6, 1e-10)
            if self.tol < sw.TOL64:             # the CPU tier: oracle against oracle
                self.check("committee full: mean", mu, rmu)
                self.check("committee full: covariance", out, rout)
        else:
            self.check("committee %s: mean" % var, mu, rmu)
            self.check("committee %s: %s" % (var, "covariance" if full else "variance"), out, rout)
        self.check("committee: beta", beta, rbeta)
        self.check("committee: prec", prec, rprec)
        if nc == 1:
            assert torch.equal(beta[0], torch.zeros_like(beta[0])) and torch.equal(beta[1], torch.ones_like(beta[1]))

        # (b) the experts
        mark = dict(spies.n)
        mg, vg = model.gpg.predict(xst, var)
        ml, vl = model.gpl.predict(xst, var)
        got = self.since(mark)
        assert got["build_factor"] == got["build_factor_batched"] == 0, "an expert was still stale after GRBCM.predict"
        ml, vl = ml.reshape(nc, m), vl.reshape((nc, m, m) if full else (nc, m))
        self.check("gpg.predict %s: mean" % var, mg, pg_[0])
        self.check("gpg.predict %s: variance" % var, vg, pg_[k])
        self.check("gpl.predict %s: mean" % var, ml, ref_l[0])
        self.check("gpl.predict %s: variance" % var, vl, ref_l[1])
        if nc == 1:
            r32 = 2.0 ** -23 if self.dtype == F32 else 0.0
            self.check("lone expert: mean", mu, N(ml[0]), 1e-12 + r32)
            if not full:
                self.entrywise("lone expert: variance", out, N(vl[0]), 1e-12 + r32)

        # (c) the aggregation alone
        inputs = (N(mg).reshape(m), N(vg).reshape((m, m) if full else m), N(ml), N(vl))
        agg = aggregate_full if full else aggregate
        ref80 = agg(*inputs)
        ref64 = agg(*inputs, dtype=np.float64) if full else None
        means = np.concatenate([inputs[0][None], inputs[2]]).astype(np.float64)
        self.tight("aggregation", (mu, out, beta, prec), ref80, ref64, means)
        amu, aout = model.aggregate(mg, vg, ml, vl, var)
        assert amu.shape == mu.shape and aout.shape == out.shape
        self.tight("aggregate()", (amu, aout, model.beta, model.prec), ref80, ref64, means)
        self.fixed = self.fixed_bits()
        return mu, out

    # -- operations ----------------------------------------------------------------------------
    def step(self, name, *args, observe=True):
        self.trace.append("%s%s" % (name, args if args else ""))
        try:
            before = self.fixed if name in QUIET else None
            getattr(self, "op_" + name)(*args)
            if name in ASSIGNS:
                assert self.model.need_upd, name + " left model.need_upd False"
            if name in CHANGES:
                self.fixed = None
            if before is not None:              # an evaluation or an update of a clean model: the fit stands, to the bit
                mark = dict(self.env.spies.n)
                assert not self.model.need_upd, name + " marked a clean committee dirty"
                assert self.fixed_bits() == before, name + " changed the predictions of a fitted committee"
                got = self.since(mark)
                assert got["build_factor"] == got["build_factor_batched"] == 0, name + " made an expert refit"
            if observe:
                self.observe()
        except BaseException:
            print("committee walk of seed %d failed; operations so far:\n  %s" % (self.seed, "\n  ".join(self.trace)))
            raise
        return self

    def rows(self):
        return np.stack([hp_for(self.terms, self.rng) for _ in range(self.nc)])

    def op_set_params(self):
        self.hg = hp_for(self.terms, self.rng)
        self.hl = np.tile(self.hg, (self.nc, 1))
        self.model.set_params(T(self.hg.copy()))
        self.dirty_g = self.dirty_l = True

    def op_set_local_vec(self):
        self.hl = np.tile(hp_for(self.terms, self.rng), (self.nc, 1))
        self.model.set_local_params(T(self.hl[0].copy()))
        self.dirty_l = True
        assert not self.model.gpg.need_upd or self.dirty_g

    def op_set_local_rows(self, rows=None):
        self.hl = self.rows() if rows is None else np.array(rows)
        self.model.set_local_params(T(self.hl.copy()))
        self.dirty_l = True
        assert not self.model.gpg.need_upd or self.dirty_g

    def op_gpg_set_params(self):
        self.hg = hp_for(self.terms, self.rng)
        self.model.gpg.set_params(T(self.hg.copy()))
        self.dirty_g = True
        assert not self.model.gpl.need_upd or self.dirty_l

    def op_gpl_set_params(self):
        self.hl = self.rows()
        self.model.gpl.set_params(T(self.hl.copy()))
        self.dirty_l = True

    def op_edit_gpl_y(self):
        self.syl = self.rnd(0.5 * self.syl + 0.1)
        self.model.gpl.y.copy_(self.t(self.syl))
        self.dirty_l = True

    def op_edit_gpg_y(self):
        self.syg = self.rnd(0.5 * self.syg - 0.1)
        self.model.gpg.y.copy_(self.t(self.syg))
        self.dirty_g = True

    def replace(self, n):
        self.sxl, self.syl = self.draw((self.nc, n))
        self.model.gpl.x = self.t(self.sxl)
        self.model.gpl.y = self.t(self.syl)
        self.dirty_l = True

    def op_replace_same(self):
        self.replace(self.n)

    def op_replace_cross(self):
        """gpl.x / gpl.y of an n on the other side of the 256 boundary of the padded size."""
        a, b = (NG + s for s in self.shards)
        self.replace(b if self.n == a else a)

    def op_replace_twice(self):
        """gpl.x replaced twice, then gpl.y twice, nothing evaluated in between and no outside reference kept; then gc.collect()."""
        npdt = np.float32 if self.dtype == F32 else np.float64
        (x1, y1), (x2, y2) = self.draw((self.nc, self.n)), self.draw((self.nc, self.n))
        gpl = self.model.gpl
        gpl.x = torch.from_numpy(np.array(x1, dtype=npdt))
        gpl.x = torch.from_numpy(np.array(x2, dtype=npdt))
        gpl.y = torch.from_numpy(np.array(y1, dtype=npdt))
        gpl.y = torch.from_numpy(np.array(y2, dtype=npdt))
        gc.collect()
        self.sxl, self.syl = x2, y2
        self.dirty_l = True

    def op_update_gpg(self):
        mark = dict(self.env.spies.n)
        self.model.gpg.update()
        assert self.since(mark)["build_factor"] == int(self.dirty_g) and not self.model.gpg.need_upd
        self.dirty_g = False

    def op_update_gpl(self):
        owed = (self.nc if self.dirty_l and not self.batched_l() else 0, int(self.dirty_l and self.batched_l()))
        mark = dict(self.env.spies.n)
        self.model.gpl.update()
        got = self.since(mark)
        assert (got["build_factor"], got["build_factor_batched"]) == owed and not self.model.gpl.need_upd, dict(got)
        self.dirty_l = False

    def op_memoize(self):
        self.loss.memoize = not self.loss.memoize
        assert self.loss._mle.memoize == self.loss.memoize

    def op_write_back(self):
        """An optimiser's last act: its vector goes into the global and every local expert."""
        p = hp_for(self.terms, self.rng)
        self.loss.loss_and_grad(p.copy())                   # (the memo now holds the very vector that is written back)
        self.loss.write_back(p.copy())
        self.hg, self.hl = p, np.tile(p, (self.nc, 1))
        self.dirty_g = self.dirty_l = True
        assert np.array_equal(N(self.model.params), p) and np.array_equal(N(self.model.gpl.params), self.hl)

    def op_nan_row(self):
        """A NaN in one local expert's row: predict and GRBCM_MLE raise; with valid rows set again every observation holds."""
        bad = self.hl.copy()
        bad[self.nc // 2, 1] = np.nan
        self.model.gpl.set_params(T(bad.copy()))
        assert self.model.need_upd
        for var in ("diag", "full"):
            with pytest.raises(torch.linalg.LinAlgError):
                self.model.predict(self.t(self.xq), var)
            assert self.model.need_upd and self.model.gpl.need_upd and not self.model.gpg.need_upd
        for what in ("loss", "grad", "loss_and_grad"):
            with pytest.raises(torch.linalg.LinAlgError):
                getattr(self.loss, what)(bad[self.nc // 2].copy())
        self.dirty_g = False                                 # the global expert was fitted before the local ones failed
        self.op_set_local_rows()

    # -- the shared-vector objective -------------------------------------------------------------
    def loss_ref(self, p):
        out = [kr.nlml_and_grad(self.terms, p, self.sxl[c], self.syl[c]) for c in range(self.nc)]
        return np.array(sum(o[0] for o in out)), sum(o[1] for o in out)

    def factorisations(self, mark):
        got = self.since(mark)
        return got["build_factor"] + got["build_factor_batched"]

    def op_mle(self, what, at="params"):
        if at == "last" and self.last_p is not None:
            p = self.last_p
        elif at == "new":
            p = hp_for(self.terms, self.rng)
        else:
            p = self.hg
        self.last_p = p.copy()
        got = getattr(self.loss, what)(p.copy())
        loss, grad = self.loss_ref(p)
        if what != "grad":
            self.check("GRBCM_MLE loss", np.asarray(got if what == "loss" else got[0]), loss)
        if what != "loss":
            self.check("GRBCM_MLE gradient", got if what == "grad" else got[1], grad, self.tol * self.env.deriv)
        return got


for _w in ("loss", "grad", "loss_and_grad"):
    setattr(CommitteeWalk, "op_mle_" + _w, (lambda w: lambda self, at="params": self.op_mle(w, at))(_w))


# ---- random walks --------------------------------------------------------------------------------------------------------------------
def plan(seed, steps=24):
    """The operations of one random walk, from the seed alone (20 to 25 of them)."""
    rng = random.Random(seed)
    weights = {k: 1 for k in ALL_KINDS}
    weights.update(set_params=2, gpg_set_params=2, set_local_rows=2)
    out = []
    while len(out) < steps:
        name = rng.choices(list(weights), list(weights.values()))[0]
        out.append((name, (rng.choice(["params", "last", "new"]),) if name in LOSSES else ()))
    return out


# (seed, kind, local experts, shard, dtype, size gates patched for the walk)
WALKS = [
    (301, "se+wn", 3, 100, F64, {}),
    (303, "m52+wn", 5, 60, F64, {"_BATCH_MAX_N": 0}),
    (304, "se+wn", 3, 100, F64, {"_CHUNK": 256, "_AGG_BATCH_MAX": 0}),
    (305, "se+wn", 3, 60, F32, {}),
]
WALK_M = (37, 1, 37, 260, 38)
# an fp32 committee: the full covariance at m <= 38 only.  cond(C) <= 14.4 m and each of the two rounds of m x m inversions loses about
# cond 2^-24: 3e-5 at m = 37, well inside TOL32 = 1e-3, but 2e-4 times a modest constant at m = 260, which is no margin.  Even places of
# the cycle are diag observations, odd ones full.
M_F32 = (300, 37, 1, 38, 260, 37)


def run_walk(env, seed, kind, nc, shard, dtype, gates):
    patch(env, **gates)
    ops = plan(seed)
    w = CommitteeWalk(env, sw.KINDS[kind], nc, shard, dtype, seed, m_cycle=WALK_M if dtype == F64 else M_F32)
    for name, args in ops:
        w.step(name, *args)
    env.table()
    return w


def coverage():
    """Operation kinds over all committed walks, the state changes of each, and the gates and precisions between them."""
    seen, changes, gates, dtypes = collections.Counter(), [], set(), set()
    for seed, _, _, _, dtype, g in WALKS:
        ops = plan(seed)
        assert 20 <= len(ops) <= 25
        seen.update(name for name, _ in ops)
        changes.append(sum(name in CHANGES for name, _ in ops))
        gates |= {k for k, v in g.items()}
        dtypes.add(dtype)
    return seen, changes, gates, dtypes


# ---- scripted sequences --------------------------------------------------------------------------------------------------------------
def seq_which_expert_refits(env, dtype=F64):
    """gpg.set_params alone refits the global expert alone, set_local_params alone the local ones alone, a second predict nobody (the
    counts are asserted by every observation from the shadow's flags; here they are spelled out)."""
    w = CommitteeWalk(env, sw.SE_WN, 3, 100, dtype, seed=41)
    spies = env.spies
    w.observe()
    for op, owed in (("gpg_set_params", (1, 0)), ("set_local_vec", (0, 1)), ("set_local_rows", (0, 1)), ("gpl_set_params", (0, 1))):
        for var in ("diag", "full"):
            w.step(op, observe=False)
            assert w.model.need_upd
            mark = dict(spies.n)
            w.model.predict(w.t(w.xq), var)
            got = w.since(mark)
            assert (got["build_factor"], got["build_factor_batched"]) == owed, "%s, then predict %s: %s" % (op, var, dict(got))
            mark = dict(spies.n)
            w.model.predict(w.t(w.xq), var)
            got = w.since(mark)
            assert got["build_factor"] == got["build_factor_batched"] == 0, "a second predict refitted"
            w.dirty_g = w.dirty_l = False
            w.observe()
    # in-place edits are seen by the next prediction, each by its own expert
    w.step("edit_gpg_y").step("edit_gpl_y").step("update_gpg").step("update_gpl")
    w.step("gpg_set_params", observe=False).step("update_gpl", observe=False).step("update_gpg")
    env.table()


def seq_terms_paths(env):
    """The stacked rows in ONE launch against the per-expert loop, reached through PG_PREDICT_SERIAL, _BATCH_MAX_N = 0 and a committee of
    one local expert; the two kernels agree bit for bit on the same state (gr_bcm.py, `_aggregate_device`)."""
    spies = env.spies
    w = CommitteeWalk(env, sw.SE_WN, 3, 100, seed=42, m_cycle=(37, 300))
    w.step("set_local_rows", observe=False)
    xs = w.t(w.rnd(w.rng.random((37, D))))
    mark = dict(spies.n)
    mu, var = w.model.predict(xs, "diag")
    need(w.since(mark), grbcm_local_terms_batched=1, grbcm_local_terms=0)
    beta, prec = w.model.beta.clone(), w.model.prec.clone()
    w.dirty_g = w.dirty_l = False
    ml, vl = w.model.gpl.predict(xs, "diag")
    mg, vg = w.model.gpg.predict(xs, "diag")
    a_stacked = w.model.aggregate(mg, vg, ml, vl, "diag") + (w.model.beta, w.model.prec)
    env.monkeypatch.setenv("PG_PREDICT_SERIAL", "1")
    mark = dict(spies.n)
    mu2, var2 = w.model.predict(xs, "diag")
    got = w.since(mark)
    assert got["grbcm_local_terms"] == 3 and got["grbcm_local_terms_batched"] == 0 and got["build_factor_batched"] == 0, dict(got)
    for name, a, b in (("mean", mu, mu2), ("variance", var, var2), ("beta", beta, w.model.beta), ("prec", prec, w.model.prec)):
        assert torch.equal(a, b), "stacked and loop paths differ in the bits of " + name
    a_loop = w.model.aggregate(mg, vg, ml, vl, "diag") + (w.model.beta, w.model.prec)
    assert w.since(mark)["grbcm_local_terms"] == 6
    for a, b in zip(a_stacked, a_loop):
        assert torch.equal(a, b), "aggregate(): stacked and loop paths differ in their bits"
    w.observe()                                                 # the loop path against the shadow, diag and full
    w.observe()
    env.monkeypatch.delenv("PG_PREDICT_SERIAL")
    w.step("set_params")
    # _BATCH_MAX_N = 0: the local experts one by one, their rows in buffers of their own
    default = gpr_mod._BATCH_MAX_N
    patch(env, _BATCH_MAX_N=0)
    w = CommitteeWalk(env, sw.SE_WN, 3, 100, seed=43, m_cycle=(37, 300))
    w.observe()
    need(w.counts, grbcm_local_terms=3, grbcm_local_terms_batched=0, build_factor=4, build_factor_batched=0)
    w.step("set_local_rows").step("gpg_set_params")
    # one local expert: beta_1 = 1, beta_0 = 0 exactly (asserted by the observation), the lone expert's own prediction
    patch(env, _BATCH_MAX_N=default)
    for shard in (60, 250):
        w = CommitteeWalk(env, sw.SE_WN, 1, shard, seed=44 + shard, m_cycle=(37, 37, 1, 1))
        w.observe()
        need(w.counts, grbcm_local_terms=1, grbcm_local_terms_batched=0, build_factor=2, build_factor_batched=0)
        w.observe()
        w.step("set_local_rows").step("gpg_set_params").step("mle_loss_and_grad").step("replace_cross")
    env.table()


def seq_full_paths(env):
    """One state, three ways through the m x m inversions: all in one batched call with the global covariance riding along; one after the
    other (_AGG_BATCH_MAX = 0); the experts' products grouped three to a launch (_FULL_VT_BYTES).  Then diag at another m directly
    after full and full after diag (`_pbuf` and `_sums` are kept between calls)."""
    nc, m = 5, 300
    w = CommitteeWalk(env, sw.SE_WN, nc, 60, seed=46)
    w.step("set_local_rows", observe=False)
    item, mp = 8, _ops.pad_to(m)
    n_pad = _ops.pad_to(w.n)
    outs = []
    state = w.rng.bit_generator.state
    defaults = dict(_AGG_BATCH_MAX=grb_mod._AGG_BATCH_MAX, _FULL_VT_BYTES=gpr_mod._FULL_VT_BYTES)        # the library's own
    assert mp <= defaults["_AGG_BATCH_MAX"] and 2 * (nc + 1) * mp * n_pad * item <= defaults["_FULL_VT_BYTES"], defaults
    for gates, inv_b, inv_1, syrk in (({}, 1, 1, 2), ({"_AGG_BATCH_MAX": 0}, 0, nc + 2, 2), ({"_FULL_VT_BYTES": 2 * 3 * mp * n_pad * item}, 1, 1, 3)):
        patch(env, **defaults)
        patch(env, **gates)
        w.rng.bit_generator.state = state                       # the same test points each time
        outs.append(w.observe(m, "full", shape3=False))
        got = w.counts                                          # of GRBCM.predict alone
        assert (got["spd_inverse_lower_batched"], got["spd_inverse_lower"]) == (inv_b, inv_1), dict(got)
        assert got["syrk_nt_sub_batched"] == syrk, dict(got)    # rank-n updates: the global expert's, and the local experts' in groups
    for other in outs[1:]:
        np.testing.assert_allclose(N(outs[0][0]), N(other[0]), rtol=1e-9, atol=1e-11)
        np.testing.assert_allclose(N(outs[0][1]), N(other[1]), rtol=1e-8, atol=1e-12)
    patch(env, **defaults)
    for m2, var in ((37, "diag"), (300, "full"), (257, "diag"), (37, "full"), (300, "diag"), (1, "full"), (1, "diag")):
        w.observe(m2, var)
    env.table()


def seq_test_point_shapes(env):
    """_CHUNK = 256 with m on both sides of one and of two chunks; m = 256 is its own padded size (`_padded_spd` then leaves `out`
    unzeroed); xs as [m, d] and as [a, b, d]."""
    patch(env, _CHUNK=256)
    w = CommitteeWalk(env, sw.SE_WN, 3, 60, seed=47)
    for m in M_SHAPES:
        w.observe(m, "diag", shape3=m % 2 == 0)
        got, chunks = w.counts, -(-m // 256)
        # (the CPU double serves the batched call by calling the single one per expert: those count too)
        assert got["predict_mean_q_kt_batched"] == chunks and got["predict_mean_q_kt"] >= chunks, "m = %d did not run in %d chunks" % (m, chunks)
    for m in M_FULL:
        w.observe(m, "full", shape3=m % 2 == 0)
    w.step("set_local_rows", observe=False)
    w.observe(256, "full")
    env.table()


def seq_fp32(env):
    """An fp32 committee: set_params, predict diag, predict full and GRBCM_MLE at TOL32."""
    w = CommitteeWalk(env, sw.SE_WN, 3, 100, F32, seed=48, m_cycle=M_F32)
    w.step("set_params").step("set_local_rows").step("mle_loss", "new").step("mle_grad", "last").step("mle_loss_and_grad")
    w.step("replace_cross").step("nan_row")
    env.table()


def seq_other_kind(env, kind="(se*per)+wn"):
    w = CommitteeWalk(env, sw.KINDS[kind], 3, 100, seed=49, m_cycle=(37, 37))
    w.step("set_params").step("set_local_rows").step("gpg_set_params").step("mle_loss_and_grad", "new").step("write_back")
    env.table()


def seq_memo(env):
    """GRBCM_MLE keeps an MLE memo on gpl: asked twice at one point it runs no second factorisation; with memoize off it does; an in-place
    edit, new tensors and other parameters of the MODEL (which the objective does not read) are each treated as they must be."""
    w = CommitteeWalk(env, sw.M52_WN, 3, 100, seed=50)
    spies = env.spies
    w.observe()
    for first, second in (("loss_and_grad", "grad"), ("loss_and_grad", "loss"), ("grad", "loss"), ("grad", "loss_and_grad"), ("loss", "loss")):
        w.step("mle_" + first, "new", observe=False)
        mark = dict(spies.n)
        w.step("mle_" + second, "last", observe=False)
        assert w.factorisations(mark) == 0, "%s after %s factorised again" % (second, first)
    w.step("memoize", observe=False)
    assert not w.loss.memoize
    w.step("mle_loss_and_grad", "new", observe=False)
    mark = dict(spies.n)
    w.step("mle_loss_and_grad", "last", observe=False)
    assert w.factorisations(mark) >= 1, "memoize is off, and the second evaluation ran no factorisation"
    w.step("memoize", observe=False)
    assert w.loss.memoize
    for change in ("edit_gpl_y", "replace_same", "replace_cross"):
        w.step("mle_loss_and_grad", "new", observe=False)
        w.step(change, observe=False)
        mark = dict(spies.n)
        w.step("mle_loss_and_grad", "last", observe=False)        # checked against the shadow's CHANGED data
        assert w.factorisations(mark) >= 1, "the evaluation of the old data was served after %s" % change
    # the objective reads the data of gpl and its own argument, nothing else: the model's parameters may move under a kept memo
    w.step("mle_loss_and_grad", "new", observe=False)
    for change in ("set_params", "set_local_rows", "edit_gpg_y"):
        w.step(change, observe=False)
        mark = dict(spies.n)
        w.step("mle_loss_and_grad", "last", observe=False)
        assert w.factorisations(mark) == 0
    w.observe()
    # a loss at other parameters between two predictions leaves the second one alone (asserted by step() on a clean model)
    w.step("mle_loss_and_grad", "new").step("mle_loss", "new").step("mle_grad", "params").step("write_back")
    env.table()


def seq_address_reuse(env, tries=8):
    """gpl.x and gpl.y replaced twice without an evaluation in between and without an outside reference, then gc.collect(): the memo key
    holds id()s, and a tensor at a re-used address must not be served the old result: every evaluation is checked against the shadow at
    the data of the moment.  Returns (and prints) how often both addresses came back; zero is what a memo that keeps its keyed tensors
    alive gives -- it never meets its address again --, and the values are held either way."""
    w = CommitteeWalk(env, sw.SE_WN, 3, 60, seed=51)
    reused = 0
    for _ in range(tries):
        w.step("mle_loss", observe=False)
        ids = (id(w.model.gpl.x), id(w.model.gpl.y))
        w.step("replace_twice", observe=False)
        reused += (id(w.model.gpl.x), id(w.model.gpl.y)) == ids
        w.trace.append("    both addresses re-used %d times so far" % reused)
        w.step("mle_loss", observe=False)
    w.step("mle_grad")
    print("both addresses of gpl.x / gpl.y came back %d times in %d tries" % (reused, tries))
    env.table()
    return reused


def seq_failed_fit(env):
    """A NaN in one local expert's row: the committee and its objective raise, the global expert stays fitted, and with valid rows set
    again everything holds -- on the stacked experts and on the one-by-one schedule."""
    for gates in ({}, {"_BATCH_MAX_N": 0}):
        patch(env, **gates)
        w = CommitteeWalk(env, sw.SE_WN, 3, 100, seed=52, m_cycle=(37, 37))
        w.step("update_gpg", observe=False).step("nan_row").step("gpg_set_params", observe=False).step("nan_row").step("set_params")
    env.table()


def seq_replay_after_a_timeout(env):
    """The status word of the LAST m x m inversion reads -1 (the coupled chain's time-out) once: `_checked` repeats the tail of the full
    aggregation, which must start from the accumulated local precisions as they were -- not from a buffer the first attempt added the
    global term to and factorised in place.  The time-out is the test's: the inversion itself ran, only its status word is replaced."""
    w = CommitteeWalk(env, sw.SE_WN, 3, 60, seed=53)
    w.observe(37, "full")
    ops, calls = env.ops, collections.Counter()
    real, real_batched = ops.spd_inverse_lower, ops.spd_inverse_lower_batched

    def batched(a_all):                 # (the CPU double serves it through the single-matrix call: those are not the tail's)
        calls["inside"] += 1
        try:
            return real_batched(a_all)
        finally:
            calls["inside"] -= 1

    def timed_out_once(a_pad):
        out, info = real(a_pad)
        if calls["inside"]:
            return out, info
        calls["inverse"] += 1
        return out, (torch.full_like(info, -1) if calls["inverse"] == 1 else info)

    env.monkeypatch.setattr(ops, "spd_inverse_lower_batched", batched)
    env.monkeypatch.setattr(ops, "spd_inverse_lower", timed_out_once)
    env.monkeypatch.setattr(ops, "recover_from_timeout", lambda: calls.update(recover=1), raising=False)
    xs = w.rnd(w.rng.random((37, D)))
    mu, cov = w.model.predict(w.t(xs), "full")
    assert calls["recover"] == 1 and calls["inverse"] == 2, dict(calls)
    env.monkeypatch.setattr(ops, "spd_inverse_lower", real)
    env.monkeypatch.setattr(ops, "spd_inverse_lower_batched", real_batched)
    mu2, cov2 = w.model.predict(w.t(xs), "full")
    assert torch.equal(mu, mu2) and torch.equal(cov, cov2), "the repeated tail did not start from the accumulated precisions"
    w.observe(37, "full")
    env.table()
