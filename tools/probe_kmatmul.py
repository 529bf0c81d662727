"""The matrix-free covariance product and Iterative_GP on the GPU.

kernel   pg_kernel_matmul (cross form, n x n pairs, d = 8, se + wn, fp64) against the composition it replaces: pg_kernel_build of a
         [8192 x n] slab and the GEMM core's NN product of that slab with V, slab by slab (V in a 128-column buffer: the core's
         narrowest NN tile).  The two alternate in one process; median of `--reps` after two warm-ups, device events.  Reported: ms,
         ps per pair, the build's share alone, the fused kernel at further widths, and the largest difference of the two outputs over
         S_ic = sum_j |K_ij V_jc| next to the tests' bound (16 own_K + (n + 2) 2^-53, own_K measured on a 256 x 256 sample in
         np.longdouble, doubled: both paths carry a K of their own).
model    Iterative_GP.update() and predict(8192 points, "diag") at n = 32768 against Exact_GP at the same parameters: times, iteration
         counts, the largest difference of mean and variance.
big      one Iterative_GP.update() at n = 262144, rank 512, which Exact_GP cannot hold.

One JSON line per section; `--out` appends them to a file.  Run the same command twice for the spread.

    python tools/probe_kmatmul.py [--what kernel,model,big] [--n 65536] [--reps 5] [--out profiles/kmatmul_probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pygpr_amd as pg  # noqa: E402
from pygpr_amd import _lib  # noqa: E402
from pygpr_amd import sparse as sp  # noqa: E402

SLAB = 8192
D = 8


def timed_pair(fns, reps, warm=2):
    """Median ms of each of `fns`, the calls alternating."""
    for _ in range(warm):
        for fn in fns:
            fn()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    return [float(np.median(m)) for m in ms]


def own_k_sample(hp, x):
    """The largest relative float64-vs-longdouble difference of a squared exponential's values on a 256 x 256 sample."""
    a, b = x[:256], x[-256:]

    def k(dt):
        sq = dt(0)
        for j in range(D):
            sq = sq + (dt(hp[1 + j]) * (a[:, j].astype(dt)[:, None] - b[:, j].astype(dt)[None, :])) ** 2
        return dt(hp[0]) ** 2 * np.exp(-sq)

    k64, kld = k(np.float64), k(np.longdouble)
    return max(float(np.max(np.abs(k64 - kld) / kld)), 2.0 ** -53)


def problem(n, seed=1):
    rng = np.random.default_rng(seed)
    x = rng.random((n, D))
    y = np.sin(x.sum(1)) + 0.1 * rng.standard_normal(n)
    hp = np.concatenate([[1.1], np.full(D, 0.9), [0.3]])
    return x, y, hp


def kernel_section(ops, n, reps):
    cov = pg.Compose([pg.Squared_exponential(), pg.White_noise()])
    (full,), _ = pg.covar.spec_of(cov, D)
    spec = sp._stationary(full)
    x, _, hp = problem(n)
    xd, hpd = ops.to_device(torch.from_numpy(x), torch.float64), ops.to_device(torch.from_numpy(hp), torch.float64)
    slab = ops.empty(SLAB, n)
    line = {"section": "kernel", "n": n, "d": D, "dtype": "fp64", "model": "se+wn", "reps": reps, "slab_rows": SLAB,
            "own_k_sample": own_k_sample(hp, x)}
    gen = torch.Generator(device="cuda").manual_seed(3)
    for nrhs in (1, 16):
        v = torch.randn(n, nrhs, dtype=torch.float64, device="cuda", generator=gen)
        vpad = ops.zeros(n, 128)
        vpad[:, :nrhs] = v
        out_f = ops.empty(n, nrhs)
        out_c = ops.empty(n, 128)

        def fused():
            ops.kernel_matmul(spec, hpd, xd, xd, v, out=out_f)

        def build_only():
            for s in range(0, n, SLAB):
                ops.kernel_build(spec, hpd, xd[s: s + SLAB], xd, slab)

        def composed():
            for s in range(0, n, SLAB):
                ops.kernel_build(spec, hpd, xd[s: s + SLAB], xd, slab)
                ops.gemm_raw(_lib.GEMM_NN, SLAB, 128, n, 1.0, slab, vpad, 0.0, out_c[s: s + SLAB])

        t_f, t_c, t_b = timed_pair([fused, composed, build_only], reps)
        scale = ops.kernel_matmul(spec, hpd, xd, xd, v.abs())          # K > 0 for this kernel: S = K |V|
        rel = float(((out_f - out_c[:, :nrhs]).abs() / scale).max())
        bound = 2 * (16 * line["own_k_sample"] + (n + 2) * 2.0 ** -53)
        line["nrhs_%d" % nrhs] = {
            "fused_ms": round(t_f, 3), "composed_ms": round(t_c, 3), "build_only_ms": round(t_b, 3),
            "fused_ps_per_pair": round(t_f * 1e9 / (float(n) * n), 3), "composed_ps_per_pair": round(t_c * 1e9 / (float(n) * n), 3),
            "build_ps_per_pair": round(t_b * 1e9 / (float(n) * n), 3), "composed_over_fused": round(t_c / t_f, 3),
            "max_diff_over_scale": rel, "bound": bound, "within_bound": bool(rel <= bound)}
    for nrhs in (32, 64):          # the fused kernel alone at further widths: two panels, then two passes over the pairs
        v = torch.randn(n, nrhs, dtype=torch.float64, device="cuda", generator=gen)
        out_f = ops.empty(n, nrhs)
        (t_f,) = timed_pair([lambda: ops.kernel_matmul(spec, hpd, xd, xd, v, out=out_f)], reps)
        line["nrhs_%d" % nrhs] = {"fused_ms": round(t_f, 3), "fused_ps_per_pair": round(t_f * 1e9 / (float(n) * n), 3)}
    return line


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t) * 1e3


def model_section(n, q):
    cov = pg.Compose([pg.Squared_exponential(), pg.White_noise()])
    x, y, hp = problem(n)
    xp = np.random.default_rng(7).random((q, D))
    xt, yt, xpt, hpt = (torch.from_numpy(a) for a in (x, y, xp, hp))
    it = pg.Iterative_GP(xt, yt, cov)
    it.set_params(hpt)
    wall(it.update)                                   # warm-up: allocator, kernels' first launches
    it.set_params(hpt)
    _, t_upd = wall(it.update)
    info = dict(it.cg_info)
    (mu_i, var_i), t_pred = wall(lambda: it.predict(xpt, var="diag"))
    ex = pg.Exact_GP(xt, yt, cov)
    ex.set_params(hpt)
    wall(ex.update)
    ex.set_params(hpt)
    _, t_upd_e = wall(ex.update)
    (mu_e, var_e), t_pred_e = wall(lambda: ex.predict(xpt, var="diag"))
    return {"section": "model", "n": n, "q": q, "d": D, "rank": it.rank, "tol": it.tol, "rhs_block": pg.iterative._RHS_BLOCK,
            "iterative_update_ms": round(t_upd, 1), "iterative_predict_diag_ms": round(t_pred, 1), "update_iterations": info["iterations"],
            "update_residual": info["residual"], "preconditioner_rank": info["rank"],
            "exact_update_ms": round(t_upd_e, 1), "exact_predict_diag_ms": round(t_pred_e, 1),
            "max_mean_diff": float((mu_i - mu_e).abs().max()), "max_var_diff": float((var_i - var_e).abs().max()),
            "max_abs_mean": float(mu_e.abs().max()), "max_var": float(var_e.max())}


def big_section(n, rank):
    cov = pg.Compose([pg.Squared_exponential(), pg.White_noise()])
    x, y, hp = problem(n)
    it = pg.Iterative_GP(torch.from_numpy(x), torch.from_numpy(y), cov, rank=rank)
    it.set_params(torch.from_numpy(hp))
    torch.cuda.reset_peak_memory_stats()
    _, t_upd = wall(it.update)
    return {"section": "big", "n": n, "d": D, "rank": rank, "tol": it.tol, "update_ms": round(t_upd, 1), "iterations": it.cg_info["iterations"],
            "residual": it.cg_info["residual"], "preconditioner_rank": it.cg_info["rank"],
            "peak_memory_gb": round(torch.cuda.max_memory_allocated() / 1e9, 2), "one_n_by_n_gb": round(8.0 * n * n / 1e9, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="kernel,model,big")
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ops = pg._ops.get_ops()
    for what in args.what.split(","):
        if what == "kernel":
            line = kernel_section(ops, args.n, args.reps)
        elif what == "model":
            line = model_section(32768, 8192)
        else:
            line = big_section(262144, 512)
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
