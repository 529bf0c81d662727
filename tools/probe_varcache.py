"""The squared-row-norm kernel and the variance cache built on it, on the GPU.

kernel   pg_kernel_rowsq (n x n pairs, d = 8, se + wn, fp64) beside pg_kernel_matmul at one column in the same process: the same walk
         over the pairs, a multiply-add per pair in the place of the matrix instructions.  The two alternate; median of `--reps` after
         two warm-ups, device events.  Reported: ms, ps per pair, the ratio, and the largest relative difference of the row norms from
         sum_j k_ij^2 formed by pg_kernel_build + torch on the first 256 rows.
model    Iterative_GP at n = 32768, rank 100: variance_cache(steps=2, bounds=True), then variance and variance(bounds=True) at 8192
         points -- the three alternating, median of `--reps` after two warm-ups, device events (the build synchronises with the host
         once a round of its orthonormalisation: the events span that) -- beside the model's own predict(512 points, "diag") scaled by
         the block count to 8192 points (what the cache replaces); the largest certified gap, and check()'s true excess and gap at 64 of
         the points.  update() is timed on its second call; predict and check are block solves of 1 to 40 s: one wall-clock sample each.
big      the same at n = 262144, rank 512, steps 1, with the peak of allocated memory; predict is measured at 64 points (one block
         solve) and scaled.

One JSON line per section; `--out` appends them to a file.  Run the same command twice for the spread.

    python tools/probe_varcache.py [--what kernel,model,big] [--n 65536] [--reps 5] [--out profiles/varcache_probe.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pygpr_amd as pg  # noqa: E402
from pygpr_amd import sparse as sp  # noqa: E402
from pygpr_amd._ops import pad_to  # noqa: E402
from probe_kmatmul import D, problem, timed_pair, wall  # noqa: E402


def kernel_section(ops, n, reps):
    cov = pg.Compose([pg.Squared_exponential(), pg.White_noise()])
    (full,), _ = pg.covar.spec_of(cov, D)
    spec = sp._stationary(full)
    x, _, hp = problem(n)
    xd, hpd = ops.to_device(torch.from_numpy(x), torch.float64), ops.to_device(torch.from_numpy(hp), torch.float64)
    v = torch.randn(n, 1, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    out_r, out_k = ops.empty(n), ops.empty(n, 1)
    t_r, t_k = timed_pair([lambda: ops.kernel_rowsq(spec, hpd, xd, xd, out=out_r), lambda: ops.kernel_matmul(spec, hpd, xd, xd, v, out=out_k)], reps)
    slab = ops.empty(256, pad_to(n))
    ops.kernel_build(spec, hpd, xd[:256], xd, slab)
    dense = (slab[:, :n] ** 2).sum(1)
    pairs = float(n) * n
    return {"section": "kernel", "n": n, "d": D, "dtype": "fp64", "model": "se+wn", "reps": reps, "rowsq_ms": round(t_r, 3),
            "kernel_matmul_1col_ms": round(t_k, 3), "rowsq_ps_per_pair": round(t_r * 1e9 / pairs, 3),
            "kernel_matmul_ps_per_pair": round(t_k * 1e9 / pairs, 3), "rowsq_over_kernel_matmul": round(t_r / t_k, 3),
            "max_rel_diff_from_built_rows": float(((out_r[:256] - dense).abs() / dense).max())}


def cache_section(name, n, rank, steps, q, q_solved, reps):
    cov = pg.Compose([pg.Squared_exponential(), pg.White_noise()])
    x, y, hp = problem(n)
    xp = torch.from_numpy(np.random.default_rng(7).random((q, D)))
    it = pg.Iterative_GP(torch.from_numpy(x), torch.from_numpy(y), cov, rank=rank)
    it.set_params(torch.from_numpy(hp))
    wall(it.update)                                   # warm-up: allocator, kernels' first launches
    it.set_params(torch.from_numpy(hp))
    _, t_upd = wall(it.update)
    torch.cuda.reset_peak_memory_stats()
    vc = it.variance_cache(steps=steps, bounds=True)
    upper, lower = vc.variance(xp, bounds=True)
    var = vc.variance(xp)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    del vc                                            # (one cache at a time: the timed builds below each replace the last)
    keep = {}
    t_build, t_var, t_bounds = timed_pair([lambda: keep.update(vc=it.variance_cache(steps=steps, bounds=True)),
                                           lambda: keep["vc"].variance(xp), lambda: keep["vc"].variance(xp, bounds=True)], reps)
    vc = keep["vc"]
    (_, solved), t_pred = wall(lambda: it.predict(xp[:q_solved], var="diag"))      # block solves: one sample each, this and check
    blocks, blocks_solved = -(-q // pg.iterative._RHS_BLOCK), -(-q_solved // pg.iterative._RHS_BLOCK)
    chk, t_check = wall(lambda: vc.check(xp[:64]))
    return {"section": name, "n": n, "q": q, "d": D, "rank": rank, "steps": steps, "tol": it.tol, "reps": reps, "cache_rank": vc.rank, "info": vc.info,
            "update_ms": round(t_upd, 1), "build_ms": round(t_build, 1), "variance_ms": round(t_var, 1), "variance_bounds_ms": round(t_bounds, 1),
            "predict_diag_points": q_solved, "predict_diag_ms": round(t_pred, 1),
            "predict_diag_scaled_to_q_ms": round(t_pred * blocks / blocks_solved, 1),
            "bits_equal_with_and_without_bounds": bool(torch.equal(var, upper)), "largest_certified_gap": float((upper - lower).max()),
            "largest_excess_at_solved_points": float((upper[:q_solved] - solved).max()), "min_excess_at_solved_points": float((upper[:q_solved] - solved).min()),
            "check_64": chk, "check_ms": round(t_check, 1), "max_var": float(upper.max()),
            "peak_memory_gb": round(peak / 1e9, 2), "one_n_by_n_gb": round(8.0 * n * n / 1e9, 1)}


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
            line = cache_section("model", 32768, 100, 2, 8192, 512, args.reps)
        else:
            line = cache_section("big", 262144, 512, 1, 8192, 64, args.reps)
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
