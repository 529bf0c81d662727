"""The low-rank gradient contraction and Stochastic_MLE on the GPU.

kernel   pg_kernel_lowrank_grad (symmetric form, n = 65536, d = 8, se + wn, r = 16, fp64) against the composition it replaces: U V^T
         into [8192 x n] slabs on the GEMM core (K = 16 in the core's 128-deep tile: the factors sit in 128-column buffers) and each
         slab fed to pg_kernel_cross_grad, accumulating.  The two alternate in one process; median of `--reps` after two warm-ups,
         device events.  Reported: ms, ps per pair (of the n^2 ordered pairs), the slabs' GEMM alone, the cross form of the fused
         kernel, and the largest difference of the two gradients over S_p next to twice the tests' bound.
model    one Stochastic_MLE.loss_and_grad at n = 65536 (rank 100), split into the loss-only evaluation (preconditioner, probes, block
         solve, quadrature) and the gradient that follows it at the same point (the kernel alone).
big      the same at n = 262144, rank 512.

One JSON line per section; `--out` appends them to a file.  Run the same command twice for the spread.

    python tools/probe_lowrank_grad.py [--what kernel,model,big] [--n 65536] [--reps 5] [--out profiles/lowrank_grad_probe.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pygpr_amd as pg  # noqa: E402
from pygpr_amd import _lib  # noqa: E402
from pygpr_amd import sparse as sp  # noqa: E402
from tools.probe_kmatmul import D, SLAB, problem, timed_pair, wall  # noqa: E402

R = 16


def kernel_section(ops, n, reps):
    cov = pg.Compose([pg.Squared_exponential(), pg.White_noise()])
    (full,), nhp = pg.covar.spec_of(cov, D)
    spec = sp._stationary(full)
    x, _, hp = problem(n)
    xd, hpd = ops.to_device(torch.from_numpy(x), torch.float64), ops.to_device(torch.from_numpy(hp), torch.float64)
    gen = torch.Generator(device="cuda").manual_seed(3)
    upad, vpad = ops.zeros(n, 128), ops.zeros(n, 128)
    upad[:, :R] = torch.randn(n, R, dtype=torch.float64, device="cuda", generator=gen)
    vpad[:, :R] = torch.randn(n, R, dtype=torch.float64, device="cuda", generator=gen)
    u, v = upad[:, :R], vpad[:, :R]                       # views at ld = 128, as the loss hands them over
    slab = ops.empty(SLAB, n)
    g_f, g_x, g_c = ops.zeros(nhp), ops.zeros(nhp), ops.zeros(nhp)
    w_f = ops.empty(max(1, ops.kernel_lowrank_grad_worksize(n, n, R, nhp)))
    w_c = ops.empty(max(1, ops.kernel_cross_grad_worksize(SLAB, n, nhp)))

    def fused():
        ops.kernel_lowrank_grad(spec, hpd, xd, None, u, v, g_f, work=w_f)

    def fused_cross():
        ops.kernel_lowrank_grad(spec, hpd, xd, xd, u, v, g_x, work=w_f)

    def gemm_only():
        for s in range(0, n, SLAB):
            ops.gemm_raw(_lib.GEMM_NT, SLAB, n, 128, 1.0, upad[s: s + SLAB], vpad, 0.0, slab)

    def composed():
        for s in range(0, n, SLAB):
            ops.gemm_raw(_lib.GEMM_NT, SLAB, n, 128, 1.0, upad[s: s + SLAB], vpad, 0.0, slab)
            ops.kernel_cross_grad(spec, hpd, xd[s: s + SLAB], xd, slab, g_c, accumulate=s > 0, work=w_c)

    t_f, t_c, t_x, t_g = timed_pair([fused, composed, fused_cross, gemm_only], reps)
    scale = ops.zeros(nhp)                                # S_p: the same contraction on |U| |V|^T (dk keeps one sign per entry here)
    ops.kernel_lowrank_grad(spec, hpd, xd, None, u.abs(), v.abs(), scale, work=w_f)
    torch.cuda.synchronize()
    mine = scale != 0
    rel = float(((g_f - g_c).abs()[mine] / scale.abs()[mine]).max())
    relx = float(((g_f - g_x).abs()[mine] / scale.abs()[mine]).max())
    pairs = float(n) * n
    return {"section": "kernel", "n": n, "d": D, "r": R, "dtype": "fp64", "model": "se+wn", "reps": reps, "slab_rows": SLAB,
            "fused_sym_ms": round(t_f, 3), "fused_cross_ms": round(t_x, 3), "composed_ms": round(t_c, 3), "gemm_only_ms": round(t_g, 3),
            "fused_sym_ps_per_pair": round(t_f * 1e9 / pairs, 3), "fused_cross_ps_per_pair": round(t_x * 1e9 / pairs, 3),
            "composed_ps_per_pair": round(t_c * 1e9 / pairs, 3), "composed_over_fused": round(t_c / t_f, 3),
            "max_diff_over_scale": rel, "sym_vs_cross_over_scale": relx, "bound": 2 * (16 * 2.0 ** -52 + (2 * R + 2) * 2.0 ** -53),
            "slab_traffic_gb": round(2 * 8.0 * pairs / 1e9, 1)}


def model_section(name, n, rank):
    cov = pg.Compose([pg.Squared_exponential(), pg.White_noise()])
    x, y, hp = problem(n)
    model = pg.Iterative_GP(torch.from_numpy(x), torch.from_numpy(y), cov, rank=rank)
    model.set_params(torch.from_numpy(hp))
    loss = pg.Stochastic_MLE(model)
    if n <= 65536:
        wall(lambda: loss.loss_and_grad(hp * 1.001))      # warm-up: allocator, kernels' first launches
    torch.cuda.reset_peak_memory_stats()
    value, t_loss = wall(lambda: loss.loss(hp))
    grad, t_grad = wall(lambda: loss.grad(hp))
    info = loss.slq_info
    return {"section": name, "n": n, "d": D, "rank": rank, "tol": model.tol, "probes": loss.probes, "loss_only_ms": round(t_loss, 1),
            "gradient_after_it_ms": round(t_grad, 1), "loss_and_grad_ms": round(t_loss + t_grad, 1), "iterations": info["iterations"],
            "residual": info["residual"], "preconditioner_rank": info["rank"], "loss": float(value), "stderr": info["stderr"],
            "grad": [float(g) for g in np.asarray(grad)], "peak_memory_gb": round(torch.cuda.max_memory_allocated() / 1e9, 2),
            "one_n_by_n_gb": round(8.0 * n * n / 1e9, 1)}


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
            line = model_section("model", 65536, 100)
        else:
            line = model_section("big", 262144, 512)
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
