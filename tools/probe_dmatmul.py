"""The derivative's matrix-free product and the two features built on it, on the GPU.

kernel   pg_kernel_matmul_dx (n x n pairs, d = 8, se + wn, fp64) at 1, 16 and 32 right-hand sides against the composition it replaces:
         one call of pg_kernel_xgrad's vector form per right-hand side, each a VALU pass that evaluates every pair again.  The two
         alternate in one process; median of `--reps` after two warm-ups, device events.  Reported: ms, ps per pair, the ratio, the
         largest difference of the two outputs over the largest entry, and pg_kernel_matmul at the same shape (the pair evaluation
         without the derivative's chains).
model    Iterative_GP at n = 65536: function_samples(16).grad at 65536 test points next to the samples' evaluation, and
         predict_grad(64 points, "diag") next to predict(64 points, "diag") -- the block solve both share.

One JSON line per section; `--out` appends them to a file.  Run the same command twice for the spread.

    python tools/probe_dmatmul.py [--what kernel,model] [--n 65536] [--reps 5] [--out profiles/dmatmul_probe.json]
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
from probe_kmatmul import D, problem, timed_pair, wall  # noqa: E402


def kernel_section(ops, n, reps):
    cov = pg.Compose([pg.Squared_exponential(), pg.White_noise()])
    (full,), _ = pg.covar.spec_of(cov, D)
    spec = sp._stationary(full)
    x, _, hp = problem(n)
    xd, hpd = ops.to_device(torch.from_numpy(x), torch.float64), ops.to_device(torch.from_numpy(hp), torch.float64)
    line = {"section": "kernel", "n": n, "d": D, "dtype": "fp64", "model": "se+wn", "reps": reps}
    gen = torch.Generator(device="cuda").manual_seed(3)
    pairs = float(n) * n
    for nrhs in (1, 16, 32):
        v = torch.randn(n, nrhs, dtype=torch.float64, device="cuda", generator=gen)
        cols = [v[:, c].contiguous() for c in range(nrhs)]
        out_f = ops.empty(n, D, nrhs)
        out_c = ops.empty(nrhs, n, D)
        out_k = ops.empty(n, nrhs)

        def fused():
            ops.kernel_matmul_dx(spec, hpd, xd, xd, v, out=out_f)

        def composed():
            for c in range(nrhs):
                ops.kernel_xgrad(spec, hpd, xd, xd, u=cols[c], out_u=out_c[c])

        def value():
            ops.kernel_matmul(spec, hpd, xd, xd, v, out=out_k)

        t_f, t_c, t_k = timed_pair([fused, composed, value], reps)
        diff = float((out_f.permute(2, 0, 1) - out_c).abs().max() / out_c.abs().max())
        line["nrhs_%d" % nrhs] = {
            "fused_ms": round(t_f, 3), "composed_ms": round(t_c, 3), "kernel_matmul_ms": round(t_k, 3),
            "fused_ps_per_pair": round(t_f * 1e9 / pairs, 3), "composed_ps_per_pair": round(t_c * 1e9 / pairs, 3),
            "kernel_matmul_ps_per_pair": round(t_k * 1e9 / pairs, 3), "composed_over_fused": round(t_c / t_f, 3),
            "fused_over_kernel_matmul": round(t_f / t_k, 3), "max_diff_over_max": diff}
    return line


def model_section(n, q, samples):
    cov = pg.Compose([pg.Squared_exponential(), pg.White_noise()])
    x, y, hp = problem(n)
    rng = np.random.default_rng(7)
    xq, x64 = torch.from_numpy(rng.random((q, D))), torch.from_numpy(rng.random((64, D)))
    it = pg.Iterative_GP(torch.from_numpy(x), torch.from_numpy(y), cov)
    it.set_params(torch.from_numpy(hp))
    _, t_upd = wall(it.update)
    fs, t_draw = wall(lambda: it.function_samples(samples, 1024, seed=5))
    wall(lambda: fs(xq))
    wall(lambda: fs.grad(xq))                          # warm-up: allocator, kernels' first launches
    _, t_eval = wall(lambda: fs(xq))
    g, t_grad = wall(lambda: fs.grad(xq))
    (_, var), t_pred = wall(lambda: it.predict(x64, var="diag"))
    (_, var2, dmean, dvar), t_pgrad = wall(lambda: it.predict_grad(x64, var="diag"))
    (_, dmean2), t_pmean = wall(lambda: it.predict_grad(x64, var="none"))
    return {"section": "model", "n": n, "q": q, "d": D, "rank": it.rank, "tol": it.tol, "samples": samples, "features": 1024,
            "update_ms": round(t_upd, 1), "function_samples_ms": round(t_draw, 1), "evaluate_ms": round(t_eval, 1),
            "grad_ms": round(t_grad, 1), "predict_diag_64_ms": round(t_pred, 1), "predict_grad_diag_64_ms": round(t_pgrad, 1),
            "predict_grad_none_64_ms": round(t_pmean, 1), "variance_bits_equal": bool(torch.equal(var, var2)),
            "max_abs_grad": float(g.abs().max()), "max_abs_dmean": float(dmean.abs().max()), "max_abs_dvar": float(dvar.abs().max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="kernel,model")
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ops = pg._ops.get_ops()
    for what in args.what.split(","):
        line = kernel_section(ops, args.n, args.reps) if what == "kernel" else model_section(args.n, args.n, 16)
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
