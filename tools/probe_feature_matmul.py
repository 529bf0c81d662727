"""The random-feature product and pathwise function samples on the GPU.

kernel   pg_feature_matmul (n x nf pairs, d = 8, fp64) against the composition it replaces: X NU^T + U into an [8192 x nf] slab
         (torch.addmm), the product with 2 pi and torch.cos in place, and the GEMM core's NN product of that slab with W, slab by slab
         (W in a 128-column buffer: the core's narrowest NN tile).  The two alternate in one process; median of `--reps` after two
         warm-ups, device events.  Reported at nrhs = 1, 16, 32: ms, ps per pair, the ratio, and the largest difference of the two
         outputs over S_c = sum_f |W_fc| next to the tests' bound (16 own + (nf + 2) 2^-53, own measured on a 256 x 256 sample in
         np.longdouble, doubled: both paths carry a Phi of their own).
model    Iterative_GP.function_samples(16) at n = 65536, rank 100, and one evaluation of the 16 functions at 65536 test points:
         wall times, the solves' iterations and residual.  Recorded, not gated.

One JSON line per section; `--out` appends them to a file.  Run the same command twice for the spread.

    python tools/probe_feature_matmul.py [--what kernel,model] [--n 65536] [--nf 4096] [--reps 5] [--out profiles/feature_matmul_probe.json]
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
from tools.probe_kmatmul import D, SLAB, problem, timed_pair, wall  # noqa: E402


def own_phi_sample(x, nu, u):
    """The largest absolute float64-vs-longdouble difference of the features on a 256 x 256 sample."""
    def phi(dt):
        t = x[:256].astype(dt) @ nu[:256].astype(dt).T + u[:256].astype(dt)[None, :]
        return np.cos(8 * np.arctan(dt(1)) * (t - np.rint(t)))

    return max(float(np.max(np.abs(phi(np.float64) - phi(np.longdouble)))), 2.0 ** -53)


def kernel_section(ops, n, nf, reps):
    rng = np.random.default_rng(1)
    x = rng.random((n, D))
    nu = 0.9 * np.sqrt(2.0) * rng.standard_normal((nf, D)) / (2.0 * np.pi)      # a squared exponential's law at l = 0.9
    u = np.tile([0.0, -0.25], nf // 2)
    xd, nud, ud = (ops.to_device(torch.from_numpy(a), torch.float64) for a in (x, nu, u))
    nut = nud.t().contiguous()
    slab = ops.empty(SLAB, nf)
    line = {"section": "kernel", "n": n, "nf": nf, "d": D, "dtype": "fp64", "reps": reps, "slab_rows": SLAB,
            "own_phi_sample": own_phi_sample(x, nu, u)}
    gen = torch.Generator(device="cuda").manual_seed(3)
    for nrhs in (1, 16, 32):
        w = torch.randn(nf, nrhs, dtype=torch.float64, device="cuda", generator=gen)
        wpad = ops.zeros(nf, 128)
        wpad[:, :nrhs] = w
        out_f = ops.empty(n, nrhs)
        out_c = ops.empty(n, 128)

        def fused():
            ops.feature_matmul(xd, nud, ud, w, out=out_f)

        def composed():
            for s in range(0, n, SLAB):
                torch.addmm(ud[None, :], xd[s: s + SLAB], nut, out=slab)
                slab.mul_(2.0 * np.pi)
                torch.cos_(slab)
                ops.gemm_raw(_lib.GEMM_NN, SLAB, 128, nf, 1.0, slab, wpad, 0.0, out_c[s: s + SLAB])

        t_f, t_c = timed_pair([fused, composed], reps)
        rel = float(((out_f - out_c[:, :nrhs]).abs() / w.abs().sum(0)[None, :]).max())
        bound = 2 * (16 * line["own_phi_sample"] + (nf + 2) * 2.0 ** -53)
        line["nrhs_%d" % nrhs] = {
            "fused_ms": round(t_f, 3), "composed_ms": round(t_c, 3), "fused_ps_per_pair": round(t_f * 1e9 / (float(n) * nf), 3),
            "composed_ps_per_pair": round(t_c * 1e9 / (float(n) * nf), 3), "composed_over_fused": round(t_c / t_f, 3),
            "max_diff_over_scale": rel, "bound": bound, "within_bound": bool(rel <= bound)}
    return line


def model_section(n, q, samples):
    cov = pg.Compose([pg.Squared_exponential(), pg.White_noise()])
    x, y, hp = problem(n)
    xp = np.random.default_rng(7).random((q, D))
    xt, yt, xpt, hpt = (torch.from_numpy(a) for a in (x, y, xp, hp))
    it = pg.Iterative_GP(xt, yt, cov)
    it.set_params(hpt)
    _, t_upd = wall(it.update)
    wall(lambda: it.function_samples(1, 16)(xpt[:64]))      # warm-up: allocator, kernels' first launches
    fs, t_draw = wall(lambda: it.function_samples(samples))
    out, t_eval = wall(lambda: fs(xpt))
    mu, _ = it.predict(xpt, var="none")
    return {"section": "model", "n": n, "q": q, "d": D, "rank": it.rank, "tol": it.tol, "rhs_block": pg.iterative._RHS_BLOCK,
            "samples": samples, "features": fs.features, "nf": int(fs.frequencies.shape[0]), "update_ms": round(t_upd, 1),
            "function_samples_ms": round(t_draw, 1), "evaluate_ms": round(t_eval, 1), "solves": fs.cg_info["solves"],
            "iterations": fs.cg_info["iterations"], "residual": fs.cg_info["residual"],
            "max_abs_sample_mean_minus_mean": float((out.mean(0) - mu).abs().max()), "max_sample_std": float(out.std(0).max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="kernel,model")
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--nf", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ops = pg._ops.get_ops()
    for what in args.what.split(","):
        line = kernel_section(ops, args.n, args.nf, args.reps) if what == "kernel" else model_section(args.n, args.n, 16)
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
