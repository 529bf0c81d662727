"""Leave-one-out timings on the GPU: Exact_GP.loo_predict on a fitted model that holds L^-1 (the pg_loo_terms pass and its share of the
HBM peak), one LOO.loss_and_grad next to one MLE.loss_and_grad (MLE's path is the parent's, unchanged), and the share of the S S^T
product in a LOO evaluation.  fp64, D = 8, median of 10 after warm-up, events on the caller stream.  One JSON line per size.

    python tools/probe_loo.py [--sizes 4096 8192 16384] [--reps 10] [--hbm-gbs 8000]
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
from oracle import pygpr_oracle as orc  # noqa: E402


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 8192, 16384])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="HBM peak the loo_predict pass is set against (MI355X: 8 TB/s)")
    args = ap.parse_args()
    d = 8
    ops = pg._ops.get_ops()
    for n in args.sizes:
        x, y = orc.synth(n, d, seed=1)
        hp = np.concatenate([[1.1], np.full(d, 0.9), [0.3]])
        gp = pg.Exact_GP(torch.from_numpy(x), torch.from_numpy(y), pg.Compose([pg.Squared_exponential(), pg.White_noise()]), eager_inverse=True)
        gp.set_params(torch.from_numpy(hp))
        gp.update()
        e = gp._experts[0]
        c, mu, var = (ops.empty(n, dtype=torch.float64) for _ in range(3))
        out = ops.zeros(1, dtype=torch.float64)
        work = ops.empty(ops.loo_terms_worksize(e.n_pad), dtype=torch.float64)
        t_terms = timed(lambda: ops.loo_terms(e.minv, e.alpha, e.y, n, c, mu, var, out, work), args.reps)
        t_predict = timed(gp.loo_predict, args.reps)
        gbytes = 8.0 * n * (n + 1) / 2 / 1e9
        mle, loo = pg.MLE(gp), pg.LOO(gp)
        mle.memoize = loo.memoize = False
        t_mle = timed(lambda: mle.loss_and_grad(hp), args.reps)
        t_loo = timed(lambda: loo.loss_and_grad(hp), args.reps)
        a, m = loo._buf["a"], loo._buf["m"]
        t_sst = timed(lambda: ops.gemm_raw(_lib.GEMM_NT, e.n_pad, e.n_pad, e.n_pad, 1.0, a, a, 0.0, m, tri=1), args.reps)
        t_sym = timed(lambda: ops.symmetrize(a, e.n_pad), args.reps)
        t_wts = timed(lambda: ops.loo_weights(c, e.alpha, a, n, loo._buf["p"], loo._buf["q"]), args.reps)
        t_fold = timed(lambda: ops.loo_fold(m, loo._buf["q"], n), args.reps)
        print(json.dumps({
            "n": n, "d": d, "dtype": "fp64", "reps": args.reps,
            "loo_terms_ms": round(t_terms, 4), "loo_terms_gbs": round(gbytes / (t_terms * 1e-3), 1),
            "loo_terms_hbm_fraction": round(gbytes / (t_terms * 1e-3) / args.hbm_gbs, 3), "loo_predict_ms": round(t_predict, 4),
            "mle_eval_ms": round(t_mle, 3), "loo_eval_ms": round(t_loo, 3), "loo_over_mle": round(t_loo / t_mle, 3),
            "sst_ms": round(t_sst, 3), "sst_share": round(t_sst / t_loo, 3), "symmetrize_ms": round(t_sym, 3), "weights_ms": round(t_wts, 3),
            "fold_ms": round(t_fold, 3),
        }), flush=True)


if __name__ == "__main__":
    main()
