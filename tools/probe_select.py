"""Greedy inducing-point selection timings on the GPU: pg_greedy_select at n = 32768, m = 512 and n = 262144, m = 2048 (d = 8, se + wn,
fp64) -- the time, the factor traffic 4 n m^2 bytes over it against the 8 TB/s HBM peak -- next to the same loop written with torch
operations on the device (the yardstick: argmax, a gathered row, the kernel column, a mat-vec against the factor so far, the residual
update and its sum, nothing read back) and to one VFE.loss_and_grad at the same n and m on the selected points.  Median of `--reps`
after two warm-up runs, events on the caller stream.  One JSON line per size; `--out` also writes them to a file.

    python tools/probe_select.py [--sizes 32768x512,262144x2048] [--d 8] [--reps 5] [--out profiles/select.json]
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
from pygpr_amd._ops import JITTER  # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s, the figure DESIGN.md's fractions are taken of


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


def torch_loop(x, sig2, l2, m, fac):
    """The selection of a squared exponential with torch operations, every step enqueued without a read-back (so without the stop
    test: at these sizes no residual falls to the floor).  fac [m, n]: the factor, one row per pivot."""
    n = x.shape[0]
    r = torch.full((n,), float(sig2), dtype=torch.float64, device=x.device)
    piv = torch.empty(m, dtype=torch.int64, device=x.device)
    trace = torch.empty(m, dtype=torch.float64, device=x.device)
    for j in range(m):
        p = torch.argmax(r).view(1)
        rp = r.index_select(0, p)
        diff = x - x.index_select(0, p)
        k = sig2 * torch.exp(-((diff * diff) * l2).sum(1))
        if j:
            k = k - fac[:j].t().mv(fac[:j].index_select(1, p).view(j))
        col = k / torch.sqrt(rp)
        fac[j] = col
        r = r - col * col
        r.index_fill_(0, p, 0.0)
        piv[j] = p[0]
        trace[j] = r.sum()
    return piv, trace, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="32768x512,262144x2048")
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    d = args.d
    ops = pg._ops.get_ops()
    cov = pg.Compose([pg.Squared_exponential(), pg.White_noise()])
    hp = np.concatenate([[1.1], np.full(d, 0.9), [0.3]])
    (full,), _ = pg.covar.spec_of(cov, d)
    spec = sp._stationary(full)
    lines = []
    for size in args.sizes.split(","):
        n, m = (int(v) for v in size.split("x"))
        rng = np.random.default_rng(1)
        x = rng.random((n, d))
        y = np.sin(x.sum(1)) + 0.1 * rng.standard_normal(n)
        xd, hpd = ops.to_device(torch.from_numpy(x), torch.float64), ops.to_device(torch.from_numpy(hp), torch.float64)
        work = ops.empty(ops.greedy_select_worksize(n, m), dtype=torch.float64)
        out = [None]

        def hip():
            out[0] = ops.greedy_select(spec, hpd, xd, m, JITTER, work=work)

        t_hip = timed(hip, args.reps)
        piv, count, trace, resid = out[0]
        c = int(count.cpu()[0])
        del work
        fac = torch.empty((m, n), dtype=torch.float64, device=xd.device)
        l2 = hpd[1: 1 + d] ** 2
        ref = [None]

        def loop():
            ref[0] = torch_loop(xd, hp[0] ** 2, l2, m, fac)

        t_torch = timed(loop, args.reps)
        same = int((ref[0][0][:c] == piv[:c].long()).sum().item())
        tr_rel = float(((ref[0][1][:c] - trace[:c]).abs().max() / trace[0]).item())
        del fac
        gp = pg.Sparse_GP(torch.from_numpy(x), torch.from_numpy(y), cov, torch.from_numpy(x[piv[:c].cpu().numpy()]))
        gp.set_params(torch.from_numpy(hp))
        vfe = pg.VFE(gp)
        vfe.memoize = False
        t_eval = timed(lambda: vfe.loss_and_grad(hp), args.reps)
        traffic = 4.0 * n * float(c) ** 2
        line = {
            "n": n, "m": m, "d": d, "dtype": "fp64", "model": "se+wn", "reps": args.reps, "count": c,
            "greedy_select_ms": round(t_hip, 2), "us_per_step": round(1e3 * t_hip / max(c, 1), 2),
            "factor_traffic_gb": round(traffic / 1e9, 1), "factor_tbs": round(traffic / (t_hip * 1e-3) / 1e12, 3),
            "fraction_of_hbm_peak": round(traffic / (t_hip * 1e-3) / HBM_PEAK, 3),
            "torch_loop_ms": round(t_torch, 2), "torch_over_hip": round(t_torch / t_hip, 2),
            "pivots_equal_to_torch_loop": same, "trace_rel_diff_to_torch_loop": tr_rel,
            "trace_first": float(trace[0]), "trace_last": float(trace[c - 1]), "n_kdiag": n * hp[0] ** 2,
            "vfe_loss_and_grad_ms": round(t_eval, 2), "workspace_gb": round(8.0 * ops.greedy_select_worksize(n, m) / 1e9, 3),
        }
        print(json.dumps(line), flush=True)
        lines.append(line)
        del gp, vfe, xd
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
