"""Sparse_GP timings on the GPU: one VFE.loss_and_grad and one predict of 8192 points at n = 262144, m = 2048, d = 8 (fp64), and where
the evaluation's time goes -- the covariance build of a chunk, the two streaming products of the GEMM core (pass 1: Phi_aug += A A^T on
the lower tiles, K = the chunk; pass 2: W = [M | -c / sigma^4] A), the rectangular contraction pg_kernel_cross_grad, and the rest (the
m x m algebra, the Kuu contraction, transfers), taken as the difference.  Each piece is timed alone on one full chunk and multiplied
by the number of chunks.  Beside them: VFE(train_z=True).loss_and_grad, which adds the gradient in the inducing inputs (one
pg_kernel_xgrad call on Kuu and one per chunk on the W the chunk already holds), that call timed alone on one full chunk, and
predict_grad on the same test points.  Median of `--reps` after two warm-up runs, events on the caller stream; `--spread` repeats the
two loss_and_grad medians that many times and reports their range.  One JSON line.

`--whitened` adds the same calls on a Sparse_GP(whitened=True) over the same tensors, in the same run, under "whitened": loss,
loss_and_grad (with and without train_z), predict and predict_grad, and the three triangular products the whitened evaluation adds,
each alone on one full chunk with its rate over the flop of the tiles it visits -- pass 1's V = Li A (NN, K range ends with the tile
row), pass 2's W = Li^T U (TN, K range starts with the tile row) and prediction's w = Ksu Li^T (NT, K range ends with the tile column).

    python tools/probe_sparse.py [--n 262144] [--m 2048] [--d 8] [--q 8192] [--reps 5] [--spread 3] [--whitened]
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
from pygpr_amd._ops import pad_to  # noqa: E402


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
    ap.add_argument("--n", type=int, default=262144)
    ap.add_argument("--m", type=int, default=2048)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--q", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spread", type=int, default=3)
    ap.add_argument("--whitened", action="store_true")
    args = ap.parse_args()
    n, m, d = args.n, args.m, args.d
    rng = np.random.default_rng(1)
    x = rng.random((n, d))
    y = np.sin(x.sum(1)) + 0.1 * rng.standard_normal(n)
    z = x[rng.choice(n, m, replace=False)]
    hp = np.concatenate([[1.1], np.full(d, 0.9), [0.3]])
    gp = pg.Sparse_GP(torch.from_numpy(x), torch.from_numpy(y), pg.Compose([pg.Squared_exponential(), pg.White_noise()]), torch.from_numpy(z))
    gp.set_params(torch.from_numpy(hp))
    vfe = pg.VFE(gp)
    vfe.memoize = False
    vfz = pg.VFE(gp, train_z=True)
    vfz.memoize = False
    pz = vfz.start_params()
    evals, evals_z = [], []
    for _ in range(max(1, args.spread)):        # interleaved: both see the same drift of the session
        evals.append(timed(lambda: vfe.loss_and_grad(hp), args.reps))
        evals_z.append(timed(lambda: vfz.loss_and_grad(pz), args.reps))
    t_eval, t_eval_z = float(np.median(evals)), float(np.median(evals_z))
    t_loss = timed(lambda: vfe.loss(hp), args.reps)
    xp = torch.from_numpy(rng.random((args.q, d)))
    gp.update()
    t_pred = timed(lambda: gp.predict(xp, var="diag"), args.reps)
    t_pred_grad = timed(lambda: gp.predict_grad(xp, var="diag"), args.reps)

    # the pieces, on one full chunk
    ops = pg._ops.get_ops()
    xd, yd, zd = gp._device_data()
    ch = min(sp._SPARSE_CHUNK, n)
    nch = -(-n // sp._SPARSE_CHUNK)
    ma, cp = pad_to(m + 1), pad_to(ch)
    (full,), nhp = pg.covar.spec_of(gp.cov, d)
    spec = sp._stationary(full)
    hpd = ops.to_device(torch.from_numpy(hp), torch.float64)
    a = ops.empty(ma, cp, dtype=torch.float64)
    phi = ops.zeros(ma, ma, dtype=torch.float64)
    mw = ops.zeros(ma, ma, dtype=torch.float64)
    w = ops.empty(ma, cp, dtype=torch.float64)
    grad = ops.zeros(nhp, dtype=torch.float64)
    work = ops.empty(ops.kernel_cross_grad_worksize(m, ch, nhp), dtype=torch.float64)
    t_build = timed(lambda: ops.kernel_build(spec, hpd, zd, xd[:ch], a), args.reps)
    t_nt = timed(lambda: ops.gemm_raw(sp._pass1_variant(ma), ma, ma, cp, 1.0, a, a, 1.0, phi, tri=1), args.reps)
    t_nt128 = timed(lambda: ops.gemm_raw(_lib.GEMM_NT, ma, ma, cp, 1.0, a, a, 1.0, phi, tri=1), args.reps)
    t_nn = timed(lambda: ops.gemm_raw(_lib.GEMM_NN, ma, cp, ma, 1.0, mw, a, 0.0, w), args.reps)
    t_cg = timed(lambda: ops.kernel_cross_grad(spec, hpd, zd, xd[:ch], w, grad, accumulate=True, work=work), args.reps)
    gz = ops.zeros(m, d, dtype=torch.float64)
    t_xg = timed(lambda: ops.kernel_xgrad(spec, hpd, zd, xd[:ch], b=w[:m], out_b=gz, accumulate=True), args.reps)
    t_xg_uu = timed(lambda: ops.kernel_xgrad(spec, hpd, zd, zd, b=mw[:m], out_b=gz), args.reps)
    pieces = nch * (2 * t_build + t_nt + t_nn + t_cg)
    white = {}
    if args.whitened:
        gw = pg.Sparse_GP(gp.x, gp.y, gp.cov, gp.z, whitened=True)
        gw.set_params(torch.from_numpy(hp))
        vw, vwz = pg.VFE(gw), pg.VFE(gw, train_z=True)
        vw.memoize = vwz.memoize = False
        gw.update()
        li = gw._state["li"]
        qp = pad_to(min(args.q, sp._CHUNK))
        kt, wq = ops.zeros(qp, ma, dtype=torch.float64), ops.empty(qp, ma, dtype=torch.float64)
        t_v = timed(lambda: ops.trmm_lower(li, a, w), args.reps)
        t_w = timed(lambda: ops.gemm_raw(_lib.GEMM_TN, ma, cp, ma, 1.0, li, a, 0.0, w, klo=1), args.reps)
        t_q = timed(lambda: ops.trmm_lower_kt(li, kt, wq), args.reps)
        tri = lambda cols, t: round(ma * (ma + 128.0) * cols / (t * 1e-3) / 1e12, 2)      # noqa: E731  (whole 128-tiles on and below the diagonal)
        white = {"whitened": {
            "loss_ms": round(timed(lambda: vw.loss(hp), args.reps), 2),
            "loss_and_grad_ms": round(timed(lambda: vw.loss_and_grad(hp), args.reps), 2),
            "loss_and_grad_train_z_ms": round(timed(lambda: vwz.loss_and_grad(pz), args.reps), 2),
            "predict_diag_q%d_ms" % args.q: round(timed(lambda: gw.predict(xp, var="diag"), args.reps), 2),
            "predict_grad_diag_q%d_ms" % args.q: round(timed(lambda: gw.predict_grad(xp, var="diag"), args.reps), 2),
            "per_chunk_whiten_nn_khi1_ms": round(t_v, 3), "whiten_nn_khi1_tflops": tri(cp, t_v),
            "per_chunk_unwhiten_tn_klo1_ms": round(t_w, 3), "unwhiten_tn_klo1_tflops": tri(cp, t_w),
            "predict_whiten_nt_khi2_q%d_ms" % qp: round(t_q, 3), "predict_whiten_nt_khi2_tflops": tri(qp, t_q),
        }}
    print(json.dumps({
        "n": n, "m": m, "d": d, "dtype": "fp64", "chunk": sp._SPARSE_CHUNK, "chunks": nch, "reps": args.reps,
        "loss_and_grad_ms": round(t_eval, 2), "loss_and_grad_ms_range": [round(min(evals), 2), round(max(evals), 2)],
        "loss_and_grad_train_z_ms": round(t_eval_z, 2), "loss_and_grad_train_z_ms_range": [round(min(evals_z), 2), round(max(evals_z), 2)],
        "predict_grad_diag_q%d_ms" % args.q: round(t_pred_grad, 2),
        "per_chunk_xgrad_ms": round(t_xg, 3), "xgrad_kuu_ms": round(t_xg_uu, 3), "xgrad_ps_per_pair": round(t_xg * 1e9 / (m * ch), 2),
        "xgrad_streamed_ms": round(nch * t_xg + t_xg_uu, 2),
        "loss_ms": round(t_loss, 2), "predict_diag_q%d_ms" % args.q: round(t_pred, 2),
        "per_chunk_build_ms": round(t_build, 3), "per_chunk_pass1_nt_ms": round(t_nt, 3), "per_chunk_pass2_nn_ms": round(t_nn, 3),
        "per_chunk_cross_grad_ms": round(t_cg, 3),
        "pass1_tiling": 64 if sp._pass1_variant(ma) == _lib.GEMM_NT_64 else 128, "per_chunk_pass1_nt_128_tiles_ms": round(t_nt128, 3),
        "pass1_nt_tflops": round(ma * (ma + 1.0) * cp / (t_nt * 1e-3) / 1e12, 2),       # the lower triangle: ma (ma + 1) / 2 outputs, 2 flop each
        "pass2_nn_tflops": round(2.0 * ma * ma * cp / (t_nn * 1e-3) / 1e12, 2),
        "cross_grad_gpairs_per_s": round(m * ch / (t_cg * 1e-3) / 1e9, 2),
        "cross_grad_w_gbs": round(8.0 * m * ch / (t_cg * 1e-3) / 1e9, 1),
        "streamed_ms": round(pieces, 2), "rest_ms": round(t_eval - pieces, 2), **white,
    }), flush=True)


if __name__ == "__main__":
    main()
