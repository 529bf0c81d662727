"""Times of the nearest-neighbour GP on one GPU: se + wn, d = 8.

  python tools/probe_vecchia.py [--out profiles/vecchia_probe.json] [--quick]

Every figure is the median of `reps` runs between two events on the current stream after a warm-up run, the device otherwise idle.
  knn        pg_knn causal at n = 65536 and 262144, m = 32: ms and ps per candidate pair (n (n - 1) / 2 of them), beside torch.cdist +
             topk in row slabs at n = 65536
  nlml       pg_vecchia_nlml_grad at n = 262144, m = 16 / 32 / 63, with and without the gradient: ms and ns per target; beside the route
             there was before it at n = 32768 (gather [n, m + 1, d], the blocks in torch, torch.linalg.cholesky batched, autograd)
  predict    Vecchia_GP.predict of 65536 points at n = 262144, m = 32 (search and blocks)
  accuracy   held-out RMSE and mean log predictive density of Vecchia_GP (m = 32, random ordering) beside Exact_GP at n = 16384"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pygpr_amd as pg  # noqa: E402
from pygpr_amd._ops import JITTER, get_ops  # noqa: E402
from pygpr_amd.covar import spec_of  # noqa: E402

D = 8


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def data(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, D, generator=g, dtype=torch.float64)
    y = torch.sin(3.0 * x.sum(1)) + 0.1 * torch.randn(n, generator=g, dtype=torch.float64)
    return x, y


def torch_route(x, y, nbr, hp, want_grad):
    """What the package offered before: gathered blocks, torch's batched Cholesky, autograd."""
    hp = hp.clone().requires_grad_(want_grad)
    n, m = nbr.shape
    idx = torch.cat([nbr.long().clamp(min=0), torch.arange(n, device=x.device)[:, None]], 1)      # (identity ordering; padded rows: point 0)
    xb, yb = x[idx], y[idx]
    df = (xb[:, :, None, :] - xb[:, None, :, :]) * hp[1: 1 + D]
    a = hp[0] ** 2 * torch.exp(-(df * df).sum(-1)) + (hp[1 + D] ** 2 + JITTER) * torch.eye(m + 1, device=x.device, dtype=x.dtype)
    L = torch.linalg.cholesky(a)
    z = torch.linalg.solve_triangular(L, yb[:, :, None], upper=False)[:, -1, 0]      # r / sqrt(v)
    loss = (torch.log(L[:, -1, -1]) + 0.5 * z * z).sum() + 0.5 * n * np.log(2 * np.pi)
    if want_grad:
        loss.backward()
    return loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="small sizes: a check that the tool runs")
    args = ap.parse_args()
    ops = get_ops()
    big, mid, acc_n = (8192, 4096, 2048) if args.quick else (262144, 65536, 16384)
    cov = pg.Compose([pg.Squared_exponential(), pg.White_noise()])
    (spec,), nhp = spec_of(cov, D)
    hp = torch.tensor([1.0] + [0.7] * D + [0.1], dtype=torch.float64)
    hpd = hp.cuda()
    res = {"d": D, "model": "se+wn", "device": torch.cuda.get_device_name(0)}

    x, y = data(big)
    xd, yd = x.cuda(), y.cuda()
    for n in (mid, big):
        out = torch.empty(n, 32, dtype=torch.int32, device="cuda")
        ms = timed(lambda: ops.knn(xd[:n], xd[:n], 32, causal=True, out=out), reps=3)
        res["knn_causal_n%d_m32" % n] = {"ms": ms, "ps_per_pair": 1e9 * ms / (0.5 * n * (n - 1))}

    def cdist_topk(n, slab=2048):
        for s in range(0, n, slab):
            dd = torch.cdist(xd[s: s + slab], xd[:n])
            dd.topk(32, dim=1, largest=False)
    ms = timed(lambda: cdist_topk(mid), reps=3)
    res["torch_cdist_topk_n%d_m32" % mid] = {"ms": ms, "ps_per_pair": 1e9 * ms / (mid * mid), "note": "full rows (no causal mask), slabs of 2048"}

    for m in (16, 32, 63):
        nbr = ops.knn(xd, xd, m, causal=True)
        cm, cv = torch.empty(big, dtype=torch.float64, device="cuda"), torch.empty(big, dtype=torch.float64, device="cuda")
        sums, info = torch.zeros(nhp + 1, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        work = torch.empty(max(ops.vecchia_nlml_grad_worksize(big, D, nhp), 1), dtype=torch.float64, device="cuda")
        for want in (0, 1):
            ms = timed(lambda: ops.vecchia_nlml_grad(spec, hpd, xd, yd, nbr, 0, big, JITTER, want, cm, cv, sums[nhp:], sums[:nhp], info, work))
            res["nlml_n%d_m%d_%s" % (big, m, "grad" if want else "loss")] = {"ms": ms, "ns_per_target": 1e6 * ms / big, "loss": float(sums[nhp]),
                                                                          "info": int(info[0])}
        if m < 63:
            nt = min(big, 32768)
            for want in (False, True):
                ms = timed(lambda: torch_route(xd[:nt], yd[:nt], nbr[:nt], hpd, want), reps=3)
                res["torch_route_n%d_m%d_%s" % (nt, m, "grad" if want else "loss")] = {"ms": ms, "ns_per_target": 1e6 * ms / nt}

    model = pg.Vecchia_GP(x, y, cov, neighbours=32)
    model.set_params(hp)
    xq = torch.rand(mid, D, dtype=torch.float64, generator=torch.Generator().manual_seed(9))
    model.predict(xq[:64])
    res["predict_q%d_n%d_m32" % (mid, big)] = {"ms": timed(lambda: model.predict(xq, "diag"), reps=3), "note": "search and blocks, with the transfers of xq"}

    xa, ya = data(acc_n + 4096, seed=3)
    xt, yt, xa, ya = xa[acc_n:], ya[acc_n:], xa[:acc_n], ya[:acc_n]
    for name, mdl in (("exact", pg.Exact_GP(xa, ya, cov)), ("vecchia_m32", pg.Vecchia_GP(xa, ya, cov, neighbours=32, order="random", seed=0))):
        mdl.set_params(hp)
        mdl.update()
        mu, var = (t.cpu() for t in mdl.predict(xt, var="diag"))
        res["accuracy_n%d_%s" % (acc_n, name)] = {"rmse": float(((mu - yt) ** 2).mean().sqrt()),
                                                  "mlpd": float((-0.5 * (torch.log(2 * np.pi * var) + (mu - yt) ** 2 / var)).mean())}
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
