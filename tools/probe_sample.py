"""Joint posterior sampling at N = 16384, D = 8, fp64, squared exponential + white noise, on one MI355X:
  * build_ms        : Exact_GP.sampler(xp, noise=True) at m = 1024 and m = 4096 (the model fitted, L^-1 held), next to what it is made of --
                      predict_full_ms: predict(xp, var="full") at that m, and potrf_ms: one pg_potrf at m_pad on a copy of that covariance;
  * draw_ms         : PosteriorSampler.draw of 1, 64 and 1024 samples at each m (generator, Z L^T, mean, the copy to the host included);
  * randn_ms        : pg_randn alone, 4096 x 8192, fp64 and fp32, with its rate against the HBM write peak (the peak of the covariance-build
                      figures in BASELINE.md / tools/kbuild_summary.py: 8000 GB/s).
Times are medians of device-event intervals (host-clock intervals around a synchronise for the calls that return host tensors) after a
warm-up of every shape; no pass/fail threshold.  One JSON document on stdout, and in --out PATH.

    python tools/probe_sample.py [--out PATH] [--n 16384] [--reps 7]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 8
HBM_GBS = 8000.0


def device_ms(fn, reps, warm=2):
    import numpy as np
    import torch

    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), [round(t, 4) for t in ts]


def host_ms(fn, reps, warm=2):
    """For calls that end in a copy to the host (a synchronise of their own)."""
    import numpy as np
    import torch

    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), [round(t, 4) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import pygpr_amd as pg
    from pygpr_amd._lib import build_id
    from pygpr_amd._ops import get_ops, pad_to

    ops = get_ops()
    res = {"build": build_id(), "n": args.n, "d": D, "dtype": "float64", "reps": args.reps, "hbm_peak_GBs": HBM_GBS, "randn": [], "sampler": []}

    # -- the generator alone
    rows, cols = 4096, 8192
    for dt, name in ((torch.float64, "float64"), (torch.float32, "float32")):
        z = torch.empty(rows, cols, dtype=dt, device="cuda")
        ms, every = device_ms(lambda: ops.randn(z, rows, cols, 1), args.reps, warm=3)
        nbytes = rows * cols * z.element_size()
        res["randn"].append({"dtype": name, "rows": rows, "cols": cols, "ms": ms, "ms_all": every, "bytes": nbytes, "GBs": nbytes / ms / 1e6,
                             "frac_of_hbm_peak": nbytes / ms / 1e6 / HBM_GBS, "normals_per_ns": rows * cols / ms / 1e6})
        print(json.dumps(res["randn"][-1]), flush=True)
        del z

    # -- the sampler on a fitted model
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.random((args.n, D)))
    y = torch.from_numpy(np.sin(3.0 * x.numpy()).sum(1) + 0.1 * rng.standard_normal(args.n))
    gp = pg.Exact_GP(x, y, pg.Compose([pg.Squared_exponential(), pg.White_noise()]))
    gp.set_params(torch.tensor([1.0] + [0.7] * D + [0.1], dtype=torch.float64))
    gp.update()
    for m in (1024, 4096):
        xp = torch.from_numpy(rng.random((m, D)))
        xpd = gp._xp_device(xp)
        row = {"m": m, "m_pad": pad_to(m)}
        row["predict_full_ms"], row["predict_full_all"] = device_ms(lambda: gp._predict_device(xpd, "full"), args.reps)
        _, c_all = gp._predict_device(xpd, "full", padded=True)
        c_all[0].diagonal()[:m].add_(1e-7)
        a = torch.empty_like(c_all[0])
        invd = ops.potrf_workspace(a.shape[0], torch.float64)
        info = torch.zeros(1, dtype=torch.int32, device="cuda")

        def factor():
            a.copy_(c_all[0])
            ops.potrf(a, invd, info)

        both_ms, _ = device_ms(factor, args.reps)
        copy_ms, _ = device_ms(lambda: a.copy_(c_all[0]), args.reps)
        row["potrf_ms"] = both_ms - copy_ms
        assert int(info.item()) == 0
        row["build_ms"], row["build_all"] = host_ms(lambda: gp.sampler(xp, noise=True), args.reps)
        row["build_over_parts"] = row["build_ms"] / (row["predict_full_ms"] + row["potrf_ms"])
        smp = gp.sampler(xp, noise=True)
        row["draw_ms"] = {}
        for ns in (1, 64, 1024):
            row["draw_ms"][str(ns)], _ = host_ms(lambda: smp.draw(ns, seed=3), args.reps)
        res["sampler"].append(row)
        print(json.dumps(row), flush=True)
        del smp, a, c_all
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
