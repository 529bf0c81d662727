"""Derivatives in the test points (pg_kernel_xgrad, Exact_GP.predict_grad), fp64 d = 8, squared exponential and Matern-5/2:
  * the contraction alone with both weight forms (u and B) at m = n = 16384 and at m = 128, n = 16384 (the column split);
  * the comparison point: the VALU gradient contraction pg_nlml_grad at N = 16384 (PG_GRAD_MFMA=0: n^2 / 2 pairs);
  * predict_grad(var="diag") against predict(var="diag") at n = 16384, m = 4096.
One child process per (kind, case), each under its own time limit; the first child that fails or runs out of time ends the probe.
Times are medians of 10 after 2 warm-ups (us); `ps/pair` divides by the pairs each call covers.

    python tools/probe_xgrad.py [--limit SECONDS]
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = [("SE", 0), ("M52", 1)]
CASES = ["xgrad_16384", "xgrad_128", "nlml_grad_valu", "predict"]
N, D = 16384, 8


def timed(fn, reps=10):
    import numpy as np
    import torch

    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def child(case, kind):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import pygpr_amd as pg
    from pygpr_amd._ops import get_ops, make_spec, pad_to

    ops = get_ops()
    rng = np.random.default_rng(5)
    hp = torch.tensor([1.0] + [0.7] * D + [0.1], dtype=torch.float64, device="cuda")
    spec = make_spec([kind], [0], [D + 1])
    x = torch.from_numpy(rng.random((N, D))).cuda()
    res = {}
    if case.startswith("xgrad"):
        m = N if case == "xgrad_16384" else 128
        xq = torch.from_numpy(rng.random((m, D))).cuda()
        u = torch.from_numpy(rng.standard_normal(N)).cuda()
        b = torch.from_numpy(rng.standard_normal((m, N))).cuda()
        ou, ob = ops.empty(m, D), ops.empty(m, D)
        res["us"] = timed(lambda: ops.kernel_xgrad(spec, hp, xq, x, u, b, ou, ob))
        res["pairs"] = m * N
    elif case == "nlml_grad_valu":
        npad = pad_to(N)
        k = ops.zeros(npad, npad)
        ops.kernel_build(spec, hp, x, None, k, lower_only=True, jitter=1e-7)     # finite stand-in values for K^-1
        alpha = torch.from_numpy(rng.standard_normal(npad) * 1e-2).cuda()
        grad = ops.zeros(D + 2)
        work = ops.empty(ops.nlml_grad_worksize(N, D + 2))
        res["us"] = timed(lambda: ops.nlml_grad(spec, hp, x, N, k, alpha, grad, work))
        res["pairs"] = N * (N + 1) // 2
    else:
        m = 4096
        y = torch.from_numpy(np.sin(3.0 * x.cpu().numpy()).sum(1))
        cov = pg.Compose([pg.Squared_exponential() if kind == 0 else pg.Matern52(), pg.White_noise()])
        gp = pg.Exact_GP(x.cpu(), y, cov)
        gp.set_params(hp.cpu())
        xp = torch.from_numpy(rng.random((m, D)))
        res["predict_us"] = timed(lambda: gp.predict(xp, var="diag"), reps=5)
        res["predict_grad_us"] = timed(lambda: gp.predict_grad(xp, var="diag"), reps=5)
    print(json.dumps(res))


def main():
    limit = 300.0
    if "--limit" in sys.argv:
        limit = float(sys.argv[sys.argv.index("--limit") + 1])
    sys.path.insert(0, ROOT)
    from pygpr_amd._lib import build_id

    print("build", json.dumps(build_id()))
    rows = {}
    for name, kind in KINDS:
        for case in CASES:
            env = dict(os.environ)
            if case == "nlml_grad_valu":
                env.update(PG_GRAD_MFMA="0")
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, str(kind)], capture_output=True, text=True,
                                   timeout=limit, env=env)
            except subprocess.TimeoutExpired:
                print("probe_xgrad: %s %s passed its %.0f s limit -- nothing more is started" % (name, case, limit))
                sys.exit(1)
            if r.returncode != 0:
                print(r.stdout[-2000:], r.stderr[-4000:], sep="\n")
                print("probe_xgrad: %s %s ended with %d -- nothing more is started" % (name, case, r.returncode))
                sys.exit(1)
            rows[(name, case)] = json.loads(r.stdout.strip().splitlines()[-1])
            print(name, case, json.dumps(rows[(name, case)]), flush=True)
    print("| kind | contraction m = n = 16384, u + B (us, ps/pair) | m = 128, n = 16384 (us, ps/pair) | pg_nlml_grad VALU N = 16384 "
          "(us, ps/pair) | predict diag n = 16384 m = 4096 (us) | predict_grad diag (us) |")
    print("|---|---:|---:|---:|---:|---:|")
    for name, _ in KINDS:
        a, b, c, p = (rows[(name, k)] for k in CASES)
        print("| %s | %.0f, %.1f | %.0f, %.1f | %.0f, %.1f | %.0f | %.0f |" % (
            name, a["us"], 1e6 * a["us"] / a["pairs"], b["us"], 1e6 * b["us"] / b["pairs"], c["us"], 1e6 * c["us"] / c["pairs"],
            p["predict_us"], p["predict_grad_us"]))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]))
    else:
        main()
