"""Covariance build (lower-only) and fused gradient contraction per stationary kind: squared exponential, Matern-1/2, -3/2, -5/2 at
N = 16384 fp64 D = 8 and 16, n = 33792 fp32 D = 16 (BASELINE config 5's shape).  One child process per (shape, kind), each under its own
time limit; the first child that fails or runs out of time ends the probe (nothing more is started on the GPU).  Prints one table (us,
median of 10 after 2 warm-ups) and the body each call takes.

    python tools/probe_matern_family.py [--limit SECONDS]
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = [("SE", 0), ("M12", 4), ("M32", 3), ("M52", 1)]
SHAPES = [(16384, 8, "fp64"), (16384, 16, "fp64"), (33792, 16, "fp32")]


def child(n, d, dt, kind):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    from pygpr_amd._ops import get_ops, make_spec, pad_to

    ops = get_ops()
    dtype = torch.float64 if dt == "fp64" else torch.float32
    npad = pad_to(n)
    rng = np.random.default_rng(n + d)
    x = torch.from_numpy(rng.random((n, d))).to("cuda", dtype)
    hp = torch.tensor([1.0] + [0.7] * d + [0.1], dtype=torch.float64, device="cuda")
    spec = make_spec([kind], [0], [d + 1])
    k = ops.zeros(npad, npad, dtype=dtype)
    alpha = torch.from_numpy(rng.standard_normal(npad) * 1e-2).to("cuda", dtype)
    grad = ops.zeros(d + 2)
    work = ops.empty(ops.nlml_grad_worksize(n, d + 2))

    def timed(fn):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(10):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        return float(np.median(ts))

    t_build = timed(lambda: ops.kernel_build(spec, hp, x, None, k, lower_only=True, jitter=1e-7))
    # the contraction reads K^-1's lower triangle and alpha: any finite values time the same, so the covariance itself stands in
    t_grad = timed(lambda: ops.nlml_grad(spec, hp, x, n, k, alpha, grad, work))
    assert torch.isfinite(grad).all()
    print(json.dumps({"build_us": t_build, "grad_us": t_grad}))


def main():
    limit = 300.0
    if "--limit" in sys.argv:
        limit = float(sys.argv[sys.argv.index("--limit") + 1])
    rows = []
    for n, d, dt in SHAPES:
        for name, kind in KINDS:
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), str(d), dt, str(kind)],
                                   capture_output=True, text=True, timeout=limit)
            except subprocess.TimeoutExpired:
                print("probe_matern_family: %s n=%d d=%d %s passed its %.0f s limit -- nothing more is started" % (name, n, d, dt, limit))
                sys.exit(1)
            if r.returncode != 0:
                print(r.stdout[-2000:], r.stderr[-4000:], sep="\n")
                print("probe_matern_family: %s n=%d d=%d %s ended with %d -- nothing more is started" % (name, n, d, dt, r.returncode))
                sys.exit(1)
            res = json.loads(r.stdout.strip().splitlines()[-1])
            rows.append((n, d, dt, name, res["build_us"], res["grad_us"]))
    def body(name, d, dt):    # the default routing of pg_kbuild / pg_nlml_grad_t for one component
        if name == "M12":
            return "VALU / VALU"
        if name == "SE" and dt == "fp64" and d <= 8:
            return "VALU fast / matrix pipe"
        return "matrix pipe / matrix pipe"

    print("| shape | kind | build lower-only (us) | gradient contraction (us) | vs M52 build / grad | bodies build / grad |")
    print("|---|---|---:|---:|---:|---|")
    for n, d, dt, name, tb, tg in rows:
        ref = [r for r in rows if r[:3] == (n, d, dt) and r[3] == "M52"][0]
        print("| N = %d %s D = %d | %s | %.0f | %.0f | %.2f / %.2f | %s |" % (n, dt, d, name, tb, tg, tb / ref[4], tg / ref[5], body(name, d, dt)))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], int(sys.argv[5]))
    else:
        main()
