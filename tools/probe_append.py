"""Conditioning on new points (pg_chol_append, Exact_GP.append) against a refit, fp64 d = 8, squared exponential + white noise, for
N in {4096, 8192, 16384} and k in {1, 8, 32, 128}:
  * append_us  : Exact_GP.append of k points to a fitted model of N - 1024 + j k points (j = 0 .. 6: every block stays inside n_pad = N),
                 covariance builds, the C call and its synchronisation included;
  * chol_us    : pg_chol_append alone at n = N - 128 (it reads rows < n and writes rows >= n only, so repeating it is idempotent);
  * update_us  : update() of a fresh model on N points (build + Cholesky + alpha), the refit an append replaces;
  * GB/s       : the algorithmic traffic of pg_chol_append -- three reads of L^-1's lower triangle, 3 n^2 / 2 x 8 bytes, plus Kt, Vt and
                 the new rows (about 6 k n x 8 bytes) -- over chol_us.
One child process per case, each under its own time limit; the first child that fails or runs out of time ends the probe.  Times are
medians of device-event intervals after a synchronise (us).

    python tools/probe_append.py [--limit SECONDS]
    python tools/probe_append.py --child-chol N K REPS     (pg_chol_append alone: the process a rocprofv3 --kernel-trace pass wraps)
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = [4096, 8192, 16384]
KS = [1, 8, 32, 128]
D = 8


def timed(fn, reps, before=None):
    import numpy as np
    import torch

    ts = []
    for _ in range(reps):
        if before is not None:
            before()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def _setup(N, k, n_fit):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import pygpr_amd as pg

    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.random((N + 8 * 128, D)))
    y = torch.from_numpy(np.sin(3.0 * x.numpy()).sum(1))
    hp = torch.tensor([1.0] + [0.7] * D + [0.1], dtype=torch.float64)
    gp = pg.Exact_GP(x[:n_fit], y[:n_fit], pg.Compose([pg.Squared_exponential(), pg.White_noise()]))
    gp.set_params(hp)
    gp.update()
    return gp, x, y, hp


def _chol_args(gp, x, k):
    """Buffers for pg_chol_append on the model's expert at its current n, for the next k points of x."""
    import torch

    from pygpr_amd._ops import JITTER, get_ops, pad_to
    from pygpr_amd.covar import spec_of

    ops = get_ops()
    e = gp._experts[0]
    spec, _ = spec_of(gp.cov, D)
    minv = gp._minv(e)
    u = ops.zeros(e.n_pad)
    ops.trmv(minv, e.y, u, 0)
    xn = ops.to_device(x[e.n: e.n + k])
    kt = ops.empty(pad_to(k, 128), e.n_pad)
    knn = ops.empty(pad_to(k, 128), pad_to(k, 128))
    ops.kernel_build(spec, e.hp, xn, e.x, kt)
    ops.kernel_build(spec, e.hp, xn, None, knn, jitter=JITTER)
    yn = ops.to_device(x[e.n: e.n + k, 0].clone())
    work = ops.empty(ops.chol_append_worksize(e.n_pad, k, torch.float64))
    info = torch.zeros(1, dtype=torch.int32, device=ops.device)
    return lambda: ops.chol_append(e.n, k, e.chol, e.invd, minv, kt, knn, yn, u, e.alpha, work, info), info


def child(N, k):
    import torch

    res = {"N": N, "k": k}
    # Exact_GP.append: blocks of k from N - 1024 on (the first one forms L^-1 and u: not timed)
    gp, x, y, hp = _setup(N, k, N - 1024)
    gp.append(x[N - 1024: N - 1024 + k], y[N - 1024: N - 1024 + k])
    pos = [N - 1024 + k]

    def one():
        gp.append(x[pos[0]: pos[0] + k], y[pos[0]: pos[0] + k])
        pos[0] += k

    res["append_us"] = timed(one, reps=5)
    res["append_n"] = pos[0] - 3 * k
    # the C call alone at n = N - 128
    gp, x, y, hp = _setup(N, k, N - 128)
    fn, info = _chol_args(gp, x, k)
    fn()
    torch.cuda.synchronize()
    assert int(info.item()) == 0
    res["chol_us"] = timed(fn, reps=10)
    n = N - 128
    res["bytes"] = 3 * n * n / 2 * 8 + 6 * k * n * 8
    # the refit on N points
    gp, x, y, hp = _setup(N, k, N)
    res["update_us"] = timed(gp.update, reps=5, before=lambda: setattr(gp, "need_upd", True))
    print(json.dumps(res))


def child_chol(N, k, reps):
    import torch

    gp, x, y, hp = _setup(N, k, N - 128)
    fn, info = _chol_args(gp, x, k)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    assert int(info.item()) == 0
    print(json.dumps({"N": N, "k": k, "reps": reps}))


def main():
    limit = 240.0
    if "--limit" in sys.argv:
        limit = float(sys.argv[sys.argv.index("--limit") + 1])
    sys.path.insert(0, ROOT)
    from pygpr_amd._lib import build_id

    print("build", json.dumps(build_id()))
    rows = []
    for N in NS:
        for k in KS:
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(N), str(k)], capture_output=True, text=True,
                                   timeout=limit)
            except subprocess.TimeoutExpired:
                print("probe_append: N=%d k=%d passed its %.0f s limit -- nothing more is started" % (N, k, limit))
                sys.exit(1)
            if r.returncode != 0:
                print(r.stdout[-2000:], r.stderr[-4000:], sep="\n")
                print("probe_append: N=%d k=%d ended with %d -- nothing more is started" % (N, k, r.returncode))
                sys.exit(1)
            rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(json.dumps(rows[-1]), flush=True)
    print("| N | k | Exact_GP.append (us) | pg_chol_append (us) | GB/s | update() refit (us) | refit / append |")
    print("|---:|---:|---:|---:|---:|---:|---:|")
    for r in rows:
        print("| %d | %d | %.0f | %.0f | %.0f | %.0f | %.1f |" % (r["N"], r["k"], r["append_us"], r["chol_us"], r["bytes"] / r["chol_us"] * 1e-3,
                                                              r["update_us"], r["update_us"] / r["append_us"]))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(int(sys.argv[2]), int(sys.argv[3]))
    elif len(sys.argv) > 1 and sys.argv[1] == "--child-chol":
        child_chol(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
    else:
        main()
