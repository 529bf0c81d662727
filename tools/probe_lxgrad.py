"""The low-rank training-input gradient and the losses built on it, on the GPU.

kernel   pg_kernel_lowrank_xgrad in its symmetric form (n x n ordered pairs, d = 8, r = 16, se + wn, fp64) against the route available
         without it: U V^T + V U^T in row slabs of 8192 on the GEMM core (one NT product of [U | V] with [V | U], the factor columns in a
         128-column buffer) and pg_kernel_xgrad with the dense slab as B.  The two alternate in one process; median of `--reps` after two
         warm-ups, device events.  Reported: ms and ps per ordered pair of both, the ratio, the slab's GEMM alone, pg_kernel_matmul_dx at 16
         right-hand sides and pg_kernel_matmul at 1 (the pair evaluation with and without the derivative's chains, for what bounds the
         kernel), the largest difference of the two outputs over the largest entry, and the memory of both routes.
model    Stochastic_MLE on an Iterative_GP at n = 65536 (15 probes): one loss_and_grads beside one loss_and_grad, each on a fresh loss.

Every section runs in a child process of its own under a time limit; a section that fails or runs out of time ends the probe.  One JSON
line per section, written to `--out`.

    python tools/probe_lxgrad.py [--what kernel,model] [--n 65536] [--reps 5] [--out profiles/lxgrad_probe.json]
"""
import argparse
import json
import os
import subprocess
import sys

LIMIT = {"kernel": 240, "model": 420}      # seconds a section may take
SLAB = 8192
R = 16


def kernel_section(n, reps):
    import torch

    import pygpr_amd as pg
    from pygpr_amd import _lib
    from pygpr_amd import sparse as sp
    from probe_kmatmul import D, problem, timed_pair

    ops = pg._ops.get_ops()
    cov = pg.Compose([pg.Squared_exponential(), pg.White_noise()])
    (full,), _ = pg.covar.spec_of(cov, D)
    spec = sp._stationary(full)
    x, _, hp = problem(n)
    xd, hpd = ops.to_device(torch.from_numpy(x), torch.float64), ops.to_device(torch.from_numpy(hp), torch.float64)
    gen = torch.Generator(device="cuda").manual_seed(3)
    u = torch.randn(n, R, dtype=torch.float64, device="cuda", generator=gen)
    v = torch.randn(n, R, dtype=torch.float64, device="cuda", generator=gen)
    uv, vu = ops.zeros(n, 128), ops.zeros(n, 128)      # [U | V] and [V | U]: (U V^T + V U^T)_slab = [U | V]_slab [V | U]^T
    uv[:, :R], uv[:, R: 2 * R], vu[:, :R], vu[:, R: 2 * R] = u, v, v, u
    slab = ops.empty(SLAB, n)
    out_f, out_c, out_d, out_k = ops.empty(n, D), ops.empty(n, D), ops.empty(n, D, R), ops.empty(n, 1)
    size = ops.kernel_lowrank_xgrad_worksize(n, n, D, R)
    work = ops.empty(size) if size > 0 else None

    def fused():
        ops.kernel_lowrank_xgrad(spec, hpd, xd, None, u, v, out=out_f, work=work)

    def gemm_only():
        for s in range(0, n, SLAB):
            ops.gemm_raw(_lib.GEMM_NT, SLAB, n, 128, 1.0, uv[s: s + SLAB], vu, 0.0, slab)

    def composed():
        for s in range(0, n, SLAB):
            ops.gemm_raw(_lib.GEMM_NT, SLAB, n, 128, 1.0, uv[s: s + SLAB], vu, 0.0, slab)
            ops.kernel_xgrad(spec, hpd, xd[s: s + SLAB], xd, b=slab, out_b=out_c[s: s + SLAB])

    def matmul_dx():
        ops.kernel_matmul_dx(spec, hpd, xd, xd, v, out=out_d)

    def matmul():
        ops.kernel_matmul(spec, hpd, xd, xd, v[:, :1], out=out_k)

    t_f, t_c, t_g, t_d, t_k = timed_pair([fused, composed, gemm_only, matmul_dx, matmul], reps)
    pairs = float(n) * n
    ps = lambda t: round(t * 1e9 / pairs, 3)      # noqa: E731
    return {"section": "kernel", "n": n, "d": D, "r": R, "dtype": "fp64", "model": "se+wn", "form": "symmetric", "reps": reps,
            "slab_rows": SLAB, "fused_ms": round(t_f, 3), "composed_ms": round(t_c, 3), "gemm_only_ms": round(t_g, 3),
            "matmul_dx_16_ms": round(t_d, 3), "matmul_1_ms": round(t_k, 3), "fused_ps_per_pair": ps(t_f), "composed_ps_per_pair": ps(t_c),
            "matmul_dx_16_ps_per_pair": ps(t_d), "matmul_1_ps_per_pair": ps(t_k), "composed_over_fused": round(t_c / t_f, 3),
            "fused_over_matmul_1": round(t_f / t_k, 3), "max_diff_over_max": float((out_f - out_c).abs().max() / out_c.abs().max()),
            "fused_work_bytes": 8 * size, "composed_slab_bytes": 8 * SLAB * n, "dense_weight_bytes": 8 * n * n}


def model_section(n):
    import torch

    import pygpr_amd as pg
    from probe_kmatmul import D, problem, wall

    cov = pg.Compose([pg.Squared_exponential(), pg.White_noise()])
    x, y, hp = problem(n)
    model = pg.Iterative_GP(torch.from_numpy(x), torch.from_numpy(y), cov)
    model.set_params(torch.from_numpy(hp))
    wall(lambda: pg.Stochastic_MLE(model).loss_and_grads(hp))      # warm-up: the upload, the allocator, the kernels' first launches
    both = pg.Stochastic_MLE(model)
    (l2, g2, gx), t_both = wall(lambda: both.loss_and_grads(hp))
    plain = pg.Stochastic_MLE(model)
    (l1, g1), t_plain = wall(lambda: plain.loss_and_grad(hp))
    _, t_x = wall(lambda: plain.grad_x(hp))
    return {"section": "model", "n": n, "d": D, "probes": both.probes, "rank": model.rank, "tol": model.tol,
            "iterations": both.slq_info["iterations"], "loss_and_grad_ms": round(t_plain, 1), "loss_and_grads_ms": round(t_both, 1),
            "grad_x_after_ms": round(t_x, 1), "solves": [plain.solves, both.solves], "xgrad_calls": [plain.xgrad_calls, both.xgrad_calls],
            "same_loss_bits": bool(float(l1) == float(l2)), "same_grad_bits": bool((g1 == g2).all()),
            "max_abs_grad_x": float(abs(gx).max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="kernel,model")
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="profiles/lxgrad_probe.json")
    ap.add_argument("--section", default=None, help="run this one section in this process and print its line")
    args = ap.parse_args()
    here = os.path.dirname(os.path.abspath(__file__))
    if args.section:
        sys.path.insert(0, os.path.dirname(here))
        sys.path.insert(0, here)
        line = kernel_section(args.n, args.reps) if args.section == "kernel" else model_section(args.n)
        print("LINE " + json.dumps(line), flush=True)
        return 0
    lines = []
    for what in args.what.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--section", what, "--n", str(args.n), "--reps", str(args.reps)]
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT[what])
        except subprocess.TimeoutExpired:
            print("section %s ran out of its %d s: the probe ends here" % (what, LIMIT[what]), flush=True)
            return 1
        got = [ln[5:] for ln in res.stdout.splitlines() if ln.startswith("LINE ")]
        if res.returncode != 0 or not got:
            print("section %s failed (exit %d): the probe ends here\n%s" % (what, res.returncode, res.stderr[-2000:]), flush=True)
            return 1
        print(got[0], flush=True)
        lines.append(got[0])
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
