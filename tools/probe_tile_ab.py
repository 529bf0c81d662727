"""A/B of the covariance tile kernels between two builds of the library in one process on the same box (raw ctypes: pg_create,
pg_kernel_build, pg_nlml_grad and pg_nlml_grad_worksize only).
  (1) bits: pg_kernel_build (mirrored, lower-only, cross) and pg_nlml_grad on small shapes that reach every branch -- n = 333 against
      m = 200 (interior, diagonal and ragged tiles, strips of several tiles), d = 2 / 8 / 13 / 20 (every staging width, every matrix-pipe
      width and none), fp64 and fp32, each stationary kind as a single child and SE + Matern-5/2 -- on the default routing and again with
      PG_KB_MFMA=0 / PG_GRAD_MFMA=0 (the VALU bodies); torch.equal per output, one line per case, the count of mismatches at the end;
  (2) time: lower-only and mirrored build and the gradient contraction at N = 16384 fp64 D = 8 / 16 (SE) and n = 33792 fp32 D = 16
      (Matern-5/2), HIP events after a warm-up call, A and B interleaved; the spread between A's own repetitions is printed beside B / A.
python tools/probe_tile_ab.py libA.so libB.so [--no-time]"""
import ctypes as C, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pygpr_amd._lib import CovSpec
vp, i_, l_, d_ = C.c_void_p, C.c_int, C.c_long, C.c_double
RBF, M52, M32, M12 = 0, 1, 3, 4
NAMES = {RBF: "se", M52: "m52", M32: "m32", M12: "m12"}
def load(path):
    lib = C.CDLL(path)
    lib.pg_create.argtypes = [C.POINTER(vp)]
    lib.pg_kernel_build.argtypes = [vp, i_, C.POINTER(CovSpec), vp, vp, l_, i_, vp, l_, i_, i_, i_, i_, d_, vp, l_, i_, i_, vp]
    lib.pg_nlml_grad.argtypes = [vp, i_, C.POINTER(CovSpec), vp, vp, l_, i_, i_, vp, l_, vp, vp, i_, vp, l_, vp]
    lib.pg_nlml_grad_worksize.argtypes = [i_, i_]; lib.pg_nlml_grad_worksize.restype = l_
    h = vp(); assert lib.pg_create(C.byref(h)) == 0
    return lib, h
def make_spec(kinds, d):
    sp = CovSpec(); sp.ncomp = len(kinds)
    for c, k in enumerate(kinds): sp.kind[c] = k; sp.off[c] = c * (d + 1)
    sp.nnoise = 1; sp.noise_off[0] = len(kinds) * (d + 1)
    return sp, len(kinds) * (d + 1) + 1
def stream(): return vp(torch.cuda.current_stream().cuda_stream)
def ptr(t): return vp(t.data_ptr() if t is not None else 0)
def build(lib, h, dt, sp, hp, xr, xc, d, lower, k):
    nr, nc = xr.shape[0], (xc.shape[0] if xc is not None else xr.shape[0])
    rc = lib.pg_kernel_build(h, dt, C.byref(sp), ptr(hp), ptr(xr), xr.stride(0), nr, ptr(xc), xc.stride(0) if xc is not None else 0, nc, d,
                             lower, 0, 1e-7, ptr(k), k.stride(0), k.shape[0], k.shape[1], stream())
    assert rc == 0, rc
def grad(lib, h, dt, sp, hp, x, n, d, kinv, alpha, g, work):
    rc = lib.pg_nlml_grad(h, dt, C.byref(sp), ptr(hp), ptr(x), x.stride(0), n, d, ptr(kinv), kinv.stride(0), ptr(alpha), ptr(g), g.numel(), ptr(work),
                          work.numel(), stream())
    assert rc == 0, rc
def pad(n): return (n + 63) // 64 * 64

(pa, pb) = [a for a in sys.argv[1:] if not a.startswith("--")]
libs = [load(pa), load(pb)]

# ---------------------------------------------------------------- (1) bits
n, m = 333, 200
npad, mpad = pad(n), pad(m)
bad = 0
for mode in ("default", "0"):
    for var in ("PG_KB_MFMA", "PG_GRAD_MFMA"):
        if mode == "default": os.environ.pop(var, None)
        else: os.environ[var] = mode
    for d in (2, 8, 13, 20):
        for dt, tdt in ((0, torch.float64), (1, torch.float32)):
            for kinds in ((RBF,), (M52,), (M32,), (M12,), (RBF, M52)):
                rng = np.random.default_rng(1000 * d + 10 * dt + len(kinds) + kinds[0])
                sp, nhp = make_spec(kinds, d)
                hph = np.concatenate([np.concatenate([[1.2 - 0.3 * c], 0.4 + 0.8 * rng.random(d)]) for c in range(len(kinds))] + [[0.1]])
                hp = torch.from_numpy(hph).cuda()
                x = torch.from_numpy(rng.random((n, d))).to(tdt).cuda()
                xp = torch.from_numpy(rng.random((m, d))).to(tdt).cuda()
                kinv = torch.zeros(npad, npad, dtype=tdt, device="cuda"); alpha = torch.zeros(npad, dtype=tdt, device="cuda")
                s = torch.from_numpy(rng.standard_normal((n, n))).to(tdt).cuda()
                kinv[:n, :n] = s + s.T; alpha[:n] = torch.from_numpy(rng.standard_normal(n)).to(tdt).cuda()
                outs = []
                for lib, h in libs:
                    full = torch.full((npad, npad), 7.0, dtype=tdt, device="cuda"); low = torch.full_like(full, 7.0)
                    cross = torch.full((mpad, npad), 7.0, dtype=tdt, device="cuda")
                    build(lib, h, dt, sp, hp, x, None, d, 0, full); build(lib, h, dt, sp, hp, x, None, d, 1, low); build(lib, h, dt, sp, hp, xp, x, d, 0, cross)
                    g = torch.zeros(nhp, dtype=torch.float64, device="cuda")
                    work = torch.empty(lib.pg_nlml_grad_worksize(n, nhp), dtype=torch.float64, device="cuda")
                    grad(lib, h, dt, sp, hp, x, n, d, kinv, alpha, g, work)
                    torch.cuda.synchronize()
                    outs.append((full, low, cross, g))
                name = "%s d=%-2d %s %-7s" % ("mfma=" + mode, d, "f64" if dt == 0 else "f32", "+".join(NAMES[k] for k in kinds))
                res = []
                for what, a, b in zip(("mirrored", "lower", "cross", "grad"), outs[0], outs[1]):
                    if what == "grad" and mode == "0" and dt == 0 and kinds == (RBF,) and d <= 8:
                        # the yardstick kernel of this input changed by design (direct differences in both, another summation order)
                        res.append("grad rel %.2e (other kernel by design)" % float(((a - b).abs() / a.abs().max()).max()))
                        continue
                    ok = torch.equal(a, b)
                    bad += 0 if ok else 1
                    res.append("%s %s" % (what, "equal" if ok else "MISMATCH (max abs %.3e)" % float((a - b).abs().max())))
                print(name, " | ".join(res), flush=True)
for var in ("PG_KB_MFMA", "PG_GRAD_MFMA"): os.environ.pop(var, None)
print("mismatches: %d" % bad, flush=True)

# ---------------------------------------------------------------- (2) time
if "--no-time" in sys.argv: sys.exit(1 if bad else 0)
def best_of(run, reps=7):
    run(); torch.cuda.synchronize(); best = 1e9
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); run(); b.record(); torch.cuda.synchronize(); best = min(best, a.elapsed_time(b))
    return best
for nn, d, dt, tdt, kind in ((16384, 8, 0, torch.float64, RBF), (16384, 16, 0, torch.float64, RBF), (33792, 16, 1, torch.float32, M52)):
    sp, nhp = make_spec((kind,), d)
    x = torch.from_numpy(np.random.default_rng(d).random((nn, d))).to(tdt).cuda()
    hp = torch.tensor([1.0] + [1.0] * d + [0.1], dtype=torch.float64).cuda()
    k = torch.empty(nn, nn, dtype=tdt, device="cuda")
    kinv = torch.randn(nn, nn, dtype=tdt, device="cuda"); alpha = torch.randn(nn, dtype=tdt, device="cuda")
    g = torch.zeros(nhp, dtype=torch.float64, device="cuda")
    work = torch.empty(libs[0][0].pg_nlml_grad_worksize(nn, nhp), dtype=torch.float64, device="cuda")
    cols = {"lower": lambda lib, h: build(lib, h, dt, sp, hp, x, None, d, 1, k), "mirrored": lambda lib, h: build(lib, h, dt, sp, hp, x, None, d, 0, k),
            "grad": lambda lib, h: grad(lib, h, dt, sp, hp, x, nn, d, kinv, alpha, g, work)}
    for what, fn in cols.items():
        t = [[], []]
        for rep in range(4):                                   # A B A B A B A B
            for which, (lib, h) in enumerate(libs): t[which].append(best_of(lambda: fn(lib, h)))
        a, b = min(t[0]), min(t[1])
        print("n=%d d=%d %s %-4s %-8s A %.4f ms (its repetitions %.4f .. %.4f: spread %.2f %%)  B %.4f ms (%.4f .. %.4f)  B/A %.4f" % (
            nn, d, "f64" if dt == 0 else "f32", NAMES[kind], what, a, min(t[0]), max(t[0]), 100 * (max(t[0]) - a) / a, b, min(t[1]), max(t[1]), b / a), flush=True)
    del k, kinv
sys.exit(1 if bad else 0)
