"""A/B of the covariance tile kernels between two builds of the library in one process on the same box (raw ctypes: pg_create,
pg_kernel_build, pg_nlml_grad and pg_nlml_grad_worksize only).
  (1) bits: pg_kernel_build (mirrored, lower-only, cross) and pg_nlml_grad on small shapes that reach every branch -- n = 333 against
      m = 200 (interior, diagonal and ragged tiles, strips of several tiles), d = 2 / 8 / 13 / 20 (every staging width, every matrix-pipe
      width and none), fp64 and fp32, each stationary kind as a single child and SE + Matern-5/2 -- on the default routing and again with
      PG_KB_MFMA=0 / PG_GRAD_MFMA=0 (the VALU bodies); torch.equal per output, one line per case, the count of mismatches at the end;
  (2) time: lower-only and mirrored build and the gradient contraction at N = 16384 fp64 D = 8 / 16 (SE) and n = 33792 fp32 D = 16
      (Matern-5/2), HIP events after a warm-up call, A and B interleaved; the spread between A's own repetitions is printed beside B / A.
python tools/probe_tile_ab.py libA.so libB.so [--no-time]

--pair [libA_copy.so] [--json=PATH]: instead of (1) and (2), the VALU kernels that evaluate a component from a pair of points by direct
differences, through pygpr_amd._ops.HipOps bound to each library:
  bits  pg_kernel_cross_grad (fp64, fp32), pg_kernel_lowrank_grad (cross, symmetric), pg_kernel_matmul (symmetric, cross; nrhs 3, 20),
        pg_feature_matmul, pg_kernel_xgrad (u, B, both), pg_greedy_select and pg_nlml_grad with PG_GRAD_MFMA=0, over d = 1, 3, 5, 9, 17, 33
        (every DMAX) and a plain (se + m52 + wn), a periodic and a product (se * per) spec at 150 x 200 points (three by four tiles,
        ragged), seeded inputs; torch.equal per output (NaN pattern included), the count of mismatches at the end;
  time  the sizes of probe_sparse.py's cross-gradient chunk, probe_lowrank_grad.py, probe_kmatmul.py, probe_feature_matmul.py,
        probe_xgrad.py's m = 128 case and probe_tile_bodies.py's VALU contraction (N = 16384, D = 8): A, B and -- when a copy of A's file
        is given as the third library -- A again from that copy, interleaved, best of 7 after a warm-up, four rounds; B/A beside A'/A,
        the spread of the method in this call."""
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

def best_of(run, reps=7):
    run(); torch.cuda.synchronize(); best = 1e9
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); run(); b.record(); torch.cuda.synchronize(); best = min(best, a.elapsed_time(b))
    return best

# ---------------------------------------------------------------- --pair
def ops_for(path):
    """A HipOps whose every call goes to the library at `path` (its own handle)."""
    from pygpr_amd import _lib, _ops
    lib = C.CDLL(path)
    for sigs in (_lib._SIGS, _lib._SIGS_LOO, _lib._SIGS_SAMPLE, _lib._SIGS_SPARSE, _lib._SIGS_SELECT, _lib._SIGS_MATMUL, _lib._SIGS_LOWRANK,
                 _lib._SIGS_FEATURE):
        for name, (res, args) in sigs.items():
            fn = getattr(lib, name); fn.restype, fn.argtypes = res, args
    o = _ops.HipOps.__new__(_ops.HipOps)
    o.lib, o.h, o.device = lib, vp(), torch.device("cuda", torch.cuda.current_device())
    assert lib.pg_create(C.byref(o.h)) == 0
    return o
def pair_model(name, d, rng):
    """(spec, hp) of 'plain' = se + m52 + wn, 'per' = per + wn, 'prod' = se * per + wn"""
    from pygpr_amd import _lib, _ops
    kinds = {"plain": [_lib.PG_KIND_RBF, _lib.PG_KIND_MATERN52], "per": [_lib.PG_KIND_PERIODIC], "prod": [_lib.PG_KIND_RBF, _lib.PG_KIND_PERIODIC]}[name]
    offs, hp = [], []
    for k in kinds:
        offs.append(len(hp))
        hp += [0.8 + 0.4 * rng.random()] + list((0.8 + 0.8 * rng.random(d)) / np.sqrt(d)) + (list(0.6 + 0.5 * rng.random(d)) if k == _lib.PG_KIND_PERIODIC else [])
    spec = _ops.make_spec(kinds, offs, [len(hp)], product=name == "prod")
    return spec, torch.from_numpy(np.array(hp + [0.3])).cuda()
def pair_outputs(o, name, d):
    """Every output of the pair kernels of one library on the seeded inputs of (model, d), as a list of (label, tensor)."""
    rng = np.random.default_rng(100 * d + len(name))
    spec, hp = pair_model(name, d, rng)
    m, n, r = 150, 200, 5
    f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    z, x, w = f64(rng.random((m, d))), f64(rng.random((n, d))), f64(rng.standard_normal((m, n)))
    u, v, un = f64(rng.standard_normal((m, r))), f64(rng.standard_normal((n, r))), f64(rng.standard_normal((n, r)))
    out = []
    for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
        out.append(("cross_grad " + tag, o.kernel_cross_grad(spec, hp, z.to(dt), x.to(dt), w.to(dt), torch.zeros_like(hp))))
    out.append(("lowrank cross", o.kernel_lowrank_grad(spec, hp, z, x, u, v)))
    out.append(("lowrank sym", o.kernel_lowrank_grad(spec, hp, x, None, un, v)))
    for nrhs in (3, 20):
        rhs = f64(rng.standard_normal((n, nrhs)))
        out.append(("matmul sym %d" % nrhs, o.kernel_matmul(spec, hp, x, None, rhs, jitter=1e-6)))
        out.append(("matmul cross %d" % nrhs, o.kernel_matmul(spec, hp, z, x, rhs)))
    if name == "plain":      # (no covariance model in it: once per d)
        out.append(("feature", o.feature_matmul(z, f64(3.0 * rng.standard_normal((n, d))), f64(rng.random(n)), f64(rng.standard_normal((n, 20))))))
    uu = f64(rng.standard_normal(n))
    for tag, a, b in (("u", uu, None), ("B", None, w), ("u+B", uu, w)):
        for i, t in enumerate(o.kernel_xgrad(spec, hp, z, x, u=a, b=b)):
            if t is not None: out.append(("xgrad %s out%d" % (tag, i), t))
    for lab, t in zip(("piv", "count", "trace", "resid"), o.greedy_select(spec, hp, x, 20, 0.0)): out.append(("select " + lab, t))
    npad = pad(n)
    kinv = torch.zeros(npad, npad, dtype=torch.float64, device="cuda"); alpha = torch.zeros(npad, dtype=torch.float64, device="cuda")
    s = f64(rng.standard_normal((n, n))); kinv[:n, :n] = s + s.T; alpha[:n] = f64(rng.standard_normal(n))
    g = torch.zeros_like(hp)
    os.environ["PG_GRAD_MFMA"] = "0"
    o.nlml_grad(spec, hp, x, n, kinv, alpha, g, o.empty(o.nlml_grad_worksize(n, hp.numel())))
    os.environ.pop("PG_GRAD_MFMA")
    out.append(("nlml_grad valu", g))
    torch.cuda.synchronize()
    return out
def pair_timed(o):
    """{name: callable} at the sizes of the existing probes (fp64, d = 8, se + wn)."""
    from pygpr_amd import _lib, _ops
    d = 8
    spec = _ops.make_spec([_lib.PG_KIND_RBF], [0], [d + 1])
    hp = torch.tensor([1.0] + [1.0] * d + [0.1], dtype=torch.float64).cuda()
    gen = torch.Generator(device="cuda").manual_seed(3)
    rnd = lambda *sh: torch.rand(*sh, dtype=torch.float64, device="cuda", generator=gen)
    nrm = lambda *sh: torch.randn(*sh, dtype=torch.float64, device="cuda", generator=gen)
    x64k, x16k, z2k, x32k, q128 = rnd(65536, d), rnd(16384, d), rnd(2048, d), rnd(32768, d), rnd(128, d)
    w = nrm(2048, 32768); g = torch.zeros_like(hp)
    wk_c = o.empty(max(1, o.kernel_cross_grad_worksize(2048, 32768, hp.numel())))
    u16, v16 = nrm(65536, 16), nrm(65536, 16)
    wk_l = o.empty(max(1, o.kernel_lowrank_grad_worksize(65536, 65536, 16, hp.numel())))
    v1, v16r = nrm(65536, 1), nrm(65536, 16); out1, out16 = o.empty(65536, 1), o.empty(65536, 16)
    nu, ph, wf = nrm(4096, d), rnd(4096), nrm(4096, 16)
    uu, bb = nrm(16384), nrm(128, 16384)
    kinv, alpha = nrm(16384, 16384), nrm(16384)
    wk_g = o.empty(o.nlml_grad_worksize(16384, hp.numel()))
    def nlml():
        os.environ["PG_GRAD_MFMA"] = "0"
        o.nlml_grad(spec, hp, x16k, 16384, kinv, alpha, g, wk_g)
        os.environ.pop("PG_GRAD_MFMA")
    return {"cross_grad m=2048 n=32768": lambda: o.kernel_cross_grad(spec, hp, z2k, x32k, w, g, work=wk_c),
            "lowrank_grad sym n=65536 r=16": lambda: o.kernel_lowrank_grad(spec, hp, x64k, None, u16, v16, grad=g, work=wk_l),
            "matmul cross n=65536 nrhs=1": lambda: o.kernel_matmul(spec, hp, x64k, x64k, v1, out=out1),
            "matmul cross n=65536 nrhs=16": lambda: o.kernel_matmul(spec, hp, x64k, x64k, v16r, out=out16),
            "feature_matmul n=65536 nf=4096 nrhs=16": lambda: o.feature_matmul(x64k, nu, ph, wf, out=out16),
            "xgrad m=128 n=16384 u+B": lambda: o.kernel_xgrad(spec, hp, q128, x16k, u=uu, b=bb),
            "nlml_grad valu n=16384": nlml}
def pair_main(paths, json_path):
    import json
    allops = [ops_for(p_) for p_ in paths]
    bad = 0
    for d in (1, 3, 5, 9, 17, 33):
        for name in ("plain", "per", "prod"):
            a, b = pair_outputs(allops[0], name, d), pair_outputs(allops[1], name, d)
            diff = [la for (la, ta), (_, tb) in zip(a, b) if not torch.equal(torch.nan_to_num(ta, nan=7.0), torch.nan_to_num(tb, nan=7.0))
                    or not torch.equal(torch.isnan(ta), torch.isnan(tb))]
            bad += len(diff)
            print("d=%-2d %-5s %d outputs %s" % (d, name, len(a), "equal" if not diff else "MISMATCH: " + ", ".join(diff)), flush=True)
    print("mismatches: %d" % bad, flush=True)
    rows = {}
    fns = [pair_timed(o) for o in allops]
    for what in fns[0]:
        t = [[] for _ in allops]
        for rep in range(4):                                   # A B A' A B A' ...
            for which in range(len(allops)): t[which].append(best_of(fns[which][what]))
        best = [min(x) for x in t]
        rows[what] = {"parent_ms": round(best[0], 4), "new_ms": round(best[1], 4), "new_over_parent": round(best[1] / best[0], 4)}
        if len(best) > 2: rows[what].update({"parent_again_ms": round(best[2], 4), "parent_again_over_parent": round(best[2] / best[0], 4)})
        print(what, rows[what], flush=True)
    if json_path:
        with open(json_path, "w") as f: json.dump({"mismatches": bad, "method": "best of 7 after a warm-up, 4 interleaved rounds, HIP events", "kernels": rows}, f, indent=1)
    for o in allops: o.close()
    return 1 if bad else 0

paths = [a for a in sys.argv[1:] if not a.startswith("--")]
if "--pair" in sys.argv:
    sys.exit(pair_main(paths, next((a.split("=", 1)[1] for a in sys.argv if a.startswith("--json=")), None)))
(pa, pb) = paths
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
