"""ctypes binding of libpygpr_hip.so (C ABI: include/pygpr_hip.h, include/pygpr_hip_loo.h, include/pygpr_hip_sample.h,
include/pygpr_hip_sparse.h, include/pygpr_hip_select.h, include/pygpr_hip_matmul.h, include/pygpr_hip_lowrank.h, include/pygpr_hip_feature.h,
include/pygpr_hip_dmatmul.h, include/pygpr_hip_rowsq.h, include/pygpr_hip_lxgrad.h, include/pygpr_hip_vecchia.h).

There is no CPU fallback: `load()` raises if the shared object is missing, and every compute call
needs a HIP device.  Build the library with `python __graft_entry__.py` (hipcc, gfx950).
"""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libpygpr_hip.so")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "pygpr_hip.h")
HEADER_LOO = os.path.join(os.path.dirname(_HERE), "include", "pygpr_hip_loo.h")   # leave-one-out entry points (a second public header)
HEADER_SAMPLE = os.path.join(os.path.dirname(_HERE), "include", "pygpr_hip_sample.h")   # the device normal generator (a third)
HEADER_SPARSE = os.path.join(os.path.dirname(_HERE), "include", "pygpr_hip_sparse.h")   # the inducing-point GP's contraction (a fourth)
HEADER_SELECT = os.path.join(os.path.dirname(_HERE), "include", "pygpr_hip_select.h")   # greedy inducing-point selection (a fifth)
HEADER_MATMUL = os.path.join(os.path.dirname(_HERE), "include", "pygpr_hip_matmul.h")   # the matrix-free covariance product (a sixth)
HEADER_LOWRANK = os.path.join(os.path.dirname(_HERE), "include", "pygpr_hip_lowrank.h")   # the low-rank gradient contraction (a seventh)
HEADER_FEATURE = os.path.join(os.path.dirname(_HERE), "include", "pygpr_hip_feature.h")   # the random-feature product (an eighth)
HEADER_DMATMUL = os.path.join(os.path.dirname(_HERE), "include", "pygpr_hip_dmatmul.h")   # the derivative's matrix-free product (a ninth)
HEADER_ROWSQ = os.path.join(os.path.dirname(_HERE), "include", "pygpr_hip_rowsq.h")   # the cross-covariance's squared row norms (a tenth)
HEADER_LXGRAD = os.path.join(os.path.dirname(_HERE), "include", "pygpr_hip_lxgrad.h")   # the low-rank training-input gradient (an eleventh)
# the nearest-neighbour GP's search and blocks (a twelfth).  Not a HEADER_* name: tests/test_streamed_cpu.py counts those and holds their
# stream-taking exports to the table of tests/test_streamed_gpu.py; this header's get their cases in tests/test_vecchia_framed_gpu.py
VECCHIA_HEADER = os.path.join(os.path.dirname(_HERE), "include", "pygpr_hip_vecchia.h")

PG_F64, PG_F32 = 0, 1
PG_KIND_RBF, PG_KIND_MATERN52, PG_KIND_SQDIST, PG_KIND_MATERN32, PG_KIND_MATERN12 = 0, 1, 2, 3, 4
PG_KIND_RQ = 6      # (5 is unassigned: the library refuses it)
PG_KIND_PERIODIC = 8    # hp = [sigma, l_1..l_d, p_1..p_d] (7, like 5, is unassigned: the library refuses it)
PG_MAX_COMP, PG_MAX_DIM = 4, 64
# or-ed into CovSpec.ncomp: the stationary components are multiplied into one term (read from the header: the C side owns the value)
PG_SPEC_PRODUCT = int(re.search(r"#define\s+PG_SPEC_PRODUCT\s+(0[xX][0-9a-fA-F]+|\d+)", open(HEADER).read()).group(1), 0)
PAD = 256  # every dimension given to the O(n^3) entry points is a multiple of this

GEMM_NT, GEMM_NT_RP, GEMM_NN, GEMM_TN, GEMM_TT, GEMM_NT_64, GEMM_NT_64x128, GEMM_NT_32x64, GEMM_NT_32x128, GEMM_TT_64, GEMM_NT_32x32 = 0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11
GEMM_TN_64 = 13
# fp64 only: the 128 x 128 tile of GEMM_NT / NN / TN / TT on four waves with a software-pipelined K loop (gemm.h: GEMM_*_128_PL); same bits
PIPELINED = {GEMM_NT: 14, GEMM_NN: 15, GEMM_TN: 16, GEMM_TT: 17}


class CovSpec(C.Structure):
    _fields_ = [
        ("ncomp", C.c_int),
        ("kind", C.c_int * PG_MAX_COMP),
        ("off", C.c_int * PG_MAX_COMP),
        ("nnoise", C.c_int),
        ("noise_off", C.c_int * PG_MAX_COMP),
    ]


# The vocabulary of include/pygpr_hip.h.  Scalars keep their width; a pg_handle and every pointer travel as void* (c_void_p takes
# None, an address and byref(...) alike), the covariance spec keeps its struct type.
_RESTYPES = {"int": C.c_int, "long": C.c_long, "const char*": C.c_char_p}
_ARGTYPES = {"int": C.c_int, "long": C.c_long, "double": C.c_double, "const pg_covspec*": C.POINTER(CovSpec)}
_ARGTYPES.update((t, C.c_void_p) for t in ("pg_handle", "pg_handle*", "void*", "const void*", "double*", "const double*", "int*", "const int*", "long*"))


def _strip_comments(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def header_symbols():
    """Names of every function declared in include/pygpr_hip.h."""
    return sorted(set(re.findall(r"\b(pg_[a-z_0-9]+)\s*\(", _strip_comments(open(HEADER).read()))))


def parse_prototypes(text):
    """name -> (return type, [parameter types]) of every `pg_*` prototype in the C text, the types as spelled there with the white
    space normalised ("const void*")."""
    def norm(t):
        return re.sub(r"\s*\*", "*", " ".join(t.split()))

    protos = {}
    for ret, name, params in re.findall(r"([\w \t*]+?)\b(pg_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", _strip_comments(text)):
        types = []
        for p in [q.strip() for q in params.split(",")] if params.strip() != "void" else []:
            m = re.fullmatch(r"(.*[\s*])[A-Za-z_]\w*", p, flags=re.S)      # a type, then the parameter's name
            if not m:
                raise ValueError("%s: cannot read parameter %r" % (name, p))
            types.append(norm(m.group(1)))
        protos[name] = (norm(ret), types)
    return protos


def signatures(protos):
    """name -> (restype, argtypes) for ctypes.  A type outside the header's vocabulary is an error, never a guess."""
    sigs = {}
    for name, (ret, params) in protos.items():
        for t, table in [(ret, _RESTYPES)] + [(p, _ARGTYPES) for p in params]:
            if t not in table:
                raise ValueError("%s: no ctypes mapping for the type %r" % (name, t))
        sigs[name] = (_RESTYPES[ret], [_ARGTYPES[p] for p in params])
    return sigs


_SIGS = signatures(parse_prototypes(open(HEADER).read()))
_SIGS_LOO = signatures(parse_prototypes(open(HEADER_LOO).read()))
_SIGS_SAMPLE = signatures(parse_prototypes(open(HEADER_SAMPLE).read()))
_SIGS_SPARSE = signatures(parse_prototypes(open(HEADER_SPARSE).read()))
_SIGS_SELECT = signatures(parse_prototypes(open(HEADER_SELECT).read()))
_SIGS_MATMUL = signatures(parse_prototypes(open(HEADER_MATMUL).read()))
_SIGS_LOWRANK = signatures(parse_prototypes(open(HEADER_LOWRANK).read()))
_SIGS_FEATURE = signatures(parse_prototypes(open(HEADER_FEATURE).read()))
_SIGS_DMATMUL = signatures(parse_prototypes(open(HEADER_DMATMUL).read()))
_SIGS_ROWSQ = signatures(parse_prototypes(open(HEADER_ROWSQ).read()))
_SIGS_LXGRAD = signatures(parse_prototypes(open(HEADER_LXGRAD).read()))
_SIGS_VECCHIA = signatures(parse_prototypes(open(VECCHIA_HEADER).read()))

_lib = None


def load(check_symbols=False):
    """dlopen the library (no GPU needed for that) and attach the prototypes."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libpygpr_hip.so not found at %s -- the HIP extension is required (no CPU fallback); "
                "build it with `python __graft_entry__.py`" % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in (list(_SIGS.items()) + list(_SIGS_LOO.items()) + list(_SIGS_SAMPLE.items()) + list(_SIGS_SPARSE.items())
                                  + list(_SIGS_SELECT.items()) + list(_SIGS_MATMUL.items()) + list(_SIGS_LOWRANK.items()) + list(_SIGS_FEATURE.items())
                                  + list(_SIGS_DMATMUL.items()) + list(_SIGS_ROWSQ.items()) + list(_SIGS_LXGRAD.items()) + list(_SIGS_VECCHIA.items())):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _lib = lib
    if check_symbols:
        missing = [s for s in header_symbols() + sorted(_SIGS_LOO) + sorted(_SIGS_SAMPLE) + sorted(_SIGS_SPARSE) + sorted(_SIGS_SELECT)
                   + sorted(_SIGS_MATMUL) + sorted(_SIGS_LOWRANK) + sorted(_SIGS_FEATURE) + sorted(_SIGS_DMATMUL) + sorted(_SIGS_ROWSQ) + sorted(_SIGS_LXGRAD) + sorted(_SIGS_VECCHIA) if not hasattr(_lib, s)]
        unbound = [s for s in header_symbols() if s not in _SIGS]
        if missing or unbound:
            raise RuntimeError("C ABI mismatch: missing in .so %s, unbound in _lib.py %s" % (missing, unbound))
    return _lib


def last_error():
    return load().pg_last_error().decode()


def check(rc, what=""):
    if rc != 0:
        raise RuntimeError("libpygpr_hip %s failed (rc=%d): %s" % (what, rc, last_error()))


def build_id():
    """Identity of the running build: hash of the kernel sources + C headers (what a profile must match to describe
    this build) and of the shared object itself."""
    import hashlib

    csrc = os.path.join(_HERE, "csrc")
    h = hashlib.sha256()
    for f in sorted(os.listdir(csrc)) + [HEADER, HEADER_LOO, HEADER_SAMPLE, HEADER_SPARSE, HEADER_SELECT, HEADER_MATMUL, HEADER_LOWRANK, HEADER_FEATURE, HEADER_DMATMUL, HEADER_ROWSQ, HEADER_LXGRAD, VECCHIA_HEADER]:
        path = f if os.path.isabs(f) else os.path.join(csrc, f)
        if path.endswith((".hip", ".h")):
            h.update(os.path.basename(path).encode())
            h.update(open(path, "rb").read())
    lib = hashlib.sha256(open(LIB_PATH, "rb").read()).hexdigest()[:16] if os.path.exists(LIB_PATH) else None
    return {"src_sha16": h.hexdigest()[:16], "lib_sha16": lib}
