"""What the tests of the covariance kinds share: the `ops` fixture, host / device conversions, the error report, the covariance object
and the specs of a model in the grammar of tests/kernel_ref.py, and the device-side inputs of the C-ABI cases.  Data and
hyper-parameter generators stay with their tests: the order of their draws decides a test's inputs."""
import numpy as np
import pytest
import torch

import pygpr_amd as pg
from pygpr_amd import _lib

CLS = {"se": pg.Squared_exponential, "m52": pg.Matern52, "m32": pg.Matern32, "m12": pg.Matern12, "rq": pg.Rational_quadratic,
       "per": pg.Periodic, "wn": pg.White_noise}


@pytest.fixture(scope="module")
def ops():
    from pygpr_amd._ops import get_ops

    return get_ops()


def dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


def host(t):
    return t.detach().cpu().double().numpy()


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def N(t):
    return t.detach().cpu().numpy()


def rel(a, ref):
    """The largest error relative to the largest reference entry, of tensors or arrays."""
    a, ref = torch.as_tensor(a).detach().cpu().double(), torch.as_tensor(ref).detach().cpu().double()
    return float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def check(name, a, ref, tol):
    e = rel(a, ref)
    print("%-52s rel err %.2e (bound %.0e)" % (name, e, tol))
    assert e <= tol, (name, e)


def compose(parts):
    """A Compose of plain parts, a lone part included."""
    return pg.Compose([CLS[p]() for p in parts])


def cov_of(model):
    """The covariance object of a term list: a tuple becomes a Product; a lone term stays bare, more than one make a Compose."""
    objs = [pg.Product([CLS[p]() for p in t]) if isinstance(t, tuple) else CLS[t]() for t in model]
    return objs[0] if len(objs) == 1 else pg.Compose(objs)


def specs_of(model, d):
    from pygpr_amd.covar import spec_of

    return spec_of(cov_of(model), d)[0]


def one_spec(model, d, product=False):
    """The single pass of a model, flagged as a product spec or not as the caller expects."""
    specs = specs_of(model, d)
    assert len(specs) == 1 and bool(specs[0].ncomp & _lib.PG_SPEC_PRODUCT) == product
    return specs[0]


def grad_inputs(ops, spec, hp, x, y, dtype):
    """hp, x, K^-1 (lower) and alpha of the model on the device, in `dtype` (as tests/test_hip_kernels.py builds them)."""
    from pygpr_amd._ops import pad_to

    n = x.shape[0]
    npad = pad_to(n)
    hpd, xd = dev(hp), dev(x, dtype)
    k = ops.empty(npad, npad, dtype=dtype)
    invd = ops.potrf_workspace(npad, dtype)
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    minv = ops.zeros(npad, npad, dtype=dtype)
    ops.build_factor(spec, hpd, xd, k, invd, info, minv)
    assert int(info.item()) == 0
    ypad = ops.zeros(npad, dtype=dtype)
    ypad[:n] = dev(y, dtype)
    u, alpha = ops.empty(npad, dtype=dtype), ops.empty(npad, dtype=dtype)
    ops.trmv(minv, ypad, u, 0)
    ops.trmv(minv, u, alpha, 1, ops.empty((npad // 256 + 1) * npad, dtype=dtype))
    kinv = ops.zeros(npad, npad, dtype=dtype)
    ops.lauum(minv, kinv)
    return hpd, xd, kinv, alpha


def builds(ops, spec, hp, x, xp, dtype):
    """The mirrored, the lower-only and the cross build of one spec, padded, on the host."""
    from pygpr_amd._ops import pad_to

    n, m = x.shape[0], xp.shape[0]
    npad, mpad = pad_to(n), pad_to(m)
    hpd, xd, xpd = dev(hp), dev(x, dtype), dev(xp, dtype)
    full, low, cross = ops.empty(npad, npad, dtype=dtype), ops.zeros(npad, npad, dtype=dtype), ops.empty(mpad, npad, dtype=dtype)
    ops.kernel_build(spec, hpd, xd, None, full, jitter=1e-7)
    ops.kernel_build(spec, hpd, xd, None, low, lower_only=True, jitter=1e-7)
    ops.kernel_build(spec, hpd, xpd, xd, cross)
    return host(full), host(low), host(cross)


def near_duplicates(rng, d, l, offset):
    """60 points, then five more at scaled distance r = 0, 1e-12, 1e-9, 1e-6, 1e-3 from points 3, 11, 19, 27, 35 (off-diagonal pairs)."""
    x = rng.random((60, d))
    extra = []
    for s, i in zip((0.0, 1e-12, 1e-9, 1e-6, 1e-3), (3, 11, 19, 27, 35)):
        u = rng.standard_normal(d)
        extra.append(x[i] + s * (u / np.linalg.norm(u)) / l)
    x = np.concatenate([x, np.array(extra)]) + offset
    return x, np.sin(-x.sum(1)) + 0.1 * rng.standard_normal(x.shape[0])
