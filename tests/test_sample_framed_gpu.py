"""The export of include/pygpr_hip_sample.h through ctypes on FRAMED operands (tests/framed.py; the harness of tests/test_framed_gpu.py:
packed call, framed call, same bits, guards, values); tests/test_sample_cpu.py checks this list against the header.  The output is a
strided view (ld = cols_pad + gap, base 16- but not 256-byte aligned) in sentinel memory.  pg_randn refuses no alignment: the odd gaps
(and every shape whose rows are not whole 16-byte words) take its single-element stores, the others its 16-byte stores, and both must
give the bits of the packed call.

Values against tests/philox_ref.py at the bounds of tests/test_sample_gpu.py: 2e-13 absolute in fp64 (|z| <= 8.57, the argument of
sincos rounded once, log / sqrt / sincos within a few ulp: about 5e-14, times 4 for another correct libm) and 1e-6 in fp32 (one float
ulp at 8.57)."""
import numpy as np
import pytest

import philox_ref as pr
from test_framed_gpu import F32, F64, both, gaps_odd, ok, ops, p, run  # noqa: F401  (ops: the module's fixture)

pytestmark = pytest.mark.gpu

ATOL = {F64: 2e-13, F32: 1e-6}

# rows, cols, rows_pad, cols_pad: padded in both directions; unpadded with an odd width (half a block, rows that are no whole words);
# one element; several workgroups along a row with a padded width that is no multiple of the word
SHAPES = [(257, 130, 512, 256), (3, 5, 3, 5), (1, 1, 1, 1), (2, 1000, 128, 1023)]


def case_randn(bed, rows, cols, rows_pad, cols_pad, seed, stream_id, row0):
    z = bed.put("Z", shape=(rows_pad, cols_pad), role="out")
    ok(bed, bed.lib.pg_randn(bed.h, bed.code, seed, stream_id, row0, rows, cols, p(z), z.ld, rows_pad, cols_pad, bed.st()))
    ref = np.zeros((rows_pad, cols_pad))
    ref[:rows, :cols] = pr.randn(seed, stream_id, row0, rows, cols)
    pad = np.ones((rows_pad, cols_pad), bool)
    pad[:rows, :cols] = False
    return [("Z", ref, ~pad, ATOL[bed.dtype], 0.0), ("Z", 0.0, pad, 0.0, 0.0)]


@both
@gaps_odd
@pytest.mark.parametrize("rows,cols,rows_pad,cols_pad", SHAPES)
def test_randn(ops, dtype, gapset, rows, cols, rows_pad, cols_pad):
    run(ops, case_randn, dtype, gapset, rows=rows, cols=cols, rows_pad=rows_pad, cols_pad=cols_pad, seed=(1 << 40) + 3, stream_id=5, row0=1000)


@both
def test_randn_negative_seed_and_no_rows(ops, dtype):
    run(ops, case_randn, dtype, "mixed", rows=5, cols=7, rows_pad=8, cols_pad=8, seed=-1, stream_id=0, row0=0)
    run(ops, case_randn, dtype, "odd", rows=0, cols=0, rows_pad=4, cols_pad=6, seed=3, stream_id=0, row0=0)      # all padding: zeros


def test_randn_refuses_bad_shapes_on_the_host(ops):
    import ctypes as C

    import torch

    z = torch.full((4, 8), 7.0, dtype=F64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    zp = C.c_void_p(z.data_ptr())
    lib, h = ops.lib, ops.h
    # rows, cols, ldz, rows_pad, cols_pad, row0, dtype
    for rows, cols, ldz, rp, cp, row0, code in ((5, 8, 8, 4, 8, 0, 0), (4, 9, 8, 4, 8, 0, 0), (4, 8, 7, 4, 8, 0, 0), (-1, 8, 8, 4, 8, 0, 0),
                                               (4, 8, 8, 0, 8, 0, 0), (4, 8, 8, 4, 8, -1, 0), (4, 8, 8, 4, 8, 2 ** 31 - 2, 0), (4, 8, 8, 4, 8, 0, 2)):
        assert lib.pg_randn(h, code, 1, 0, row0, rows, cols, zp, ldz, rp, cp, st) != 0
    assert lib.pg_randn(h, 0, 1, 0, 0, 4, 8, None, 8, 4, 8, st) != 0
    torch.cuda.synchronize()
    assert bool((z == 7.0).all())      # nothing was enqueued
