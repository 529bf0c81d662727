/*
 * libpygpr_hip -- standard normal variates from a counter-based generator on the device: the random input of joint posterior and
 * prior draws (Exact_GP.sampler, PosteriorSampler.draw).  A third public header of the same library: the entry point below is new
 * (the reference exports sample_gp, whose body cannot run), pygpr_amd/_lib.py binds it from this file as it binds
 * include/pygpr_hip.h and include/pygpr_hip_loo.h, and the same closed type vocabulary applies (the seed travels as long).
 *
 * normal(seed, stream_id, row, q), the ONE definition of every value this header produces:
 *   generator  Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): ten rounds with the
 *              multipliers 0xD2511F53 (on counter word 0) and 0xCD9E8D57 (on counter word 2); the key words grow by the Weyl
 *              increments 0x9E3779B9 and 0xBB67AE85 before every round but the first
 *   key        (low 32 bits of seed, high 32 bits of seed), the seed read as its two's-complement bit pattern: negative seeds are legal
 *   counter    (q >> 1, row, stream_id, 0): one block x0..x3 yields the two normals of the columns 2j and 2j + 1 of a row
 *   uniforms   k1 = (x0 >> 5) 2^26 + (x1 >> 6),  u1 = (k1 + 1) 2^-53 in (0, 1];   k2 = (x2 >> 5) 2^26 + (x3 >> 6),  u2 = k2 2^-53 in [0, 1)
 *              (both exact in fp64)
 *   Box-Muller in fp64: rad = sqrt(-2 log u1), ang = fl(2 pi) u2 (one rounding); the even column is rad cos(ang), the odd column
 *              rad sin(ang).  |z| <= sqrt(2 * 53 * ln 2) = 8.57, never inf or NaN
 *   dtype      PG_F32 stores the fp64 value rounded to float: an fp32 draw is the rounding of the fp64 draw, not another stream
 * so an element depends on (seed, stream_id, row, q) alone -- not on how many rows or columns a call generates, on the chunks a caller
 * splits its rows into, on the padding or on the dtype.  log, sqrt and sincos are the accurate ones (the library is built without
 * fast-math): against a NumPy restatement of the above (tests/philox_ref.py) the values agree to a few ulp.
 *
 * Conventions: those of include/pygpr_hip.h --
 *   - every matrix pointer is a DEVICE pointer owned by the caller; the library allocates nothing
 *   - matrices are row-major with a leading dimension in elements; dtype is PG_F64 or PG_F32
 *   - alignment: nothing is refused.  pg_randn stores 16-byte words when Z and ldz are multiples of 16 bytes and single elements
 *     otherwise (and for the last word of a row when cols_pad is no multiple of the word); both give the same bits
 *   - calls are asynchronous on `stream`; return 0 = enqueued, <0 = bad argument / HIP error (text via pg_last_error())
 */
#ifndef PYGPR_HIP_SAMPLE_H
#define PYGPR_HIP_SAMPLE_H

#include "pygpr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Z[r * ldz + q] = normal(seed, stream_id, row0 + r, q) for r < rows and q < cols; every other element of rows_pad x cols_pad is
 * written as zero (the padding the GEMM core wants), and nothing outside rows_pad x cols_pad is touched -- the gap [cols_pad, ldz) of
 * a row neither.  0 <= rows <= rows_pad, 0 <= cols <= cols_pad <= ldz, rows_pad >= 1, cols_pad >= 1, row0 >= 0 and
 * row0 + rows <= 2^31 - 1.  One launch; a thread produces one 16-byte word (one Philox block in fp64, two in fp32), consecutive
 * lanes consecutive words of a row.  The draw mean + Z L^T of PosteriorSampler is pg_trmm_lower_kt_batched with Minv := L and
 * Kt := Z (L with a cleared upper triangle: that product reads the whole diagonal 128-blocks). */
int pg_randn(pg_handle h, int dtype, long seed, int stream_id, int row0, int rows, int cols, void* Z, long ldz, int rows_pad, int cols_pad,
             void* stream);

#ifdef __cplusplus
}
#endif
#endif
