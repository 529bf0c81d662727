"""NumPy restatement of the library's normal generator (include/pygpr_hip_sample.h), vectorised: Philox4x32-10 (Salmon, Moraes,
Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) keyed by the seed, one block per pair of columns of a row, two
53-bit uniforms from the block's four words and a Box-Muller transform in fp64.  Element (row, column) depends on (seed, stream, row,
column) alone."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # Weyl key increments
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (anything np.asarray takes, values < 2^32) -> the block's four output words, uint32 [..., 4]."""
    c = [np.asarray(counter, dtype=np.uint64)[..., i] & MASK for i in range(4)]
    k = [np.asarray(key, dtype=np.uint64)[..., i] & MASK for i in range(2)]
    for r in range(10):
        if r:
            k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
        p0, p1 = M0 * c[0], M1 * c[2]                  # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> 32) ^ c[3] ^ k[1], p0 & MASK]
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


def normal_pairs(seed, stream, rows, blocks):
    """(even, odd): the two normals of every block; rows [R] (absolute row indices), blocks [B] (column pair indices) -> [R, B] each."""
    s = int(seed) & 0xFFFFFFFFFFFFFFFF                 # the two's-complement bit pattern
    rows = np.asarray(rows, dtype=np.uint64)[:, None]
    blocks = np.asarray(blocks, dtype=np.uint64)[None, :]
    shape = np.broadcast(rows, blocks).shape
    ctr = np.stack([np.broadcast_to(blocks, shape), np.broadcast_to(rows, shape), np.full(shape, int(stream) & MASK, dtype=np.uint64),
                    np.zeros(shape, dtype=np.uint64)], axis=-1)
    x = philox4x32_10(ctr, np.array([s & MASK, s >> 32], dtype=np.uint64)).astype(np.uint64)
    k1 = ((x[..., 0] >> 5) << 26) + (x[..., 1] >> 6)
    k2 = ((x[..., 2] >> 5) << 26) + (x[..., 3] >> 6)
    u1 = (k1 + 1).astype(np.float64) * 2.0 ** -53      # (0, 1], exact
    u2 = k2.astype(np.float64) * 2.0 ** -53            # [0, 1), exact
    rad = np.sqrt(-2.0 * np.log(u1))
    ang = (2.0 * np.pi) * u2
    return rad * np.cos(ang), rad * np.sin(ang)


def randn(seed, stream, first_row, rows, cols):
    """[rows, cols] float64: element (r, q) = normal(seed, stream, first_row + r, q)."""
    nb = (cols + 1) // 2
    ev, od = normal_pairs(seed, stream, np.arange(first_row, first_row + rows), np.arange(nb))
    out = np.empty((rows, 2 * nb))
    out[:, 0::2], out[:, 1::2] = ev, od
    return out[:, :cols]
