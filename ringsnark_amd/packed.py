"""The packed key format of include/ringsnark_amd/packed.h ("RSPK") in numpy: an exact mirror of the device kernels.

A row of n residues becomes a little-endian bit stream of w bits a residue -- residue p in bits [p w, (p + 1) w), bit b in
word b >> 6 at position b & 63 -- in 2 ceil(n w / 128) 64-bit words; the padding bits are zero."""
import numpy as np


def pack_bits(prm):
    """w: the widest data prime of the parameter set, in bits"""
    w = max(int(Q).bit_length() for Q in prm.Q)
    if not 2 <= w <= 62:
        raise ValueError("data prime out of range")
    return w


def words_per_row(n, w):
    return 2 * ((n * w + 127) // 128)


def row_words(prm):
    return words_per_row(prm.N_enc, pack_bits(prm))


_CHUNK = 16  # rows expanded to bits at a time (a row of 16384 residues at w = 49 is 6 MiB of bit words)


def _by_rows(a, width, f):
    flat = a.reshape(-1, a.shape[-1])
    out = np.empty((flat.shape[0], width), dtype=np.uint64)
    for r in range(0, flat.shape[0], _CHUNK):
        out[r:r + _CHUNK] = f(flat[r:r + _CHUNK])
    return out.reshape(a.shape[:-1] + (width,))


def pack_rows(words, w):
    """[..., n] residues -> [..., row_words] packed words (uint64); the low w bits of every residue are stored."""
    a = np.ascontiguousarray(words).astype(np.uint64, copy=False)
    n = a.shape[-1]
    rw = words_per_row(n, w)

    def pack(rows):
        bits = (rows[:, :, None] >> np.arange(w, dtype=np.uint64)) & np.uint64(1)  # [rows, n, w], bit 0 first
        stream = np.zeros((rows.shape[0], rw * 64), dtype=np.uint64)
        stream[:, :n * w] = bits.reshape(rows.shape[0], n * w)
        return np.bitwise_or.reduce(stream.reshape(rows.shape[0], rw, 64) << np.arange(64, dtype=np.uint64), axis=-1)

    return _by_rows(a, rw, pack)


def unpack_rows(packed, w, n):
    """[..., row_words] packed words -> [..., n] residues (uint64)"""
    a = np.ascontiguousarray(packed).astype(np.uint64, copy=False)
    assert a.shape[-1] == words_per_row(n, w), (a.shape, n, w)

    def unpack(rows):
        bits = (rows[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)  # [rows, row_words, 64]
        bits = bits.reshape(rows.shape[0], -1)[:, :n * w].reshape(rows.shape[0], n, w)
        return np.bitwise_or.reduce(bits << np.arange(w, dtype=np.uint64), axis=-1)

    return _by_rows(a, n, unpack)
