"""A host restatement of the keyed row permutation of csrc/bsx_shuffle.hip (include/battlespace_hip.h: bsx_shuffle_rows), in numpy on
tests/philox_util.philox4x32_10: a balanced Feistel network over the domain 2^(2b) with cycle walking, eight round keys from two Philox
blocks keyed by (seed, seq).  Integer arithmetic only, so the GPU tests compare the kernels with it exactly.

  perm_at(N, seed, seq, positions)   the source rows of the given positions: vectorised over positions only (N = 2^31 - 1 is cheap)
  perm(N, seed, seq)                 the whole permutation, int64 [N]
  evaluations(N, seed, seq, positions)  how many times the network ran per position (the length of the cycle walk)

Nothing here imports the native library."""
import numpy as np

import philox_util as P

SHUFFLE_SALT = 0x5AFF1E00
ROUNDS = 8
U32 = np.uint64(0xFFFFFFFF)


def half_bits(N):
    """b of the domain 2^(2b): bits = max(2, bit_length(N - 1)), b = (bits + 1) // 2."""
    return (max(2, int(N - 1).bit_length()) + 1) // 2


def round_keys(seed, seq):
    """The eight round keys: words x y z w of the blocks of counter (j, 0, seq_lo, seq_hi), j = 0, 1, key (seed_lo, seed_hi ^ salt)."""
    seed, seq = int(seed), int(seq) & ((1 << 64) - 1)
    keys = []
    for j in range(ROUNDS // 4):
        w = P.philox4x32_10(j, 0, seq & 0xFFFFFFFF, seq >> 32, seed & 0xFFFFFFFF, (seed >> 32) ^ SHUFFLE_SALT)
        keys += [int(x) for x in w]
    return keys


def _network(x, b, keys):
    """One pass of the eight rounds over uint64 arrays holding uint32 values."""
    mask, sh = np.uint64((1 << b) - 1), np.uint64(b)
    L, R = x >> sh, x & mask
    for k in keys:
        h = ((R ^ np.uint64(k)) * np.uint64(0x9E3779B1)) & U32
        h ^= h >> np.uint64(15)
        h = (h * np.uint64(0x85EBCA77)) & U32
        h ^= h >> np.uint64(13)
        L, R = R, (L ^ (h >> np.uint64(32 - b))) & mask
    return (L << sh) | R


def _walk(N, seed, seq, positions):
    N = int(N)
    assert 1 <= N < 1 << 31
    x = np.array(positions, dtype=np.uint64).ravel()
    assert x.size == 0 or int(x.max()) < N
    b, keys = half_bits(N), round_keys(seed, seq)
    count = np.zeros(x.shape, dtype=np.int64)
    todo = np.arange(x.size)
    while todo.size:
        x[todo] = _network(x[todo], b, keys)
        count[todo] += 1
        todo = todo[x[todo] >= np.uint64(N)]
    return x.astype(np.int64), count


def perm_at(N, seed, seq, positions):
    """int64 array, shaped like `positions`: perm(N, seed, seq)[positions]."""
    return _walk(N, seed, seq, positions)[0].reshape(np.shape(positions))


def evaluations(N, seed, seq, positions):
    return _walk(N, seed, seq, positions)[1].reshape(np.shape(positions))


def perm(N, seed, seq):
    return perm_at(N, seed, seq, np.arange(int(N), dtype=np.uint64))
