"""Counter-based shuffles of the bootstrap significance test (utils.py:183-216), restated in NumPy.

The reference draws every shuffle from NumPy's global RNG, one after the other.  The device path
(``Engine.bootstrap_peaks``, csrc/bootstrap.hip) instead makes shuffle ``s`` of pair ``(i, j)`` a pure
function of ``(seed, i, j, s, L, mode, block_size)``: keyed on the row indices, so a sub-list of the
pairs, another round size or a rank's block of the pair list draws exactly the same shuffles.  Only
exact 64-bit integer arithmetic is used; this module is the specification the HIP kernel reproduces
bit for bit, and the reference the tests compare against.

Row ``j`` (``sig2``) is shuffled, row ``i`` stays fixed; ``row[shuffle_indices(...)]`` is the shuffled row.

- key: splitmix64 finaliser chained over (seed, i, j, s);
- permutation: a balanced Feistel network of ``ROUNDS`` rounds over the smallest power of two with an
  even number of bits that holds ``L``, cycle-walked back into ``[0, L)``; the round function is the
  finaliser of (key, round, half);
- block: the same bijection over the ``ceil(L / block_size)`` blocks gives the block order; the short
  last block keeps its length wherever it lands (``np.concatenate(blocks)[:len(sig2)]``);
- circular: ``np.roll(row, shift)`` with ``shift`` = finaliser of (key, round 255) mod ``L``.
"""
from __future__ import annotations

import numpy as np

MODES = {"permutation": 0, "block": 1, "circular": 2}     # PAL_BOOT_PERMUTATION / _BLOCK / _CIRCULAR
ROUNDS = 8
GOLDEN = 0x9E3779B97F4A7C15
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)
_MASK64 = (1 << 64) - 1
_SHIFT_ROUND = 255                                        # the circular shift's "round" of the round function


def mode_code(mode) -> int:
    """'permutation' | 'block' | 'circular' (or their codes 0 | 1 | 2) -> code; ValueError otherwise."""
    if isinstance(mode, str) and mode in MODES:
        return MODES[mode]
    if isinstance(mode, (int, np.integer)) and not isinstance(mode, bool) and int(mode) in MODES.values():
        return int(mode)
    raise ValueError(f"unknown bootstrap_mode {mode!r}; use 'permutation', 'block' or 'circular'")


def check_args(mode, block_size: int, num_bootstrap: int = 1) -> int:
    """Argument checks shared by every entry point of the device bootstrap -> mode code."""
    code = mode_code(mode)
    if int(block_size) < 1:
        raise ValueError(f"block_size must be at least 1 (got {block_size})")
    if int(num_bootstrap) < 1:
        raise ValueError(f"num_bootstrap must be at least 1 (got {num_bootstrap})")
    return code


def mix64(z):
    """splitmix64 finaliser on uint64 (arrays wrap modulo 2^64)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        return z ^ (z >> np.uint64(31))


def shuffle_key(seed: int, i: int, j: int, s: int) -> np.uint64:
    """Key of shuffle s of pair (i, j): mix(mix(mix(mix(seed + GOLDEN) ^ i) ^ j) ^ s)."""
    k = mix64(np.uint64((int(seed) + GOLDEN) & _MASK64))
    for v in (i, j, s):
        k = mix64(k ^ np.uint64(int(v) & _MASK64))
    return np.uint64(k)


def _half_bits(n: int) -> int:
    h = 1
    while (1 << (2 * h)) < n:
        h += 1
    return h


def _feistel(x: np.ndarray, key: np.uint64, h: int) -> np.ndarray:
    mask = np.uint64((1 << h) - 1)
    left, right = x >> np.uint64(h), x & mask
    for r in range(ROUNDS):
        f = mix64(key ^ (right + np.uint64(r << 32))) & mask
        left, right = right, left ^ f
    return (left << np.uint64(h)) | right


def bijection(x, key: np.uint64, n: int) -> np.ndarray:
    """Keyed bijection of [0, n): the Feistel network over 4^h >= n points, cycle-walked back into [0, n)."""
    h = _half_bits(n)
    out = _feistel(np.asarray(x, dtype=np.uint64), key, h)
    walk = out >= np.uint64(n)
    while walk.any():
        out[walk] = _feistel(out[walk], key, h)
        walk = out >= np.uint64(n)
    return out.astype(np.int64)


def circular_shift(key: np.uint64, length: int) -> int:
    return int(mix64(key ^ np.uint64(_SHIFT_ROUND << 32)) % np.uint64(length))


def shuffle_indices(L: int, i: int, j: int, s: int, mode="permutation", block_size: int = 50, seed: int = 0) -> np.ndarray:
    """Source index of every output sample of shuffle s of pair (i, j): int64[L], a permutation of 0..L-1."""
    code = check_args(mode, block_size)
    L = int(L)
    if L < 1:
        raise ValueError("L must be at least 1")
    if min(int(i), int(j), int(s)) < 0:
        raise ValueError("row indices and the shuffle index must be non-negative")
    key = shuffle_key(seed, i, j, s)
    if code == 0:
        return bijection(np.arange(L), key, L)
    if code == 1:
        bs = int(block_size)
        nb = -(-L // bs)
        starts = bijection(np.arange(nb), key, nb) * bs          # source block of every output block position
        lens = np.minimum(bs, L - starts)
        first = np.cumsum(lens) - lens                            # where each block lands in the output
        return np.repeat(starts - first, lens) + np.arange(L)
    return (np.arange(L) - circular_shift(key, L)) % L
