"""Shapes and shared inputs of the bootstrap's edge tests: the case grid that ``tests/test_host_bootstrap_map.py`` runs through
``csrc/bootstrap_map.h`` on the host, and the lengths, block sizes, keys and frames at which ``tests/test_gpu_bootstrap_edges.py``
(and ``tests/test_gpu_bootstrap.py``) run ``k_bootstrap_shuffle`` and the rounds of ``bootstrap_peaks_dev``.  Inputs and the oracle
only, no GPU; plain helper module like ``peak_positions.py`` and ``second_path.py``.

The reference everywhere is ``pyaudiolocalization_amd/bootstrap.py`` (the specification of the shuffles) with the oracle's PHAT
(``oracle/pal_oracle.py``).
"""
from __future__ import annotations

from typing import Iterator, List, Tuple

import numpy as np

from oracle import pal_oracle as O
from pyaudiolocalization_amd import bootstrap as B
from pyaudiolocalization_amd import synthetic

MODES = ("permutation", "block", "circular")
TOL = dict(rtol=1e-10, atol=1e-13)            # the smoke test's tolerance on cmax: engine against the oracle
CLOSE = dict(rtol=1e-11, atol=1e-15)          # two engine paths whose rows sit beside different partners in a complex transform


def frame(mics: int, L: int) -> np.ndarray:
    return synthetic.metric_frames(1, mics, L)[0]


def oracle_peak(fixed: np.ndarray, row: np.ndarray, i: int, j: int, s: int, mode, block_size: int, seed: int) -> float:
    perm = B.shuffle_indices(row.shape[0], i, j, s, mode, block_size, seed)
    return float(np.max(O.phat_correlation(fixed, row[perm])))


def oracle_peaks(rows, pairs, S, mode, block_size, seed, shuffles=None) -> np.ndarray:
    """peaks[p][k] of shuffle shuffles[k] (default 0 .. S-1) of every pair of the list, by the specification and the oracle's PHAT"""
    shuffles = range(S) if shuffles is None else shuffles
    out = np.empty((len(pairs), len(shuffles)))
    for p, (i, j) in enumerate(pairs):
        for k, s in enumerate(shuffles):
            out[p, k] = oracle_peak(rows[i], rows[j], int(i), int(j), int(s), mode, block_size, seed)
    return out


# ---- the specification's cases for the host build of ShuffleMap -------------------------------------------------------------
# lengths on either side of 4^h (with and without cycle walking), and one that is no neighbour of a power of four
MAP_LENGTHS = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 2026)
MAP_LIMIT = 1 << 20                                            # the ABI's longest frame (h = 10)
KEYS = ((0, 1, 0, 0),                                          # (i, j, s, seed)
        (4, 9, 1000, 2**63 + 12345),
        (2**31 - 1, 0, 2**62, 1),
        (255, 254, 2**40 + 7, 2**64 - 1))
WIDE_KEYS = KEYS[2:]                                           # counters beyond 32 bits: sign extension into the key


def map_block_sizes(L: int) -> List[int]:
    """one block, a full 'short' block, single samples, a last block of one sample, ordinary sizes, the largest int32"""
    sizes = (1, 2, 3, L - 1, L, L + 1, -(-L // 2), L // 4, 16, 47, 2**31 - 1)
    return sorted({v for v in sizes if v >= 1})


def map_cases() -> Iterator[Tuple[int, int, int, int, str, int, int]]:
    """(L, i, j, s, mode, block_size, seed) of every case of the host test"""
    for L in MAP_LENGTHS:
        for i, j, s, seed in KEYS:
            yield L, i, j, s, "permutation", 50, seed
            yield L, i, j, s, "circular", 50, seed
            for bs in map_block_sizes(L):
                yield L, i, j, s, "block", bs, seed
    i, j, s, seed = KEYS[1]
    yield MAP_LIMIT, i, j, s, "permutation", 50, seed
    yield MAP_LIMIT, i, j, s, "circular", 50, seed
    for bs in (1, 50, MAP_LIMIT):
        yield MAP_LIMIT, i, j, s, "block", bs, seed


def fnv1a64(indices: np.ndarray) -> int:
    """64-bit FNV-1a hash of the indices as little-endian 32-bit words"""
    h = 0xCBF29CE484222325
    for byte in np.asarray(indices).astype("<u4").tobytes():
        h = ((h ^ byte) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


# ---- the shuffle kernel on the device -----------------------------------------------------------------------------------------
SHUFFLE_KEY = (4, 9, 7)                                        # (i, j, seed) of the tiling and block-size cases
# one workgroup writes 1024 samples (256 lanes x 4): a lone sample, one lane's worth, one pass of the lanes and its neighbours, one
# workgroup and its neighbours, two whole workgroups, four and one sample
TILING_LENGTHS = (1, 2, 255, 256, 257, 1023, 1024, 1025, 2048, 4097)
ROWS_PER_LAUNCH = 65536                                        # kMaxRows of bootstrap_shuffle_dev


def device_block_sizes(L: int) -> List[int]:
    """single samples, a last block of one sample, one block (exactly, and with room), the largest int32, a divisor of L (the 'short'
    block is full), and 47 (divides none of the lengths)"""
    divisor = {37: 37, 1000: 50, 1025: 41}[L]
    return sorted({1, L - 1, L, L + 1, 2**31 - 1, divisor, 47})


BLOCK_LENGTHS = (37, 1000, 1025)
# Found on the CPU with the specification alone (tests/test_host_bootstrap_map.py asserts it again): of the shuffles of L = 1000 in
# blocks of 50 under SHUFFLE_KEY, 15 is the first that puts the last source block first in the output and 27 the first that puts it
# last (shuffles 0 .. 19 hold no such one), hence 28 shuffles.
BLOCK_SHUFFLES = 28
SHORT_BLOCK_FIRST = 15
SHORT_BLOCK_LAST = 27


def short_block_position(L: int, s: int, block_size: int) -> int:
    """where the last source block starts in the output of shuffle s under SHUFFLE_KEY (specification only)"""
    i, j, seed = SHUFFLE_KEY
    idx = B.shuffle_indices(L, i, j, s, "block", block_size, seed)
    return int(np.nonzero(idx == (-(-L // block_size) - 1) * block_size)[0][0])


# ---- the rounds of bootstrap_peaks_dev ------------------------------------------------------------------------------------------
# (L, n1, n2, tile_len) as Engine.plan_info reports them: a one-tile prime-factor plan, Rader rows, no cut (four-step), 9 x 455
ROUTES = ((50, 1, 99, 512), (496, 1, 991, 990), (1000, 0, 0, 0), (2048, 9, 455, 1024))
BOUNDARY_SHUFFLES = (0, 1, 1918, 1919, 1920, 1921, 1999)       # L = 600: rounds of 1920 rows at the default group size
LONG_L = 136688                                                # n = 273 375 = 3^7 5^3: a round below one launch group
LONG_S = 700
LONG_ORACLE_SHUFFLES = tuple(range(0, LONG_S - 1, 29)) + (LONG_S - 1,)
PAIR_FORMS = ((1, 1), (2, 1), (1, 2), (1, 2), (3, 0))
