"""Crafted correlation rows for the peak-selection kernels (csrc/peaks.hip), handed to them through
``Engine.select_peaks`` without a PHAT transform in front.  A PHAT row is white noise with one spike; the rows
on which a lazily evaluated ``find_peaks(height, distance)`` can go wrong (plateaus on tile and wavefront edges,
equal heights, long suppression chains, rows without a local maximum, medians with thousands of ties) have to be
written down sample by sample.  Plain helper module like ``stages.py``: every row is deterministic and named.

``corpus(family)`` yields ``Entry(name, rows[R][n], n2, fs, num_peaks, method, mult, med)``; one entry is one call
of the engine.  ``expected(entry)`` is the oracle's answer per row, computed once and shared.

Margin condition: thresholds that are floating sums (the 'adaptive' ``mean + std`` and the fallback chain's
``mean(|corr|)``) differ from NumPy's in their last bits on the device, so a local maximum that sits ON such a
threshold would test rounding, not logic.  ``expected`` asserts for every row that no local maximum lies within
relative ``MARGIN`` of any sum-based threshold the chain evaluates for it.  That is a condition on the inputs: no
row is left out of a comparison.  The median is an order statistic, exact on both sides, and needs no margin.
"""
from __future__ import annotations

import warnings
from collections import namedtuple
from typing import Dict, Iterator, List

import numpy as np

from oracle import pal_oracle as O

Entry = namedtuple("Entry", "name rows n2 fs num_peaks method mult med")

MARGIN = 1e-9
TILE = 2048                      # samples per tile of the stream launch
FAMILIES = ("plateaus", "tile_edges", "comb", "chains", "chains_long", "no_peaks", "window_edges", "tiny", "medians",
            "offsets", "segments_300", "segments_1100", "segments_1", "mixed")
TINY_LENGTHS = (1, 2, 3, 4, 5, 9, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193)
OFFSETS = (0.0, 1.0, 1e3, 1e6)   # c / sigma of the offset rows


def _entry(name, rows, fs, num_peaks=1, method="median", mult=1.0, med=None, n2=None) -> Entry:
    rows = np.ascontiguousarray(np.atleast_2d(rows), dtype=np.float64)
    assert np.all(np.isfinite(rows))
    big = np.abs(rows[rows != 0])
    assert big.size == 0 or (big.min() >= 1e-100 and big.max() <= 1e100), name     # every sum of squares stays finite
    rows.setflags(write=False)
    return Entry(name, rows, (rows.shape[1] + 1) // 2 if n2 is None else n2, float(fs), num_peaks, method, float(mult), med)


def _floor(rng, shape, amp=1e-3):
    """low noise floor: local maxima everywhere, all far below the crafted features"""
    return amp * rng.uniform(-1.0, 1.0, shape)


def tent(n, p, lo=0.0, hi=1.0):
    """strictly rising to sample p, strictly falling behind it: exactly one local maximum (none if p is an end)"""
    return hi - (hi - lo) * np.abs(np.arange(n, dtype=np.float64) - p) / n


def staircase(n, lo=0.1, hi=1.0):
    """x[1::2] rising linearly lo -> hi, zero elsewhere: every odd sample is a peak, higher than all before it"""
    x = np.zeros(n)
    x[1::2] = np.linspace(lo, hi, x[1::2].size)
    return x


# ------------------------------------------------------------------------------------------------ families
def _plateaus() -> List[Entry]:
    n = 6145
    rng = np.random.default_rng(101)
    rows = _floor(rng, (8, n))
    # row r: a plateau of length 2 + k % 4 starting at 8 k + r (k = 0 of row 0 runs into sample 0); over the 8 rows every
    # start residue modulo the tile occurs three times.  One k of every residue class k % 256 is drawn into the high tier, so
    # that the 256 selected peaks of a row cover all 256 of its start residues; heights are distinct.
    ks = np.arange((n - 1) // 8 + 1)
    for r in range(8):
        high = rng.integers(0, 3, 256)
        order = rng.permutation(ks.size)
        for k in ks:
            s, length = 8 * k + r, 2 + k % 4
            if s + length > n:
                continue
            tier = 0.6 if (k // 256 == high[k % 256]) else 0.2
            rows[r, s:s + length] = tier + 0.3 * (order[k] + 0.5) / ks.size + 1e-4 * r
    out = [_entry("plateaus/sweep", rows, 8000.0, num_peaks=256)]

    rng = np.random.default_rng(102)
    special = []

    def base():
        x = _floor(rng, n)
        at = rng.choice(np.arange(10, n - 10, 20), 12, replace=False)
        x[at] = rng.uniform(0.3, 0.5, at.size)                     # a few strict peaks of middle height
        return x
    x = base(); x[0:3] = 0.9; special.append(x)                    # runs into sample 0: the maximum, not a peak
    x = base(); x[n - 3:n] = 0.9; special.append(x)                # runs into sample n - 1
    x = base(); x[0:2] = 0.9; x[n - 2:n] = 0.9; special.append(x)
    for b in (128, TILE, 2 * TILE):                                # wavefront edge, tile edges (= segment edges here)
        for s in range(b - 4, b + 2):
            for length in (2, 3, 4, 5):                            # floor-midpoints b - 4 .. b + 3, 2047 and 2048 among them
                x = base(); x[s:s + length] = 0.9; special.append(x)
    out.append(_entry("plateaus/special", np.array(special), 8000.0, num_peaks=4))
    return out


def _tile_edges() -> List[Entry]:
    n = 4 * TILE + 3
    rng = np.random.default_rng(111)
    rows = []
    for t in (1, 2, 3, 4):
        for off in (-2, -1, 0, 1):                                 # strict peaks at 2048 t' + off, the row's maximum at t' = t
            x = _floor(rng, n)
            for t2 in (1, 2, 3, 4):
                x[TILE * t2 + off] = 0.9 if t2 == t else 0.4 + 0.05 * t2
            rows.append(x)
    x = _floor(rng, n); x[1000] = 0.9; x[3 * TILE + 5] = 0.9; rows.append(x)      # equal maxima in different tiles: k_argmax the first
    x = _floor(rng, n); x[TILE - 1] = 0.9; x[TILE + 1] = 0.9; rows.append(x)      # ... and on either side of a tile edge
    for end in (0, n - 1):                                         # the maximum at an end: no peak, but k_argmax and the (clipped) SNR window
        x = _floor(rng, n); x[end] = 2.0; x[TILE] = 0.5; rows.append(x)
    return [_entry("tile_edges/median", np.array(rows), 8000.0, num_peaks=4),
            _entry("tile_edges/adaptive", np.array(rows), 8000.0, num_peaks=4, method="adaptive")]


def _comb() -> List[Entry]:
    n = 4501
    x = _floor(np.random.default_rng(121), n)
    x[100:4000:7] = 0.5                                            # equal heights closer than `distance`: the later position wins
    return [_entry("comb/unwindowed", x, 48000.0, num_peaks=16),
            _entry("comb/windowed", x, 48000.0, num_peaks=16, med=0.01)]


def _chains() -> List[Entry]:
    # the window around index 4096 holds low steps only: resolving a candidate there climbs the staircase in strides of 46
    # samples to its top, about 88 frames - more than the 64-frame stack
    rows = np.array([staircase(8193), staircase(8193)[::-1]])
    return [_entry("chains/n%d" % k, rows, 48000.0, num_peaks=k, med=0.001) for k in (1, 5)]


def _chains_long() -> List[Entry]:
    x = staircase(100001)                                          # about 1090 frames: past the 1024-entry memo as well
    return [_entry("chains_long/n%d" % k, x, 48000.0, num_peaks=k, med=0.001) for k in (1, 5)]


def _no_peaks() -> List[Entry]:
    n = 3001
    rng = np.random.default_rng(131)
    inc = np.cumsum(rng.uniform(0.1, 1.0, n)) * 1e-3 - 1.0         # strictly increasing through zero
    hill = -1.0 - np.abs(np.concatenate((-np.cumsum(rng.uniform(0.1, 1.0, 1200))[::-1], [0.0], np.cumsum(rng.uniform(0.1, 1.0, n - 1201))))) * 1e-3
    rows = np.array([inc, inc[::-1], np.full(n, 0.25), np.zeros(n),
                     hill,                                         # all negative, one interior maximum below every threshold
                     tent(n, 200)])                                # one peak, outside the window: branches 12 / 13
    out = []
    for method in ("median", "adaptive"):
        for med in (None, 0.01):
            for mult in (1.0, 4.0):
                out.append(_entry("no_peaks/%s_%s_x%g" % (method, "win" if med else "all", mult), rows, 8000.0, 2, method, mult, med))
    return out


def _window_edges() -> List[Entry]:
    n, fs = 1201, 8000.0
    out = []
    for n2 in (401, 601):                                          # 401: the unequal-length lag mapping
        c = n2 - 1
        for tag, med in (("0", 0.0), ("1", 1.0 / fs), ("2p5", 2.5 / fs), ("long", 1.0)):
            w = int(round(med * fs))
            rows = []
            at = sorted({c - w, c + w, c - w - 1, c + w + 1} & set(range(1, n - 1))) or [1, c, n - 2]   # (a window longer than the row)
            for p in at:
                x = tent(n, p)                                     # the only peak on the window's edge, or one sample outside it
                if n2 == 401:
                    x[0] = 2.0                                     # the maximum elsewhere: argmax fallbacks differ from the peak
                rows.append(x)
            out.append(_entry("window_edges/n2_%d_med_%s" % (n2, tag), np.array(rows), fs, 2, "median", 1.0, med, n2))
    return out


def _tiny() -> List[Entry]:
    out = []
    for n in TINY_LENGTHS:
        rows = np.random.default_rng(1000 + n).standard_normal((3, n))
        out.append(_entry("tiny/n%d_median" % n, rows, 8000.0, num_peaks=3))
        out.append(_entry("tiny/n%d_adaptive_win" % n, rows, 8000.0, num_peaks=1, method="adaptive", med=2.5 / 8000.0))
    return out


def _medians() -> List[Entry]:
    rng = np.random.default_rng(151)
    out = []
    # more than 16384 samples equal the median (0.5): the bracket list overflows; plateaus and equal heights everywhere
    q = rng.choice([0.0, 0.5, -0.5, 1.0, -1.0], 65537, p=[0.2, 0.2, 0.2, 0.2, 0.2])
    out.append(_entry("medians/quantised", q, 8000.0, num_peaks=16))
    for n in (20001, 20000):                                       # bimodal: the median sits at (odd) or between (even) the two modes
        small = n // 2 + n % 2
        mag = np.concatenate((1e-12 * rng.uniform(1, 2, small), rng.uniform(1, 2, n - small)))
        out.append(_entry("medians/bimodal_n%d" % n, rng.permutation(mag * rng.choice([-1.0, 1.0], n)), 8000.0, num_peaks=4))
    mag = np.sort(np.abs(rng.standard_normal(20000)))
    out.append(_entry("medians/sorted", mag * rng.choice([-1.0, 1.0], mag.size), 8000.0, num_peaks=4))
    for at in (100, 4000):                                         # inside / outside the pivot launch's block sample (n > 8192)
        x = 1e-100 * rng.uniform(1, 9, 9001) * rng.choice([-1.0, 1.0], 9001)
        x[at] = 1e100
        out.append(_entry("medians/giant_at%d" % at, x, 8000.0, num_peaks=4))
        out.append(_entry("medians/giant_at%d_adaptive" % at, x, 8000.0, num_peaks=4, method="adaptive"))
    return out


def offset_rows() -> np.ndarray:
    rng = np.random.default_rng(161)
    return np.array([c + rng.standard_normal(10007) for c in OFFSETS])


def _offsets() -> List[Entry]:
    rows = offset_rows()
    # 'adaptive' without c / sigma = 1e6: relative 1e-9 of that threshold is 1e-3 sigma, which thousands of local maxima cannot
    # all avoid (the margin condition); the median is exact at every offset
    return [_entry("offsets/median", rows, 8000.0, num_peaks=4),
            _entry("offsets/adaptive", rows[:3], 8000.0, num_peaks=4, method="adaptive")]


def _segments(rows, n, seed) -> List[Entry]:
    x = np.random.default_rng(seed).standard_normal((rows, n))
    return [_entry("segments_%d/n%d" % (rows, n), x, 48000.0, num_peaks=1, mult=4.0)]


def mixed_rows() -> np.ndarray:
    n = 8193
    rng = np.random.default_rng(181)
    rows = rng.standard_normal((208, n))                           # 208 rows: three segments a row, where a row sent alone has five
    rows[0] = 0.25
    rows[1] = staircase(n)
    rows[2] = staircase(n)[::-1]
    rows[3] = _floor(rng, n)
    for k in range(1, 1000):
        rows[3, 8 * k:8 * k + 2 + k % 4] = 0.2 + 0.7 * ((k * 389) % 1000) / 1000.0
    return rows


def _mixed() -> List[Entry]:
    rows = mixed_rows()
    return [_entry("mixed/windowed", rows, 48000.0, num_peaks=5, med=0.001), _entry("mixed/unwindowed", rows, 48000.0, num_peaks=5)]


_BUILD = {"plateaus": _plateaus, "tile_edges": _tile_edges, "comb": _comb, "chains": _chains, "chains_long": _chains_long,
          "no_peaks": _no_peaks, "window_edges": _window_edges, "tiny": _tiny, "medians": _medians, "offsets": _offsets,
          "segments_300": lambda: _segments(300, 6145, 171),       # two segments of two tiles
          "segments_1100": lambda: _segments(1100, 24577, 172),    # 13 tiles, the 11-tile cap: two segments
          "segments_1": lambda: _segments(1, 282625, 173),         # more single-tile segments than the finish launch stages through LDS
          "mixed": _mixed}
_ENTRIES: Dict[str, List[Entry]] = {}
_EXPECTED: Dict[str, List[dict]] = {}


def corpus(family: str = None) -> Iterator[Entry]:
    for fam in (FAMILIES if family is None else (family,)):
        if fam not in _ENTRIES:
            _ENTRIES[fam] = _BUILD[fam]()
            for e in _ENTRIES[fam]:
                expected(e)                                        # (asserts the margin condition for every row)
        yield from _ENTRIES[fam]


# ------------------------------------------------------------------------------------------------ the oracle's answers
def sum_thresholds(row, method, mult, branch) -> List[float]:
    """the thresholds made of floating sums that the fallback chain evaluates for this row"""
    thr = []
    if method == "adaptive":
        thr.append(float(O.primary_threshold(row, method, mult)))
    if branch & (O.BR_ALT_THRESHOLD | O.BR_WINDOW_RETRY):
        thr.append(float(np.mean(np.abs(row))))
    return thr


def margin(row, method, mult, branch) -> float:
    """smallest relative distance of a local maximum from a sum-based threshold of the row (inf: none to compare)"""
    h = row[O.local_maxima(row)]
    best = np.inf
    for t in sum_thresholds(row, method, mult, branch):
        if h.size:
            best = min(best, float(np.min(np.abs(h - t))) / abs(t) if t != 0 else (np.inf if np.all(h != 0) else 0.0))
    return best


def expected(e: Entry) -> List[dict]:
    """per row: O.select_peaks with the entry's num_peaks, and O.pair_record (with num_peaks = 1 the record's selection IS that
    call, so it is not run a second time: the same fields from the same functions)"""
    if e.name not in _EXPECTED:
        out = []
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")                         # np.std of an empty noise region (n = 1, 2): NaN, as the reference
            for r, row in enumerate(e.rows):
                ks, branch = O.select_peaks(row, e.n2, e.fs, e.num_peaks, e.method, e.mult, e.med)
                if e.num_peaks == 1:
                    rec = {"k_sel": int(ks[0]), "branch": int(branch), "cmax": float(np.max(row)), "cmin": float(np.min(row)),
                           "k_argmax": int(np.argmax(row)), "snr": float(O.compute_snr(row))}
                else:
                    rec = O.pair_record(row, e.n2, e.fs, e.method, e.mult, e.med)
                    assert rec["k_sel"] == int(ks[0]) and rec["branch"] == int(branch)
                m = margin(row, e.method, e.mult, branch)
                rec.update(k=np.asarray(ks, dtype=np.int64), n_sel=int(len(ks)), sel_height=float(row[rec["k_sel"]]), margin=m)
                assert m > MARGIN, "%s row %d: a local maximum within %.3g of a sum-based threshold" % (e.name, r, m)
                out.append(rec)
        _EXPECTED[e.name] = out
    return _EXPECTED[e.name]
