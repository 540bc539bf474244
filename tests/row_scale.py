"""Inputs for the row-scale tests: rows of very different amplitude that share one packed complex transform.

Several kernels put two independent real rows into one complex transform (real part / imaginary part): the forward
spectra of the Rader plans (csrc/pfa_forward.h), the cross-correlation rows of ``xcorr_vs_ref`` / ``sync_measure_dev``
and the inverse of ``fractional_delay`` / ``simulate_multipath`` (csrc/sim.hip), and the PHAT inverse (two whitened
pairs).  The reference transforms every row on its own, so a row's result does not depend on any other row and its error
is relative to that row's own scale.  These builders scale ONE row by ``2.0 ** e`` (exact in NumPy) and move it through
every position of the packing.  Plain helper module like ``second_path.py``: seeded, deterministic, no engine import.

Frames are the "delayed" family of tests/test_gpu_parity.py: one common ``standard_normal`` base, every microphone a
copy at an integer offset in 0 .. 63 plus 0.3 x its own noise, so every pair has one clear peak.

The oracle side is computed once per (shape, frame, pair, exponents) and shared: a pair that does not contain the scaled
microphone has the same inputs as in the unscaled frame, hence the same oracle row and record (test_host_row_scale.py
pins that bit for bit), and is taken from the cache.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

from oracle import pal_oracle as O

EXPS = (-40, -20, 20, 40)
MARGIN = 1e-9                                    # peak margins below are conditions on the inputs, not tolerances

# name -> (B, M, L, fs): 0.01 s is 160 (441) samples at 16 kHz (44.1 kHz), wider than the 0 .. 63 offsets
PHAT_SHAPES: Dict[str, Tuple[int, int, int, float]] = {
    "rader496": (2, 5, 496, 16000.0),            # n = 991: Rader forward, one row tile
    "head44100": (1, 5, 44100, 44100.0),         # n = 89 x 991: the headline route with the finishing column pass
    "four1000": (2, 5, 1000, 16000.0),           # n = 1999 (prime): four-step on both sides, one frame per forward transform
    "pfa2048": (2, 5, 2048, 16000.0),            # n = 9 x 455: four-step forward, prime-factor inverse
}
PHAT_SEEDS = {"rader496": 0, "head44100": 0, "four1000": 0, "pfa2048": 0}
MEDS = (0.01, None)
METHODS = ("median", "adaptive")


def delayed(seed, rows: int, n: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    base = rng.standard_normal(n + 64)
    out = np.stack([base[d:d + n] for d in rng.integers(0, 64, rows)]) + 0.3 * rng.standard_normal((rows, n))
    return np.ascontiguousarray(out)


_FRAMES: Dict[str, np.ndarray] = {}


def phat_frames(name: str) -> np.ndarray:
    if name not in _FRAMES:
        b, m, length, _ = PHAT_SHAPES[name]
        fr = delayed([3000, PHAT_SEEDS[name], length], b * m, length).reshape(b, m, length)
        fr.setflags(write=False)
        _FRAMES[name] = fr
    return _FRAMES[name]


def phat_positions(name: str) -> List[Tuple[str, int, int]]:
    """(tag, frames used, scaled microphone of frame 0).  Row r = b M + m of the flattened list rides the transform r // 2:
    'even' / 'odd' are microphones 2 and 1; 'edge' is the last microphone of frame 0, whose partner is microphone 0 of
    frame 1 (M odd; needs two frames); 'half' is the last row of an odd row count (frame 0 alone), in a half-empty transform."""
    b, m, _, _ = PHAT_SHAPES[name]
    assert m % 2 == 1
    pos = [("even", b, 2), ("odd", b, 1)]
    if b >= 2:
        pos.append(("edge", b, m - 1))
    pos.append(("half", 1, m - 1))
    return pos


def scaled_frames(name: str, nframes: int, mic: int, e: int) -> np.ndarray:
    fr = np.array(phat_frames(name)[:nframes])
    fr[0, mic] *= 2.0 ** e
    return fr


def pairs_of(m: int) -> List[Tuple[int, int]]:
    return [(i, j) for i in range(m) for j in range(i + 1, m)]


def pairs_with(m: int, mic: int) -> List[int]:
    return [p for p, (i, j) in enumerate(pairs_of(m)) if mic in (i, j)]


_CORR: Dict[tuple, np.ndarray] = {}
_REC: Dict[tuple, dict] = {}
_MARGIN: Dict[tuple, float] = {}


def oracle_corr(name: str, b: int, i: int, j: int, ei: int = 0, ej: int = 0) -> np.ndarray:
    """O.phat_correlation of microphones i, j of frame b scaled by 2^ei, 2^ej"""
    key = (name, b, i, j, ei, ej)
    if key not in _CORR:
        fr = phat_frames(name)
        c = O.phat_correlation(fr[b, i] * 2.0 ** ei, fr[b, j] * 2.0 ** ej)
        c.setflags(write=False)
        _CORR[key] = c
    return _CORR[key]


def oracle_record(name: str, b: int, i: int, j: int, ei: int, ej: int, med, method: str) -> dict:
    key = (name, b, i, j, ei, ej, med, method)
    if key not in _REC:
        _, _, length, fs = PHAT_SHAPES[name]
        _REC[key] = O.pair_record(oracle_corr(name, b, i, j, ei, ej), length, fs, method, 1.0, med)
    return _REC[key]


def oracle_table(name: str, b: int, exps: Dict[int, int], med, method: str) -> Dict[str, np.ndarray]:
    """the table O.all_pairs gives for frame b with microphone q scaled by 2^exps[q]"""
    m = PHAT_SHAPES[name][1]
    recs = [oracle_record(name, b, i, j, exps.get(i, 0), exps.get(j, 0), med, method) for i, j in pairs_of(m)]
    out = {}
    for key in ("k_sel", "branch", "k_argmax"):
        out[key] = np.array([r[key] for r in recs], dtype=np.int32)
    for key in ("cmax", "cmin", "snr"):
        out[key] = np.array([r[key] for r in recs], dtype=np.float64)
    return out


def row_margin(corr: np.ndarray, length: int, fs: float, med, method: str) -> float:
    """height of the oracle's selected peak of `corr` above the runner-up of O.select_peaks (inf: a single candidate); where
    the oracle falls back to the argmax, the largest sample above the second largest"""
    ks, branch = O.select_peaks(corr, length, fs, 2, method, 1.0, med)
    top = np.sort(corr)[-2:]
    if branch & (O.BR_ARGMAX_NO_PEAKS | O.BR_ARGMAX_WINDOW):
        margin = float(top[1] - top[0])
    else:
        margin = float("inf") if ks.size < 2 else float(corr[ks[0]] - corr[ks[1]])
    return min(margin, float(top[1] - top[0]))                      # (k_argmax is compared exactly as well)


def peak_margin(name: str, b: int, i: int, j: int, ei: int, ej: int, med, method: str) -> float:
    """row_margin() of the oracle row of microphones i, j of frame b scaled by 2^ei, 2^ej"""
    key = (name, b, i, j, ei, ej, med, method)
    if key not in _MARGIN:
        _, _, length, fs = PHAT_SHAPES[name]
        _MARGIN[key] = row_margin(oracle_corr(name, b, i, j, ei, ej), length, fs, med, method)
    return _MARGIN[key]


# ------------------------------------------------------------------------------------------------ quiet pairs
# Two microphones of a frame scaled by 2^QUIET_EXP each: their cross spectrum |R| ~ 4^e L comes near (and below) the 1e-10
# of the whitening, so that pair's whitened row is much smaller than the row packed beside it in the PHAT inverse.  The
# oracle's selected peak must still lead by MARGIN (absolute).  At 2^-40 it cannot: |R| ~ 1e-21, the whole row is below
# 1e-10.  QUIET_EXP[shape] is the largest negative exponent of -40, -38, ... at which it does (found with
# quiet_exponent_search(), pinned by test_host_row_scale.py): margins 1.3e-9 at L = 496 and 5.7e-9 at L = 44 100.
QUIET_MICS = (1, 3)
QUIET_EXP = {"rader496": -32, "head44100": -38}
QUIET_SHAPES = tuple(QUIET_EXP)


def quiet_margin(name: str, e: int) -> float:
    i, j = QUIET_MICS
    return min(peak_margin(name, 0, i, j, e, e, med, method) for med in MEDS for method in METHODS)


def quiet_exponent_search(name: str) -> int:
    for e in range(-40, 0, 2):
        if quiet_margin(name, e) > MARGIN:
            return e
    raise AssertionError("no exponent holds the margin")


# ------------------------------------------------------------------------------------------------ xcorr / sync
XCORR_N = 700
XCORR_R = (5, 7)


def xcorr_rows(r: int) -> np.ndarray:
    rows = delayed([3100, r], r, XCORR_N)
    rows.setflags(write=False)
    return rows


def xcorr_refs(r: int) -> Tuple[int, ...]:
    return tuple(sorted({0, r // 2, r - 1}))


def xcorr_positions(r: int, ref: int) -> Tuple[int, ...]:
    """the scaled row: an odd index, an even index, the last row (R is odd: a half-empty transform) and the reference row"""
    return tuple(sorted({1, 2, r - 1, ref}))


def xcorr_exact(rows: np.ndarray, ref: int) -> List[np.ndarray]:
    return [O.xcorr_full(row, rows[ref]) for row in rows]


def xcorr_margin(seq: np.ndarray) -> float:
    """lead of the largest |value| over the runner-up, relative to the peak"""
    mag = np.sort(np.abs(seq))
    return float((mag[-1] - mag[-2]) / mag[-1])


SYNC_B, SYNC_M = 3, 5
SYNC_LOUD = (0, 2, 4)                            # the row of frame f that is three times louder (the unscaled reference)
SYNC_SCALED = ((1, 1), (1, 4))                   # (frame, microphone) scaled in turn: an odd row, and the half-empty transform


def sync_frames() -> np.ndarray:
    fr = delayed([3200], SYNC_B * SYNC_M, XCORR_N).reshape(SYNC_B, SYNC_M, XCORR_N)
    for f, q in enumerate(SYNC_LOUD):
        fr[f, q] *= 3.0
    fr.setflags(write=False)
    return fr


def numpy_ref(frame: np.ndarray) -> int:
    return int(np.argmax([np.sum(row ** 2) for row in frame]))


# ------------------------------------------------------------------------------------------------ fractional_delay
FD_R, FD_N, FD_FS = 5, 1501, 8000.0
FD_DELAYS = np.array([0.0, 1.0, 7.0, 0.37, 12.5]) / FD_FS          # FD_DELAYS of test_gpu_second_path.py
FD_POSITIONS = (1, 2, 4)                         # an odd row, an even row, the last row (half-empty transform)


def fd_rows() -> np.ndarray:
    rows = np.random.default_rng([3300]).standard_normal((FD_R, FD_N))
    rows.setflags(write=False)
    return rows


# ------------------------------------------------------------------------------------------------ simulate_multipath
SIM_B, SIM_M, SIM_K, SIM_NBASE, SIM_TOTAL, SIM_FS = 3, 5, 4, 1500, 1700, 8000.0
SIM_EXPS = (-40, -20, 20, 40)


def sim_tables():
    """base[B][nbase], delays / gains[B][M][K].  Flattened rows (b, m): M is odd, so (0, 4) rides with (1, 0) and (1, 4) with
    (2, 0); the last row (2, 4) sits in a half-empty transform.  Scaling base b scales the five rows of frame b."""
    rng = np.random.default_rng([3400])
    base = rng.standard_normal((SIM_B, SIM_NBASE))
    delays = rng.uniform(0.0, 0.02, (SIM_B, SIM_M, SIM_K))
    gains = rng.choice([-1.0, 1.0], (SIM_B, SIM_M, SIM_K)) * 10.0 ** rng.uniform(-3.0, 0.0, (SIM_B, SIM_M, SIM_K))
    for a in (base, delays, gains):
        a.setflags(write=False)
    return base, delays, gains


_SIM_WANT: Dict[int, np.ndarray] = {}


def sim_want(f: int) -> np.ndarray:
    """O.simulate_from_base of frame f with the unscaled base (the oracle normalises: a scaled base gives the same bits)"""
    if f not in _SIM_WANT:
        base, delays, gains = sim_tables()
        _SIM_WANT[f] = O.simulate_from_base(base[f], delays[f], gains[f], SIM_FS, SIM_TOTAL, None)
        _SIM_WANT[f].setflags(write=False)
    return _SIM_WANT[f]
