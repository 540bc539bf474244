"""Inputs for the Rader-row family tests: every frame length L with 2 L - 1 = N1 x 991 plans onto the Rader row pass
(csrc/pfa_rader.h) and takes its forward spectra through the transposed cut (csrc/pfa_forward.h).  N2 = 991 is fixed by the
kernel, so a case is an N1, and each N1 below is the smallest member of its class: the edges of the forward column kernel's
unroll (h = (N1 - 1) / 2 below, at and above 4), of its chunks of eleven output indices (one full chunk, one index in the
next, a second block row in the grid) and of the three column passes behind the rows (strips for one chunk, the finishing
pass with two / three / four wavefronts for two to four chunks, the plain column kernel for five and six).
Plain helper module like ``row_scale.py``: seeded, deterministic, no engine import.  The oracle side is computed once per
(case, shape, frame, pair, exponent) and shared between the host test and the device test.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np

from oracle import pal_oracle as O

import row_scale as RS

N2 = 991
FS = 44100.0                                     # 0.01 s is 441 samples, wider than the 0 .. 63 offsets of RS.delayed
COL_CHUNK = 11                                   # plan_geometry.h kColChunk

# N1 -> what it is the edge of
CASES: Dict[int, str] = {
    3: "h = 1 < unroll; the smallest real two-row plan",
    9: "h = 4 = unroll; composite N1",
    11: "h = 5 = unroll + 1",
    23: "h = 11: one full chunk; the last plan on the strips / fused pass",
    25: "two chunks, one index in the second; first plan on the finishing pass, two wavefronts, not full",
    45: "two full chunks",
    47: "three chunks, one index in the third; three-wavefront body",
    67: "three full chunks",
    69: "four chunks, dense four-wavefront body without Rader-89",
    87: "h = 43: one short of full, the neighbour of 89",
    91: "five chunks: a second block row with one live wavefront; a padded length",
    97: "prime N1, five chunks; a padded length",
    113: "six chunks, one index in the sixth",
    127: "the largest N1, h = 63",
}
N1S = tuple(CASES)
WIDE = (3, 9, 25)                                # these also get B = 2, M = 5: ten pairs per frame, the odd / even edge between frames
AMPLITUDE = (3, 25, 91, 127)                     # the amplitude-sensitive variant
UNEQUAL = (3, 25)                                # unequal lengths through phat_correlation
BODIES = (3, 91)                                 # both first-stage bodies of the inverse row pass
SILENT = (1, 0)                                  # (frame, microphone) of the wide frames that is silent
# shape tag -> (B, M).  B = 1, M = 3: three frames are one packed forward transform plus a half-empty one, three pairs one
# shared-microphone inverse transform plus a half-empty one
SHAPES: Dict[str, Tuple[int, int]] = {"narrow": (1, 3), "wide": (2, 5)}
SHAPE_CASES: List[Tuple[int, str]] = [(n1, "narrow") for n1 in N1S] + [(n1, "wide") for n1 in WIDE]
SEEDS: Dict[Tuple[int, str], int] = {c: 0 for c in SHAPE_CASES}    # a seed that fails a peak margin is replaced here
MEDS = RS.MEDS
METHODS = RS.METHODS


def length_of(n1: int) -> int:
    return (N2 * n1 + 1) // 2


def half(n1: int) -> int:
    return (n1 - 1) // 2


def chunks(n1: int) -> int:
    return (half(n1) + COL_CHUNK - 1) // COL_CHUNK


def column_kernel(n1: int) -> str:
    """profile name of the column pass behind the Rader rows in a call that wants records only (csrc/pair_route.h: four
    column blocks of strips stay on the fused pass, sixteen blocks take the finishing pass, more than four chunks neither)"""
    return "k_pfa_cols_stats" if chunks(n1) <= 1 else "k_pfa_cols_fin" if chunks(n1) <= 4 else "k_pfa_cols"


_FRAMES: Dict[tuple, np.ndarray] = {}


def frames(n1: int, shape: str) -> np.ndarray:
    """[B][M][L], read-only.  The wide frames have SILENT zeroed: its pairs' rows are exact zeros in the reference."""
    key = (n1, shape)
    if key not in _FRAMES:
        b, m = SHAPES[shape]
        length = length_of(n1)
        fr = RS.delayed([3500 + SEEDS[key], n1], b * m, length).reshape(b, m, length)
        if shape == "wide":
            fr[SILENT] = 0.0
        fr.setflags(write=False)
        _FRAMES[key] = fr
    return _FRAMES[key]


def silent_pair(shape: str, b: int, i: int, j: int) -> bool:
    return shape == "wide" and b == SILENT[0] and SILENT[1] in (i, j)


def amplitude_exponent(n1: int) -> int:
    """2^e on every microphone puts |S_a conj S_b| ~ 4^e L beside the 1e-10 of the whitening: -22 ... -25 over the cases"""
    return int(round(0.5 * np.log2(1e-10 / length_of(n1))))


def five_microphones(n1: int) -> np.ndarray:
    """[5][L] for the comparison of the two first-stage bodies (no oracle involved: the two engines must agree bit for bit)"""
    return RS.delayed([3600, n1], 5, length_of(n1))


_CORR: Dict[tuple, np.ndarray] = {}
_REC: Dict[tuple, dict] = {}
_MARGIN: Dict[tuple, float] = {}


def oracle_corr(n1: int, shape: str, b: int, i: int, j: int, e: int = 0) -> np.ndarray:
    """O.phat_correlation of microphones i, j of frame b, both scaled by 2^e"""
    key = (n1, shape, b, i, j, e)
    if key not in _CORR:
        fr = frames(n1, shape)
        c = O.phat_correlation(fr[b, i] * 2.0 ** e, fr[b, j] * 2.0 ** e)
        c.setflags(write=False)
        _CORR[key] = c
    return _CORR[key]


def oracle_record(n1: int, shape: str, b: int, i: int, j: int, med, method: str) -> dict:
    key = (n1, shape, b, i, j, med, method)
    if key not in _REC:
        _REC[key] = O.pair_record(oracle_corr(n1, shape, b, i, j), length_of(n1), FS, method, 1.0, med)
    return _REC[key]


def oracle_table(n1: int, shape: str, b: int, med, method: str) -> Dict[str, np.ndarray]:
    """the table O.all_pairs gives for frame b"""
    recs = [oracle_record(n1, shape, b, i, j, med, method) for i, j in RS.pairs_of(SHAPES[shape][1])]
    out = {}
    for key in ("k_sel", "branch", "k_argmax"):
        out[key] = np.array([r[key] for r in recs], dtype=np.int32)
    for key in ("cmax", "cmin", "snr"):
        out[key] = np.array([r[key] for r in recs], dtype=np.float64)
    return out


def peak_margin(n1: int, shape: str, b: int, i: int, j: int, med, method: str, e: int = 0) -> float:
    key = (n1, shape, b, i, j, med, method, e)
    if key not in _MARGIN:
        _MARGIN[key] = RS.row_margin(oracle_corr(n1, shape, b, i, j, e), length_of(n1), FS, med, method)
    return _MARGIN[key]


# ------------------------------------------------------------------------------------------------ unequal lengths
def unequal_cases(n1: int) -> List[Tuple[str, int, int, object]]:
    """(tag, len1, len2, launches of k_pfa_fwd_cols or None: not pinned).  A signal of `len` samples takes the packed forward
    transform while (len - 1) // 991 <= h (Engine::pfa_forward_applies); a longer one falls back to the four-step storer."""
    n, edge = N2 * n1, N2 * (half(n1) + 1)
    return [("upper-edge", edge, n + 1 - edge, 2),               # both through the cut, the first at the rule's upper edge
            ("mixed-producers", edge + 1, n - edge, 1),          # the first from the four-step storer, the second through the cut
            ("one-sample", n, 1, 1),                             # a one-sample signal through the cut
            ("short-second", n - 30, 31, None)]                  # fifteen of the sixteen column blocks see nothing inside the signal


def unequal_signals(n1: int, tag: str, len1: int, len2: int) -> Tuple[np.ndarray, np.ndarray]:
    rng = np.random.default_rng([3700, n1, len1, len2])
    return rng.standard_normal(len1), rng.standard_normal(len2)
