"""Frames of more than 98 304 samples: inputs for the LDS-tile rungs of the four-step chirp convolution that the shorter cases
never launch (conv_kernels.h k_cols_* / k_cols3_* / k_rows with 1024- and 2048-point rows), for the long prime-factor cuts and
for ``xcorr_vs_ref`` beyond N = 1025.  Inputs only, no GPU; plain helper module like ``peak_positions.py`` and ``second_path.py``.
tests/host/test_plan_geometry.cpp pins the same geometry from csrc/plan_geometry.h.

Three kinds of input:

``impulse_frames(L)``  three microphones ``x_m = a_m delta[p_m]``, no noise.  The spectrum of an impulse has one modulus in every
    bin, so the whitened cross spectrum of pair (i, j) is ``a_i a_j / (|a_i a_j| + 1e-10)`` times a pure phase ramp and the row is
    exactly that value at index ``(p_i - p_j) mod n`` and exactly 0 elsewhere: a reference without rounding error.  Three pairs
    fill one packed complex transform and half of another (the real part of a packed transform is one pair, the imaginary part
    the other).  The three peak indices of a frame satisfy d02 = d01 + d12 (mod n), so 0, n - 1 and L - 1 cannot share one frame:
    frame ``ends`` holds 0 and L - 1, frame ``wrap`` holds n - 1, L - 2 and L - 1.  Frame ``row`` puts peaks on M2 - 1 and M2 (a
    column index wrapping a row of the inverse convolution), frame ``tile`` on 4095 and 4096 (a border of the 4096-point tiles)
    with the amplitudes 2^-20 against 2^+20.

``noise_case(L)``  one frame of three microphones, rows 1 and 2 carrying 0.6 x row 0 rolled by 37 and by -1234, against
    ``O.phat_correlation`` / ``O.pair_record``.  ``NOISE_SEEDS`` were drawn until every row is decided in the sense of
    ``peak_positions.decided`` (``find_noise_seed``); tests/test_host_long_frames.py holds them to it.

``sparse_case(N)``  three integer rows with 64 non-zero samples each for ``xcorr_vs_ref``: 48 of them are a pattern the rows
    share at different shifts (a correlation of independent sparse rows is a list of single products, whose largest magnitude
    ties), 16 are the row's own, samples 0 and N - 1 among them.  The exact correlation is a 64 x 64 loop in int64.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Dict, List, Optional, Tuple

import numpy as np

from oracle import pal_oracle as O

import peak_positions as PP
import second_path as S

FS = 48000.0
ROW_BOUND = 1e-13                # absolute, on rows with a unit peak: what the suite holds the register geometries to

# (first length, last length) of every rung and the geometry (kind, l1 or m1, l2) of its PHAT inverse (4L - 3 points) and of its
# forward transform (2L - 1 points): "lds" columns of 2^l1 points, "lds3" of 3 * 2^l1, "reg2" m1-point columns in two lanes
Geom = namedtuple("Geom", "kind l1 l2 m1")


def _g(kind: str, a: int, l2: int) -> Geom:
    return Geom(kind, 0 if kind == "reg2" else a, l2, {"lds": 1 << a, "lds3": 3 << a, "reg2": a}[kind])


RUNGS = [
    (98305, 131072, _g("lds", 9, 10), _g("reg2", 32, 13)),
    (131073, 196608, _g("lds3", 8, 10), _g("reg2", 48, 13)),
    (196609, 262144, _g("lds", 9, 11), _g("lds", 9, 10)),
    (262145, 393216, _g("lds3", 8, 11), _g("lds3", 8, 10)),
    (393217, 524288, _g("lds", 10, 11), _g("lds", 9, 11)),
    (524289, 786432, _g("lds", 11, 11), _g("lds3", 8, 11)),
    (786433, 1048576, _g("lds", 11, 11), _g("lds", 10, 11)),
]
BOTTOMS = (98305, 131073, 196609, 262145, 393217, 524289)
TOPS = (131072, 196608, 262144, 393216, 524288, 1048576)
# length -> (N1, N2, log2 of the row tile, accumulator chunks of the column pass)
CUTS = {131072: (73, 3591, 13, 4), 131073: (65, 4033, 13, 3), 131079: (119, 2203, 13, 6), 196649: (93, 4229, 14, 5),
        520129: (127, 8191, 14, 6)}
RUNG_LENGTHS = tuple(sorted(set(BOTTOMS) | set(TOPS)))
IMPULSE_LENGTHS = tuple(sorted(set(RUNG_LENGTHS) | set(CUTS)))
NOISE_LENGTHS = BOTTOMS + (1048576,)
MAX_FRAME = 1 << 20


def geometry(L: int) -> Tuple[Geom, Geom]:
    """(inverse, forward) convolution of frames of L samples; the same with and without PAL_PFA=0"""
    for lo, hi, inv, fwd in RUNGS:
        if lo <= L <= hi:
            return inv, fwd
    raise KeyError(L)


def plan_pin(L: int, pfa: bool = True) -> dict:
    """what Engine.plan_info(L) returns under default switches (pfa) or PAL_PFA=0"""
    inv, _ = geometry(L)
    n1, n2, lm, _ = CUTS[L] if pfa and L in CUTS else (0, 0, 0, 0)
    return {"n": 2 * L - 1, "conv_len": inv.m1 << inv.l2, "m1": inv.m1, "m2": 1 << inv.l2, "n1": n1, "n2": n2,
            "tile_len": (1 << lm) if n1 else 0}


def conv_instances(g: Geom, loader: str = "", storer: str = "") -> List[str]:
    """prefixes of the profile entries of one convolution of geometry g (loader and storer names vary with the caller)"""
    if g.kind == "reg2":
        return ["k_colsreg_fwd<%d,%s" % (g.m1, loader), "k_rowsreg<%d,conv>" % g.l2, "k_colsreg_inv<%d,%s" % (g.m1, storer)]
    three = "3" if g.kind == "lds3" else ""
    return ["k_cols%s_fwd<%d,%s" % (three, g.l1, loader), "k_rows<%d,conv>" % g.l2, "k_cols%s_inv<%d,%s" % (three, g.l1, storer)]


def setup_instances(g: Geom) -> List[str]:
    """... of the chirp-spectrum setup of a plan's convolution"""
    rows = "k_rowsreg<%d,fwd>" if g.kind == "reg2" else "k_rows<%d,fwd>"
    return [conv_instances(g, "ChirpLoader")[0], rows % g.l2]


def missing_instances(entries: dict, prefixes) -> List[str]:
    return [p for p in prefixes if not any(name.startswith(p) and entries[name][1] >= 1 for name in entries)]


# ------------------------------------------------------------------------------------------------ exact impulse rows
ImpulseFrame = namedtuple("ImpulseFrame", "name frame peaks")     # frame[3][L]; peaks = [(i, j, index, value)] in pair order
PAIRS3 = ((0, 1), (0, 2), (1, 2))


def impulse_value(ai: float, aj: float) -> float:
    r = ai * aj
    return r / (abs(r) + 1e-10)


def _impulse_frame(name: str, L: int, positions, amps) -> ImpulseFrame:
    n = 2 * L - 1
    x = np.zeros((3, L))
    for m in range(3):
        x[m, positions[m]] = amps[m]
    peaks = [(i, j, (positions[i] - positions[j]) % n, impulse_value(amps[i], amps[j])) for i, j in PAIRS3]
    x.setflags(write=False)
    return ImpulseFrame(name, x, peaks)


def impulse_frames(L: int) -> List[ImpulseFrame]:
    inv, _ = geometry(L)
    m2 = 1 << inv.l2
    frames = [
        _impulse_frame("ends", L, (L - 1, L - 1, 0), (1.7, 0.9, 2.3)),                 # 0, L - 1, L - 1
        _impulse_frame("wrap", L, (L - 2, L - 1, 0), (-1.3, -0.7, 3.1)),               # n - 1, L - 2 (negative), L - 1 (negative)
        _impulse_frame("row", L, (m2, 1, 0), (0.3, -2.9, -1.1)),                       # M2 - 1 (negative), M2 (negative), 1
        _impulse_frame("tile", L, (4096, 1, 0), (2.0 ** -20, 2.0 ** 20, 3 * 2.0 ** -20)),   # 4095: 1, 4096: 0.027, 1: 1
    ]
    n = 2 * L - 1
    want = {"ends": (0, L - 1, L - 1), "wrap": (n - 1, L - 2, L - 1), "row": (m2 - 1, m2, 1), "tile": (4095, 4096, 1)}
    for f in frames:
        assert tuple(p[2] for p in f.peaks) == want[f.name], (L, f.name)
    return frames


def impulse_row(L: int, index: int, value: float) -> np.ndarray:
    row = np.zeros(2 * L - 1)
    row[index] = value
    return row


# ------------------------------------------------------------------------------------------------ noise with a common component
# length -> seed, drawn with find_noise_seed(L): the first seed at which all three rows are decided under every window setting
NOISE_SEEDS = {98305: 0, 131073: 0, 196609: 0, 262145: 0, 393217: 0, 524289: 0, 1048576: 0}


def noise_windows(L: int) -> Tuple[Optional[float], ...]:
    """max_expected_delay settings of a length: the oracle's peak selection is the cost of these tests"""
    return (None, 0.05) if L <= 262145 else (0.05,)


def noise_frame(L: int, seed: int) -> np.ndarray:
    x = np.random.default_rng([2026, L, seed]).standard_normal((3, L))
    x[1] += 0.6 * np.roll(x[0], 37)
    x[2] += 0.6 * np.roll(x[0], -1234)
    return x


NoiseCase = namedtuple("NoiseCase", "frame corr records")         # corr[3][n]; records[window] = [O.pair_record per pair]
_NOISE: Dict[Tuple[int, int], NoiseCase] = {}


def noise_case(L: int, seed: Optional[int] = None) -> NoiseCase:
    """computed once per process and shared (nothing writes to it)"""
    seed = NOISE_SEEDS[L] if seed is None else seed
    if (L, seed) not in _NOISE:
        x = noise_frame(L, seed)
        spec = PP.spectra(x)
        corr = np.stack([PP.corr_from_spectra(spec[i], spec[j]) for i, j in PAIRS3])
        records = {med: [O.pair_record(row, L, FS, "median", 1.0, med) for row in corr] for med in noise_windows(L)}
        x.setflags(write=False)
        corr.setflags(write=False)
        _NOISE[(L, seed)] = NoiseCase(x, corr, records)
    return _NOISE[(L, seed)]


def noise_decided(L: int, seed: Optional[int] = None) -> bool:
    case = noise_case(L, seed)
    return all(PP.decided(case.corr[p], L, FS, "median", 1.0, med, case.records[med][p])
               for med in noise_windows(L) for p in range(3))


def find_noise_seed(L: int) -> int:
    seed = 0
    while not noise_decided(L, seed):
        seed += 1
    return seed


# ------------------------------------------------------------------------------------------------ cuts
def cut_indices(L: int) -> List[int]:
    """first, middle and last column class x first and last tile point"""
    n1, n2, _, _ = CUTS[L]
    return sorted(PP._crt(r1, n1, r2, n2) for r1 in (0, (n1 - 1) // 2, n1 - 1) for r2 in (0, n2 - 1))


CUT_MED = 0.05
CUT_METHODS = ("median", "adaptive")
# length -> seed of the star frames, drawn with find_cut_seed(L): the first at which every designed row is decided under both methods
CUT_SEEDS = {131072: 0, 131073: 0, 131079: 0, 196649: 0, 520129: 0}
CutCase = namedtuple("CutCase", "frames rows corr records")       # frames[f] = [mics][L]; rows = [(f, j, k)]; corr[(f, j)]; records[method][(f, j)]
_CUT: Dict[Tuple[int, int], CutCase] = {}


def cut_case(L: int, seed: Optional[int] = None) -> CutCase:
    """Star frames of peak_positions (impulses of sqrt(L) in unit noise) cut down to microphone 0 and the microphones whose pair
    (0, j) has its maximum designed on cut_indices(L), the oracle's rows of those pairs and its records: once per process"""
    seed = CUT_SEEDS[L] if seed is None else seed
    if (L, seed) not in _CUT:
        star = PP.star_frames(L, cut_indices(L), [3000, L, seed])
        frames = [np.ascontiguousarray(star.frames[f][: 1 + len(star.designed[f])]) for f in range(star.frames.shape[0])]
        rows = [(f, j, k) for f in range(len(frames)) for j, k in sorted(star.designed[f].items())]
        assert sorted(k for _, _, k in rows) == cut_indices(L) and all(j < frames[f].shape[0] for f, j, _ in rows)
        spec = [PP.spectra(fr) for fr in frames]
        corr = {(f, j): PP.corr_from_spectra(spec[f][0], spec[f][j]) for f, j, _ in rows}
        records = {m: {key: O.pair_record(row, L, FS, m, 1.0, CUT_MED) for key, row in corr.items()} for m in CUT_METHODS}
        for (f, j, k) in rows:
            assert records["median"][(f, j)]["k_argmax"] == k, (L, f, j, k)
        _CUT[(L, seed)] = CutCase(frames, rows, corr, records)
    return _CUT[(L, seed)]


def cut_decided(L: int, seed: Optional[int] = None) -> bool:
    case = cut_case(L, seed)
    return all(PP.decided(case.corr[key], L, FS, m, 1.0, CUT_MED, case.records[m][key]) for m in CUT_METHODS for key in case.corr)


def find_cut_seed(L: int) -> int:
    seed = 0
    while not cut_decided(L, seed):
        seed += 1
    return seed


# ------------------------------------------------------------------------------------------------ sparse integer rows
SPARSE_N = (196609, 262145, 393217, 524289, 1048576)
SPARSE_GEOM = {196609: _g("lds", 9, 10), 262145: _g("lds3", 8, 10), 393217: _g("lds", 9, 11), 524289: _g("lds3", 8, 11),
               1048576: _g("lds", 10, 11)}                         # of the 2N - 1 points
SPARSE_REF, SPARSE_NONZERO, SPARSE_SHARED = 1, 64, 48
# N -> seed, drawn with find_sparse_seed(N): the first whose rows all have a unique correlation peak with margin 1
SPARSE_SEEDS = {700: 0, 196609: 0, 262145: 0, 393217: 0, 524289: 0, 1048576: 0}


def sparse_shifts(n: int) -> Tuple[int, int, int]:
    return (-(n // 3), 0, n // 2 - 5)


def sparse_rows(n: int, seed: int):
    """-> (positions[3][64], values[3][64]) ascending in position"""
    rng = np.random.default_rng([2027, n, seed])
    core = np.sort(rng.choice(np.arange(n // 3 + 1, n // 2), SPARSE_SHARED, replace=False))
    core_v = rng.choice(np.array([v for v in range(-8, 9) if v]), SPARSE_SHARED)
    pos, val = [], []
    for shift in sparse_shifts(n):
        p = core + shift
        free = np.setdiff1d(np.arange(1, n - 1), p)
        own = np.concatenate(([0, n - 1], rng.choice(free, SPARSE_NONZERO - SPARSE_SHARED - 2, replace=False)))
        own_v = rng.choice(np.array([v for v in range(-8, 9) if v]), own.size)
        allp, allv = np.concatenate((p, own)), np.concatenate((core_v, own_v))
        order = np.argsort(allp)
        pos.append(allp[order].astype(np.int64))
        val.append(allv[order].astype(np.int64))
        assert np.unique(pos[-1]).size == SPARSE_NONZERO and pos[-1][0] == 0 and pos[-1][-1] == n - 1
    return pos, val


def sparse_exact(pa, va, pb, vb, n: int) -> np.ndarray:
    """np.correlate(a, b, 'full') of two sparse integer rows: a 64 x 64 loop in int64"""
    seq = np.zeros(2 * n - 1, dtype=np.int64)
    for i, x in zip(pa.tolist(), va.tolist()):
        for j, y in zip(pb.tolist(), vb.tolist()):
            seq[i - j + n - 1] += x * y
    return seq


def dense(pos, val, n: int) -> np.ndarray:
    rows = np.zeros((len(pos), n))
    for q in range(len(pos)):
        rows[q, pos[q]] = val[q]
    return rows


def _sparse_table(n: int, seed: int):
    pos, val = sparse_rows(n, seed)
    exact = [sparse_exact(pos[q], val[q], pos[SPARSE_REF], val[SPARSE_REF], n).astype(np.float64) for q in range(3)]
    return pos, val, exact


def find_sparse_seed(n: int) -> int:
    seed = 0
    while not all(S.peak_margin(seq) >= 1.0 for seq in _sparse_table(n, seed)[2]):
        seed += 1
    return seed


_SPARSE: Dict[int, S.XcorrCase] = {}


def sparse_case(n: int) -> S.XcorrCase:
    if n not in _SPARSE:
        pos, val, exact = _sparse_table(n, SPARSE_SEEDS[n])
        for q, seq in enumerate(exact):
            assert S.peak_margin(seq) >= 1.0, "sparse N=%d: row %d has no unique peak" % (n, q)
            assert int(np.argmax(np.abs(seq))) == sparse_shifts(n)[q] + n - 1, (n, q)
        rows = dense(pos, val, n)
        rows.setflags(write=False)
        _SPARSE[n] = S.XcorrCase("sparse/n%d" % n, rows, (SPARSE_REF,), {SPARSE_REF: exact})
    return _SPARSE[n]
