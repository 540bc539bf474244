"""Frames whose PHAT rows have their maximum at a chosen array index, for the statistics passes behind
``Engine.gcc_phat_all_pairs`` (the finishing column pass in both bodies, the same pass storing rows, the fused column pass,
k_rows_lean, the three launches).  Each of them keeps partial results per column block, wavefront, strip, chunk of output
indices or 64-sample chunk and merges them afterwards; this module puts a row's peak ON those borders.  Inputs only, no GPU;
plain helper module like ``second_path.py`` and ``peak_rows.py``.

PHAT whitening rules out hand-written correlation rows, but an impulse passes through it: with frame rows
``x_m = noise(sigma = 1) + sqrt(L) * delta[p_m]`` the row of pair (i, j) has its maximum at ``(p_i - p_j) mod n``, n = 2L - 1,
about 0.5 high over a runner-up of 0.02 .. 0.06.  Two "star" frames reach every index: microphone 0 with its impulse at L - 1
reaches k <= L - 1 through p_j = L - 1 - k, microphone 0 with its impulse at 0 reaches k > L - 1 through p_j = n - k.

The amplitude is sqrt(L) and not more: the finishing pass hands a row whose SNR window holds more than 3 / 4 of the row's energy
to the stored-row path (at 3 sqrt(L) the peak holds 88 % of it), and a row that is handed on tests the stored-row path again, not
the pass.  At sqrt(L) at least 0.69 of the energy lies outside the window.

``decided`` is the condition on the inputs: a row whose integer fields change in the oracle when it is perturbed by
1e-11 max|corr| is not compared (its answer is a matter of rounding, not of logic).
"""
from __future__ import annotations

from collections import namedtuple
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from oracle import pal_oracle as O

MODES = (("median", 1.0), ("adaptive", 1.0), ("median", 4.2))   # lean body through the bound, 'adaptive', histogram body
INT_FIELDS = ("k_sel", "branch", "k_argmax")
MAX_MICS = 40
OTHERS = 32                      # seeded sample of the pairs (i, j), i > 0, per frame
UNDECIDED_SHARE = 0.02           # of a case's designed rows
PERTURB = 1e-11                  # x max|corr| x N(0, 1), two draws
# layout of k_rows_lean as its header documents it: a wavefront reads 22 overlapping chunks of 64 consecutive samples, 62 of
# them its own (the two border lanes hold the neighbours); the three launches work on 64-sample chunks
CHUNK = 64
WAVE_SPAN = 22 * 62

Star = namedtuple("Star", "frames designed implied")   # frames[F][M][L]; designed[f] = {j: k of pair (0, j)}; implied[f][i][j] = k (i < j)
TwoArrival = namedtuple("TwoArrival", "frames rows")   # frames[2 copies][4][L]; rows = [(frame, j, name, strong k, weak k)]
TWO_ARRIVAL_COPIES = 8           # noise draws per side of the window: 16 frames, 96 rows a call, so that a share of the call's rows means something


def window_half_width(fs: float, med: float) -> int:
    """largest w with |w / fs| <= med (the reference's comparison, utils.py:163, on lag_t = lag / fs)"""
    w = int(med * fs) + 2
    while w >= 0 and not abs(w / fs) <= med:
        w -= 1
    return w


def _crt(r1: int, n1: int, r2: int, n2: int) -> int:
    """the unique m < n1 n2 with m mod n1 = r1 and m mod n2 = r2 (n1, n2 coprime), by residues alone"""
    return next(m for m in range(r2, n1 * n2, n2) if m % n1 == r1)


def designed_indices(L: int, n1: int, n2: int, fs: float, med: float, stored: bool = False,
                     r2_values: Optional[Sequence[int]] = None) -> List[int]:
    """Sorted array indices at which a row's maximum is to sit.  `stored`: the borders of the passes over stored rows as well;
    `r2_values`: another list of column residues (the full-size case restricts them)."""
    n = 2 * L - 1
    c = L - 1
    w = window_half_width(fs, med)
    d = int(fs * 0.001)
    out = {0, 1, 2, n - 3, n - 2, n - 1, c - 1, c, c + 1}
    for off in (w, w + 1, w - d + 2, w - d, w + d - 1):             # the window's edges and its `distance - 1` margins
        out |= {c - off, c + off}
    if n1 > 0:
        assert n1 * n2 == n
        r1s = sorted({0, 1, (n1 - 1) // 2, (n1 + 1) // 2, n1 - 1} & set(range(n1)))
        if r2_values is None:                                       # grid edges; 62-column block and 248-column strip borders
            r2_values = (0, 1, n2 - 2, n2 - 1, 61, 62, 63, 124, 247, 248, 249)
        for r2 in sorted({r for r in r2_values if 0 <= r < n2}):
            out |= {_crt(r1, n1, r2, n2) for r1 in r1s}
    if stored:
        for unit in (CHUNK, WAVE_SPAN):
            for mult in (1, 2, 3, 4, (n - 1) // unit):
                out |= {unit * mult - 1, unit * mult, unit * mult + 1}
    return sorted(k for k in out if 0 <= k < n)


def _impulse_frame(rng, L: int, positions: Sequence[int]) -> np.ndarray:
    x = rng.standard_normal((len(positions), L))
    x[np.arange(len(positions)), positions] += np.sqrt(L)
    return x


def star_frames(L: int, indices: Sequence[int], seed: int) -> Star:
    """Star frames for `indices`: every frame has the same number of microphones (at most MAX_MICS); frames with fewer designed
    indices than the largest are filled with impulse positions drawn at random (their pairs count among the implied ones)."""
    n = 2 * L - 1
    rng = np.random.default_rng(seed)
    low = [k for k in indices if k <= L - 1]
    high = [k for k in indices if k > L - 1]
    plan = []                                                       # (impulse of microphone 0, [(k, p_j)])
    for p0, ks, pos in ((L - 1, low, lambda k: L - 1 - k), (0, high, lambda k: n - k)):
        parts = -(-len(ks) // (MAX_MICS - 1))
        for q in range(parts):
            plan.append((p0, [(k, pos(k)) for k in ks[q::parts]]))
    mics = 1 + max(len(p[1]) for p in plan)
    frames, designed, implied = [], [], []
    for p0, kp in plan:
        positions = [p0] + [p for _, p in kp]
        free = np.setdiff1d(np.arange(L), positions)
        positions += [int(p) for p in rng.choice(free, mics - len(positions), replace=False)]
        frames.append(_impulse_frame(rng, L, positions))
        designed.append({1 + q: k for q, (k, _) in enumerate(kp)})
        implied.append({(i, j): (positions[i] - positions[j]) % n for i in range(mics) for j in range(i + 1, mics)})
        assert all(implied[-1][(0, j)] == k for j, k in designed[-1].items())
    return Star(np.stack(frames), designed, implied)


def two_arrival_frames(L: int, fs: float, med: float, seed: int, copies: int = TWO_ARRIVAL_COPIES) -> TwoArrival:
    """Rows with two arrivals at the window's edge: the second microphone of the pair carries a second impulse of 0.6 sqrt(L).
    `copies` noise draws of two frames each (even frames the low side of the window, odd frames the high side), pairs (0, 1),
    (0, 2), (0, 3) of every frame:
      outside  the strong peak 3 samples outside the window, the weak one inside and distance - 1 from it: the distance rule
               removes the weak peak, a noise peak elsewhere in the window is selected;
      inside   the reverse: the strong peak inside, the weak one 3 samples outside: the inside peak is kept;
      apart    as `outside`, the weak peak exactly `distance` from the strong one: not removed, it is selected."""
    n = 2 * L - 1
    c = L - 1
    w = window_half_width(fs, med)
    d = int(fs * 0.001)
    assert d >= 5 and w - d - 3 > d
    rng = np.random.default_rng(seed)
    frames, rows = [], []
    for f, side in enumerate((-1, +1) * copies):
        p0 = L - 1 if side < 0 else 0
        pos = (lambda k: L - 1 - k) if side < 0 else (lambda k: n - k)
        out_k = c + side * (w + 3)
        arrangements = (("outside", out_k, out_k - side * (d - 1)), ("inside", out_k - side * (d - 1), out_k),
                        ("apart", out_k, out_k - side * d))
        x = rng.standard_normal((4, L))
        x[0, p0] += np.sqrt(L)
        for j, (name, strong, weak) in enumerate(arrangements, start=1):
            x[j, pos(strong)] += np.sqrt(L)
            x[j, pos(weak)] += 0.6 * np.sqrt(L)
            rows.append((f, j, name, strong, weak))
        frames.append(x)
    return TwoArrival(np.stack(frames), rows)


# ------------------------------------------------------------------------------------------------ the oracle's answers
def spectra(frame: np.ndarray) -> np.ndarray:
    """every microphone's spectrum once, on the grid n = 2L - 1 of O.phat_correlation"""
    return np.fft.fft(np.asarray(frame, dtype=np.float64), n=2 * frame.shape[1] - 1, axis=-1)


def corr_from_spectra(fa: np.ndarray, fb: np.ndarray) -> np.ndarray:
    """O.phat_correlation behind its two forward transforms, statement by statement (test_host_peak_positions holds the two equal)"""
    cross = fa * np.conj(fb)
    cross /= np.abs(cross) + 1e-10
    return np.fft.ifft(cross).real


def record(corr: np.ndarray, L: int, fs: float, method: str, mult: float, med: Optional[float]) -> dict:
    rec = O.pair_record(corr, L, fs, method, mult, med)
    rec["sel_height"] = float(corr[rec["k_sel"]])
    return rec


def decided(corr: np.ndarray, L: int, fs: float, method: str, mult: float, med: Optional[float], want: Optional[dict] = None) -> bool:
    """The integer fields of O.pair_record do not change under two seeded perturbations of PERTURB x max|corr| x N(0, 1)."""
    want = O.pair_record(corr, L, fs, method, mult, med) if want is None else want
    scale = PERTURB * float(np.max(np.abs(corr)))
    for draw in (1, 2):
        other = O.pair_record(corr + scale * np.random.default_rng(draw).standard_normal(corr.shape[0]), L, fs, method, mult, med)
        if any(other[f] != want[f] for f in INT_FIELDS):
            return False
    return True


def outside_energy_share(corr: np.ndarray) -> float:
    """share of sum(corr^2) outside the oracle's SNR window (O.compute_snr's bounds)"""
    n = corr.shape[0]
    pk = int(np.argmax(corr))
    w = max(1, int(0.01 * n))
    lo, hi = max(0, pk - w), min(n, pk + w)
    total = float(np.sum(corr ** 2))
    return (total - float(np.sum(corr[lo:hi] ** 2))) / total


def param_sets(med: float):
    """the six calls of a case: unwindowed and windowed, three modes each"""
    return [(method, mult, m) for m in (None, med) for method, mult in MODES]


class Case:
    """One frame length: its star frames, the pairs that are compared, and the oracle's records of them, computed once per
    process and shared by the host test and the GPU tests (nothing writes to them)."""

    def __init__(self, L, n1, n2, fs, med, stored=False, r2_values=None, others=OTHERS, seed=None):
        self.L, self.n1, self.n2, self.fs, self.med = L, n1, n2, float(fs), med
        self.n = 2 * L - 1
        self.indices = designed_indices(L, n1, n2, fs, med, stored, r2_values)
        self._seed = 1000 + L if seed is None else seed
        self._star: Optional[Star] = None
        self.mics = self.star.frames.shape[1]
        pairs = [(i, j) for i in range(self.mics) for j in range(i + 1, self.mics)]
        self.pair_index = {p: q for q, p in enumerate(pairs)}
        rng = np.random.default_rng(L)
        self.rows = []                                              # (frame, i, j, designed k or None)
        for f in range(self.star.frames.shape[0]):
            self.rows += [(f, 0, j, k) for j, k in sorted(self.star.designed[f].items())]
            rest = [p for p in pairs if p[0] > 0]
            pick = rng.choice(len(rest), min(others, len(rest)), replace=False)
            self.rows += [(f,) + rest[q] + (None,) for q in sorted(pick)]
        self.designed_rows = [r for r in self.rows if r[3] is not None]
        assert sorted(r[3] for r in self.designed_rows) == self.indices
        self._spec: Dict[int, np.ndarray] = {}
        self._corr: Dict[Tuple[int, int, int], np.ndarray] = {}
        self._want: Dict[tuple, dict] = {}

    @property
    def star(self) -> Star:
        """the star frames (seeded: built again after release())"""
        if self._star is None:
            self._star = star_frames(self.L, self.indices, self._seed)
        return self._star

    def corr(self, f, i, j) -> np.ndarray:
        if (f, i, j) not in self._corr:
            if f not in self._spec:
                self._spec[f] = spectra(self.star.frames[f])
            self._corr[(f, i, j)] = corr_from_spectra(self._spec[f][i], self._spec[f][j])
        return self._corr[(f, i, j)]

    def want(self, f, i, j, method, mult, med) -> dict:
        """the oracle's record of one row for one parameter set, with 'decided'"""
        key = (f, i, j, method, mult, med)
        if key not in self._want:
            corr = self.corr(f, i, j)
            rec = record(corr, self.L, self.fs, method, mult, med)
            rec["decided"] = decided(corr, self.L, self.fs, method, mult, med, rec)
            self._want[key] = rec
        return self._want[key]

    def release(self):
        """drop the frames and the rows (records stay): tens of megabytes a case"""
        self._star = None
        self._spec.clear()
        self._corr.clear()


_CASES: Dict[tuple, Case] = {}


def case(L, n1, n2, fs, med, stored=False, r2_values=None, others=OTHERS) -> Case:
    key = (L, n1, n2, fs, med, stored, None if r2_values is None else tuple(r2_values), others)
    if key not in _CASES:
        _CASES[key] = Case(L, n1, n2, fs, med, stored, r2_values, others)
    return _CASES[key]


def rates(L: int) -> Tuple[float, float]:
    """(fs, max_expected_delay) of a frame length: 16 kHz and 20 ms, 8 kHz and 10 ms below L = 4000"""
    return (8000.0, 0.01) if L < 4000 else (16000.0, 0.02)
