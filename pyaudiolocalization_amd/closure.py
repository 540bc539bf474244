"""Loop closure of a TDOA table: the device check (csrc/closure.hip, pal_tdoa_closure*) restated in NumPy.

For three microphones x < y < z the lags of a consistent table close: ``lag_xy + lag_yz - lag_xz = 0`` up to rounding.  Microphone
positions, speed of sound and calibration delays do not enter (``calib[j] - calib[i]`` cancels around a triangle).  A pair whose
GCC-PHAT row picked a multipath or noise peak breaks every triangle it belongs to; a pair with the right lag closes most of its own.
Per frame, from the ``k_sel`` column of the record table (``_ffi.RECORD``, row-major i<j) and the frame's length L:

- ``lag[p] = k_sel[p] - (L - 1)``, and ``A`` the antisymmetric matrix with ``A[i][j] = lag_ij``, ``A[j][i] = -lag_ij`` (``lag_matrix``);
- ``votes[p]`` of pair (i, j): the number of third microphones k not in {i, j} with ``|A[i][k] - A[j][k] - A[i][j]| <= tol`` - for
  i < j < k that is ``|lag_ik - lag_jk - lag_ij|``, the triangle's sum, and the other orders of k give the same sum up to its sign;
- ``mic_closed[m]``: the closed triangles that contain microphone m = half the sum of the votes of its pairs;
- ``weights[p]``: ``mask``: 1 where ``votes >= min_votes``, else 0; ``soft``: ``votes / (M - 2)`` there (one float64 division), else 0;
- ``summary``: closed triangles (a third of the sum of all votes), triangles M (M-1) (M-2) / 6, kept pairs (weight > 0), and the
  microphone with the fewest closed triangles (lowest index at ties).

Everything is integer arithmetic (int64 here, int32 on the device, where the argument checks keep every sum far inside the range), so
the two are compared bit for bit.  What the check cannot see: a constant clock offset of one microphone shifts all its lags
consistently and closes every triangle - it finds dead or noisy channels, not unsynchronised ones.
"""
from __future__ import annotations

import numpy as np

MODES = {"mask": 0, "soft": 1}                                          # PAL_CLOSURE_W_*
MIN_MICS, MAX_MICS = 3, 256
MAX_TOL = 1 << 20
MAX_LENGTH = 1 << 24

# one row of the summary (pal_closure_frame, 16 bytes)
SUMMARY = np.dtype([("closed", "<i4"), ("triangles", "<i4"), ("kept_pairs", "<i4"), ("worst_mic", "<i4")])
assert SUMMARY.itemsize == 16
OUTPUTS = ("votes", "mic_closed", "weights", "summary")                 # the order of the C ABI's four output pointers


def check_args(nframes, m, lengths, tol, min_votes, mode):
    """The argument checks of pal_tdoa_closure* -> (mode code, lengths[B] as int32); ValueError otherwise."""
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError(f"mode: one of {sorted(MODES)}")
    nframes, m, tol, min_votes = int(nframes), int(m), int(tol), int(min_votes)
    if nframes < 1:
        raise ValueError("need at least one frame")
    if not MIN_MICS <= m <= MAX_MICS:
        raise ValueError(f"the closure check takes {MIN_MICS}..{MAX_MICS} microphones (got {m})")
    if not 0 <= tol <= MAX_TOL:
        raise ValueError(f"tol {tol} outside 0..2^20")
    if min_votes < 0:
        raise ValueError("min_votes must not be negative")
    ln = np.broadcast_to(np.asarray(lengths, dtype=np.int64), (nframes,))
    if np.any(ln < 1) or np.any(ln > MAX_LENGTH):
        raise ValueError("a frame length outside 1..2^24")
    return MODES[mode], np.ascontiguousarray(ln, dtype=np.int32)


def empty_outputs(nframes: int, m: int, outputs=OUTPUTS):
    """Zeroed (votes[B][P], mic_closed[B][M], weights[B][P], summary[B]), None in place of a name that ``outputs`` does not list."""
    unknown = [name for name in outputs if name not in OUTPUTS]
    if unknown or not outputs:
        raise ValueError(f"outputs: at least one of {OUTPUTS}")
    p = int(m) * (int(m) - 1) // 2
    shapes = {"votes": ((nframes, p), np.int32), "mic_closed": ((nframes, int(m)), np.int32), "weights": ((nframes, p), np.float64),
              "summary": ((nframes,), SUMMARY)}
    return tuple(np.zeros(*shapes[name]) if name in outputs else None for name in OUTPUTS)


def lags(k_sel, length: int) -> np.ndarray:
    """k_sel[P] -> lag[P] (int64); ValueError for an index outside 0..2 length - 2."""
    k = np.asarray(k_sel, dtype=np.int64)
    if np.any(k < 0) or np.any(k > 2 * int(length) - 2):
        raise ValueError(f"k_sel outside 0..{2 * int(length) - 2}")
    return k - (int(length) - 1)


def lag_matrix(lag, m: int) -> np.ndarray:
    """lag[P] in row-major i<j order -> A[m][m] with A[i][j] = lag_ij, A[j][i] = -lag_ij, zero diagonal."""
    m = int(m)
    lag = np.asarray(lag, dtype=np.int64)
    if lag.shape != (m * (m - 1) // 2,):
        raise ValueError("the table must have M (M - 1) / 2 rows")
    a = np.zeros((m, m), dtype=np.int64)
    p = 0
    for i in range(m):
        for j in range(i + 1, m):
            a[i, j] = lag[p]
            a[j, i] = -lag[p]
            p += 1
    return a


def votes(lag, m: int, tol: int = 1) -> np.ndarray:
    """votes[P] (int32) of one frame: microphone i by microphone i, its pairs (i, j > i) as rows and the third microphones k as columns."""
    m = int(m)
    a = lag_matrix(lag, m)
    out = np.zeros(m * (m - 1) // 2, dtype=np.int32)
    third = np.arange(m)
    p = 0
    for i in range(m - 1):
        j = np.arange(i + 1, m)
        closes = np.abs(a[i][None, :] - a[j] - a[i, j][:, None]) <= int(tol)           # [j][k]
        others = (third[None, :] != i) & (third[None, :] != j[:, None])                # k not in {i, j}
        out[p:p + j.shape[0]] = np.count_nonzero(closes & others, axis=1)
        p += j.shape[0]
    return out


def mic_closed(votes_p, m: int) -> np.ndarray:
    """mic_closed[m] (int32): every closed triangle of microphone m votes for two of m's pairs."""
    m = int(m)
    v = np.asarray(votes_p, dtype=np.int64)
    total = np.zeros(m, dtype=np.int64)
    p = 0
    for i in range(m):
        for j in range(i + 1, m):
            total[i] += v[p]
            total[j] += v[p]
            p += 1
    assert np.all(total % 2 == 0)
    return (total // 2).astype(np.int32)


def weights(votes_p, m: int, min_votes: int = 1, mode: str = "soft") -> np.ndarray:
    v = np.asarray(votes_p, dtype=np.int64)
    keep = v >= int(min_votes)
    if mode == "mask":
        return keep.astype(np.float64)
    if mode != "soft":
        raise ValueError(f"mode: one of {sorted(MODES)}")
    return np.where(keep, v.astype(np.float64) / float(int(m) - 2), 0.0)


def summary(votes_p, m: int, min_votes: int = 1, mode: str = "soft") -> np.ndarray:
    m = int(m)
    v = np.asarray(votes_p, dtype=np.int64)
    rec = np.zeros((), dtype=SUMMARY)
    total = int(v.sum())
    assert total % 3 == 0
    rec["closed"] = total // 3
    rec["triangles"] = m * (m - 1) * (m - 2) // 6
    rec["kept_pairs"] = int(np.count_nonzero(weights(v, m, min_votes, mode) > 0))
    rec["worst_mic"] = int(np.argmin(mic_closed(v, m)))            # np.argmin: the first of equal values
    return rec


def tdoa_closure(k_sel, lengths, m: int, tol: int = 1, min_votes: int = 1, mode: str = "soft"):
    """k_sel[B][P] (or [P]; a record table's column), lengths[B] (or one length) -> (votes[B][P] int32, mic_closed[B][M] int32,
    weights[B][P] float64, summary[B] of SUMMARY): what Engine.tdoa_closure returns, frame by frame."""
    k = np.asarray(k_sel, dtype=np.int64)
    if k.ndim == 1:
        k = k[None]
    if k.ndim != 2:
        raise ValueError("k_sel must be [P] or [B][P]")
    m = int(m)
    _, ln = check_args(k.shape[0], m, lengths, tol, min_votes, mode)
    if k.shape[1] != m * (m - 1) // 2:
        raise ValueError("the table must have M (M - 1) / 2 rows")
    out_v = np.zeros(k.shape, dtype=np.int32)
    out_m = np.zeros((k.shape[0], m), dtype=np.int32)
    out_w = np.zeros(k.shape, dtype=np.float64)
    out_s = np.zeros(k.shape[0], dtype=SUMMARY)
    for b in range(k.shape[0]):
        out_v[b] = votes(lags(k[b], int(ln[b])), m, tol)
        out_m[b] = mic_closed(out_v[b], m)
        out_w[b] = weights(out_v[b], m, min_votes, mode)
        out_s[b] = summary(out_v[b], m, min_votes, mode)
    return out_v, out_m, out_w, out_s
