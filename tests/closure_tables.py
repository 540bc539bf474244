"""Inputs of the loop-closure tests (pal_tdoa_closure*, pyaudiolocalization_amd/closure.py), built on ``robust_tables.table``.

``dead_table(m, seed, mic)``: the clean table of (m, seed) with every pair of microphone ``mic`` redrawn from +-2400 samples (a dead or
noisy channel).  ``random_tables(b, m, seed, span)``: k_sel[b][P] with independent lags in +-span, which close almost no triangle at a
small tolerance and many at a large one.  ``records(k_sel)``: a record table around a k_sel array.  ``spec(...)``: the specification's four
outputs, computed once per argument set and shared between the tests."""
import functools

import numpy as np

import robust_tables as T
from pyaudiolocalization_amd import closure as CL
from pyaudiolocalization_amd import solve as S
from pyaudiolocalization_amd._ffi import RECORD

DEAD_CASES = [(16, 3, 5), (65, 3, 5)]          # (microphones, seed, dead microphone)


def records(k_sel):
    k = np.asarray(k_sel)
    rec = np.zeros(k.shape, dtype=RECORD)
    rec["k_sel"] = k
    rec["snr"] = 1.0
    return rec


@functools.lru_cache(maxsize=None)
def dead_table(m, seed, mic):
    """-> dict like robust_tables.table's, ``bad`` the pairs of the dead microphone.  The lags are drawn after the table's own draws,
    from a generator of their own, in row-major pair order."""
    t = dict(T.table(m, seed, 0))
    pi, pj = S.pair_indices(m)
    bad = np.flatnonzero((pi == mic) | (pj == mic))
    lag = t["true_lag"].copy()
    lag[bad] = np.random.default_rng([seed, mic]).integers(-2400, 2401, bad.shape[0])
    t.update(lag=lag, k_sel=lag + T.LENGTH - 1, bad=bad, records=records(lag + T.LENGTH - 1))
    return t


def random_tables(b, m, seed, span=40, length=T.LENGTH):
    """k_sel[b][P] (int64) with lags uniform in +-span: at tol 1 a triangle closes with probability ~ 3 / (2 span), so the votes take many values."""
    rng = np.random.default_rng([seed, b, m])
    return rng.integers(-span, span + 1, (b, m * (m - 1) // 2)) + length - 1


_SPEC = {}


def spec(k_sel, lengths, m, tol=1, min_votes=1, mode="soft"):
    """closure.tdoa_closure, remembered per argument set (the arrays by their bytes); the caller leaves the result unchanged."""
    k = np.ascontiguousarray(k_sel, dtype=np.int64)
    ln = np.ascontiguousarray(np.broadcast_to(np.asarray(lengths, dtype=np.int64), (1 if k.ndim == 1 else k.shape[0],)))
    key = (k.tobytes(), k.shape, ln.tobytes(), m, tol, min_votes, mode)
    if key not in _SPEC:
        _SPEC[key] = CL.tdoa_closure(k, ln, m, tol, min_votes, mode)
    return _SPEC[key]
