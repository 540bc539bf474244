"""Delay-and-sum beamformer: the specification of ``Engine.steer`` (csrc/beamform.hip) and the helpers that turn positions,
directions and SRP records into steering delays.  Pure NumPy, no engine call - the role closure.py, consensus.py and srp.py play for
their features.

``steer(frames[B][M][L], fs, delays[B][S][M], weights[B][S][M]) -> out[B][S][L]``::

    X[b,m]   = np.fft.fft(frames[b,m], n=2L)
    f        = np.fft.fftfreq(2L, d=1/fs)
    acc      = 0;  for m = 0 .. M-1 in this order:
               acc = acc + weights[b,s,m] * (X[b,m] * np.exp(-1j*2*np.pi*f*delays[b,s,m]))
    out[b,s] = np.fft.ifft(acc).real[:L] * fade_window(L)

so ``out[b,s] = sum_m w[b,s,m] * fractional_delay(frames[b,m], delays[b,s,m], fs)`` in exact arithmetic: every microphone row is
delayed so that the chosen point lines up, then the rows are summed.  With ``M`` microphones and independent noise that is up to
``10 log10(M)`` dB over one microphone.

Delays are >= 0 in what the helpers return (the farthest, or latest, microphone gets 0); ``steer`` itself takes any sign.
"""
from __future__ import annotations

import numpy as np

from . import _ffi, srp


def fade_window(n: int) -> np.ndarray:
    """The 1 % linear fade of the reference's fractional_delay: int(0.01 n) samples at each end (signal_processing.py:75-78)."""
    fl = int(0.01 * n)
    if fl < 1:
        raise ValueError("the fade window needs at least 100 samples")
    w = np.ones(n)
    w[:fl] *= np.linspace(0, 1, fl)
    w[-fl:] *= np.linspace(1, 0, fl)
    return w


def _tables(frames, delays, weights):
    x = np.asarray(frames, dtype=np.float64)
    d = np.asarray(delays, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    if x.ndim != 3:
        raise ValueError("frames must be [B][M][L]")
    if d.ndim != 3 or d.shape != w.shape or d.shape[0] != x.shape[0] or d.shape[2] != x.shape[1]:
        raise ValueError("delays and weights must be [B][S][M] matching frames[B][M][L]")
    return x, d, w


def steer(frames, fs, delays, weights) -> np.ndarray:
    """frames[B][M][L], delays / weights[B][S][M] -> out[B][S][L] (the rule in the module's docstring, m ascending)."""
    x, d, w = _tables(frames, delays, weights)
    length = x.shape[2]
    spec = np.fft.fft(x, n=2 * length, axis=-1)                                 # [B][M][2L]
    f = np.fft.fftfreq(2 * length, d=1.0 / fs)
    acc = np.zeros((d.shape[0], d.shape[1], 2 * length), dtype=np.complex128)
    for m in range(x.shape[1]):
        phase = np.exp(-1j * 2 * np.pi * f[None, None, :] * d[:, :, m, None])
        product = spec[:, None, m, :] * phase
        acc = acc + w[:, :, m, None] * product
    return np.fft.ifft(acc, axis=-1).real[..., :length] * fade_window(length)


def _calibrated(d: np.ndarray, calib_delays) -> np.ndarray:
    """Microphone m's row is late by calib[m] (main.py corrects a pair's delay by calib[j] - calib[i]): it needs that much less delay."""
    cal = np.asarray(calib_delays, dtype=np.float64)
    if cal.shape != (d.shape[-1],):
        raise ValueError("one calibration delay per microphone")
    d = d + (np.max(cal) - cal)
    return d - np.min(d, axis=-1, keepdims=True)


def point_delays(points, mics, c, calib_delays=None):
    """points[...][3] -> (delays[...][M], valid[...]): r_m = |p - mic_m|, d_m = (max_m r - r_m) / c; every delay is >= 0 and the
    farthest microphone gets 0.  With ``calib_delays``: d_m = (max_m r_m/c - r_m/c) + (max calib - calib[m]), minus its minimum over m.
    A point with a non-finite coordinate is not valid and gets delays of 0."""
    p = np.asarray(points, dtype=np.float64)
    mic = np.asarray(mics, dtype=np.float64).reshape(-1, 3)
    if p.shape[-1:] != (3,):
        raise ValueError("points must be [...][3]")
    valid = np.all(np.isfinite(p), axis=-1)
    safe = np.where(valid[..., None], p, 0.0)
    r = np.sqrt(np.sum((safe[..., None, :] - mic) ** 2, axis=-1))               # [...][M]
    if calib_delays is None:
        d = (np.max(r, axis=-1, keepdims=True) - r) / np.float64(c)
    else:
        t = r / np.float64(c)
        d = _calibrated(np.max(t, axis=-1, keepdims=True) - t, calib_delays)
    return np.where(valid[..., None], d, 0.0), valid


def direction_delays(directions, mics, c, calib_delays=None):
    """directions[...][3] (the direction map's unit vectors) -> (delays[...][M], valid[...]): with a = srp.doa_advances(u, mics) a
    microphone with larger a hears the plane wave earlier, d_m = (a_m - min_m a) / c.  ``calib_delays`` and non-finite directions
    as in point_delays."""
    u = np.asarray(directions, dtype=np.float64)
    mic = np.asarray(mics, dtype=np.float64).reshape(-1, 3)
    if u.shape[-1:] != (3,):
        raise ValueError("directions must be [...][3]")
    valid = np.all(np.isfinite(u), axis=-1)
    safe = np.where(valid[..., None], u, 0.0)
    a = srp.doa_advances(safe.reshape(-1, 3), mic).reshape(u.shape[:-1] + (mic.shape[0],))
    d = (a - np.min(a, axis=-1, keepdims=True)) / np.float64(c)
    if calib_delays is not None:
        d = _calibrated(d, calib_delays)
    return np.where(valid[..., None], d, 0.0), valid


def uniform_weights(valid, m: int) -> np.ndarray:
    """valid[...] -> weights[...][M]: 1/M where valid, 0 elsewhere (such a beam is a row of zeros)."""
    v = np.asarray(valid, dtype=bool)
    return np.where(v[..., None], 1.0 / int(m), 0.0) * np.ones(int(m))


def records_to_points(records) -> np.ndarray:
    """_ffi.SRP_PEAK or _ffi.SRP_ZOOM records[...] -> points[...][3] from x, y, z.  An absent peak (index < 0) or zoom result
    (seed < 0 or levels == 0) becomes a NaN point, which steers to a row of zeros."""
    rec = np.asarray(records)
    names = rec.dtype.names or ()
    if rec.dtype == _ffi.SRP_PEAK or ("index" in names and "seed" not in names):
        present = rec["index"] >= 0
    elif rec.dtype == _ffi.SRP_ZOOM or ("seed" in names and "levels" in names):
        present = (rec["seed"] >= 0) & (rec["levels"] != 0)
    else:
        raise ValueError("records must be _ffi.SRP_PEAK or _ffi.SRP_ZOOM arrays")
    p = np.stack([rec["x"], rec["y"], rec["z"]], axis=-1).astype(np.float64)
    return np.where(present[..., None], p, np.nan)
