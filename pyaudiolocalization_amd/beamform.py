"""Delay-and-sum, null-steering and MVDR beamformers: the specifications of ``Engine.steer``, ``Engine.separate`` and ``Engine.mvdr``
(csrc/beamform.hip) and the helpers that turn positions, directions and SRP records into steering delays.  Pure NumPy, no engine call - the role closure.py,
consensus.py and srp.py play for their features.

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

``separate(frames[B][M][L], fs, delays[B][S][M], gains[B][S][M], loading) -> out[B][S][L]`` is the beamformer that cancels the other
sources: with the S positions known, the S beams of a bin are the least-squares solution of ``X = A s``, ``A[m,s] = gains[b,s,m] *
conj(p[s,m])`` the steering matrix (null steering / zero forcing with diagonal loading, an LCMV beamformer under white noise)::

    p[s,m]   = np.exp(-1j*2*np.pi*f*delays[b,s,m])
    Y[s]     = 0;  for m = 0 .. M-1:  Y[s] = Y[s] + gains[b,s,m] * (X[b,m] * p[s,m])                      (steer's sum, weights = gains)
    G[s,t]   = 0;  for m = 0 .. M-1:  G[s,t] = G[s,t] + (gains[b,s,m]*gains[b,t,m]) * (p[s,m] * np.conj(p[t,m]))     for t < s
    q[s]     = 0;  for m = 0 .. M-1:  q[s] = q[s] + gains[b,s,m]*gains[b,s,m]                             (G's diagonal, every bin's)
    delta    = loading * max_s q[s]
    Z        = solve_loaded(q + delta, G, Y)            ((G + delta I) Z = Y by Cholesky; its docstring states the operation order)
    out[b,s] = np.fft.ifft(Z[s]).real[:L] * fade_window(L)

Consequences: ``Z(-f) = conj(Z(f))``, so L + 1 bins carry everything (the device computes those, and only the real part of the Nyquist
bin survives ``.real``).  With S = 1 and loading 0 the result is ``steer(frames, fs, delays, gains / q)``.  A source whose gains are
all zero has a zero row and column in G: its output is a row of exact zeros and the others do not notice it.  A frame without a live
weighted row gives S rows of exact zeros.  Two sources with the same delays do not break the solve (delta > 0 keeps the factor
positive) and give two equal rows.  ``cond(G + delta I) <= (S + loading) / loading`` where q is equal across sources, and
``|(G + delta I)^-1| <= 1 / delta`` always - the bound the test tolerances rest on.

``mvdr(frames[B][M][L], fs, delays[G][S][M], gains[G][S][M], loading, groups) -> out[B][S][L]`` takes the weights from the data: the
frames are G groups of snapshots, each group's covariance per bin gives ``w = R~^-1 a / (a^H R~^-1 a)``, the beam that passes source s
unchanged and has the least power otherwise - an interferer nobody located is cancelled where it is stationary over the group.  The
rule stands in ``mvdr``'s docstring, its steps are ``mvdr_covariance`` and ``mvdr_weights``.
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


def solve_loaded(diag, g, y):
    """(G + delta I) z = y for Hermitian positive definite systems of n unknowns, vectorised over any trailing axes (the bins):
    ``diag[n][...]`` is the real diagonal G[i][i] + delta, ``g[n][n][...]`` complex of which only the strict lower triangle is read,
    ``y[n][...]`` complex.  -> z[n][...].  Cholesky, on real and imaginary parts with every product written out, so that the bits do
    not depend on how a library multiplies complex numbers (csrc/separate_math.h runs the same operations in the same order)::

        factor, j = 0 .. n-1:   s = diag[j];  for k = 0 .. j-1:  s = s - (Lre[j,k]*Lre[j,k] + Lim[j,k]*Lim[j,k])
                                r[j] = 1 / sqrt(s)
                                for i = j+1 .. n-1:  v = g[i,j];  for k = 0 .. j-1:  v = v - L[i,k] conj(L[j,k]);   L[i,j] = v * r[j]
        forward, i = 0 .. n-1:  v = y[i];  for k = 0 .. i-1:    v = v - L[i,k] z[k];         z[i] = v * r[i]
        back, i = n-1 .. 0:     v = z[i];  for k = i+1 .. n-1:  v = v - conj(L[k,i]) z[k];   z[i] = v * r[i]

    (a+jb)(c+jd) = (a*c - b*d) + j(a*d + b*c), (a+jb) conj(c+jd) = (a*c + b*d) + j(b*c - a*d), conj(a+jb)(c+jd) = (a*c + b*d) +
    j(a*d - b*c): each bracket is formed first, then subtracted from the running part."""
    g = np.asarray(g, dtype=np.complex128)
    y = np.asarray(y, dtype=np.complex128)
    n = y.shape[0]
    tail = np.broadcast_shapes(g.shape[2:], y.shape[1:], np.shape(diag)[1:])
    dg = np.broadcast_to(np.asarray(diag, dtype=np.float64), (n,) + tail)
    lre = np.array(np.broadcast_to(g.real, (n, n) + tail))
    lim = np.array(np.broadcast_to(g.imag, (n, n) + tail))
    zre = np.array(np.broadcast_to(y.real, (n,) + tail))
    zim = np.array(np.broadcast_to(y.imag, (n,) + tail))
    r = np.empty((n,) + tail)
    for j in range(n):
        s = dg[j].copy()
        for k in range(j):
            s = s - (lre[j, k] * lre[j, k] + lim[j, k] * lim[j, k])
        r[j] = 1.0 / np.sqrt(s)
        for i in range(j + 1, n):
            vre, vim = lre[i, j], lim[i, j]
            for k in range(j):
                a, b, c, d = lre[i, k], lim[i, k], lre[j, k], lim[j, k]
                vre = vre - (a * c + b * d)
                vim = vim - (b * c - a * d)
            lre[i, j] = vre * r[j]
            lim[i, j] = vim * r[j]
    for i in range(n):
        vre, vim = zre[i], zim[i]
        for k in range(i):
            a, b, c, d = lre[i, k], lim[i, k], zre[k], zim[k]
            vre = vre - (a * c - b * d)
            vim = vim - (a * d + b * c)
        zre[i] = vre * r[i]
        zim[i] = vim * r[i]
    for i in range(n - 1, -1, -1):
        vre, vim = zre[i], zim[i]
        for k in range(i + 1, n):
            a, b, c, d = lre[k, i], lim[k, i], zre[k], zim[k]
            vre = vre - (a * c + b * d)
            vim = vim - (a * d - b * c)
        zre[i] = vre * r[i]
        zim[i] = vim * r[i]
    return zre + 1j * zim


def check_loading(loading, s: int) -> float:
    """loading >= 0 and finite; 0 only with one source (bin 0 of G is the singular all-ones matrix otherwise)"""
    loading = float(loading)
    if not np.isfinite(loading) or loading < 0:
        raise ValueError("loading must be finite and >= 0")
    if loading == 0 and s > 1:
        raise ValueError("loading 0 is for one source only: bin 0 of the steering matrix's Gram matrix is singular")
    return loading


def separate(frames, fs, delays, gains, loading=0.01) -> np.ndarray:
    """frames[B][M][L], delays / gains[B][S][M] -> out[B][S][L]: the null-steering beams (the rule in the module's docstring, m
    ascending, the solve in solve_loaded's order).  A source without gains has the diagonal delta, or 1 where delta is 0 too: its
    row and column of G are zeros, so the value only keeps the factor finite."""
    x, d, g = _tables(frames, delays, gains)
    b, s, _ = d.shape
    loading = check_loading(loading, s)
    length = x.shape[2]
    spec = np.fft.fft(x, n=2 * length, axis=-1)                                 # [B][M][2L]
    f = np.fft.fftfreq(2 * length, d=1.0 / fs)
    y = np.zeros((b, s, 2 * length), dtype=np.complex128)
    gram = np.zeros((b, s, s, 2 * length), dtype=np.complex128)
    q = np.zeros((b, s))
    for m in range(x.shape[1]):
        phase = np.exp(-1j * 2 * np.pi * f[None, None, :] * d[:, :, m, None])
        product = spec[:, None, m, :] * phase
        y = y + g[:, :, m, None] * product
        q = q + g[:, :, m] * g[:, :, m]
        for i in range(s):
            for t in range(i):
                gram[:, i, t] = gram[:, i, t] + (g[:, i, m] * g[:, t, m])[:, None] * (phase[:, i] * np.conj(phase[:, t]))
    delta = loading * np.max(q, axis=1)                                         # [B]
    diag = q + delta[:, None]
    diag = np.where(diag == 0.0, 1.0, diag)
    z = solve_loaded(np.moveaxis(diag, 0, 1)[:, :, None], np.moveaxis(gram, 0, 2), np.moveaxis(y, 0, 1))   # [S][B][2L]
    return np.fft.ifft(np.moveaxis(z, 0, 1), axis=-1).real[..., :length] * fade_window(length)


def check_mvdr(loading, b: int, groups: int) -> tuple[float, int]:
    """loading finite and > 0 (with fewer snapshots than microphones it is what makes the factor exist); groups >= 1 divides b"""
    loading = float(loading)
    if not np.isfinite(loading) or loading <= 0:
        raise ValueError("loading must be finite and > 0")
    groups = int(groups)
    if groups < 1 or b % groups:
        raise ValueError("groups must be >= 1 and divide the number of frames")
    return loading, groups


def _mvdr_tables(frames, delays, gains, groups):
    x = np.asarray(frames, dtype=np.float64)
    d = np.asarray(delays, dtype=np.float64)
    g = np.asarray(gains, dtype=np.float64)
    if x.ndim != 3:
        raise ValueError("frames must be [B][M][L]")
    if d.ndim != 3 or d.shape != g.shape or d.shape[0] != groups or d.shape[2] != x.shape[1]:
        raise ValueError("delays and gains must be [G][S][M] matching frames[B][M][L] in G groups")
    return x, d, g


def mvdr_covariance(frames, groups=1) -> np.ndarray:
    """frames[B][M][L] in G groups of Q = B / G consecutive frames -> R[G][M][M][2L] complex: the lower triangle (j <= i) of the
    groups' sample covariances per bin, R[i,j] = sum_b X[b,i] conj(X[b,j]) over the group's frames b ascending, the products written
    out ((a+jb) conj(c+jd) = (ac + bd) + j(bc - ad), each bracket formed first, then added); the diagonal is real, j > i stays 0."""
    x = np.asarray(frames, dtype=np.float64)
    if x.ndim != 3:
        raise ValueError("frames must be [B][M][L]")
    b, m, length = x.shape
    groups = int(groups)
    if groups < 1 or b % groups:
        raise ValueError("groups must be >= 1 and divide the number of frames")
    q = b // groups
    spec = np.fft.fft(x, n=2 * length, axis=-1).reshape(groups, q, m, 2 * length)
    re, im = spec.real, spec.imag
    rre = np.zeros((groups, m, m, 2 * length))
    rim = np.zeros((groups, m, m, 2 * length))
    for i in range(m):
        for t in range(q):
            a, bb = re[:, t, i, None], im[:, t, i, None]                        # [G][1][2L] against columns 0 .. i
            c, dd = re[:, t, : i + 1], im[:, t, : i + 1]
            rre[:, i, : i + 1] = rre[:, i, : i + 1] + (a * c + bb * dd)
            rim[:, i, : i + 1] = rim[:, i, : i + 1] + (bb * c - a * dd)
    return rre + 1j * rim


def mvdr_weights(frames, fs, delays, gains, loading=0.1, groups=1) -> np.ndarray:
    """frames[B][M][L], delays / gains[G][S][M] -> w[G][S][M][2L]: the MVDR weights of every group, source and bin (the rule in
    ``mvdr``'s docstring): w = R~^-1 a / (a^H R~^-1 a) with R~ the group's covariance under the loading ``loading * tr(R) / M``."""
    loading, groups = check_mvdr(loading, np.shape(frames)[0] if np.ndim(frames) == 3 else 0, groups)
    x, d, g = _mvdr_tables(frames, delays, gains, groups)
    m, length = x.shape[1], x.shape[2]
    s = d.shape[1]
    r = mvdr_covariance(x, groups)
    lre = np.ascontiguousarray(np.moveaxis(r.real, 0, 2))                       # [M][M][G][2L]
    lim = np.ascontiguousarray(np.moveaxis(r.imag, 0, 2))
    tr = np.zeros(lre.shape[2:])
    for i in range(m):
        tr = tr + lre[i, i]
    delta = loading * (tr / m)
    rinv = np.empty((m,) + tr.shape)
    for j in range(m):                                                          # the factor, column by column (solve_loaded's order)
        dg = lre[j, j] + delta
        sj = np.where(dg == 0.0, 1.0, dg)
        for k in range(j):
            sj = sj - (lre[j, k] * lre[j, k] + lim[j, k] * lim[j, k])
        rinv[j] = 1.0 / np.sqrt(sj)
        if j + 1 < m:
            vre, vim = lre[j + 1:, j], lim[j + 1:, j]                           # rows i > j at once: each keeps its own k-ascending sum
            for k in range(j):
                a, b, c, dd = lre[j + 1:, k], lim[j + 1:, k], lre[j, k], lim[j, k]
                vre = vre - (a * c + b * dd)
                vim = vim - (b * c - a * dd)
            lre[j + 1:, j] = vre * rinv[j]
            lim[j + 1:, j] = vim * rinv[j]
    f = np.fft.fftfreq(2 * length, d=1.0 / fs)
    ure = np.empty((m, groups, s, 2 * length))
    uim = np.empty_like(ure)
    for i in range(m):                                                          # a, then u = L^-1 a
        p = np.exp(-1j * 2 * np.pi * f[None, None, :] * d[:, :, i, None])       # [G][S][2L]
        vre, vim = g[:, :, i, None] * p.real, g[:, :, i, None] * (-p.imag)      # a = gains * conj(p)
        for k in range(i):
            a, b, c, dd = lre[i, k][:, None], lim[i, k][:, None], ure[k], uim[k]
            vre = vre - (a * c - b * dd)
            vim = vim - (a * dd + b * c)
        ure[i] = vre * rinv[i][:, None]
        uim[i] = vim * rinv[i][:, None]
    den = np.zeros(ure.shape[1:])
    for i in range(m):
        den = den + (ure[i] * ure[i] + uim[i] * uim[i])
    den = np.where(den == 0.0, 1.0, den)
    for i in range(m - 1, -1, -1):                                              # z = L^-H u in place
        vre, vim = ure[i], uim[i]
        for k in range(i + 1, m):
            a, b, c, dd = lre[k, i][:, None], lim[k, i][:, None], ure[k], uim[k]
            vre = vre - (a * c + b * dd)
            vim = vim - (a * dd - b * c)
        ure[i] = vre * rinv[i][:, None]
        uim[i] = vim * rinv[i][:, None]
    return np.moveaxis(ure / den + 1j * (uim / den), 0, 2)                      # [G][S][M][2L]


def mvdr(frames, fs, delays, gains, loading=0.1, groups=1) -> np.ndarray:
    """frames[B][M][L], delays / gains[G][S][M] -> out[B][S][L]: the minimum-variance distortionless-response beams.  B = G Q; group g
    is the Q consecutive frames g Q .. g Q + Q - 1, the snapshots of one covariance under one steering table.  Per group and bin of
    the 2L-point spectrum, with steer's X and f::

        R[i,j]  = sum over the group's frames b ascending of  X[b,i] * conj(X[b,j])              for j <= i   (diagonal real)
        tr      = sum over i ascending of R[i,i]
        delta   = loading * (tr / M)                          (per bin: the weights do not depend on the data's scale)
        diag[i] = R[i,i] + delta,  1 where that is 0          (a silent bin)
        L       = lower Cholesky factor of (R with that diagonal), solve_loaded's column order and spelled-out products
        a[m]    = gains[g,s,m] * conj(p[s,m]),   p[s,m] = exp(-1j*2*pi*f*delays[g,s,m])          (separate's steering vector)
        u       = L^-1 a  (forward substitution, k ascending);   den = sum over i ascending of |u[i]|^2,  1 where that is 0
        w       = L^-H u / den  (back substitution, k ascending)                                 (w = R~^-1 a / (a^H R~^-1 a))
        Y[b,s]  = sum over m ascending of conj(w[m]) * X[b,m]                                    for every frame b of the group
        out[b,s] = ifft(Y[b,s]).real[:L] * fade_window(L)

    Consequences: ``w(-f) = conj(w(f))``, so L + 1 bins carry everything.  Beams and groups do not see each other.  A group scaled by a
    power of two gives its output times that power (2^+-40: byte for byte).  A source without gains is a row of exact zeros, and so
    is a zero frame in a live group.  ``|w|_2 <= kappa / |a|_2`` with ``kappa = M / loading + 1``, and as loading -> inf the beam
    tends to ``steer(frames, fs, delays, gains / q)``, ``q = sum_m gains^2``, within ``2 M / loading`` of steer's scale."""
    w = mvdr_weights(frames, fs, delays, gains, loading, groups)
    x = np.asarray(frames, dtype=np.float64)
    b, m, length = x.shape
    groups = w.shape[0]
    q = b // groups
    spec = np.fft.fft(x, n=2 * length, axis=-1).reshape(groups, q, 1, m, 2 * length)
    xr, xi = spec.real, spec.imag
    wr, wi = w.real[:, None], w.imag[:, None]                                   # [G][1][S][M][2L]
    yre = np.zeros((groups, q, w.shape[1], 2 * length))
    yim = np.zeros_like(yre)
    for i in range(m):
        yre = yre + (wr[:, :, :, i] * xr[:, :, :, i] + wi[:, :, :, i] * xi[:, :, :, i])
        yim = yim + (wr[:, :, :, i] * xi[:, :, :, i] - wi[:, :, :, i] * xr[:, :, :, i])
    y = (yre + 1j * yim).reshape(b, w.shape[1], 2 * length)
    return np.fft.ifft(y, axis=-1).real[..., :length] * fade_window(length)


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
