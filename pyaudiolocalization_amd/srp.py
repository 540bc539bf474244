"""Steered-response power (SRP-PHAT) map: the device rule (csrc/srp.hip, csrc/srp_math.h, pal_gcc_phat_all_pairs_strips*, pal_srp_map*,
pal_srp_peaks*) in NumPy.

For every candidate position the map sums, over all microphone pairs, the pair's GCC-PHAT row at the lag that position predicts.  It
uses the whole row and picks no peak per pair, so a wrong first peak of some pairs costs a little power and nothing else, the table's
index mapping plays no part, and several sources show as several maxima.  Conventions:

- the row of pair p = (i, j), i < j (row-major over pairs), is the circular correlation of n = 2L - 1 samples with zero lag at index 0;
  it peaks at the circular lag d_i - d_j.  Everything here uses the centred lag s = d_j - d_i in samples, the sign of closure.py and
  consensus.py: ``raw[p][u] = row_p[(-u) mod n]`` for |u| <= L - 1;
- a **strip** of half-width T keeps ``raw[p][-T .. T]`` (``out[p][T + s]``), smoothed by a triangle of half-width W: a PHAT peak is one
  sample wide and a grid cell spans many samples of lag, so without smoothing the map's maximum is decided by which cell centre happens
  to hit a sample;
- a grid has ``count[a]`` cells per axis over the box ``lo .. hi``; the point of cell (ix, iy, iz) is the cell's centre and its linear
  index is ``g = (ix * ny + iy) * nz + iz``;
- ``power[g] = sum_p w_p * strips[p][T + s(g, p)]`` with ``s(g, p) = rint(((d_j - d_i) * fs) / c)``; a term with ``|s| > T`` is clipped: it
  contributes nothing and is counted;
- a cell is a **peak** iff no cell of its (2R+1)^3 neighbourhood, cut at the grid's border, is higher, and among equal cells of that
  neighbourhood it has the lowest linear index; a NaN cell is no peak and hides none.  Peaks are ordered by power descending, then by
  index.

Every product is rounded before it is added (no fused multiply-add), square root and division are correctly rounded and rint rounds
half to even, so the device's grid points, lags, clip decisions, smoothing sums and peak marks equal these bit for bit.  The order of
the map's sum over pairs is the kernel's own: the map is compared exactly where the terms are integers, and within the bound of
``srp_map(..., return_abs=True)`` otherwise.
"""
from __future__ import annotations

import numpy as np

from ._ffi import SRP_FRAME as FRAME                                   # pal_srp_frame
from ._ffi import SRP_MAX_PEAKS as MAX_PEAKS
from ._ffi import SRP_MAX_RADIUS as MAX_RADIUS
from ._ffi import SRP_MAX_SMOOTH as MAX_SMOOTH
from ._ffi import SRP_PEAK as PEAK                                      # pal_srp_peak

MAX_COUNT = 1024                                                        # cells per axis
MAX_CELLS = 1 << 24


def _mics(mics) -> np.ndarray:
    m = np.ascontiguousarray(mics, dtype=np.float64)
    if m.ndim != 2 or m.shape[1] != 3 or m.shape[0] < 2:
        raise ValueError("mics must be [M][3] with M >= 2")
    return m


def check_grid(lo, hi, count):
    """-> (lo[3], hi[3] float64, count[3] int64); ValueError as pal_srp_map refuses a grid."""
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(-1), np.asarray(hi, dtype=np.float64).reshape(-1)
    count = np.asarray(count, dtype=np.int64).reshape(-1)
    if lo.shape != (3,) or hi.shape != (3,) or count.shape != (3,):
        raise ValueError("lo, hi and count have three entries each")
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))):
        raise ValueError("a grid coordinate is not finite")
    if np.any(hi <= lo):
        raise ValueError("hi must be above lo on every axis")
    if np.any(count < 1) or np.any(count > MAX_COUNT):
        raise ValueError(f"cells per axis outside 1..{MAX_COUNT}")
    if int(np.prod(count)) > MAX_CELLS:
        raise ValueError("more than 2^24 cells")
    return lo, hi, count


def half_width(mics, fs, c) -> int:
    """The strip half-width T for which no lag of any position is ever clipped: ceil(largest microphone distance * fs / c) + 1."""
    m = _mics(mics)
    d = np.sqrt(np.sum((m[:, None, :] - m[None, :, :]) ** 2, axis=2))
    return int(np.ceil(np.max(d) * float(fs) / float(c))) + 1


def raw_index(u, n):
    """Index of raw[u] in a row of n samples: (-u) mod n."""
    return np.mod(-np.asarray(u, dtype=np.int64), int(n))


def strips(rows, L: int, T: int, W: int = 0) -> np.ndarray:
    """rows[P][n] (n = 2L - 1) -> strips[P][2T + 1]: ``out[p][T + s] = sum_{u = -W..W} (W + 1 - |u|) * raw[p][s + u]`` accumulated in
    increasing u, each product rounded, the first product starting the sum.  W = 0 copies the samples."""
    r = np.asarray(rows, dtype=np.float64)
    L, T, W = int(L), int(T), int(W)
    n = 2 * L - 1
    if r.ndim != 2 or r.shape[1] != n:
        raise ValueError("rows must be [P][2L - 1]")
    if T < 0 or not 0 <= W <= MAX_SMOOTH or T + W > L - 1:
        raise ValueError("need T >= 0, 0 <= W <= 32 and T + W <= L - 1")
    s = np.arange(-T, T + 1)
    out = None
    for u in range(-W, W + 1):
        term = float(W + 1 - abs(u)) * r[:, raw_index(s + u, n)]
        out = term if out is None else out + term
    return np.ascontiguousarray(out)


def grid_points(lo, hi, count) -> np.ndarray:
    """points[G][3]: the cell centres ``lo + (i + 0.5) * step`` with ``step = (hi - lo) / count``, g = (ix * ny + iy) * nz + iz."""
    lo, hi, count = check_grid(lo, hi, count)
    axes = []
    for a in range(3):
        step = (hi[a] - lo[a]) / np.float64(count[a])
        axes.append(lo[a] + (np.arange(count[a], dtype=np.float64) + 0.5) * step)
    x, y, z = np.meshgrid(*axes, indexing="ij")
    return np.ascontiguousarray(np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1))


def distances(points, mics) -> np.ndarray:
    """d[G][M]: q = dx*dx; q = q + dy*dy; q = q + dz*dz; sqrt(q)."""
    p, m = np.asarray(points, dtype=np.float64).reshape(-1, 3), _mics(mics)
    dx, dy, dz = (p[:, None, a] - m[None, :, a] for a in range(3))
    q = dx * dx
    q = q + dy * dy
    q = q + dz * dz
    return np.sqrt(q)


def lag_quotients(points, mics, fs, c) -> np.ndarray:
    """The unrounded lags ((d_j - d_i) * fs) / c as float64 [G][P]."""
    d = distances(points, mics)
    i, j = np.triu_indices(d.shape[1], k=1)
    return ((d[:, j] - d[:, i]) * np.float64(fs)) / np.float64(c)


def lag_values(points, mics, fs, c) -> np.ndarray:
    """rint of the quotients (half to even) as float64 [G][P]: what the clip test ``not |r| <= T`` is decided on."""
    return np.rint(lag_quotients(points, mics, fs, c))


def lags(points, mics, fs, c) -> np.ndarray:
    """s[G][P] int32 (a value beyond +-2^30 enters as +-2^30: far outside every strip)."""
    return np.clip(lag_values(points, mics, fs, c), -2.0 ** 30, 2.0 ** 30).astype(np.int32)


def lag_margin(points, mics, fs, c) -> float:
    """The smallest distance of an unrounded lag from a half-integer: where it is not tiny, no rounding of the last bit of a distance can
    move a lag, whatever computes it."""
    q = lag_quotients(points, mics, fs, c)
    return float(np.min(np.abs(np.abs(q - np.floor(q)) - 0.5)))


def srp_map(strips_, T: int, mics, fs, c, lo, hi, count, pair_weights=None, return_abs=False, chunk: int = 4096):
    """strips[P][2T + 1] of one frame -> (power[G] float64, clipped int): ``power[g] = sum_p w_p * strips[p][T + s(g, p)]``, the terms in
    pair order; clipped terms contribute 0 and are counted.  ``return_abs``: also ``sum_p |w_p * strips[p][T + s]|`` per cell, the
    scale of the rounding bound for a sum taken in another order."""
    st = np.asarray(strips_, dtype=np.float64)
    m = _mics(mics)
    T = int(T)
    npairs = m.shape[0] * (m.shape[0] - 1) // 2
    if st.shape != (npairs, 2 * T + 1):
        raise ValueError("strips must be [P][2T + 1]")
    if not (fs > 0 and c > 0):
        raise ValueError("fs and c must be positive")
    w = None if pair_weights is None else np.asarray(pair_weights, dtype=np.float64).reshape(npairs)
    pts = grid_points(lo, hi, count)
    power, total = np.zeros(pts.shape[0]), np.zeros(pts.shape[0])
    clipped = 0
    rows = np.arange(npairs)[None, :]
    for g0 in range(0, pts.shape[0], int(chunk)):
        r = lag_values(pts[g0:g0 + chunk], m, fs, c)
        out = ~(np.abs(r) <= T)
        clipped += int(np.count_nonzero(out))
        s = np.where(out, 0, r).astype(np.int64)
        v = st[rows, T + s]
        if w is not None:
            v = w[None, :] * v
        v = np.where(out, 0.0, v)
        acc = np.zeros(v.shape[0])
        for p in range(npairs):                                                          # in pair order, one rounded addition each
            acc = acc + v[:, p]
        power[g0:g0 + chunk] = acc
        total[g0:g0 + chunk] = np.sum(np.abs(v), axis=1)
    return (power, clipped, total) if return_abs else (power, clipped)


def peak_marks(power, R: int) -> np.ndarray:
    """bool [nx][ny][nz]: the cells that are peaks by the neighbourhood rule."""
    p = np.asarray(power, dtype=np.float64)
    if p.ndim != 3:
        raise ValueError("power must be [nx][ny][nz]")
    R = int(R)
    if not 1 <= R <= MAX_RADIUS:
        raise ValueError(f"R outside 1..{MAX_RADIUS}")
    nx, ny, nz = p.shape
    idx = np.arange(p.size, dtype=np.int64).reshape(p.shape)
    pad = np.full((nx + 2 * R, ny + 2 * R, nz + 2 * R), np.nan)                          # NaN: neither higher nor equal
    pad[R:R + nx, R:R + ny, R:R + nz] = p
    pidx = np.full(pad.shape, np.iinfo(np.int64).max, dtype=np.int64)
    pidx[R:R + nx, R:R + ny, R:R + nz] = idx
    mark = ~np.isnan(p)
    for dx in range(2 * R + 1):
        for dy in range(2 * R + 1):
            for dz in range(2 * R + 1):
                o = pad[dx:dx + nx, dy:dy + ny, dz:dz + nz]
                oi = pidx[dx:dx + nx, dy:dy + ny, dz:dz + nz]
                mark &= ~((o > p) | ((o == p) & (oi < idx)))
    return mark


def map_peaks(power, K: int, R: int, lo=None, hi=None):
    """power[nx][ny][nz] -> peaks[K] of PEAK: the first K peaks by power descending, then index; absent entries have index -1 and all
    else 0.  With ``lo`` and ``hi`` the records carry the cells' centres, otherwise x = y = z = 0."""
    p = np.asarray(power, dtype=np.float64)
    K = int(K)
    if not 1 <= K <= MAX_PEAKS:
        raise ValueError(f"K outside 1..{MAX_PEAKS}")
    mark = peak_marks(p, R).reshape(-1)
    flat = p.reshape(-1)
    cand = np.flatnonzero(mark)
    order = cand[np.lexsort((cand, -flat[cand]))][:K]
    out = np.zeros(K, dtype=PEAK)
    out["index"] = -1
    out["index"][:order.shape[0]] = order
    out["power"][:order.shape[0]] = flat[order]
    if lo is not None:
        pts = grid_points(lo, hi, p.shape)
        for a, name in enumerate("xyz"):
            out[name][:order.shape[0]] = pts[order, a]
    return out
