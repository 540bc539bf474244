"""Steered-response power (SRP-PHAT) map: the device rule (csrc/srp.hip, csrc/srp_math.h, pal_gcc_phat_all_pairs_strips*, pal_srp_map*,
pal_srp_peaks*, pal_srp_zoom*) in NumPy.

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
  index;
- the map is piecewise constant in space (``rint`` picks one sample), so below about c / fs a finer grid finds plateaus.  The **zoom**
  (``zoom``) refines a peak with a continuous rule instead: the strip read at the fractional lag with linear interpolation, over small
  boxes that shrink around the best cell, the terms added in the fixed order ``tile_order``;
- the **direction map** (``doa_map``, ``doa_peaks``, ``doa_zoom``; pal_srp_doa*, csrc/srp.hip) sums the same strips over a grid of
  azimuth and elevation under the plane-wave model, for arrays that resolve direction and not range: see the section at the end.

Every product is rounded before it is added (no fused multiply-add), square root and division are correctly rounded and rint rounds
half to even, so the device's grid points, lags, clip decisions, smoothing sums and peak marks equal these bit for bit.  The order of
the map's sum over pairs is the kernel's own: the map is compared exactly where the terms are integers, and within the bound of
``srp_map(..., return_abs=True)`` otherwise.
"""
from __future__ import annotations

import numpy as np

from ._ffi import SRP_FRAME as FRAME                                   # pal_srp_frame
from ._ffi import SRP_MAX_DOA_COUNT as MAX_DOA_COUNT                   # azimuths, and elevations, of a direction grid
from ._ffi import SRP_MAX_PEAKS as MAX_PEAKS
from ._ffi import SRP_MAX_RADIUS as MAX_RADIUS
from ._ffi import SRP_MAX_SMOOTH as MAX_SMOOTH
from ._ffi import SRP_MAX_ZOOM_CELLS as MAX_ZOOM_CELLS
from ._ffi import SRP_MAX_ZOOM_LEVELS as MAX_ZOOM_LEVELS
from ._ffi import SRP_PEAK as PEAK                                      # pal_srp_peak
from ._ffi import SRP_ZOOM as ZOOM                                      # pal_srp_zoom_record

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


def tile_order(M: int) -> np.ndarray:
    """The pair indices (row-major over i < j) in the order k_srp_map and k_srp_zoom add their terms: microphone tiles of 16, the loops
    nested (ti, tj >= ti, i in tile ti, j in tile tj, j > i).  For M <= 16 it is pair order."""
    M = int(M)
    if M < 2:
        raise ValueError("M >= 2")
    tiles = (M + 15) // 16
    out = []
    for ti in range(tiles):
        for tj in range(ti, tiles):
            for i in range(16 * ti, min(16 * ti + 16, M - 1)):
                row0 = i * M - i * (i + 1) // 2 - i - 1
                out.extend(row0 + j for j in range(max(16 * tj, i + 1), min(16 * tj + 16, M)))
    return np.asarray(out, dtype=np.int64)


def zoom_terms(strips_, T: int, points, mics, fs, c, pair_weights=None):
    """The zoom's terms of every point: (v[G][P] with 0 where clipped, out[G][P] bool: clipped, q, k, f [G][P]).  For pair p = (i, j):
    ``q = ((d_j - d_i) * fs) / c``, ``k = floor(q)``, ``f = q - k``; clipped iff not (k >= -T and k <= T - 1), decided on the doubles;
    otherwise ``v = s0 + f * (s1 - s0)`` with ``s0 = strips[p][T + k]``, ``s1 = strips[p][T + k + 1]`` (the product rounded before the
    addition), then ``v = w_p * v``."""
    return terms_at(strips_, T, lag_quotients(points, mics, fs, c), pair_weights)


def terms_at(strips_, T: int, q, pair_weights=None):
    """``zoom_terms`` from the quotients q[G][P] themselves, wherever they come from."""
    st = np.asarray(strips_, dtype=np.float64)
    T = int(T)
    with np.errstate(invalid="ignore"):
        k = np.floor(q)
        f = q - k
        out = ~((k >= -T) & (k <= T - 1))
    at = np.where(out, 0, k).astype(np.int64) + T
    rows = np.arange(st.shape[0])[None, :]
    s0, s1 = st[rows, at], st[rows, at + 1]                                                      # at <= 2T - 1: T >= 1
    with np.errstate(invalid="ignore", over="ignore"):
        v = s0 + np.where(out, 0.0, f) * (s1 - s0)
        if pair_weights is not None:
            v = np.asarray(pair_weights, dtype=np.float64).reshape(1, -1) * v
    return np.where(out, 0.0, v), out, q, k, f


def zoom_box(ctr, half):
    """-> (lo[3], hi[3]) of a level: ctr - half, ctr + half."""
    ctr, half = np.asarray(ctr, dtype=np.float64), np.asarray(half, dtype=np.float64)
    return ctr - half, ctr + half


def zoom_next_half(lo, hi, Z: int) -> np.ndarray:
    """The next level's half-extent: one cell of this level, (hi - lo) / Z."""
    return (np.asarray(hi, dtype=np.float64) - np.asarray(lo, dtype=np.float64)) / np.float64(int(Z))


def zoom_level(strips_, T: int, mics, fs, c, ctr, half, Z: int, pair_weights=None, order=None):
    """One level -> (power[Z^3], clipped, best index or -1, points[Z^3][3]).  The terms are added in ``tile_order``; the best cell is the
    first by (power descending, index ascending) among the cells that are not NaN."""
    lo, hi = zoom_box(ctr, half)
    with np.errstate(invalid="ignore", over="ignore"):
        step = [(hi[a] - lo[a]) / np.float64(Z) for a in range(3)]
        axes = [lo[a] + (np.arange(Z, dtype=np.float64) + 0.5) * step[a] for a in range(3)]
    # grid_points' arithmetic without its checks: after many levels a box collapses to a point (hi == lo), and that is still a level
    x, y, z = np.meshgrid(*axes, indexing="ij")
    pts = np.ascontiguousarray(np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1))
    with np.errstate(invalid="ignore", over="ignore"):
        v, out, _, _, _ = zoom_terms(strips_, T, pts, mics, fs, c, pair_weights)
        acc = np.zeros(pts.shape[0])
        for p in (tile_order(np.asarray(mics).shape[0]) if order is None else order):
            acc = acc + v[:, p]                            # v is 0.0 where clipped, and acc is never -0.0: adding it adds nothing
    ok = ~np.isnan(acc)
    best = -1
    if np.any(ok):
        best = int(np.flatnonzero(ok & (acc == np.max(acc[ok])))[0])
    return acc, int(np.count_nonzero(out)), best, pts


def zoom(strips_, T: int, mics, fs, c, seeds, half0, Z: int = 8, levels: int = 3, pair_weights=None, return_levels=False):
    """strips[P][2T + 1] of one frame and seeds[K] of PEAK -> out[K] of ZOOM: a coarse-to-fine search around every seed with a continuous
    rule, the strip read at the fractional lag with linear interpolation (``zoom_terms``).

    A level has a centre and a half-extent per axis; its Z^3 points are ``grid_points(ctr - half, ctr + half, (Z, Z, Z))`` (the same
    arithmetic and linear index; a box that many levels have shrunk to a point is still a level: every cell ties, index 0 wins).  Level 0:
    the seed's (x, y, z) and ``half0[3]`` in metres.  The next level has the best cell's centre and the half-extent ``(hi - lo) / Z``,
    one cell: its box covers the best cell and half of each neighbour, and extents shrink by Z / 2 per level.  Where every cell of a
    level is NaN the zoom stops: the record keeps the centre that level started from, ``power`` = NaN and ``levels`` = the levels
    completed before it.  ``clipped`` counts the clipped terms over all cells of all levels run.  A seed with ``index < 0`` is absent:
    ``seed`` = -1 and all else 0.

    The order of the sum, ``tile_order``, is part of the rule: the device equals this byte for byte on any strips, so a last-bit
    difference can never send the two down different paths.  ``T = half_width(...)`` still clips nothing: |q| <= T - 1 gives
    -(T - 1) <= k <= T - 1.  ``return_levels``: also, per seed, the list of (centre[3], power) after every completed level."""
    st = np.asarray(strips_, dtype=np.float64)
    m = _mics(mics)
    T, Z, levels = int(T), int(Z), int(levels)
    npairs = m.shape[0] * (m.shape[0] - 1) // 2
    if T < 1 or st.shape != (npairs, 2 * T + 1):
        raise ValueError("strips must be [P][2T + 1] with T >= 1")
    if not (fs > 0 and c > 0):
        raise ValueError("fs and c must be positive")
    if not 2 <= Z <= MAX_ZOOM_CELLS or not 1 <= levels <= MAX_ZOOM_LEVELS:
        raise ValueError(f"need Z in 2..{MAX_ZOOM_CELLS} and levels in 1..{MAX_ZOOM_LEVELS}")
    half0 = np.asarray(half0, dtype=np.float64).reshape(-1)
    if half0.shape != (3,) or not np.all(np.isfinite(half0)) or np.any(half0 <= 0):
        raise ValueError("half0 has three finite positive entries")
    sd = np.asarray(seeds, dtype=PEAK).reshape(-1)
    if not 1 <= sd.shape[0] <= MAX_PEAKS:
        raise ValueError(f"K outside 1..{MAX_PEAKS}")
    w = None if pair_weights is None else np.asarray(pair_weights, dtype=np.float64).reshape(npairs)
    order = tile_order(m.shape[0])
    out = np.zeros(sd.shape[0], dtype=ZOOM)
    trail = []
    for n, seed in enumerate(sd):
        trail.append([])
        if seed["index"] < 0:
            out[n]["seed"] = -1
            continue
        ctr, half = np.array([seed["x"], seed["y"], seed["z"]], dtype=np.float64), half0.copy()
        power, done, clipped = np.float64(0.0), 0, 0
        for _ in range(levels):
            acc, clip, best, pts = zoom_level(st, T, m, fs, c, ctr, half, Z, w, order)
            clipped += clip
            if best < 0:
                power = np.float64(np.nan)
                break
            lo, hi = zoom_box(ctr, half)
            with np.errstate(invalid="ignore", over="ignore"):
                ctr, half, power = pts[best].copy(), zoom_next_half(lo, hi, Z), acc[best]
            done += 1
            trail[-1].append((ctr.copy(), float(power)))
        out[n] = (ctr[0], ctr[1], ctr[2], power, clipped, seed["index"], done)
    return (out, trail) if return_levels else out


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


# ---- the direction map: far-field azimuth / elevation power, its peaks and a zoom on the sphere (pal_srp_doa*) -------------------
# The arrays this project runs on resolve direction, not range: everything the map can know about a far source lies on the sphere
# of directions.  A source far away in the direction u reaches microphone m earlier than the origin by the advance a_m = u . m, so
# d_j - d_i = a_i - a_j and the lag of pair (i, j) is rint(((a_i - a_j) * fs) / c).  The device evaluates no sine: the grid is two host
# tables of (cos, sin), and the zoom works in the tangent plane of its centre.  The terms of every sum are added in ``tile_order``, so
# the device equals these functions byte for byte on any strips.
def doa_axes(n_az: int, n_el: int, az_lo=0.0, az_hi=2.0 * np.pi, el_lo=-0.5 * np.pi, el_hi=0.5 * np.pi):
    """-> (az[n_az][2], el[n_el][2], wrap): (cos, sin) of the cell centres ``lo + (i + 0.5) * ((hi - lo) / n)`` of both axes, in radians.
    ``wrap`` = 1 iff the azimuths span the full circle; with the default limits no cell centre sits on a pole."""
    n_az, n_el = int(n_az), int(n_el)
    if not (1 <= n_az <= MAX_DOA_COUNT and 1 <= n_el <= MAX_DOA_COUNT):
        raise ValueError(f"n_az and n_el outside 1..{MAX_DOA_COUNT}")
    lim = np.asarray([az_lo, az_hi, el_lo, el_hi], dtype=np.float64)
    if not np.all(np.isfinite(lim)) or not (lim[1] > lim[0] and lim[3] > lim[2]):
        raise ValueError("need finite limits with hi above lo")
    out = []
    for lo, hi, n in ((lim[0], lim[1], n_az), (lim[2], lim[3], n_el)):
        a = lo + (np.arange(n, dtype=np.float64) + 0.5) * ((hi - lo) / np.float64(n))
        out.append(np.ascontiguousarray(np.stack([np.cos(a), np.sin(a)], axis=1)))
    return out[0], out[1], int(abs((lim[1] - lim[0]) - 2.0 * np.pi) <= 1e-12)


def check_doa_tables(az, el):
    """-> (az[n_az][2], el[n_el][2]) float64; ValueError as pal_srp_doa refuses them."""
    az, el = np.ascontiguousarray(az, dtype=np.float64), np.ascontiguousarray(el, dtype=np.float64)
    if az.ndim != 2 or el.ndim != 2 or az.shape[1] != 2 or el.shape[1] != 2:
        raise ValueError("az must be [n_az][2] and el [n_el][2]: (cos, sin)")
    if not (1 <= az.shape[0] <= MAX_DOA_COUNT and 1 <= el.shape[0] <= MAX_DOA_COUNT):
        raise ValueError(f"n_az and n_el outside 1..{MAX_DOA_COUNT}")
    if not (np.all(np.isfinite(az)) and np.all(np.isfinite(el))):
        raise ValueError("a direction table entry is not finite")
    return az, el


def doa_directions(az, el) -> np.ndarray:
    """u[G][3], g = ia * n_el + ie: ux = ce * ca, uy = ce * sa, uz = se."""
    az, el = check_doa_tables(az, el)
    ca, sa, ce, se = az[:, None, 0], az[:, None, 1], el[None, :, 0], el[None, :, 1]
    u = np.stack([ce * ca, ce * sa, np.broadcast_to(se, (az.shape[0], el.shape[0]))], axis=2)
    return np.ascontiguousarray(u.reshape(-1, 3))


def doa_advances(directions, mics) -> np.ndarray:
    """a[G][M]: a = ux*mx; a = a + uy*my; a = a + uz*mz."""
    u, m = np.asarray(directions, dtype=np.float64).reshape(-1, 3), _mics(mics)
    with np.errstate(invalid="ignore", over="ignore"):
        a = u[:, None, 0] * m[None, :, 0]
        a = a + u[:, None, 1] * m[None, :, 1]
        a = a + u[:, None, 2] * m[None, :, 2]
    return a


def doa_lag_quotients(directions, mics, fs, c) -> np.ndarray:
    """The unrounded lags ((a_i - a_j) * fs) / c as float64 [G][P]."""
    a = doa_advances(directions, mics)
    i, j = np.triu_indices(a.shape[1], k=1)
    with np.errstate(invalid="ignore", over="ignore"):
        return ((a[:, i] - a[:, j]) * np.float64(fs)) / np.float64(c)


def doa_lag_margin(directions, mics, fs, c) -> float:
    """``lag_margin`` of the direction map's lags."""
    q = doa_lag_quotients(directions, mics, fs, c)
    return float(np.min(np.abs(np.abs(q - np.floor(q)) - 0.5)))


def _sum_in_tile_order(v, M):
    acc = np.zeros(v.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for p in tile_order(M):
            acc = acc + v[:, p]                                # v is 0.0 where clipped, and acc is never -0.0: adding it adds nothing
    return acc


def doa_map(strips_, T: int, mics, fs, c, az, el, pair_weights=None):
    """strips[P][2T + 1] of one frame -> (power[G] float64, clipped int), G = n_az * n_el: ``power[g] = sum_p w_p * strips[p][T + s]``
    with ``s = rint(((a_i - a_j) * fs) / c)`` (half to even), the terms added in ``tile_order``; a term with not |s| <= T is clipped:
    it adds nothing and is counted.  ``T = half_width(...)`` clips nothing for unit directions: |a_i - a_j| <= |m_i - m_j|."""
    st = np.asarray(strips_, dtype=np.float64)
    m = _mics(mics)
    T = int(T)
    npairs = m.shape[0] * (m.shape[0] - 1) // 2
    if T < 0 or st.shape != (npairs, 2 * T + 1):
        raise ValueError("strips must be [P][2T + 1]")
    if not (fs > 0 and c > 0):
        raise ValueError("fs and c must be positive")
    r = np.rint(doa_lag_quotients(doa_directions(az, el), m, fs, c))
    out = ~(np.abs(r) <= T)
    v = st[np.arange(npairs)[None, :], T + np.where(out, 0, r).astype(np.int64)]
    with np.errstate(invalid="ignore", over="ignore"):
        if pair_weights is not None:
            v = np.asarray(pair_weights, dtype=np.float64).reshape(1, npairs) * v
    return _sum_in_tile_order(np.where(out, 0.0, v), m.shape[0]), int(np.count_nonzero(out))


def doa_peak_marks(power, R: int, wrap) -> np.ndarray:
    """bool [n_az][n_el]: cell (ia, ie) is a peak iff it is not NaN and no cell at offsets (da, de) in -R .. R is higher, or equal with
    a lower linear index.  Elevation is cut at the border; azimuth is taken mod n_az when ``wrap`` and cut otherwise."""
    p = np.asarray(power, dtype=np.float64)
    if p.ndim != 2:
        raise ValueError("power must be [n_az][n_el]")
    R = int(R)
    if not 1 <= R <= MAX_RADIUS:
        raise ValueError(f"R outside 1..{MAX_RADIUS}")
    n_az, n_el = p.shape
    idx = np.arange(p.size, dtype=np.int64).reshape(p.shape)
    rows = np.arange(n_az)
    mark = ~np.isnan(p)
    for da in range(-R, R + 1):
        at = rows + da
        inside = np.ones(n_az, dtype=bool) if wrap else (at >= 0) & (at < n_az)
        at = np.mod(at, n_az)
        for de in range(-R, R + 1):
            o = np.full(p.shape, np.nan)                                                 # NaN: neither higher nor equal
            oi = np.zeros(p.shape, dtype=np.int64)
            e0, e1 = max(0, -de), min(n_el, n_el - de)                                   # the cells whose ie + de is inside
            if e0 < e1:
                o[:, e0:e1] = np.where(inside[:, None], p[at][:, e0 + de:e1 + de], np.nan)
                oi[:, e0:e1] = idx[at][:, e0 + de:e1 + de]
            mark &= ~((o > p) | ((o == p) & (oi < idx)))
    return mark


def doa_peaks(power, K: int, R: int, wrap, az=None, el=None):
    """power[n_az][n_el] -> peaks[K] of PEAK: the first K peaks by power descending, then index; absent entries have index -1 and all
    else 0.  With the tables the records carry the cells' directions, otherwise x = y = z = 0."""
    p = np.asarray(power, dtype=np.float64)
    K = int(K)
    if not 1 <= K <= MAX_PEAKS:
        raise ValueError(f"K outside 1..{MAX_PEAKS}")
    mark = doa_peak_marks(p, R, wrap).reshape(-1)
    flat = p.reshape(-1)
    cand = np.flatnonzero(mark)
    order = cand[np.lexsort((cand, -flat[cand]))][:K]
    out = np.zeros(K, dtype=PEAK)
    out["index"] = -1
    out["index"][:order.shape[0]] = order
    out["power"][:order.shape[0]] = flat[order]
    if az is not None:
        u = doa_directions(az, el)
        if u.shape[0] != p.size:
            raise ValueError("the tables do not match the map")
        for a, name in enumerate("xyz"):
            out[name][:order.shape[0]] = u[order, a]
    return out


def _norm3(x, y, z):
    q = x * x
    q = q + y * y
    q = q + z * z
    return np.sqrt(q)


def doa_basis(u):
    """-> (k, e1[3], e2[3]): the tangent basis of a level's centre.  k is the coordinate axis of the smallest |u_k|, the lowest axis
    winning ties (a NaN is never smaller); ``e1 = (k x u) / |k x u|``: two copies or negations and a zero, each divided by the norm
    ``q = ex*ex; q = q + ey*ey; q = q + ez*ez; sqrt(q)``; ``e2 = u x e1``, each component p1 - p2 of two rounded products."""
    u = np.asarray(u, dtype=np.float64).reshape(3)
    k, m = 0, abs(u[0])
    if abs(u[1]) < m:
        k, m = 1, abs(u[1])
    if abs(u[2]) < m:
        k = 2
    zero = np.float64(0.0)
    e = ((zero, -u[2], u[1]), (u[2], zero, -u[0]), (-u[1], u[0], zero))[k]
    with np.errstate(all="ignore"):
        n = _norm3(*e)
        e1 = np.array([e[0] / n, e[1] / n, e[2] / n])
        e2 = np.array([u[1] * e1[2] - u[2] * e1[1], u[2] * e1[0] - u[0] * e1[2], u[0] * e1[1] - u[1] * e1[0]])
    return k, e1, e2


def doa_zoom_offsets(half, Z: int) -> np.ndarray:
    """off[Z]: the cell centres of -half .. half, ``-half + (i + 0.5) * ((half - (-half)) / Z)``."""
    half = np.float64(half)
    with np.errstate(all="ignore"):
        return -half + (np.arange(int(Z), dtype=np.float64) + 0.5) * ((half - (-half)) / np.float64(int(Z)))


def doa_zoom_points(u, half, Z: int) -> np.ndarray:
    """points[Z^2][3], cell (i, j) at index i * Z + j: ``v = u + off_i * e1`` per component, then ``v = v + off_j * e2``, then ``v / |v|``."""
    u = np.asarray(u, dtype=np.float64).reshape(3)
    _, e1, e2 = doa_basis(u)
    off = doa_zoom_offsets(half, Z)
    oi, oj = np.meshgrid(off, off, indexing="ij")
    with np.errstate(all="ignore"):
        v = [u[a] + oi * e1[a] for a in range(3)]
        v = [v[a] + oj * e2[a] for a in range(3)]
        n = _norm3(*v)
        return np.ascontiguousarray(np.stack([(v[a] / n).reshape(-1) for a in range(3)], axis=1))


def doa_zoom_next_half(half, Z: int):
    """The next level's half-extent: one cell of this level, (half - (-half)) / Z."""
    half = np.float64(half)
    with np.errstate(all="ignore"):
        return (half - (-half)) / np.float64(int(Z))


def doa_zoom_level(strips_, T: int, mics, fs, c, u, half, Z: int, pair_weights=None):
    """One level -> (power[Z^2], clipped, best index or -1, points[Z^2][3]): the power of a point sums ``terms_at`` on the quotients
    ``((a_i - a_j) * fs) / c`` of the point's advances in ``tile_order``; the best cell is the first by (power descending, index
    ascending) among the cells that are not NaN."""
    pts = doa_zoom_points(u, half, Z)
    v, out, _, _, _ = terms_at(strips_, T, doa_lag_quotients(pts, mics, fs, c), pair_weights)
    acc = _sum_in_tile_order(v, np.asarray(mics).shape[0])
    ok = ~np.isnan(acc)
    best = int(np.flatnonzero(ok & (acc == np.max(acc[ok])))[0]) if np.any(ok) else -1
    return acc, int(np.count_nonzero(out)), best, pts


def doa_zoom(strips_, T: int, mics, fs, c, seeds, half0, Z: int = 8, levels: int = 3, pair_weights=None, return_levels=False):
    """strips[P][2T + 1] of one frame and seeds[K] of PEAK, as ``doa_peaks`` writes them -> out[K] of ZOOM with the direction in x, y, z:
    the zoom on the sphere.  A level has a centre u and one half-extent h in tangent units (radians, for small h); its Z^2 points are
    ``doa_zoom_points(u, h, Z)``.  Level 0: the seed's (x, y, z) as given, and ``half0``.  The next level has the best point as its
    centre and ``doa_zoom_next_half(h, Z)``.  The stop rule, the absent-seed rule and the meaning of ``levels`` and ``clipped`` are
    those of ``zoom``.  A seed whose direction is zero or not finite gives whatever this arithmetic gives.  ``return_levels``: also, per
    seed, the list of (centre[3], power) after every completed level."""
    st = np.asarray(strips_, dtype=np.float64)
    m = _mics(mics)
    T, Z, levels = int(T), int(Z), int(levels)
    npairs = m.shape[0] * (m.shape[0] - 1) // 2
    if T < 1 or st.shape != (npairs, 2 * T + 1):
        raise ValueError("strips must be [P][2T + 1] with T >= 1")
    if not (fs > 0 and c > 0):
        raise ValueError("fs and c must be positive")
    if not 2 <= Z <= MAX_ZOOM_CELLS or not 1 <= levels <= MAX_ZOOM_LEVELS:
        raise ValueError(f"need Z in 2..{MAX_ZOOM_CELLS} and levels in 1..{MAX_ZOOM_LEVELS}")
    half0 = np.asarray(half0, dtype=np.float64)
    if half0.shape != () or not np.isfinite(half0) or half0 <= 0:
        raise ValueError("half0 is one finite positive number")
    sd = np.asarray(seeds, dtype=PEAK).reshape(-1)
    if not 1 <= sd.shape[0] <= MAX_PEAKS:
        raise ValueError(f"K outside 1..{MAX_PEAKS}")
    w = None if pair_weights is None else np.asarray(pair_weights, dtype=np.float64).reshape(npairs)
    out = np.zeros(sd.shape[0], dtype=ZOOM)
    trail = []
    for n, seed in enumerate(sd):
        trail.append([])
        if seed["index"] < 0:
            out[n]["seed"] = -1
            continue
        ctr, half = np.array([seed["x"], seed["y"], seed["z"]], dtype=np.float64), np.float64(half0)
        power, done, clipped = np.float64(0.0), 0, 0
        for _ in range(levels):
            acc, clip, best, pts = doa_zoom_level(st, T, m, fs, c, ctr, half, Z, w)
            clipped += clip
            if best < 0:
                power = np.float64(np.nan)
                break
            ctr, half, power = pts[best].copy(), doa_zoom_next_half(half, Z), acc[best]
            done += 1
            trail[-1].append((ctr.copy(), float(power)))
        out[n] = (ctr[0], ctr[1], ctr[2], power, clipped, seed["index"], done)
    return (out, trail) if return_levels else out


def doa_angles(records):
    """(azimuth, elevation) in degrees of the directions in records' x, y, z (PEAK or ZOOM), by arctan2 on the host: azimuth in
    0 .. 360, elevation in -90 .. 90.  For reporting only; no rule reads it."""
    r = np.asarray(records)
    x, y, z = (np.asarray(r[name], dtype=np.float64) for name in "xyz")
    return np.mod(np.degrees(np.arctan2(y, x)), 360.0), np.degrees(np.arctan2(z, np.hypot(x, y)))
