"""Shared inputs of the direction-map tests (tests/test_host_srp_doa.py on the CPU, tests/test_gpu_srp_doa.py on the GPU) and the
rules of srp.doa_map, srp.doa_peak_marks and srp.doa_zoom as plain Python loops over (g, i, j), (ia, ie, da, de) and
(level, cell, i, j).  The geometries, strips and weights are those of tests/srp_cases.py and tests/srp_zoom_cases.py; the scenes are
srp_cases' with the sources moved out to 6 m."""
import functools
import math

import numpy as np

import srp_cases as S
import srp_zoom_cases as Z
from oracle import pal_oracle as O
from pyaudiolocalization_amd import srp

FS = S.MAP_FS
MAP_MICS = [2, 3, 16, 17, 33, 64]
MAP_GRIDS = [(1, 1), (1, 257), (257, 1), (3, 5), (72, 36)]         # under one workgroup, two workgroups with one lane in the second, 11 workgroups
HALF0 = 0.2                                                          # tangent units: the first level of the synthetic zoom cases


@functools.lru_cache(maxsize=None)
def axes(n_az, n_el):
    return srp.doa_axes(n_az, n_el)


def seeds(b, k, absent=()):
    """seeds[b][k] of srp.PEAK with unit directions all over the sphere; the entries named in ``absent`` are absent records."""
    rng = np.random.default_rng([81, b, k])
    out = np.zeros((b, k), dtype=srp.PEAK)
    u = rng.standard_normal((b, k, 3))
    u = u / np.linalg.norm(u, axis=2, keepdims=True)
    out["x"], out["y"], out["z"] = u[..., 0], u[..., 1], u[..., 2]
    out["power"] = rng.standard_normal((b, k))
    out["index"] = rng.integers(0, 2592, (b, k))
    for n in absent:
        out[:, n] = np.zeros((), dtype=srp.PEAK)
        out["index"][:, n] = -1
    return out


def one_seed(x, y, z, index=7):
    return Z.one_seed(x, y, z, index)


# seeds along each coordinate axis (two of |u_k| tie at zero: the lowest axis wins), on the ties |ux| == |uy| and |uy| == |uz|, and the
# two that only agree NaN for NaN
AXIS_SEEDS = [(1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0),
              (0.6, 0.6, 0.5), (0.6, -0.6, 0.7), (0.8, 0.3, 0.3), (0.5, 0.5, 0.5)]


def special_seeds():
    """seeds[1][8]: the first six of AXIS_SEEDS, a zero direction and a NaN direction."""
    out = np.zeros((1, 8), dtype=srp.PEAK)
    for n, (x, y, z) in enumerate(AXIS_SEEDS[:6] + [(0.0, 0.0, 0.0), (0.3, np.nan, 0.1)]):
        out[0, n] = (x, y, z, 0.0, 10 + n, 0)
    return out


def records_equal(a, b):
    """Records field by field with NaN equal to NaN (a NaN's sign and payload are no part of the rule)."""
    return a.shape == b.shape and all(np.array_equal(a[name], b[name], equal_nan=a[name].dtype.kind == "f") for name in a.dtype.names)


# ---- the rules as plain loops -------------------------------------------------------------------------------------------------
def loops_directions(az, el):
    return [[float(ce) * float(ca), float(ce) * float(sa), float(se)] for ca, sa in az for ce, se in el]


def loops_advance(u, mic):
    a = u[0] * mic[0]
    a = a + u[1] * mic[1]
    a = a + u[2] * mic[2]
    return a


def loops_doa_map(strips_, t, mics, fs, c, az, el, weights=None):
    m = mics.shape[0]
    order = Z.tile_order_loops(m)
    mic = [[float(v) for v in row] for row in mics]
    dirs = loops_directions(az, el)
    power, clipped = np.zeros(len(dirs)), 0
    for g, u in enumerate(dirs):
        a = [loops_advance(u, row) for row in mic]
        acc = 0.0
        for i, j, p in order:
            r = float(np.rint(((a[i] - a[j]) * float(fs)) / float(c)))
            if not abs(r) <= t:
                clipped += 1
                continue
            v = float(strips_[p][t + int(r)])
            if weights is not None:
                v = float(weights[p]) * v
            acc = acc + v
        power[g] = acc
    return power, clipped


def loops_doa_marks(power, radius, wrap):
    n_az, n_el = power.shape
    mark = np.zeros(power.shape, dtype=bool)
    for ia in range(n_az):
        for ie in range(n_el):
            v, g, ok = power[ia, ie], ia * n_el + ie, True
            if v != v:
                continue
            for da in range(-radius, radius + 1):
                for de in range(-radius, radius + 1):
                    x, e = ia + da, ie + de
                    if e < 0 or e >= n_el:
                        continue
                    if wrap:
                        x %= n_az
                    elif x < 0 or x >= n_az:
                        continue
                    o, h = power[x, e], x * n_el + e
                    if o > v or (o == v and h < g):
                        ok = False
            mark[ia, ie] = ok
    return mark


def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))        # 0 / 0 and x / 0 as IEEE has them, where Python raises


def _norm(v):
    q = v[0] * v[0]
    q = q + v[1] * v[1]
    q = q + v[2] * v[2]
    return math.sqrt(q) if q == q and q >= 0 else math.nan


def loops_basis(u):
    k, m = 0, abs(u[0])
    if abs(u[1]) < m:
        k, m = 1, abs(u[1])
    if abs(u[2]) < m:
        k = 2
    e = ([0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0])[k]
    with np.errstate(all="ignore"):
        n = _norm(e)
        e1 = [_div(e[a], n) for a in range(3)]
    e2 = [u[1] * e1[2] - u[2] * e1[1], u[2] * e1[0] - u[0] * e1[2], u[0] * e1[1] - u[1] * e1[0]]
    return k, e1, e2


def loops_doa_zoom(strips_, t, mics, fs, c, seeds_, half0, z, levels, weights=None):
    """srp.doa_zoom as plain loops -> out[K] of srp.ZOOM."""
    order = Z.tile_order_loops(mics.shape[0])
    st = [[float(v) for v in row] for row in strips_]
    wt = None if weights is None else [float(v) for v in weights]
    mic = [[float(v) for v in row] for row in mics]
    fs, c = float(fs), float(c)
    out = np.zeros(len(seeds_), dtype=srp.ZOOM)
    for n, seed in enumerate(seeds_):
        if seed["index"] < 0:
            out[n]["seed"] = -1
            continue
        ctr, half = [float(seed["x"]), float(seed["y"]), float(seed["z"])], float(half0)
        power, done, clipped = 0.0, 0, 0
        for _ in range(levels):
            _, e1, e2 = loops_basis(ctr)
            step = (half - (-half)) / float(z)
            off = [-half + (float(i) + 0.5) * step for i in range(z)]
            best, best_p, best_pt = -1, 0.0, None
            for g in range(z * z):
                i_, j_ = g // z, g % z
                v = [ctr[a] + off[i_] * e1[a] for a in range(3)]
                v = [v[a] + off[j_] * e2[a] for a in range(3)]
                with np.errstate(all="ignore"):
                    nv = _norm(v)
                    pt = [_div(v[a], nv) for a in range(3)]
                a_m = [loops_advance(pt, row) for row in mic]
                acc = 0.0
                for i, j, p in order:
                    q = _div((a_m[i] - a_m[j]) * fs, c)
                    if q != q or math.isinf(q):
                        clipped += 1
                        continue
                    k = math.floor(q)
                    if not (k >= -t and k <= t - 1):
                        clipped += 1
                        continue
                    f = q - float(k)
                    s0, s1 = st[p][t + k], st[p][t + k + 1]
                    term = s0 + f * (s1 - s0)
                    if wt is not None:
                        term = wt[p] * term
                    acc = acc + term
                if acc == acc and (best < 0 or acc > best_p):                      # cells come in index order: the first of equals stays
                    best, best_p, best_pt = g, acc, pt
            if best < 0:
                power = math.nan
                break
            ctr, half, power = best_pt, step, best_p                                # (half - (-half)) / z: one cell
            done += 1
        out[n] = (ctr[0], ctr[1], ctr[2], power, clipped, seed["index"], done)
    return out


# ---- crafted maps of the peak rule -------------------------------------------------------------------------------------------
def crafted_maps():
    """[(name, power[n_az][n_el], R, K)]: every one is checked with wrap on and off."""
    rng = np.random.default_rng(82)
    out = []
    seam = np.zeros((12, 7))
    seam[0, 3] = seam[11, 3] = 5.0                                                   # equal maxima on both sides of the seam
    seam[6, 1] = 4.0
    out.append(("equal maxima at ia = 0 and n_az - 1", seam, 1, 4))
    out.append(("the same, R = 3", seam, 3, 4))
    out.append(("n_az = 1, R = 4", rng.standard_normal((1, 9)), 4, 3))
    out.append(("n_az = 2, R = 4", rng.standard_normal((2, 9)), 4, 3))
    two = np.zeros((2, 5))
    two[1, 2] = 1.0
    out.append(("n_az = 2, the maximum at ia = 1", two, 4, 2))
    plateau = rng.standard_normal((9, 8)) * 0.01
    plateau[7:9, 2:5] = 2.0
    plateau[0, 2:5] = 2.0                                                            # a plateau across the seam: one peak wrapped, two cut
    out.append(("a plateau across the seam", plateau, 2, 8))
    holes = rng.standard_normal((10, 6))
    holes[rng.random((10, 6)) < 0.3] = np.nan
    holes[0, 0] = np.nan
    out.append(("NaN cells", holes, 1, 8))
    out.append(("all NaN", np.full((4, 3), np.nan), 2, 2))
    out.append(("K beyond the number of peaks", np.arange(15.0).reshape(5, 3), 4, 8))
    out.append(("random 37 x 29", rng.standard_normal((37, 29)), 2, 8))
    out.append(("constant", np.full((6, 5), 0.25), 2, 3))
    return out


# ---- the scenes of srp_cases.py with the sources 6 m from the array's centroid, W = 2, a 72 x 36 sphere ------------------------
SCENE_W = 2
SCENE_RANGE = 6.0
SCENE_AZ, SCENE_EL = 72, 36
SCENE_Z, SCENE_LEVELS = 8, 3
SCENE_HALF0 = np.pi / 36                                               # one cell of elevation
MAP_BOUND_DEG = 3.6                                                    # the half-diagonal of a 5-degree cell
ZOOM_BOUND_DEG = 1.5


def scene_directions():
    """The true directions from the array's centroid, unit vectors [2][3]."""
    d = np.stack(S.SCENE_SOURCES)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def scene_sources(distance=SCENE_RANGE):
    return S.scene_mics().mean(axis=0)[None, :] + distance * scene_directions()


@functools.lru_cache(maxsize=None)
def scene_frames_oracle(two, distance=SCENE_RANGE):
    """frames[M][L] of the one-source scene, or of that frame plus 0.8 times the second source's."""
    out = None
    for which in range(2 if two else 1):
        delays, gains, total = S.scene_paths(scene_sources(distance)[which])
        f = O.simulate_from_base(S.scene_base(which), delays, gains, S.SCENE_FS, total, S.SCENE_LEN)
        out = f if out is None else out + S.SCENE_GAIN2 * f
    return out


@functools.lru_cache(maxsize=None)
def scene_strips_oracle(two, distance=SCENE_RANGE):
    t = srp.half_width(S.scene_mics(), S.SCENE_FS, S.C_SOUND)
    return t, srp.strips(S.oracle_rows(scene_frames_oracle(two, distance)), S.SCENE_LEN, t, SCENE_W)


def angles_deg(records, two):
    """Angles [source][record] in degrees between the records' directions (present ones) and the true directions."""
    ok = (records["index"] >= 0) if "index" in records.dtype.names else (records["seed"] >= 0)
    u = np.stack([records["x"], records["y"], records["z"]], axis=1)[ok]
    u = u / np.linalg.norm(u, axis=1, keepdims=True)
    cos = np.clip(scene_directions()[:2 if two else 1] @ u.T, -1.0, 1.0)
    return np.degrees(np.arccos(cos))


def scene_check(records, two, bound):
    """Every source has a record within ``bound`` degrees, the two sources' records being different ones (paired by nearness, as
    srp_cases.scene_check pairs them) -> the angles [source]."""
    ang = angles_deg(records, two)
    assert ang.shape[1] >= (2 if two else 1), ang
    if not two:
        assert ang[0, 0] <= bound, ang
        return (float(ang[0, 0]),)
    near = np.argmin(ang, axis=1)
    assert near[0] != near[1], ang
    assert ang[0, near[0]] <= bound and ang[1, near[1]] <= bound, ang
    return float(ang[0, near[0]]), float(ang[1, near[1]])
