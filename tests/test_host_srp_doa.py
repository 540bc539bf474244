"""The direction map's specification on the host: srp.doa_map, srp.doa_peak_marks and srp.doa_zoom against plain Python loops
(tests/srp_doa_cases.py); csrc/srp_math.h compiled for the CPU (tests/host/test_srp_doa.cpp, with the address and undefined-behaviour
sanitizers, -ffp-contract=off) against srp.py bit for bit on directions, advances, lags on and next to half-integers, clip decisions,
bases for each choice of axis, points, quotients and terms at the borders, next half-extents and peak marks; constant, all-clipped,
NaN and absent inputs; half_width clips nothing; the lag margins; and the scenes with the sources 6 m away.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import srp_cases as S
import srp_doa_cases as D
import srp_zoom_cases as Z
from pyaudiolocalization_amd import srp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = [(S.map_mics(m), D.FS) for m in D.MAP_MICS] + [(S.scene_mics(), S.SCENE_FS)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    out = tmp_path_factory.mktemp("srp_doa") / "test_srp_doa"
    subprocess.run(["hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "pyaudiolocalization_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "test_srp_doa.cpp"), "-o", str(out)], check=True)
    return str(out)


def _run(exe, mode, tmp_path, values):
    np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1) for v in values]).tofile(tmp_path / "in.bin")
    run = subprocess.run([exe, mode, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert run.returncode == 0 and "ALL OK" in run.stdout, run.stdout + run.stderr
    return np.fromfile(tmp_path / "out.bin")


def _same(a, b):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes() == np.ascontiguousarray(b, dtype=np.float64).tobytes()


# ---- the specification against the loops ---------------------------------------------------------------------------------------
def test_axes():
    az, el, wrap = srp.doa_axes(72, 36)
    assert az.shape == (72, 2) and el.shape == (36, 2) and wrap == 1
    a = (np.arange(72) + 0.5) * ((2 * np.pi) / 72)
    assert _same(az, np.stack([np.cos(a), np.sin(a)], axis=1))
    assert np.all(el[:, 0] > 0.04)                                                  # no cell centre on a pole
    assert srp.doa_axes(5, 3, 0.0, np.pi)[2] == 0 and srp.doa_axes(5, 3, -np.pi, np.pi)[2] == 1
    u = srp.doa_directions(az, el)
    assert u.shape == (2592, 3) and np.max(np.abs(np.linalg.norm(u, axis=1) - 1.0)) < 4e-16
    assert _same(u[5 * 36 + 7], [el[7, 0] * az[5, 0], el[7, 0] * az[5, 1], el[7, 1]])
    azd, eld = srp.doa_angles(np.array([(1.0, 1.0, 0.0, 0, 0, 0), (0.0, -1.0, 1.0, 0, 0, 0)], dtype=srp.PEAK))
    assert np.allclose(azd, [45.0, 270.0]) and np.allclose(eld, [0.0, 45.0])
    for bad in (dict(n_az=0), dict(n_az=1025), dict(n_el=0), dict(n_el=1025), dict(az_hi=0.0), dict(el_lo=np.nan)):
        a = dict(n_az=4, n_el=4)
        a.update(bad)
        with pytest.raises(ValueError):
            srp.doa_axes(**a)


@pytest.mark.parametrize("grid", [(3, 5), (5, 4)])
@pytest.mark.parametrize("m", [2, 3, 17, 33])
def test_map_equals_the_loops(m, grid):
    mics = S.map_mics(m)
    az, el, _ = D.axes(*grid)
    t = srp.half_width(mics, D.FS, S.C_SOUND)
    st, wt = Z.real_strips(m, t, 1)[0], Z.real_weights(m, 1)[0]
    for weights in (None, wt):
        power, clipped = srp.doa_map(st, t, mics, D.FS, S.C_SOUND, az, el, weights)
        want, want_clipped = D.loops_doa_map(st, t, mics, D.FS, S.C_SOUND, az, el, weights)
        assert _same(power, want) and clipped == want_clipped == 0
    power, clipped = srp.doa_map(Z.real_strips(m, 3, 1)[0], 3, mics, D.FS, S.C_SOUND, az, el, wt)            # T = 3 clips
    want, want_clipped = D.loops_doa_map(Z.real_strips(m, 3, 1)[0], 3, mics, D.FS, S.C_SOUND, az, el, wt)
    assert _same(power, want) and clipped == want_clipped and (clipped > 0 or m == 2)


@pytest.mark.parametrize("wrap", [0, 1])
def test_marks_equal_the_loops(wrap):
    for name, power, radius, k in D.crafted_maps():
        for r in sorted({1, radius}):
            assert np.array_equal(srp.doa_peak_marks(power, r, wrap), D.loops_doa_marks(power, r, wrap)), (name, r)


def test_crafted_peaks():
    maps = {name: (power, r, k) for name, power, r, k in D.crafted_maps()}
    seam, r, k = maps["equal maxima at ia = 0 and n_az - 1"]
    cut, wrapped = srp.doa_peaks(seam, k, r, 0), srp.doa_peaks(seam, k, r, 1)
    assert cut["index"].tolist()[:3] == [3, 80, 43] and cut["power"].tolist()[:3] == [5.0, 5.0, 4.0]         # both sides are peaks when cut
    assert wrapped["index"].tolist()[:2] == [3, 43] and 80 not in wrapped["index"]                            # the lower index wins across the seam
    for name in ("n_az = 1, R = 4", "n_az = 2, R = 4", "n_az = 2, the maximum at ia = 1", "constant"):      # a wrapped offset that lands on
        power, r, k = maps[name]                                                                            # a cell twice changes nothing
        assert srp.doa_peaks(power, k, r, 0).tobytes() == srp.doa_peaks(power, k, r, 1).tobytes(), name
    plateau, r, k = maps["a plateau across the seam"]
    assert np.count_nonzero(srp.doa_peaks(plateau, k, r, 1)["power"] == 2.0) == 1
    assert np.count_nonzero(srp.doa_peaks(plateau, k, r, 0)["power"] == 2.0) == 2
    nan, r, k = maps["all NaN"]
    absent = srp.doa_peaks(nan, k, r, 1)
    assert np.all(absent["index"] == -1) and not absent.tobytes().strip(b"\xff\0")
    ramp, r, k = maps["K beyond the number of peaks"]
    got = srp.doa_peaks(ramp, k, r, 1, *D.axes(5, 3)[:2])
    assert got["index"].tolist() == [14] + [-1] * 7 and _same([got["x"][0], got["y"][0], got["z"][0]], srp.doa_directions(*D.axes(5, 3)[:2])[14])


@pytest.mark.parametrize("levels", [1, 3])
@pytest.mark.parametrize("z", [2, 3, 8])
@pytest.mark.parametrize("m", [2, 3, 17, 33])
def test_zoom_equals_the_loops(m, z, levels):
    mics = S.map_mics(m)
    t = srp.half_width(mics, D.FS, S.C_SOUND)
    st, wt = Z.real_strips(m, t, 1)[0], Z.real_weights(m, 1)[0]
    sd = D.seeds(1, 3, absent=(1,))[0]
    for weights in (None, wt):
        got = srp.doa_zoom(st, t, mics, D.FS, S.C_SOUND, sd, D.HALF0, z, levels, weights)
        want = D.loops_doa_zoom(st, t, mics, D.FS, S.C_SOUND, sd, D.HALF0, z, levels, weights)
        assert got.tobytes() == want.tobytes(), (got, want)
        assert np.all(got["clipped"] == 0)                                   # half_width clips nothing under the zoom's test
        assert got["seed"].tolist() == [sd["index"][0], -1, sd["index"][2]] and got["levels"].tolist() == [levels, 0, levels]
        u = np.stack([got["x"], got["y"], got["z"]], axis=1)[[0, 2]]
        assert np.max(np.abs(np.linalg.norm(u, axis=1) - 1.0)) < 4e-16        # a centre is a normalised point


def test_zoom_special_seeds_equal_the_loops():
    m = 5
    mics = S.map_mics(m)
    t = srp.half_width(mics, D.FS, S.C_SOUND)
    st, sd = Z.real_strips(m, t, 1)[0], D.special_seeds()[0]
    got = srp.doa_zoom(st, t, mics, D.FS, S.C_SOUND, sd, D.HALF0, 4, 2)
    want = D.loops_doa_zoom(st, t, mics, D.FS, S.C_SOUND, sd, D.HALF0, 4, 2)
    assert D.records_equal(got, want) and got[:6].tobytes() == want[:6].tobytes()
    # a zero or NaN direction: every point is NaN, every term is clipped, every power is 0.0 and index 0 wins
    assert np.all(got["power"][6:] == 0.0) and np.all(got["clipped"][6:] == 2 * 16 * 10) and np.all(np.isnan(got["x"][6:]))
    assert [srp.doa_basis(u)[0] for u in D.AXIS_SEEDS] == [1, 1, 0, 0, 0, 0, 2, 0, 1, 0]


# ---- half_width and the margins ------------------------------------------------------------------------------------------------
def test_half_width_clips_nothing_and_margins():
    """|a_i - a_j| <= |m_i - m_j| for a unit direction: |q| <= T - 1, so neither the map's rint nor the zoom's floor leaves the strip.
    The smallest distance of a lag from a half-integer stays far above what a last-bit difference of an advance could move."""
    for mics, fs in GEOMETRIES:
        t = srp.half_width(mics, fs, S.C_SOUND)
        for grid in D.MAP_GRIDS:
            u = srp.doa_directions(*D.axes(*grid)[:2])
            q = srp.doa_lag_quotients(u, mics, fs, S.C_SOUND)
            assert np.max(np.abs(q)) <= t - 1
            assert srp.doa_lag_margin(u, mics, fs, S.C_SOUND) >= 1e-9, (mics.shape[0], grid)
        pts = np.concatenate([srp.doa_zoom_points(s, h, 16) for s in D.AXIS_SEEDS for h in (D.HALF0, 1.5, 1e-9)])
        assert np.max(np.abs(np.linalg.norm(pts, axis=1) - 1.0)) < 4e-16
        q = srp.doa_lag_quotients(pts, mics, fs, S.C_SOUND)
        k = np.floor(q)
        assert np.max(np.abs(q)) <= t - 1 and k.min() >= -(t - 1) and k.max() <= t - 1


# ---- the header against the specification --------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,grid,t,wrap,radius", [(2, (1, 1), 40, 1, 1), (3, (3, 5), 40, 0, 2), (17, (9, 7), 40, 1, 4), (33, (2, 11), 3, 1, 4),
                                                  (64, (5, 3), 40, 0, 1)])
def test_header_grid_equals_the_specification(exe, tmp_path, m, grid, t, wrap, radius):
    mics = S.map_mics(m)
    az, el, _ = D.axes(*grid)
    g, p = grid[0] * grid[1], m * (m - 1) // 2
    power = np.random.default_rng([83, m]).integers(0, 4, grid).astype(np.float64)     # many ties
    power[0, 0] = np.nan
    got = _run(exe, "grid", tmp_path, [[grid[0], grid[1], m, D.FS, S.C_SOUND, t, wrap, radius], az, el, mics, power])
    u = srp.doa_directions(az, el)
    a = srp.doa_advances(u, mics)
    r = np.rint(srp.doa_lag_quotients(u, mics, D.FS, S.C_SOUND))
    assert _same(got[:3 * g], u) and _same(got[3 * g:3 * g + g * m], a)
    terms = got[3 * g + g * m:3 * g + g * m + 2 * g * p].reshape(g, p, 2)
    assert _same(terms[:, :, 0], r) and np.array_equal(terms[:, :, 1] == 1.0, ~(np.abs(r) <= t))
    assert (np.count_nonzero(terms[:, :, 1]) > 0) == (t == 3)
    assert np.array_equal(got[3 * g + g * m + 2 * g * p:] == 1.0, srp.doa_peak_marks(power, radius, wrap).reshape(-1))


@pytest.mark.parametrize("wrap", [0, 1])
def test_header_marks_on_the_crafted_maps(exe, tmp_path, wrap):
    mics = S.map_mics(2)
    for name, power, radius, _ in D.crafted_maps():
        az, el, _ = D.axes(*power.shape)
        got = _run(exe, "grid", tmp_path, [[power.shape[0], power.shape[1], 2, D.FS, S.C_SOUND, 5, wrap, radius], az, el, mics, power])
        assert np.array_equal(got[-power.size:] == 1.0, srp.doa_peak_marks(power, radius, wrap).reshape(-1)), name


def _spec_pairs(fs, c, t, strip, a):
    """The map's and the zoom's arithmetic on given advances (aj, ai) of one pair -> [N][7]."""
    with np.errstate(invalid="ignore", over="ignore"):
        q = ((a[:, 1] - a[:, 0]) * np.float64(fs)) / np.float64(c)
        r = np.rint(q)
    v, out, _, k, f = srp.terms_at(strip[None, :], t, q[:, None])
    return np.stack([r, (~(np.abs(r) <= t)).astype(np.float64), q, k[:, 0], f[:, 0], out[:, 0].astype(np.float64), v[:, 0]], axis=1)


def test_header_lags_and_terms_at_the_borders(exe, tmp_path):
    """fs = c = 1 and aj = 0 make q = ai exactly: lags on half-integers (half to even) and next to them, and the zoom's borders
    q = -T (kept), just below -T (clipped), just below T (kept, k = T - 1), q = T (clipped), far outside, infinite and NaN."""
    t = 5
    strip = np.random.default_rng(84).standard_normal(2 * t + 1)
    halves = [s + 0.5 for s in range(-t - 1, t + 1)]
    q = np.array([float(s) for s in range(-t - 1, t + 2)] + halves + [np.nextafter(h, np.inf) for h in halves]
                 + [np.nextafter(h, -np.inf) for h in halves]
                 + [np.nextafter(-float(t), -np.inf), np.nextafter(-float(t), np.inf), np.nextafter(t - 1.0, np.inf), np.nextafter(float(t), 0.0),
                    -0.0, np.nextafter(0.0, -1.0), 2.25, -2.75, 1e300, -1e300, 2.0 ** 31, -2.0 ** 31, 2.0 ** 63, np.inf, -np.inf, np.nan])
    a = np.stack([np.zeros_like(q), q], axis=1)
    got = _run(exe, "pairs", tmp_path, [[1.0, 1.0, t, q.shape[0]], strip, a]).reshape(-1, 7)
    want = _spec_pairs(1.0, 1.0, t, strip, a)
    assert np.array_equal(want[:, 2], q, equal_nan=True) and np.array_equal(got, want, equal_nan=True)
    fin = np.isfinite(q)
    assert got[fin].tobytes() == want[fin].tobytes()
    lag = {float(v): (r, c == 0.0) for v, r, c in zip(q, got[:, 0], got[:, 1])}
    assert lag[0.5] == (0.0, True) and lag[1.5] == (2.0, True) and lag[-2.5] == (-2.0, True) and lag[4.5] == (4.0, True)
    assert lag[5.5] == (6.0, False) and lag[-5.5] == (-6.0, False) and lag[float(np.nextafter(5.5, -np.inf))] == (5.0, True)
    kept = {float(v): c == 0.0 for v, c in zip(q, got[:, 5])}
    assert kept[-float(t)] and kept[float(np.nextafter(float(t), 0.0))] and kept[t - 1.0] and not kept[float(t)]
    assert not kept[float(np.nextafter(-float(t), -np.inf))] and np.all(got[~fin, 5] == 1.0) and np.all(got[~fin, 1] == 1.0)


@pytest.mark.parametrize("fs,c,t", [(8000.0, S.C_SOUND, 40), (48000.0, S.C_SOUND, 119), (8000.0, S.C_SOUND, 3)])
def test_header_lags_and_terms_on_random_advances(exe, tmp_path, fs, c, t):
    rng = np.random.default_rng([85, t])
    strip = rng.standard_normal(2 * t + 1)
    a = rng.uniform(-0.4, 0.4, (4000, 2))
    # and quotients a rounding away from a half-integer, where the shortcut of srp_lag must fall back on the division
    near = (rng.integers(-t, t, 500) + 0.5) * c / fs
    a = np.concatenate([a, np.stack([np.zeros(500), near], axis=1), np.stack([np.zeros(500), np.nextafter(near, np.inf)], axis=1)])
    got = _run(exe, "pairs", tmp_path, [[fs, c, t, a.shape[0]], strip, a]).reshape(-1, 7)
    assert got.tobytes() == _spec_pairs(fs, c, t, strip, a).tobytes()
    assert (0 < np.count_nonzero(got[:4000, 1]) < 4000) == (t == 3)


@pytest.mark.parametrize("m,z,t,half", [(2, 2, 40, 0.2), (3, 3, 40, 1.5), (17, 8, 40, 0.2), (33, 5, 40, 1e-9), (5, 16, 3, 0.2)])
def test_header_level_equals_the_specification(exe, tmp_path, m, z, t, half):
    mics = S.map_mics(m)
    st = Z.real_strips(m, t, 1)[0]
    g, p = z * z, m * (m - 1) // 2
    for u in D.AXIS_SEEDS + [(0.0, 0.0, 0.0), (0.3, np.nan, 0.1), (3.0, -4.0, 12.0)]:
        got = _run(exe, "level", tmp_path, [[D.FS, S.C_SOUND, t, m, z, half], u, mics, st])
        k, e1, e2 = srp.doa_basis(u)
        pts = srp.doa_zoom_points(u, half, z)
        q = srp.doa_lag_quotients(pts, mics, D.FS, S.C_SOUND)
        v, out, _, kk, f = srp.terms_at(st, t, q)
        want = np.concatenate([[k], e1, e2, srp.doa_zoom_offsets(half, z), pts.reshape(-1),
                               np.stack([q, kk, f, out.astype(np.float64), v], axis=2).reshape(-1), [srp.doa_zoom_next_half(half, z)]])
        assert got.shape == want.shape == (7 + z + 3 * g + 5 * g * p + 1,)
        assert np.array_equal(got, want, equal_nan=True), u
        if np.all(np.isfinite(u)) and np.any(np.asarray(u) != 0.0):
            assert got.tobytes() == want.tobytes(), u
            assert (np.count_nonzero(out) > 0) == (t == 3 and m > 2)
            power, clipped, best, _ = srp.doa_zoom_level(st, t, mics, D.FS, S.C_SOUND, u, half, z)
            acc = np.zeros(g)
            for pair in srp.tile_order(m):
                acc = acc + v[:, pair]
            assert _same(acc, power) and clipped == np.count_nonzero(out) and best == int(np.argmax(power))


# ---- constant, all-clipped, NaN and absent inputs ------------------------------------------------------------------------------
def test_constant_strips_index_zero_wins():
    m, z, levels = 5, 4, 3
    mics = S.map_mics(m)
    t = srp.half_width(mics, D.FS, S.C_SOUND)
    st = np.full((m * (m - 1) // 2, 2 * t + 1), 0.75)
    az, el, wrap = D.axes(6, 5)
    power, clipped = srp.doa_map(st, t, mics, D.FS, S.C_SOUND, az, el)
    assert np.all(power == 7.5) and clipped == 0
    pk = srp.doa_peaks(power.reshape(6, 5), 2, 2, wrap, az, el)
    assert pk["index"].tolist() == [0, -1]                                              # one plateau over the whole sphere
    out, trail = srp.doa_zoom(st, t, mics, D.FS, S.C_SOUND, pk, D.HALF0, z, levels, return_levels=True)
    assert out["power"][0] == 7.5 and out["levels"][0] == levels and out["seed"].tolist() == [0, -1] and [p for _, p in trail[0]] == [7.5] * 3
    ctr, half = np.array([pk["x"][0], pk["y"][0], pk["z"][0]]), D.HALF0
    for _ in range(levels):
        ctr, half = srp.doa_zoom_points(ctr, half, z)[0], srp.doa_zoom_next_half(half, z)
    assert _same([out["x"][0], out["y"][0], out["z"][0]], ctr)
    assert out.tobytes() == D.loops_doa_zoom(st, t, mics, D.FS, S.C_SOUND, pk, D.HALF0, z, levels).tobytes()


def test_all_terms_clipped():
    """Non-unit tables are allowed: directions of length 100 put every lag of two microphones 0.9 m apart far outside T = 3."""
    mics = np.array([[0.0, 0.0, 0.0], [0.9, 0.0, 0.0]])
    az, el = np.array([[100.0, 0.0], [-100.0, 0.0]]), np.array([[1.0, 0.0]])
    st = np.random.default_rng(86).standard_normal((1, 7))
    power, clipped = srp.doa_map(st, 3, mics, D.FS, S.C_SOUND, az, el)
    want, want_clipped = D.loops_doa_map(st, 3, mics, D.FS, S.C_SOUND, az, el)
    assert power.tolist() == want.tolist() == [0.0, 0.0] and clipped == want_clipped == 2
    # the zoom normalises its points, so it is the strip that is short here: along the axis |q| is about 21, outside T = 3
    seed = D.one_seed(1.0, 0.0, 0.0)
    out = srp.doa_zoom(st, 3, mics, D.FS, S.C_SOUND, seed, 0.01, 4, 2)
    assert out["power"][0] == 0.0 and out["clipped"][0] == 2 * 16 and out["levels"][0] == 2
    first = srp.doa_zoom_points((1.0, 0.0, 0.0), 0.01, 4)[0]                            # every cell ties at 0.0: index 0 wins twice
    assert _same([out["x"][0], out["y"][0], out["z"][0]], srp.doa_zoom_points(first, srp.doa_zoom_next_half(0.01, 4), 4)[0])
    assert out.tobytes() == D.loops_doa_zoom(st, 3, mics, D.FS, S.C_SOUND, seed, 0.01, 4, 2).tobytes()


def test_nan_strips_stop_the_zoom():
    m = 3
    mics = S.map_mics(m)
    t = srp.half_width(mics, D.FS, S.C_SOUND)
    st = np.full((3, 2 * t + 1), np.nan)
    az, el, wrap = D.axes(3, 5)
    power, clipped = srp.doa_map(st, t, mics, D.FS, S.C_SOUND, az, el)
    assert np.all(np.isnan(power)) and clipped == 0 and np.all(srp.doa_peaks(power.reshape(3, 5), 2, 1, wrap)["index"] == -1)
    seed = D.one_seed(0.6, 0.0, 0.8, index=11)
    out = srp.doa_zoom(st, t, mics, D.FS, S.C_SOUND, seed, D.HALF0, 3, 4)
    assert (out["x"][0], out["y"][0], out["z"][0]) == (0.6, 0.0, 0.8) and np.isnan(out["power"][0])
    assert out["levels"][0] == 0 and out["seed"][0] == 11 and out["clipped"][0] == 0
    assert D.records_equal(out, D.loops_doa_zoom(st, t, mics, D.FS, S.C_SOUND, seed, D.HALF0, 3, 4))


def test_absent_seed_and_limits():
    m = 3
    mics = S.map_mics(m)
    t = srp.half_width(mics, D.FS, S.C_SOUND)
    st = Z.real_strips(m, t, 1)[0]
    sd = D.seeds(1, 3, absent=(0, 2))[0]
    out = srp.doa_zoom(st, t, mics, D.FS, S.C_SOUND, sd, D.HALF0, 2, 2)
    want = np.zeros((), dtype=srp.ZOOM)
    want["seed"] = -1
    assert out[0].tobytes() == out[2].tobytes() == want.tobytes() and out["seed"][1] == sd["index"][1]
    alone = srp.doa_zoom(st, t, mics, D.FS, S.C_SOUND, sd[1:2], D.HALF0, 2, 2)
    assert alone[0].tobytes() == out[1].tobytes()                                   # a seed's record does not depend on its neighbours
    for kw in (dict(z=1), dict(z=17), dict(levels=0), dict(levels=17), dict(half0=0.0), dict(half0=-1.0), dict(half0=np.nan),
               dict(half0=np.inf), dict(half0=(0.1, 0.1, 0.1)), dict(fs=0.0), dict(c=-1.0), dict(seeds=sd[:0]),
               dict(seeds=np.zeros(9, dtype=srp.PEAK))):
        a = dict(z=2, levels=2, half0=D.HALF0, fs=D.FS, c=S.C_SOUND, seeds=sd)
        a.update(kw)
        with pytest.raises(ValueError):
            srp.doa_zoom(st, t, mics, a["fs"], a["c"], a["seeds"], a["half0"], a["z"], a["levels"])
    with pytest.raises(ValueError):
        srp.doa_zoom(st[:, :1], 0, mics, D.FS, S.C_SOUND, sd, D.HALF0, 2, 2)         # T = 0: no second sample to blend with
    az, el, _ = D.axes(3, 5)
    for bad_az, bad_el in ((az[:, :1], el), (az, np.full((5, 2), np.nan)), (np.zeros((0, 2)), el), (np.zeros((1025, 2)), el)):
        with pytest.raises(ValueError):
            srp.doa_map(st, t, mics, D.FS, S.C_SOUND, bad_az, bad_el)
    for r in (0, 5):
        with pytest.raises(ValueError):
            srp.doa_peaks(np.zeros((3, 5)), 1, r, 1)
    for k in (0, 9):
        with pytest.raises(ValueError):
            srp.doa_peaks(np.zeros((3, 5)), k, 1, 1)


# ---- the scenes ----------------------------------------------------------------------------------------------------------------
def _scene(two, n_az=D.SCENE_AZ, n_el=D.SCENE_EL, half0=D.SCENE_HALF0, radii=(1,)):
    mics = S.scene_mics()
    az, el, wrap = D.axes(n_az, n_el)
    t, st = D.scene_strips_oracle(two)
    assert t == 119
    power, clipped = srp.doa_map(st, t, mics, S.SCENE_FS, S.C_SOUND, az, el)
    assert clipped == 0
    peaks = [srp.doa_peaks(power.reshape(n_az, n_el), 2 if two else 1, r, wrap, az, el) for r in radii]
    assert all(p.tobytes() == peaks[0].tobytes() for p in peaks)
    zoomed = srp.doa_zoom(st, t, mics, S.SCENE_FS, S.C_SOUND, peaks[0], half0, D.SCENE_Z, D.SCENE_LEVELS)
    assert np.all(zoomed["clipped"] == 0) and np.all(zoomed["levels"] == D.SCENE_LEVELS)
    return peaks[0], zoomed


def test_scene_one_source():
    """W = 2, T = 119, a 72 x 36 sphere: the map's first peak lies within half a cell diagonal of the true direction (2.54 degrees),
    the zoom's (Z = 8, three levels, half0 = one cell) within 1.5 degrees (0.83)."""
    peaks, zoomed = _scene(False)
    d, = D.scene_check(peaks, False, D.MAP_BOUND_DEG)
    z, = D.scene_check(zoomed, False, D.ZOOM_BOUND_DEG)
    print(f"[srp doa] one source: map {d:.3f} deg, zoom {z:.3f} deg")


def test_scene_two_sources():
    """K = 2, identically for R = 1, 2 and 3: 2.54 and 1.01 degrees from the sources on the map, 0.83 and 0.77 after the zoom; each
    peak is 85 degrees or more from the other source, and the stronger peak is the second source's."""
    peaks, zoomed = _scene(True, radii=(1, 2, 3))
    d = D.scene_check(peaks, True, D.MAP_BOUND_DEG)
    z = D.scene_check(zoomed, True, D.ZOOM_BOUND_DEG)
    ang = D.angles_deg(peaks, True)
    assert np.argmin(ang[:, 0]) == 1 and min(ang[0, 0], ang[1, 1]) >= 85.0, ang
    print(f"[srp doa] two sources: map {d[0]:.3f} and {d[1]:.3f} deg, zoom {z[0]:.3f} and {z[1]:.3f} deg")


def test_scene_from_the_coarse_map():
    """The same from the 36 x 18 map's seeds (4.3 and 3.9 degrees off) with half0 = one of its cells: 0.87 and 0.73 degrees."""
    peaks, zoomed = _scene(True, 36, 18, np.pi / 18)
    d = D.scene_check(peaks, True, 2 * D.MAP_BOUND_DEG)
    z = D.scene_check(zoomed, True, D.ZOOM_BOUND_DEG)
    print(f"[srp doa] two sources from 36 x 18: map {d[0]:.3f} and {d[1]:.3f} deg, zoom {z[0]:.3f} and {z[1]:.3f} deg")


def test_scene_margin():
    u = srp.doa_directions(*D.axes(D.SCENE_AZ, D.SCENE_EL)[:2])
    margin = srp.doa_lag_margin(u, S.scene_mics(), S.SCENE_FS, S.C_SOUND)
    print(f"[srp doa] scene lag margin {margin:.2e}")
    assert margin >= 1e-9
