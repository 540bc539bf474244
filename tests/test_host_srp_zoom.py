"""The zoom's specification on the host: srp.zoom against plain Python loops over (level, cell, i, j) in tile order
(tests/srp_zoom_cases.py); srp.tile_order; csrc/srp_math.h compiled for the CPU (tests/host/test_srp_zoom.cpp, with the address and
undefined-behaviour sanitizers, -ffp-contract=off) against srp.py bit for bit on points, quotients, floors, fractions, clip decisions,
blended terms and next boxes; constant, NaN and absent inputs; and the two scenes on the oracle's rows.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import srp_cases as S
import srp_zoom_cases as Z
from pyaudiolocalization_amd import pair_list, srp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    out = tmp_path_factory.mktemp("srp_zoom") / "test_srp_zoom"
    subprocess.run(["hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "pyaudiolocalization_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "test_srp_zoom.cpp"), "-o", str(out)], check=True)
    return str(out)


def _run(exe, *args):
    run = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True)
    assert run.returncode == 0 and "ALL OK" in run.stdout, run.stdout + run.stderr


@pytest.mark.parametrize("m", [2, 16, 17, 33, 64])
def test_tile_order(m):
    order = srp.tile_order(m)
    npairs = m * (m - 1) // 2
    assert order.shape == (npairs,) and np.array_equal(np.sort(order), np.arange(npairs))
    assert order.tolist() == [p for _, _, p in Z.tile_order_loops(m)]
    pairs = pair_list(m)
    assert all(tuple(pairs[p]) == (i, j) for i, j, p in Z.tile_order_loops(m))
    if m <= 16:
        assert np.array_equal(order, np.arange(npairs))
    else:
        assert not np.array_equal(order, np.arange(npairs))


@pytest.mark.parametrize("levels", [1, 3])
@pytest.mark.parametrize("z", [2, 3, 8])
@pytest.mark.parametrize("m", [2, 3, 17, 33])
def test_zoom_equals_the_loops(m, z, levels):
    mics = S.map_mics(m)
    t = srp.half_width(mics, Z.FS, S.C_SOUND)
    st, wt = Z.real_strips(m, t, 1)[0], Z.real_weights(m, 1)[0]
    sd = Z.seeds(1, 3, absent=(1,))[0]
    for weights in (None, wt):
        got = srp.zoom(st, t, mics, Z.FS, S.C_SOUND, sd, Z.HALF0, z, levels, weights)
        want = Z.loops_zoom(st, t, mics, Z.FS, S.C_SOUND, sd, Z.HALF0, z, levels, weights)
        assert got.tobytes() == want.tobytes(), (got, want)
        assert np.all(got["clipped"] == 0)                                   # half_width clips nothing under the zoom's test
        assert got["seed"].tolist() == [sd["index"][0], -1, sd["index"][2]] and got["levels"].tolist() == [levels, 0, levels]


def test_half_width_clips_nothing_under_the_zoom():
    """|q| <= T - 1 gives -(T - 1) <= floor(q) <= T - 1: inside -T .. T - 1, for points far outside the array too."""
    far = srp.grid_points((-50.0, -60.0, -70.0), (80.0, 90.0, 100.0), (3, 4, 5))
    for mics, fs in [(S.map_mics(m), Z.FS) for m in S.MAP_MICS] + [(S.scene_mics(), S.SCENE_FS)]:
        t = srp.half_width(mics, fs, S.C_SOUND)
        st = np.zeros((mics.shape[0] * (mics.shape[0] - 1) // 2, 2 * t + 1))
        for pts in (far, srp.grid_points(S.MAP_LO, S.MAP_HI, (5, 4, 3))):
            _, out, q, k, _ = srp.zoom_terms(st, t, pts, mics, fs, S.C_SOUND)
            assert not np.any(out) and np.max(np.abs(q)) <= t - 1 and k.min() >= -(t - 1) and k.max() <= t - 1


def _pairs(exe, tmp_path, fs, c, t, strip, d):
    np.concatenate([[fs, c, t, d.shape[0]], strip, d.reshape(-1)]).tofile(tmp_path / "in.bin")
    _run(exe, "pairs", tmp_path / "in.bin", tmp_path / "out.bin")
    return np.fromfile(tmp_path / "out.bin").reshape(-1, 5)


def _spec_pairs(fs, c, t, strip, d):
    """srp.zoom_terms' arithmetic on given distances (di, dj) of one pair -> [N][5]: q, k, f, clipped, term."""
    with np.errstate(invalid="ignore"):
        q = ((d[:, 1] - d[:, 0]) * np.float64(fs)) / np.float64(c)
        k = np.floor(q)
        f = q - k
        out = ~((k >= -t) & (k <= t - 1))
        at = np.where(out, 0, k).astype(np.int64) + t
        v = strip[at] + np.where(out, 0.0, f) * (strip[at + 1] - strip[at])
    return np.stack([q, k, f, out.astype(np.float64), np.where(out, 0.0, v)], axis=1)


def test_header_terms_at_the_borders(exe, tmp_path):
    """fs = c = 1 and di = 0 make q = dj exactly: lags on integers (f = 0: the term is s0), and the borders q = -T (kept), just below
    -T (clipped), just above T - 1 and just below T (kept, k = T - 1), q = T (clipped), far outside, infinite and NaN."""
    t = 5
    strip = np.random.default_rng(94).standard_normal(2 * t + 1)
    q = np.array([float(s) for s in range(-t - 1, t + 2)]
                 + [np.nextafter(-float(t), -np.inf), np.nextafter(-float(t), np.inf), np.nextafter(t - 1.0, np.inf), np.nextafter(float(t), 0.0),
                    -0.0, np.nextafter(0.0, -1.0), 0.5, -0.5, 2.25, -2.75, 1e300, -1e300, 2.0 ** 31, -2.0 ** 31, 2.0 ** 63, np.inf, -np.inf, np.nan])
    d = np.stack([np.zeros_like(q), q], axis=1)
    got, want = _pairs(exe, tmp_path, 1.0, 1.0, t, strip, d), _spec_pairs(1.0, 1.0, t, strip, d)
    assert np.array_equal(want[:, 0], q, equal_nan=True)
    assert np.array_equal(got, want, equal_nan=True)
    fin = np.isfinite(q)
    assert got[fin].tobytes() == want[fin].tobytes()
    kept = {float(v): (c == 0.0, term) for v, c, term in zip(q, got[:, 3], got[:, 4])}
    for s in range(-t, t):                                                           # integers: f = 0 and the term is s0 itself
        assert kept[float(s)] == (True, strip[t + s])
    assert not kept[float(t)][0] and not kept[float(-t - 1)][0] and not kept[float(t + 1)][0]
    assert not kept[float(np.nextafter(-float(t), -np.inf))][0]
    assert kept[float(np.nextafter(t - 1.0, np.inf))][0] and kept[float(np.nextafter(float(t), 0.0))][0] and kept[-float(t)][0]
    assert np.all(got[~fin, 3] == 1.0) and np.all(got[np.abs(q) >= 1e300, 3] == 1.0)


@pytest.mark.parametrize("fs,c,t", [(8000.0, S.C_SOUND, 40), (48000.0, S.C_SOUND, 119), (8000.0, S.C_SOUND, 3)])
def test_header_terms_on_random_distances(exe, tmp_path, fs, c, t):
    rng = np.random.default_rng([95, t])
    strip = rng.standard_normal(2 * t + 1)
    d = rng.uniform(0.0, 0.8, (4000, 2))                                           # |dj - di| fs / c < 112 at 48 kHz
    got, want = _pairs(exe, tmp_path, fs, c, t, strip, d), _spec_pairs(fs, c, t, strip, d)
    assert got.tobytes() == want.tobytes()
    assert (0 < np.count_nonzero(want[:, 3]) < d.shape[0]) == (t == 3)              # T = 3 clips some, the others none


@pytest.mark.parametrize("m,z,t", [(2, 2, 40), (3, 3, 40), (17, 8, 40), (33, 5, 40), (5, 16, 3)])
def test_header_level_equals_the_specification(exe, tmp_path, m, z, t):
    mics = S.map_mics(m)
    st = Z.real_strips(m, t, 1)[0]
    ctr, half = np.array([0.3, 0.55, 0.7]), np.asarray(Z.HALF0)
    power, clipped, best, pts = srp.zoom_level(st, t, mics, Z.FS, S.C_SOUND, ctr, half, z)
    np.concatenate([[Z.FS, S.C_SOUND, t, m, z, best], ctr, half, mics.reshape(-1), st.reshape(-1)]).tofile(tmp_path / "in.bin")
    _run(exe, "level", tmp_path / "in.bin", tmp_path / "out.bin")
    got = np.fromfile(tmp_path / "out.bin")
    g, p = z ** 3, m * (m - 1) // 2
    lo, hi = srp.zoom_box(ctr, half)
    assert got[:6].tobytes() == np.concatenate([lo, hi]).tobytes()
    assert got[6:6 + 3 * g].tobytes() == pts.tobytes() == srp.grid_points(lo, hi, (z, z, z)).tobytes()
    v, out, q, k, f = srp.zoom_terms(st, t, pts, mics, Z.FS, S.C_SOUND)
    terms = got[6 + 3 * g:6 + 3 * g + 5 * g * p].reshape(g, p, 5)
    for n, want in enumerate((q, k, f, out.astype(np.float64), v)):
        assert terms[:, :, n].tobytes() == np.ascontiguousarray(want).tobytes(), n
    assert int(np.count_nonzero(out)) == clipped and (clipped > 0) == (t == 3)
    tail = got[6 + 3 * g + 5 * g * p:]
    assert tail[:3].tobytes() == pts[best].tobytes() and tail[3:6].tobytes() == srp.zoom_next_half(lo, hi, z).tobytes()
    assert tail[6:].tolist() == [1.0, 0.0, 1.0, 0.0]                                # absent(-1), absent(0), stops(-1), stops(0)
    # the power is the sum of these terms in tile order
    acc = np.zeros(g)
    for pair in srp.tile_order(m):
        acc = acc + v[:, pair]
    assert acc.tobytes() == power.tobytes()


def test_constant_strips_index_zero_wins():
    """Every cell of every level has the same power: the blend of two equal samples is the sample, so every cell sums P equal terms in
    one order.  Index 0, the corner cell at lo + step / 2, wins at every level: after L levels of Z = 4 the centre has moved by
    -half (1 - 1 / Z) (1 + 2 / Z + ... + (2 / Z)^(L - 1)) on every axis - here exactly, all figures being dyadic."""
    m, z, levels = 5, 4, 3
    mics = S.map_mics(m)
    t = srp.half_width(mics, Z.FS, S.C_SOUND)
    st = np.full((m * (m - 1) // 2, 2 * t + 1), 0.75)
    out, trail = srp.zoom(st, t, mics, Z.FS, S.C_SOUND, Z.one_seed(0.5, 0.25, 0.125), (0.5, 0.25, 1.0), z, levels, return_levels=True)
    shift = (1 - 1 / z) * (1 + 2 / z + (2 / z) ** 2)                                   # 1.3125
    assert (out["x"][0], out["y"][0], out["z"][0]) == (0.5 - 0.5 * shift, 0.25 - 0.25 * shift, 0.125 - 1.0 * shift)
    assert out["power"][0] == 0.75 * 10 and out["levels"][0] == levels and out["clipped"][0] == 0 and out["seed"][0] == 7
    assert [p for _, p in trail[0]] == [7.5] * levels
    assert out.tobytes() == Z.loops_zoom(st, t, mics, Z.FS, S.C_SOUND, Z.one_seed(0.5, 0.25, 0.125), (0.5, 0.25, 1.0), z, levels).tobytes()


def test_all_terms_clipped_index_zero_wins():
    """Z.all_clipped: every power is 0.0, index 0 wins at each level, every term is counted."""
    mics, t, st, seed, half0, z, levels = Z.all_clipped()
    out = srp.zoom(st, t, mics, Z.FS, S.C_SOUND, seed, half0, z, levels)
    assert out["power"][0] == 0.0 and out["clipped"][0] == 2 * 64 and out["levels"][0] == 2
    assert (out["x"][0], out["y"][0], out["z"][0]) == (100.0 - 0.5 * 0.75 * 1.5,) + (-0.5 * 0.75 * 1.5,) * 2
    assert out.tobytes() == Z.loops_zoom(st, t, mics, Z.FS, S.C_SOUND, seed, half0, z, levels).tobytes()


def test_nan_strips_stop_the_zoom():
    m = 3
    mics = S.map_mics(m)
    t = srp.half_width(mics, Z.FS, S.C_SOUND)
    seed = Z.one_seed(0.3, 0.4, 0.5, index=11)
    out = srp.zoom(np.full((3, 2 * t + 1), np.nan), t, mics, Z.FS, S.C_SOUND, seed, Z.HALF0, 3, 4)
    assert (out["x"][0], out["y"][0], out["z"][0]) == (0.3, 0.4, 0.5) and np.isnan(out["power"][0])
    assert out["levels"][0] == 0 and out["seed"][0] == 11 and out["clipped"][0] == 0
    assert out.tobytes() == Z.loops_zoom(np.full((3, 2 * t + 1), np.nan), t, mics, Z.FS, S.C_SOUND, seed, Z.HALF0, 3, 4).tobytes()


def test_nan_level_after_a_completed_one():
    """Z.nan_second_level: the first level completes, the second has no cell that is not NaN."""
    mics, t, st, seed, half0, z, centre = Z.nan_second_level()
    out = srp.zoom(st, t, mics, Z.FS, S.C_SOUND, seed, half0, z, 3)
    assert out["levels"][0] == 1 and np.isnan(out["power"][0]) and out["seed"][0] == 3 and out["clipped"][0] == 0
    assert (out["x"][0], out["y"][0], out["z"][0]) == tuple(centre)
    assert out.tobytes() == Z.loops_zoom(st, t, mics, Z.FS, S.C_SOUND, seed, half0, z, 3).tobytes()


def test_absent_seed_and_limits():
    m = 3
    mics = S.map_mics(m)
    t = srp.half_width(mics, Z.FS, S.C_SOUND)
    st = Z.real_strips(m, t, 1)[0]
    sd = Z.seeds(1, 3, absent=(0, 2))[0]
    out = srp.zoom(st, t, mics, Z.FS, S.C_SOUND, sd, Z.HALF0, 2, 2)
    want = np.zeros((), dtype=srp.ZOOM)
    want["seed"] = -1
    assert out[0].tobytes() == out[2].tobytes() == want.tobytes() and out["seed"][1] == sd["index"][1]
    alone = srp.zoom(st, t, mics, Z.FS, S.C_SOUND, sd[1:2], Z.HALF0, 2, 2)
    assert alone[0].tobytes() == out[1].tobytes()                                   # a seed's record does not depend on its neighbours
    for kw in (dict(z=1), dict(z=17), dict(levels=0), dict(levels=17), dict(half0=(0.1, 0.0, 0.1)), dict(half0=(0.1, -1.0, 0.1)),
               dict(half0=(0.1, np.nan, 0.1)), dict(half0=(0.1, np.inf, 0.1)), dict(fs=0.0), dict(c=-1.0), dict(seeds=sd[:0]),
               dict(seeds=np.zeros(9, dtype=srp.PEAK))):
        a = dict(z=2, levels=2, half0=Z.HALF0, fs=Z.FS, c=S.C_SOUND, seeds=sd)
        a.update(kw)
        with pytest.raises(ValueError):
            srp.zoom(st, t, mics, a["fs"], a["c"], a["seeds"], a["half0"], a["z"], a["levels"])
    with pytest.raises(ValueError):
        srp.zoom(st[:, :1], 0, mics, Z.FS, S.C_SOUND, sd, Z.HALF0, 2, 2)             # T = 0: no second sample to blend with


def _scene(two):
    mics = S.scene_mics()
    t, st = Z.scene_strips_oracle(two)
    power, clipped = srp.srp_map(st, t, mics, S.SCENE_FS, S.C_SOUND, S.SCENE_LO, S.SCENE_HI, S.SCENE_COUNT)
    assert clipped == 0
    peaks = srp.map_peaks(power.reshape(S.SCENE_COUNT), 2 if two else 1, 3 if two else 1, S.SCENE_LO, S.SCENE_HI)
    zoomed, trail = srp.zoom(st, t, mics, S.SCENE_FS, S.C_SOUND, peaks, Z.scene_half0(), Z.SCENE_Z, Z.SCENE_LEVELS, return_levels=True)
    seed_d = np.linalg.norm(np.stack([peaks["x"], peaks["y"], peaks["z"]], axis=1)[None] - np.stack(S.SCENE_SOURCES)[:, None], axis=2)
    print(f"[srp zoom] seeds' distances [source][peak]: {np.round(seed_d, 3).tolist()}")
    return zoomed, trail, [tr[0][1] for tr in trail]


def test_scene_one_source():
    """W = 2, a 16^3 map, Z = 8, four levels: the zoomed first peak lies within 0.02 m of the source."""
    zoomed, trail, first = _scene(False)
    d, = Z.scene_zoom_check(zoomed, trail, first, False)
    print(f"[srp zoom] one source: {d:.4f} m from the source")


def test_scene_two_sources():
    """K = 2, R = 3: each source has a zoomed peak within 0.03 m."""
    zoomed, trail, first = _scene(True)
    d0, d1 = Z.scene_zoom_check(zoomed, trail, first, True)
    print(f"[srp zoom] two sources: {d0:.4f} m and {d1:.4f} m")
