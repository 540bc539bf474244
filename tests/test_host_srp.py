"""The SRP specification on the host: pyaudiolocalization_amd/srp.py against plain Python loops over (g, p, u) and over the
neighbourhood; csrc/srp_math.h compiled for the CPU (tests/host/test_srp_math.cpp, with the address and undefined-behaviour
sanitizers, -ffp-contract=off) against srp.py bit for bit on grid points, lags, clip decisions, smoothing sums and peak marks; and
the two scenes on the oracle's rows.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import srp_cases as S
from pyaudiolocalization_amd import srp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (M, grid, T): small enough for the plain loops; T = 3 clips most terms
LOOP_CASES = [(2, (1, 1, 1), 40), (3, (2, 3, 5), 40), (5, (7, 1, 40), 40), (5, (1, 1, 257), 3), (17, (4, 4, 4), 40)]
GEOMETRY_CASES = [(m, grid) for m in (2, 3, 5, 17, 64) for grid in S.MAP_GRIDS if m * (m - 1) // 2 * int(np.prod(grid)) <= 2_100_000]
STRIP_CASES = [(64, 0, 0), (64, 5, 0), (64, 63, 0), (64, 31, 32), (64, 7, 3), (257, 256 - 32, 32), (2, 1, 0), (2, 0, 1), (1, 0, 0)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    out = tmp_path_factory.mktemp("srp_math") / "test_srp_math"
    subprocess.run(["hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "pyaudiolocalization_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "test_srp_math.cpp"), "-o", str(out)], check=True)
    return str(out)


def _run(exe, *args):
    run = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True)
    assert run.returncode == 0 and "ALL OK" in run.stdout, run.stdout + run.stderr


def test_half_width_clips_nothing():
    for m in S.MAP_MICS:
        mics = S.map_mics(m)
        t = srp.half_width(mics, S.MAP_FS, S.C_SOUND)
        far = srp.grid_points((-50.0, -60.0, -70.0), (80.0, 90.0, 100.0), (3, 4, 5))       # the largest lags: points far outside the array
        assert np.max(np.abs(srp.lag_values(far, mics, S.MAP_FS, S.C_SOUND))) <= t - 1
    assert srp.half_width(S.scene_mics(), S.SCENE_FS, S.C_SOUND) == 119


@pytest.mark.parametrize("length,t,w", STRIP_CASES)
def test_strips_equal_the_loops(length, t, w):
    rows = np.random.default_rng([length, t, w]).standard_normal((3, 2 * length - 1))
    got = srp.strips(rows, length, t, w)
    assert got.shape == (3, 2 * t + 1) and got.tobytes() == S.loops_strips(rows, length, t, w).tobytes()
    if w == 0:
        n = 2 * length - 1
        assert np.array_equal(got, rows[:, (-np.arange(-t, t + 1)) % n])
    for bad in ((-1, 0), (0, -1), (0, 33), (length - w, w) if w else (length, 0)):
        with pytest.raises(ValueError):
            srp.strips(rows, length, *bad)


@pytest.mark.parametrize("m,grid,t", LOOP_CASES)
def test_map_equals_the_loops(m, grid, t):
    mics = S.map_mics(m)
    assert srp.lag_margin(S.grid_of(grid), mics, S.MAP_FS, S.C_SOUND) >= 1e-9
    st = np.random.default_rng([m, t]).standard_normal((m * (m - 1) // 2, 2 * t + 1))
    for weights in (None, np.random.default_rng(m).uniform(0.5, 2.0, m * (m - 1) // 2)):
        power, clipped, total = srp.srp_map(st, t, mics, S.MAP_FS, S.C_SOUND, S.MAP_LO, S.MAP_HI, grid, weights, return_abs=True, chunk=37)
        want, want_clipped = S.loops_map(st, t, mics, S.MAP_FS, S.C_SOUND, S.MAP_LO, S.MAP_HI, grid, weights)
        assert power.tobytes() == want.tobytes() and clipped == want_clipped
        assert np.all(total >= np.abs(power))
    if t == 3:
        assert clipped > power.size * st.shape[0] // 2                                      # most terms clip


@pytest.mark.parametrize("shape,radius", [((5, 6, 7), 1), ((5, 6, 7), 2), ((1, 1, 9), 1), ((1, 4, 4), 3), ((3, 3, 3), 4), ((9, 2, 1), 1)])
def test_peak_marks_equal_the_loops(shape, radius):
    rng = np.random.default_rng([*shape, radius])
    power = rng.integers(0, 4, shape).astype(np.float64)                                    # many ties and plateaus
    power[rng.integers(0, shape[0]), rng.integers(0, shape[1]), rng.integers(0, shape[2])] = np.nan
    marks = srp.peak_marks(power, radius)
    assert np.array_equal(marks, S.loops_marks(power, radius))
    peaks = srp.map_peaks(power, 8, radius, S.MAP_LO, S.MAP_HI)
    idx = np.flatnonzero(marks.reshape(-1))
    order = sorted(idx, key=lambda g: (-power.reshape(-1)[g], g))[:8]
    assert list(peaks["index"][:len(order)]) == order and np.all(peaks["index"][len(order):] == -1)
    assert np.all(peaks["power"][len(order):] == 0) and np.all(peaks["x"][len(order):] == 0)
    pts = srp.grid_points(S.MAP_LO, S.MAP_HI, shape)
    assert np.array_equal(peaks["x"][:len(order)], pts[order, 0]) and np.array_equal(peaks["z"][:len(order)], pts[order, 2])


def test_plateau_has_one_peak_the_lowest_index():
    power = np.zeros((4, 4, 3))
    power[1:3, 1:3, 1] = 5.0
    peaks = srp.map_peaks(power, 3, 1)
    assert peaks["index"][0] == (1 * 4 + 1) * 3 + 1 and peaks["power"][0] == 5.0
    assert np.count_nonzero(srp.peak_marks(power, 1)[1:3, 1:3, 1]) == 1


@pytest.mark.parametrize("m,grid", GEOMETRY_CASES)
def test_header_geometry_equals_the_specification(exe, tmp_path, m, grid):
    mics = S.map_mics(m)
    t = 30
    np.concatenate([S.MAP_LO, S.MAP_HI, np.asarray(grid, dtype=np.float64), [S.MAP_FS, S.C_SOUND, t, m], mics.reshape(-1)]).tofile(tmp_path / "in.bin")
    _run(exe, "geometry", tmp_path / "in.bin", tmp_path / "points.bin", tmp_path / "lags.bin", tmp_path / "clip.bin")
    pts = srp.grid_points(S.MAP_LO, S.MAP_HI, grid)
    assert np.fromfile(tmp_path / "points.bin").tobytes() == pts.tobytes()
    want = srp.lag_values(pts, mics, S.MAP_FS, S.C_SOUND)
    assert np.fromfile(tmp_path / "lags.bin").tobytes() == want.tobytes()
    assert np.array_equal(np.fromfile(tmp_path / "clip.bin", dtype=np.uint8).reshape(want.shape), ~(np.abs(want) <= t))
    assert np.array_equal(srp.lags(pts, mics, S.MAP_FS, S.C_SOUND), want.astype(np.int32))


def test_header_lag_near_a_half_integer_takes_the_division(exe, tmp_path):
    """Two microphones on the x axis and points on it: the lag is (x_j - x_i) fs / c exactly, and c is chosen so that lags land on and
    next to half-integers, where the product with 1 / c may not decide."""
    mics = np.array([[0.0, 0.0, 0.0], [0.4375, 0.0, 0.0]])
    for c in (0.4375 * 8000.0 / 10.5, 0.4375 * 8000.0 / 11.5, np.nextafter(0.4375 * 8000.0 / 10.5, 1e9), np.nextafter(0.4375 * 8000.0 / 12.5, 0.0)):
        np.concatenate([(-9.0, -0.5, -0.5), (-1.0, 0.5, 0.5), (4.0, 1.0, 1.0), [8000.0, c, 11, 2], mics.reshape(-1)]).tofile(tmp_path / "in.bin")
        _run(exe, "geometry", tmp_path / "in.bin", tmp_path / "points.bin", tmp_path / "lags.bin", tmp_path / "clip.bin")
        pts = srp.grid_points((-9.0, -0.5, -0.5), (-1.0, 0.5, 0.5), (4, 1, 1))
        want = srp.lag_values(pts, mics, 8000.0, c)
        assert np.fromfile(tmp_path / "lags.bin").tobytes() == want.tobytes(), c


@pytest.mark.parametrize("length,t,w", [c for c in STRIP_CASES if c[0] > 1] + [(1500, 1499 - 32, 32)])
def test_header_smoothing_equals_the_specification(exe, tmp_path, length, t, w):
    rows = np.random.default_rng([length, t, w, 1]).standard_normal((2, 2 * length - 1))
    np.concatenate([[length, t, w, 2], rows.reshape(-1)]).tofile(tmp_path / "in.bin")
    _run(exe, "strips", tmp_path / "in.bin", tmp_path / "out.bin")
    assert np.fromfile(tmp_path / "out.bin").tobytes() == srp.strips(rows, length, t, w).tobytes()


@pytest.mark.parametrize("shape,radius", [((5, 6, 7), 1), ((5, 6, 7), 3), ((1, 1, 257), 2), ((16, 1, 4), 4), ((2, 2, 1), 1)])
def test_header_peak_marks_equal_the_specification(exe, tmp_path, shape, radius):
    rng = np.random.default_rng([*shape, radius, 2])
    power = rng.integers(0, 5, shape).astype(np.float64)
    power.reshape(-1)[rng.integers(0, power.size)] = np.nan
    np.concatenate([[*shape, radius], power.reshape(-1)]).tofile(tmp_path / "in.bin")
    _run(exe, "marks", tmp_path / "in.bin", tmp_path / "out.bin")
    assert np.array_equal(np.fromfile(tmp_path / "out.bin", dtype=np.uint8).astype(bool), srp.peak_marks(power, radius).reshape(-1))


@pytest.fixture(scope="module")
def scene_strips():
    """strips[two][P][2T + 1] of the two scenes from the oracle's rows."""
    t = srp.half_width(S.scene_mics(), S.SCENE_FS, S.C_SOUND)
    return t, [srp.strips(S.oracle_rows(S.scene_frames_oracle(two)), S.SCENE_LEN, t, S.SCENE_W) for two in (False, True)]


def _scene_map(scene_strips, two):
    t, st = scene_strips
    power, clipped = srp.srp_map(st[int(two)], t, S.scene_mics(), S.SCENE_FS, S.C_SOUND, S.SCENE_LO, S.SCENE_HI, S.SCENE_COUNT)
    assert clipped == 0
    return power.reshape(S.SCENE_COUNT)


def test_scene_geometry_is_far_from_half_integers():
    pts = srp.grid_points(S.SCENE_LO, S.SCENE_HI, S.SCENE_COUNT)
    assert srp.lag_margin(pts, S.scene_mics(), S.SCENE_FS, S.C_SOUND) >= 1e-9
    for m in S.MAP_MICS:
        for grid in S.MAP_GRIDS:
            assert srp.lag_margin(S.grid_of(grid), S.map_mics(m), S.MAP_FS, S.C_SOUND) >= 1e-9, (m, grid)


def test_scene_one_source(scene_strips):
    peaks = srp.map_peaks(_scene_map(scene_strips, False), 1, 1, S.SCENE_LO, S.SCENE_HI)
    d, = S.scene_check(peaks, False)
    print(f"[srp] one source: the map's maximum is {d:.3f} m from the source")


def test_scene_two_sources(scene_strips):
    power = _scene_map(scene_strips, True)
    for radius in (1, 3):
        peaks = srp.map_peaks(power, 2, radius, S.SCENE_LO, S.SCENE_HI)
        pos = np.stack([peaks["x"], peaks["y"], peaks["z"]], axis=1)
        print(f"[srp] two sources, R = {radius}: peaks at distances "
              f"{np.round(np.linalg.norm(pos[None] - np.stack(S.SCENE_SOURCES)[:, None], axis=2), 3).tolist()} [source][peak]")
    d0, d1 = S.scene_check(peaks, True)                                                       # R = 3
    print(f"[srp] two sources, R = 3: {d0:.3f} m and {d1:.3f} m")


def test_grid_checks():
    for lo, hi, count in (((0, 0, 0), (1, 1, 0), (2, 2, 2)), ((0, 0, 0), (1, 1, np.inf), (2, 2, 2)), ((0, 0, 0), (1, 1, 1), (2, 0, 2)),
                          ((0, 0, 0), (1, 1, 1), (1025, 1, 1)), ((0, 0, 0), (1, 1, 1), (1024, 1024, 17))):
        with pytest.raises(ValueError):
            srp.grid_points(lo, hi, count)
