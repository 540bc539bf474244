"""The direction map on the device (pal_srp_doa*, pal_srp_doa_peaks*, pal_srp_doa_zoom*; k_srp_doa, k_srp_doa_peaks, k_srp_doa_zoom)
against its NumPy specification (srp.doa_map, srp.doa_peaks, srp.doa_zoom).

- Maps byte for byte (``tobytes()``) on integer strips and on real strips with weights: the order of the sum is part of the rule, so
  there is no tolerance.  M = 2, 3, 16, 17, 33, 64 cover the tile borders; the grids (1, 1), (1, 257), (257, 1), (3, 5) and (72, 36)
  cover one lane, a second workgroup with one lane, both axes alone and the scene's sphere; B = 1 equals one frame of B = 3; a T = 3
  case clips, with the count checked; every output may be NULL.
- Peaks on crafted maps: equal maxima on both sides of the azimuth seam with wrap on and off, n_az = 1 and 2 with R = 4, a plateau,
  NaN cells, K beyond the number of peaks.
- The zoom byte for byte: M = 2 .. 64, Z = 2, 7, 16 (4, 49 and 256 lanes of the one chunk), 1, 2 and 16 levels, K = 1 and K = 3 with an
  absent seed, B = 1 and 3, seeds along every coordinate axis, a zero and a NaN seed (NaN equal to NaN).
- The _dev forms against the host forms, every refusal, the chain simulate -> strips -> direction map -> zoom on the scenes, and
  main.srp_directions_device."""
import numpy as np
import pytest

import srp_cases as S
import srp_doa_cases as D
import srp_zoom_cases as Z
from pyaudiolocalization_amd import _ffi, main, srp

pytestmark = pytest.mark.gpu

# (M, grid, B, integer strips, weighted)
MAP_SHAPES = [(2, (1, 1), 1, True, False), (2, (72, 36), 1, False, True), (3, (1, 257), 3, False, True), (3, (3, 5), 1, True, True),
              (16, (257, 1), 1, False, False), (16, (3, 5), 3, True, True), (17, (72, 36), 1, True, False), (17, (1, 257), 1, False, True),
              (33, (3, 5), 3, False, True), (33, (257, 1), 1, True, True), (64, (72, 36), 1, False, True), (64, (1, 1), 3, True, False)]
# (M, Z, levels, K, B, weighted)
ZOOM_SHAPES = [(2, 2, 1, 1, 1, False), (2, 16, 16, 3, 1, True), (3, 7, 2, 3, 3, True), (16, 7, 16, 1, 1, False), (16, 16, 1, 3, 3, True),
               (17, 2, 16, 3, 3, True), (17, 16, 2, 1, 1, False), (33, 7, 1, 1, 3, True), (33, 16, 2, 3, 1, False), (64, 2, 2, 1, 1, False),
               (64, 7, 16, 3, 1, True), (64, 16, 1, 1, 3, True)]


def test_shapes_cover_the_table():
    assert sorted({s[0] for s in MAP_SHAPES}) == D.MAP_MICS and sorted({s[1] for s in MAP_SHAPES}) == sorted(D.MAP_GRIDS)
    assert all({s[n] for s in MAP_SHAPES} == {False, True} for n in (3, 4)) and {s[2] for s in MAP_SHAPES} == {1, 3}
    for n, values in enumerate((D.MAP_MICS, [2, 7, 16], [1, 2, 16], [1, 3], [1, 3], [False, True])):
        assert sorted({s[n] for s in ZOOM_SHAPES}) == values


def _spec_map(st, t, mics, az, el, wt=None):
    out = [srp.doa_map(st[f], t, mics, D.FS, S.C_SOUND, az, el, None if wt is None else wt[f]) for f in range(st.shape[0])]
    return np.stack([p for p, _ in out]), np.array([c for _, c in out])


def _spec_peaks(power, grid, k, r, wrap, az, el):
    return np.stack([srp.doa_peaks(p.reshape(grid), k, r, wrap, az, el) for p in power])


@pytest.mark.parametrize("m,grid,b,integer,weighted", MAP_SHAPES)
def test_map_equals_the_specification(engine, m, grid, b, integer, weighted):
    mics = S.map_mics(m)
    az, el, wrap = D.axes(*grid)
    t = srp.half_width(mics, D.FS, S.C_SOUND)
    st = S.integer_strips(m, t, b) if integer else Z.real_strips(m, t, b)
    wt = None if not weighted else S.integer_weights(m, b) if integer else Z.real_weights(m, b)
    power, peaks, summ = engine.srp_doa(st, mics, D.FS, S.C_SOUND, az, el, wrap, wt, K=3, R=2)
    want, clipped = _spec_map(st, t, mics, az, el, wt)
    assert power.shape == (b, grid[0] * grid[1]) and power.tobytes() == want.tobytes()
    assert not np.any(clipped) and not np.any(summ["clipped"])                       # half_width clips nothing
    want_peaks = _spec_peaks(want, grid, 3, 2, wrap, az, el)
    assert peaks.tobytes() == want_peaks.tobytes() and summ["n_peaks"].tolist() == np.count_nonzero(want_peaks["index"] >= 0, axis=1).tolist()
    if b == 3:
        alone = engine.srp_doa(st[1], mics, D.FS, S.C_SOUND, az, el, wrap, None if wt is None else wt[1], K=3, R=2)
        assert alone[0][0].tobytes() == power[1].tobytes() and alone[1][0].tobytes() == peaks[1].tobytes()


@pytest.mark.parametrize("m,grid", [(5, (3, 5)), (17, (1, 257)), (33, (72, 36))])
def test_map_clips(engine, m, grid):
    """T = 3: most lags fall outside the strip; power and counts equal the specification's."""
    mics, t, b = S.map_mics(m), 3, 2
    az, el, wrap = D.axes(*grid)
    st, wt = Z.real_strips(m, t, b), Z.real_weights(m, b)
    power, _, summ = engine.srp_doa(st, mics, D.FS, S.C_SOUND, az, el, wrap, wt)
    want, clipped = _spec_map(st, t, mics, az, el, wt)
    assert np.all(clipped > 0) and summ["clipped"].tolist() == clipped.tolist() and power.tobytes() == want.tobytes()


def test_map_null_outputs(engine):
    m, grid, b = 17, (3, 5), 2
    mics = S.map_mics(m)
    az, el, wrap = D.axes(*grid)
    t = srp.half_width(mics, D.FS, S.C_SOUND)
    st = Z.real_strips(m, t, b)
    full = engine.srp_doa(st, mics, D.FS, S.C_SOUND, az, el, wrap, K=2, R=1)
    for names in (("power",), ("peaks",), ("summary",), ("power", "summary"), ("peaks", "summary"), ("power", "peaks")):
        got = engine.srp_doa(st, mics, D.FS, S.C_SOUND, az, el, wrap, K=2, R=1, outputs=names)
        for n, name in enumerate(("power", "peaks", "summary")):
            assert (got[n] is None) == (name not in names)
            assert got[n] is None or got[n].tobytes() == full[n].tobytes(), (names, name)
    power, peaks, summ = engine.srp_doa(st, mics, D.FS, S.C_SOUND, az, el, wrap, K=0)       # K = 0: the map and the clip counts alone
    assert peaks is None and power.tobytes() == full[0].tobytes() and summ["n_peaks"].tolist() == [0, 0]


@pytest.mark.parametrize("wrap", [0, 1])
def test_peaks_on_crafted_maps(engine, wrap):
    for name, power, radius, k in D.crafted_maps():
        az, el, _ = D.axes(*power.shape)
        both = np.stack([power, power[::-1].copy()])                                   # two frames: another map in the second
        peaks, summ = engine.srp_doa_peaks(both, az, el, wrap, k, radius)
        want = _spec_peaks(both.reshape(2, -1), power.shape, k, radius, wrap, az, el)
        assert peaks.tobytes() == want.tobytes(), (name, peaks, want)
        assert summ["n_peaks"].tolist() == np.count_nonzero(want["index"] >= 0, axis=1).tolist() and not np.any(summ["clipped"])
    seam = D.crafted_maps()[0][1]
    got = engine.srp_doa_peaks(seam, *D.axes(*seam.shape)[:2], wrap, 4, 1)[0][0]
    assert got["index"].tolist() == ([3, 43, 0, -1] if wrap else [3, 80, 43, 0])        # cell 0 leads the plateau of zeros


@pytest.mark.parametrize("m,z,levels,k,b,weighted", ZOOM_SHAPES)
def test_zoom_equals_the_specification(engine, m, z, levels, k, b, weighted):
    mics = S.map_mics(m)
    t = srp.half_width(mics, D.FS, S.C_SOUND)
    st = Z.real_strips(m, t, b)
    wt = Z.real_weights(m, b) if weighted else None
    sd = D.seeds(b, k, absent=(1,) if k == 3 else ())
    got = engine.srp_doa_zoom(st, mics, D.FS, S.C_SOUND, sd, D.HALF0, z, levels, wt)
    want = np.stack([srp.doa_zoom(st[f], t, mics, D.FS, S.C_SOUND, sd[f], D.HALF0, z, levels, None if wt is None else wt[f]) for f in range(b)])
    assert got.shape == (b, k) and got.dtype == _ffi.SRP_ZOOM
    assert got.tobytes() == want.tobytes(), (got, want)
    assert np.all(got["clipped"] == 0) and np.all(got["levels"][got["seed"] >= 0] == levels)
    if k == 3:
        assert np.all(got["seed"][:, 1] == -1) and np.all(got["seed"][:, [0, 2]] == sd["index"][:, [0, 2]])
    if b == 3:
        alone = engine.srp_doa_zoom(st[1], mics, D.FS, S.C_SOUND, sd[1, :1], D.HALF0, z, levels, None if wt is None else wt[1])
        assert alone.shape == (1, 1) and alone[0, 0].tobytes() == got[1, 0].tobytes()      # a record depends neither on B nor on K


@pytest.mark.parametrize("m,z", [(5, 7), (17, 16)])
def test_zoom_special_seeds_and_clips(engine, m, z):
    """Seeds along each coordinate axis, a zero seed and a NaN seed (NaN equal to NaN); then T = 3, where most terms clip."""
    mics = S.map_mics(m)
    t = srp.half_width(mics, D.FS, S.C_SOUND)
    st, wt, sd = Z.real_strips(m, t, 1), Z.real_weights(m, 1), D.special_seeds()
    got = engine.srp_doa_zoom(st, mics, D.FS, S.C_SOUND, sd, D.HALF0, z, 2, wt)
    want = srp.doa_zoom(st[0], t, mics, D.FS, S.C_SOUND, sd[0], D.HALF0, z, 2, wt[0])
    assert D.records_equal(got[0], want), (got, want)
    assert got[0, :6].tobytes() == want[:6].tobytes() and np.all(got["clipped"][0, 6:] == 2 * z * z * st.shape[1])
    st3 = Z.real_strips(m, 3, 1)
    got = engine.srp_doa_zoom(st3, mics, D.FS, S.C_SOUND, sd[:, :6], D.HALF0, z, 2, wt)
    want = srp.doa_zoom(st3[0], 3, mics, D.FS, S.C_SOUND, sd[0, :6], D.HALF0, z, 2, wt[0])
    assert np.all(want["clipped"] > 0) and got[0].tobytes() == want.tobytes()


def test_zoom_constant_and_nan_strips(engine):
    m, z = 5, 4
    mics = S.map_mics(m)
    t = srp.half_width(mics, D.FS, S.C_SOUND)
    seed = D.one_seed(0.6, 0.0, 0.8, index=11)
    for value in (0.75, np.nan):                                                       # every cell ties: index 0 wins; no cell counts: the zoom stops
        st = np.full((1, m * (m - 1) // 2, 2 * t + 1), value)
        got = engine.srp_doa_zoom(st, mics, D.FS, S.C_SOUND, seed, D.HALF0, z, 3)
        assert D.records_equal(got[0], srp.doa_zoom(st[0], t, mics, D.FS, S.C_SOUND, seed, D.HALF0, z, 3))
    assert got["levels"][0, 0] == 0 and np.isnan(got["power"][0, 0]) and (got["x"][0, 0], got["y"][0, 0], got["z"][0, 0]) == (0.6, 0.0, 0.8)


def test_dev_forms_equal_the_host_forms(engine):
    m, b, k, z, levels, grid = 17, 3, 3, 7, 2, (9, 31)
    mics = S.map_mics(m)
    az, el, wrap = D.axes(*grid)
    g = grid[0] * grid[1]
    t = srp.half_width(mics, D.FS, S.C_SOUND)
    st, wt = Z.real_strips(m, t, b), Z.real_weights(m, b)
    power, peaks, summ = (np.zeros((b, g)), np.zeros((b, k), dtype=_ffi.SRP_PEAK), np.zeros(b, dtype=_ffi.SRP_FRAME))
    zoomed = np.zeros((b, k), dtype=_ffi.SRP_ZOOM)
    dev = [engine.alloc(a.nbytes) for a in (st, wt, power, peaks, summ, zoomed)]
    try:
        engine.upload(dev[0], st)
        engine.upload(dev[1], wt)
        for weights in (wt, None):
            want = engine.srp_doa(st, mics, D.FS, S.C_SOUND, az, el, wrap, weights, K=k, R=2)
            for d, a in zip(dev[2:], (power, peaks, summ, zoomed)):
                engine.upload(d, np.full(a.nbytes, 0xA5, dtype=np.uint8))
            engine.srp_doa_dev(dev[0], b, t, mics, D.FS, S.C_SOUND, az, el, wrap, dev[1] if weights is not None else 0, k, 2, dev[2], dev[3], dev[4])
            engine.synchronize()
            for d, a, w in zip(dev[2:5], (power, peaks, summ), want):
                assert engine.download(a, d).tobytes() == w.tobytes()
            engine.upload(dev[3], np.full(peaks.nbytes, 0xA5, dtype=np.uint8))
            engine.srp_doa_peaks_dev(dev[2], b, az, el, wrap, k, 2, dev[3], dev[4])     # the stored map's peaks: the same, clipped = 0
            engine.synchronize()
            assert engine.download(peaks, dev[3]).tobytes() == want[1].tobytes() == engine.srp_doa_peaks(want[0], az, el, wrap, k, 2)[0].tobytes()
            assert not np.any(engine.download(summ, dev[4])["clipped"])
            want_zoom = engine.srp_doa_zoom(st, mics, D.FS, S.C_SOUND, want[1], D.HALF0, z, levels, weights)
            engine.srp_doa_zoom_dev(dev[0], b, t, mics, D.FS, S.C_SOUND, dev[3], k, D.HALF0, z, levels, dev[5], dev[1] if weights is not None else 0)
            engine.synchronize()
            assert engine.download(zoomed, dev[5]).tobytes() == want_zoom.tobytes()
    finally:
        for d in dev:
            engine.free(d)


def _raw(engine, symbol, *args):
    return getattr(engine._lib, symbol)(engine._h, *args)


def _ptr(a):
    return None if a is None else a.ctypes.data


def test_errors(engine):
    m, t = 3, 5
    mics = S.map_mics(m)
    az, el, _ = D.axes(3, 5)
    st, sd = Z.real_strips(m, t, 1), D.seeds(1, 8)
    power, peaks, summ = np.zeros((1, 15)), np.zeros((1, 8), dtype=_ffi.SRP_PEAK), np.zeros(1, dtype=_ffi.SRP_FRAME)
    out = np.zeros((1, 8), dtype=_ffi.SRP_ZOOM)
    big_az, nan_el = np.zeros((1025, 2)), el.copy()
    nan_el[2, 1] = np.nan
    good = dict(B=1, M=m, T=t, fs=D.FS, c=S.C_SOUND, K=1, R=1, n_az=3, n_el=5, az=az, el=el, mics=mics, strips=st, grid=True,
                power=power, peaks=peaks, summary=summ)
    common = [dict(B=0), dict(fs=0.0), dict(fs=np.nan), dict(c=0.0), dict(c=np.inf), dict(M=1), dict(mics=None), dict(strips=None)]
    tables = [dict(n_az=0), dict(n_el=0), dict(n_az=-1), dict(az=None), dict(el=None), dict(grid=False), dict(el=nan_el)]
    map_invalid = common + tables + [dict(T=-1), dict(K=-1), dict(K=9), dict(R=0), dict(R=5), dict(power=None, peaks=None, summary=None),
                                     dict(K=0, power=None, summary=None), dict(mics=np.full((3, 3), np.inf))]
    unsupported = [dict(n_az=1025, az=big_az), dict(n_el=1025, el=big_az)]

    def call_map(a, symbol):
        grid = _ffi.SrpDoaGrid(a["n_az"], a["n_el"], 1, 0)
        return _raw(engine, symbol, _ptr(a["strips"]), a["B"], a["M"], a["T"], _ptr(a["mics"]), a["fs"], a["c"], grid if a["grid"] else None,
                    _ptr(a["az"]), _ptr(a["el"]), None, a["K"], a["R"], _ptr(a["power"]), _ptr(a["peaks"]), _ptr(a["summary"]))

    def call_peaks(a, symbol):
        grid = _ffi.SrpDoaGrid(a["n_az"], a["n_el"], 1, 0)
        return _raw(engine, symbol, _ptr(a["power"]), a["B"], grid if a["grid"] else None, _ptr(a["az"]), _ptr(a["el"]), a["K"], a["R"],
                    _ptr(a["peaks"]), _ptr(a["summary"]))

    for cases, code in ((map_invalid, _ffi.ERR_INVALID), (unsupported, _ffi.ERR_UNSUPPORTED)):
        for kw in cases:
            a = dict(good)
            a.update(kw)
            for symbol in ("pal_srp_doa", "pal_srp_doa_dev"):
                assert call_map(a, symbol) == code, (symbol, kw)
    assert call_map(dict(good, M=4097, mics=np.zeros((4097, 3))), "pal_srp_doa") == _ffi.ERR_UNSUPPORTED
    peaks_invalid = [dict(B=0), dict(K=0), dict(K=9), dict(R=0), dict(R=5), dict(power=None), dict(peaks=None)] + tables
    for cases, code in ((peaks_invalid, _ffi.ERR_INVALID), (unsupported, _ffi.ERR_UNSUPPORTED)):
        for kw in cases:
            a = dict(good)
            a.update(kw)
            for symbol in ("pal_srp_doa_peaks", "pal_srp_doa_peaks_dev"):
                assert call_peaks(a, symbol) == code, (symbol, kw)
    zoom_good = dict(B=1, M=m, T=t, fs=D.FS, c=S.C_SOUND, K=1, Z=2, levels=1, half0=0.1, mics=mics, strips=st, seeds=sd, out=out)
    zoom_invalid = common + [dict(Z=1), dict(Z=17), dict(Z=-3), dict(levels=0), dict(levels=17), dict(K=0), dict(K=9), dict(T=0), dict(T=-1),
                             dict(half0=0.0), dict(half0=-0.1), dict(half0=np.nan), dict(half0=np.inf), dict(seeds=None), dict(out=None)]
    for kw in zoom_invalid:
        a = dict(zoom_good)
        a.update(kw)
        for symbol in ("pal_srp_doa_zoom", "pal_srp_doa_zoom_dev"):
            rc = _raw(engine, symbol, _ptr(a["strips"]), a["B"], a["M"], a["T"], _ptr(a["mics"]), a["fs"], a["c"], None, _ptr(a["seeds"]), a["K"],
                      a["half0"], a["Z"], a["levels"], _ptr(a["out"]))
            assert rc == _ffi.ERR_INVALID, (symbol, kw, rc)
    # refused before any buffer is touched
    assert not any(a.tobytes().strip(b"\0") for a in (power, peaks, summ, out))
    # the same through Python
    for kw in (dict(az=az[:, :1]), dict(el=nan_el), dict(K=9), dict(R=5), dict(fs=0.0), dict(mics=mics[:2]), dict(strips=st[:, :, :2])):
        a = dict(good, K=1)
        a.update(kw)
        with pytest.raises(ValueError):
            engine.srp_doa(a["strips"], a["mics"], a["fs"], a["c"], a["az"], a["el"], 1, None, a["K"], a["R"])
    with pytest.raises(_ffi.PalError):
        engine.srp_doa(st, mics, D.FS, S.C_SOUND, big_az, el)
    for kw in (dict(Z=1), dict(levels=17), dict(half0=0.0), dict(half0=(0.1, 0.1, 0.1)), dict(seeds=np.zeros((1, 9), dtype=_ffi.SRP_PEAK))):
        a = dict(zoom_good, seeds=sd[:, :1])
        a.update(kw)
        with pytest.raises(ValueError):
            engine.srp_doa_zoom(st, mics, D.FS, S.C_SOUND, a["seeds"], a["half0"], a["Z"], a["levels"])
    with pytest.raises(ValueError):
        engine.srp_doa_peaks(np.zeros((3, 5)), az, el, 1, 0, 1)
    # a refused call leaves the engine usable
    got = engine.srp_doa(st, mics, D.FS, S.C_SOUND, az, el)[0]
    assert got[0].tobytes() == srp.doa_map(st[0], t, mics, D.FS, S.C_SOUND, az, el)[0].tobytes()


@pytest.fixture(scope="module")
def scene_frames(engine):
    """frames[2][M][L]: the one-source and the two-source scene, 6 m away, from engine.simulate_multipath."""
    one = []
    for which in range(2):
        delays, gains, total = S.scene_paths(D.scene_sources()[which])
        one.append(engine.simulate_multipath(S.scene_base(which)[None], S.SCENE_FS, total, delays[None], gains[None], S.SCENE_LEN)[0])
    return np.stack([one[0], one[0] + S.SCENE_GAIN2 * one[1]])


def test_chain(engine, scene_frames):
    mics = S.scene_mics()
    az, el, wrap = D.axes(D.SCENE_AZ, D.SCENE_EL)
    t = srp.half_width(mics, S.SCENE_FS, S.C_SOUND)
    strips, _ = engine.gcc_phat_all_pairs_strips(scene_frames, S.SCENE_FS, t, D.SCENE_W)
    power, peaks, summ = engine.srp_doa(strips, mics, S.SCENE_FS, S.C_SOUND, az, el, wrap, K=2, R=1)
    zoomed = engine.srp_doa_zoom(strips, mics, S.SCENE_FS, S.C_SOUND, peaks, D.SCENE_HALF0, D.SCENE_Z, D.SCENE_LEVELS)
    assert not np.any(summ["clipped"]) and not np.any(zoomed["clipped"])
    for f in range(2):                                                                 # the device's own strips through the specification
        want, _ = srp.doa_map(strips[f], t, mics, S.SCENE_FS, S.C_SOUND, az, el)
        assert power[f].tobytes() == want.tobytes()
        assert peaks[f].tobytes() == srp.doa_peaks(want.reshape(D.SCENE_AZ, D.SCENE_EL), 2, 1, wrap, az, el).tobytes()
        assert zoomed[f].tobytes() == srp.doa_zoom(strips[f], t, mics, S.SCENE_FS, S.C_SOUND, peaks[f], D.SCENE_HALF0, D.SCENE_Z, D.SCENE_LEVELS).tobytes()
    d, = D.scene_check(peaks[0][:1], False, D.MAP_BOUND_DEG)
    z, = D.scene_check(zoomed[0][:1], False, D.ZOOM_BOUND_DEG)
    d2, z2 = D.scene_check(peaks[1], True, D.MAP_BOUND_DEG), D.scene_check(zoomed[1], True, D.ZOOM_BOUND_DEG)
    print(f"[srp doa] device chain: one source map {d:.3f} zoom {z:.3f} deg; two sources map {d2[0]:.3f} {d2[1]:.3f} zoom {z2[0]:.3f} {z2[1]:.3f} deg")
    got = main.srp_directions_device(scene_frames, mics, S.SCENE_FS, S.C_SOUND, K=2, engine=engine, zoom=(D.SCENE_Z, D.SCENE_LEVELS))
    assert isinstance(got, tuple) and got[0].tobytes() == peaks.tobytes() and got[1].tobytes() == zoomed.tobytes()
    plain = main.srp_directions_device(scene_frames, mics, S.SCENE_FS, S.C_SOUND, K=2, engine=engine)
    assert isinstance(plain, np.ndarray) and plain.dtype == _ffi.SRP_PEAK and plain.tobytes() == peaks.tobytes()
    wide = main.srp_directions_device(scene_frames[0], mics, S.SCENE_FS, S.C_SOUND, 36, 18, engine=engine, zoom=(D.SCENE_Z, D.SCENE_LEVELS, 1.0))
    assert wide[0].shape == (1,) and wide[1].shape == (1,)
    z, = D.scene_check(wide[1], False, D.ZOOM_BOUND_DEG)
    azd, eld = srp.doa_angles(wide[1])
    print(f"[srp doa] from the 36 x 18 map: {z:.3f} deg from the source, azimuth {azd[0]:.2f} elevation {eld[0]:.2f} deg")
