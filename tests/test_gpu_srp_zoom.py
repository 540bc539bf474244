"""The coarse-to-fine zoom on the device (pal_srp_zoom*, k_srp_zoom) against its NumPy specification (srp.zoom).

- Records byte for byte (``tobytes()``) on real-valued strips and weights: the order of the sum is part of the rule, so there is no
  tolerance.  The shapes cover the tile borders (M = 2, 3, 16, 17, 33, 64), Z = 2 (8 cells, under one wavefront), 6 (216: one chunk, not
  full), 7 (343: two chunks, the second nearly empty) and 16 (4096: sixteen full chunks), 1, 2 and 16 levels (at 16 the box has shrunk to
  a point: every cell ties), K = 1 and K = 3 with the middle seed absent, B = 1 and B = 3 with frame 1 of the batch against that frame
  alone.  Every value appears; the cross product is thinned so that the specification, P * Z^3 * levels terms per seed, stays cheap.
- A clip case (T = 3), all terms clipped, constant strips, NaN strips before and after a completed level.
- The _dev form against the host form.
- Every refusal of include/pal_hip.h, as the return code of the raw symbols and as ValueError from Python.
- Chain: the two scenes of tests/test_host_srp_zoom.py through simulate -> strips -> map -> zoom, and main.srp_positions_device."""
import numpy as np
import pytest

import srp_cases as S
import srp_zoom_cases as Z
from pyaudiolocalization_amd import _ffi, main, srp

pytestmark = pytest.mark.gpu

# (M, Z, levels, K, B, weighted)
SHAPES = [(2, 2, 1, 1, 1, False), (2, 16, 16, 1, 1, True), (3, 6, 2, 3, 3, True), (3, 7, 16, 3, 1, False), (16, 7, 2, 1, 3, True),
          (16, 16, 1, 3, 1, False), (17, 2, 16, 3, 3, True), (17, 6, 1, 1, 1, False), (17, 16, 2, 1, 1, True), (33, 7, 2, 3, 1, True),
          (33, 6, 16, 1, 1, False), (33, 16, 1, 1, 3, True), (64, 2, 2, 1, 1, False), (64, 6, 1, 3, 3, True), (64, 7, 16, 1, 1, True),
          (64, 16, 2, 1, 1, False)]


def test_shapes_cover_the_table():
    for n, values in enumerate(([2, 3, 16, 17, 33, 64], [2, 6, 7, 16], [1, 2, 16], [1, 3], [1, 3], [False, True])):
        assert sorted({s[n] for s in SHAPES}) == values


def _spec(st, t, mics, fs, sd, half0, z, levels, wt=None):
    """srp.zoom frame by frame -> out[B][K]."""
    return np.stack([srp.zoom(st[f], t, mics, fs, S.C_SOUND, sd[f], half0, z, levels, None if wt is None else wt[f]) for f in range(st.shape[0])])


@pytest.mark.parametrize("m,z,levels,k,b,weighted", SHAPES)
def test_zoom_equals_the_specification(engine, m, z, levels, k, b, weighted):
    mics = S.map_mics(m)
    t = srp.half_width(mics, Z.FS, S.C_SOUND)
    st = Z.real_strips(m, t, b)
    wt = Z.real_weights(m, b) if weighted else None
    sd = Z.seeds(b, k, absent=(1,) if k == 3 else ())
    got = engine.srp_zoom(st, mics, Z.FS, S.C_SOUND, sd, Z.HALF0, z, levels, wt)
    want = _spec(st, t, mics, Z.FS, sd, Z.HALF0, z, levels, wt)
    assert got.shape == (b, k) and got.dtype == _ffi.SRP_ZOOM
    assert got.tobytes() == want.tobytes(), (got, want)
    assert np.all(got["clipped"] == 0) and np.all(got["levels"][got["seed"] >= 0] == levels)
    if k == 3:
        assert np.all(got["seed"][:, 1] == -1) and np.all(got["seed"][:, [0, 2]] == sd["index"][:, [0, 2]])
    if b == 3:
        alone = engine.srp_zoom(st[1], mics, Z.FS, S.C_SOUND, sd[1], Z.HALF0, z, levels, None if wt is None else wt[1])
        assert alone.shape == (1, k) and alone[0].tobytes() == got[1].tobytes()
        first = engine.srp_zoom(st[1], mics, Z.FS, S.C_SOUND, sd[1, :1], Z.HALF0, z, levels, None if wt is None else wt[1])
        assert first[0, 0].tobytes() == got[1, 0].tobytes()                           # nor does a record depend on K


@pytest.mark.parametrize("m,z,levels", [(5, 7, 2), (17, 16, 1)])
def test_zoom_clips(engine, m, z, levels):
    """T = 3: most terms clip; the counts equal the specification's, and so do the records."""
    mics, t = S.map_mics(m), 3
    st, wt, sd = Z.real_strips(m, t, 2), Z.real_weights(m, 2), Z.seeds(2, 2)
    got = engine.srp_zoom(st, mics, Z.FS, S.C_SOUND, sd, Z.HALF0, z, levels, wt)
    want = _spec(st, t, mics, Z.FS, sd, Z.HALF0, z, levels, wt)
    assert np.all(want["clipped"] > levels * z ** 3 * st.shape[1] // 2)
    assert np.array_equal(got["clipped"], want["clipped"]) and got.tobytes() == want.tobytes()


def test_all_terms_clipped(engine):
    mics, t, st, seed, half0, z, levels = Z.all_clipped()
    got = engine.srp_zoom(st, mics, Z.FS, S.C_SOUND, seed, half0, z, levels)
    assert got[0].tobytes() == srp.zoom(st, t, mics, Z.FS, S.C_SOUND, seed, half0, z, levels).tobytes()
    assert got["power"][0, 0] == 0.0 and got["clipped"][0, 0] == levels * z ** 3 and got["levels"][0, 0] == levels
    assert (got["x"][0, 0], got["y"][0, 0], got["z"][0, 0]) == (100.0 - 0.5 * 0.75 * 1.5,) + (-0.5 * 0.75 * 1.5,) * 2    # index 0 twice


@pytest.mark.parametrize("m,z", [(5, 4), (17, 7)])
def test_constant_strips(engine, m, z):
    """Every cell ties at every level: index 0, the corner cell, wins whatever the reduction's shape."""
    mics = S.map_mics(m)
    t = srp.half_width(mics, Z.FS, S.C_SOUND)
    st = np.full((1, m * (m - 1) // 2, 2 * t + 1), 0.75)
    seed, half0, levels = Z.one_seed(0.5, 0.25, 0.125), (0.5, 0.25, 1.0), 3
    got = engine.srp_zoom(st, mics, Z.FS, S.C_SOUND, seed, half0, z, levels)
    want = srp.zoom(st[0], t, mics, Z.FS, S.C_SOUND, seed, half0, z, levels)
    assert got[0].tobytes() == want.tobytes()
    # index 0 at every level: the centre moves by -half (1 - 1 / Z) per level, half shrinking by Z / 2
    ctr, half = np.array([0.5, 0.25, 0.125]), np.array(half0)
    for _ in range(levels):
        lo, hi = srp.zoom_box(ctr, half)
        ctr, half = srp.grid_points(lo, hi, (z, z, z))[0], srp.zoom_next_half(lo, hi, z)
    assert (got["x"][0, 0], got["y"][0, 0], got["z"][0, 0]) == tuple(ctr)
    if z == 4:
        assert tuple(ctr) == (0.5 - 0.5 * 1.3125, 0.25 - 0.25 * 1.3125, 0.125 - 1.3125)     # exact: every figure is dyadic


def test_nan_strips(engine):
    m = 3
    mics = S.map_mics(m)
    t = srp.half_width(mics, Z.FS, S.C_SOUND)
    seed = Z.one_seed(0.3, 0.4, 0.5, index=11)
    st = np.full((1, 3, 2 * t + 1), np.nan)
    got = engine.srp_zoom(st, mics, Z.FS, S.C_SOUND, seed, Z.HALF0, 3, 4)
    assert got[0].tobytes() == srp.zoom(st[0], t, mics, Z.FS, S.C_SOUND, seed, Z.HALF0, 3, 4).tobytes()
    assert got["levels"][0, 0] == 0 and np.isnan(got["power"][0, 0]) and (got["x"][0, 0], got["y"][0, 0], got["z"][0, 0]) == (0.3, 0.4, 0.5)
    mics, t, st, seed, half0, z, centre = Z.nan_second_level()                         # the stop after a completed level
    got = engine.srp_zoom(st, mics, Z.FS, S.C_SOUND, seed, half0, z, 3)
    assert got[0].tobytes() == srp.zoom(st, t, mics, Z.FS, S.C_SOUND, seed, half0, z, 3).tobytes()
    assert got["levels"][0, 0] == 1 and np.isnan(got["power"][0, 0]) and (got["x"][0, 0], got["y"][0, 0], got["z"][0, 0]) == tuple(centre)


def test_zoom_dev_equals_the_host_form(engine):
    m, b, k, z, levels = 17, 3, 3, 6, 2
    mics = S.map_mics(m)
    t = srp.half_width(mics, Z.FS, S.C_SOUND)
    st, wt, sd = Z.real_strips(m, t, b), Z.real_weights(m, b), Z.seeds(b, k, absent=(1,))
    out = np.zeros((b, k), dtype=_ffi.SRP_ZOOM)
    dev = [engine.alloc(a.nbytes) for a in (st, wt, sd, out)]
    try:
        engine.upload(dev[0], st)
        engine.upload(dev[1], wt)
        engine.upload(dev[2], sd)
        for weights in (wt, None):
            want = engine.srp_zoom(st, mics, Z.FS, S.C_SOUND, sd, Z.HALF0, z, levels, weights)
            engine.upload(dev[3], np.full(out.nbytes, 0xA5, dtype=np.uint8))
            engine.srp_zoom_dev(dev[0], b, t, mics, Z.FS, S.C_SOUND, dev[2], k, Z.HALF0, z, levels, dev[3], dev[1] if weights is not None else 0)
            engine.synchronize()
            assert engine.download(out, dev[3]).tobytes() == want.tobytes()
    finally:
        for d in dev:
            engine.free(d)


def _raw(engine, symbol, *args):
    return getattr(engine._lib, symbol)(engine._h, *args)


def test_errors(engine):
    m, t = 3, 5
    mics = S.map_mics(m)
    st, sd = Z.real_strips(m, t, 1), Z.seeds(1, 8)
    out = np.zeros((1, 8), dtype=_ffi.SRP_ZOOM)
    good = dict(B=1, M=m, T=t, fs=Z.FS, c=S.C_SOUND, K=1, Z=2, levels=1, half0=(0.1, 0.1, 0.1), mics=mics, strips=st, seeds=sd, out=out)
    invalid = [dict(Z=1), dict(Z=17), dict(Z=0), dict(Z=-3), dict(levels=0), dict(levels=17), dict(levels=-1), dict(K=0), dict(K=9), dict(K=-1),
               dict(T=0), dict(T=-1), dict(half0=(0.1, 0.0, 0.1)), dict(half0=(-0.1, 0.1, 0.1)), dict(half0=(0.1, 0.1, np.nan)),
               dict(half0=(np.inf, 0.1, 0.1)), dict(half0=None), dict(strips=None), dict(seeds=None), dict(out=None), dict(mics=None),
               dict(M=1), dict(B=0), dict(fs=0.0), dict(fs=-1.0), dict(fs=np.nan), dict(c=0.0), dict(c=-343.0), dict(c=np.inf)]
    for kw in invalid:
        a = dict(good)
        a.update(kw)
        h0 = None if a["half0"] is None else np.asarray(a["half0"], dtype=np.float64)
        ptrs = {name: None if a[name] is None else a[name].ctypes.data for name in ("strips", "mics", "seeds", "out")}
        for symbol in ("pal_srp_zoom", "pal_srp_zoom_dev"):
            rc = _raw(engine, symbol, ptrs["strips"], a["B"], a["M"], a["T"], ptrs["mics"], a["fs"], a["c"], None, ptrs["seeds"], a["K"],
                      None if h0 is None else h0.ctypes.data, a["Z"], a["levels"], ptrs["out"])
            assert rc == _ffi.ERR_INVALID, (symbol, kw, rc)                           # refused before any buffer is touched
    assert not out.tobytes().strip(b"\0")
    # the same through Python
    for kw in (dict(Z=1), dict(Z=17), dict(levels=0), dict(levels=17), dict(half0=(0.1, 0.0, 0.1)), dict(half0=(0.1, np.nan, 0.1)),
               dict(half0=(0.1, 0.1)), dict(fs=0.0), dict(c=-1.0), dict(seeds=np.zeros((1, 9), dtype=_ffi.SRP_PEAK)), dict(mics=mics[:2]),
               dict(strips=st[:, :, :1])):
        a = dict(fs=Z.FS, c=S.C_SOUND, Z=2, levels=1, half0=(0.1, 0.1, 0.1), seeds=sd[:, :1], mics=mics, strips=st)
        a.update(kw)
        with pytest.raises(ValueError):
            engine.srp_zoom(a["strips"], a["mics"], a["fs"], a["c"], a["seeds"], a["half0"], a["Z"], a["levels"])
    # a refused call leaves the engine usable
    got = engine.srp_zoom(st, mics, Z.FS, S.C_SOUND, sd[:, :1], (0.1, 0.1, 0.1), 2, 1)
    assert got[0].tobytes() == srp.zoom(st[0], t, mics, Z.FS, S.C_SOUND, sd[0, :1], (0.1, 0.1, 0.1), 2, 1).tobytes()


@pytest.fixture(scope="module")
def scene_frames(engine):
    """frames[2][M][L]: the one-source and the two-source scene from engine.simulate_multipath."""
    one = []
    for which in range(2):
        delays, gains, total = S.scene_paths(S.SCENE_SOURCES[which])
        one.append(engine.simulate_multipath(S.scene_base(which)[None], S.SCENE_FS, total, delays[None], gains[None], S.SCENE_LEN)[0])
    return np.stack([one[0], one[0] + S.SCENE_GAIN2 * one[1]])


def test_chain(engine, scene_frames):
    mics = S.scene_mics()
    t = srp.half_width(mics, S.SCENE_FS, S.C_SOUND)
    args = (mics, S.SCENE_FS, S.C_SOUND, S.SCENE_LO, S.SCENE_HI, S.SCENE_COUNT)
    strips, _ = engine.gcc_phat_all_pairs_strips(scene_frames, S.SCENE_FS, t, Z.SCENE_W)
    peaks = engine.srp_map(strips, *args, K=2, R=3, outputs=("peaks",))[1]
    zoomed = engine.srp_zoom(strips, mics, S.SCENE_FS, S.C_SOUND, peaks, Z.scene_half0(), Z.SCENE_Z, Z.SCENE_LEVELS)
    first = engine.srp_zoom(strips, mics, S.SCENE_FS, S.C_SOUND, peaks, Z.scene_half0(), Z.SCENE_Z, 1)
    for f in range(2):
        want, trail = srp.zoom(strips[f], t, mics, S.SCENE_FS, S.C_SOUND, peaks[f], Z.scene_half0(), Z.SCENE_Z, Z.SCENE_LEVELS, return_levels=True)
        assert zoomed[f].tobytes() == want.tobytes()
        assert [tr[0][1] for tr in trail if tr] == first[f]["power"][first[f]["seed"] >= 0].tolist()
    d, = Z.scene_zoom_check(zoomed[0][:1], None, first[0]["power"][:1], False)
    d0, d1 = Z.scene_zoom_check(zoomed[1], None, first[1]["power"], True)
    print(f"[srp zoom] device chain: one source {d:.4f} m; two sources {d0:.4f} m and {d1:.4f} m")
    got = main.srp_positions_device(scene_frames, *args, W=Z.SCENE_W, K=2, R=3, engine=engine, zoom=(Z.SCENE_Z, Z.SCENE_LEVELS))
    assert isinstance(got, tuple) and len(got) == 2
    assert got[0].tobytes() == peaks.tobytes() and got[1].tobytes() == zoomed.tobytes()
    wide = main.srp_positions_device(scene_frames, *args, W=Z.SCENE_W, K=2, R=3, engine=engine, zoom=(Z.SCENE_Z, 1, 1.0))
    assert wide[1].tobytes() == first.tobytes()
    plain = main.srp_positions_device(scene_frames, *args, W=Z.SCENE_W, K=2, R=3, engine=engine, zoom=None)      # exactly what it returned before
    assert isinstance(plain, np.ndarray) and plain.dtype == _ffi.SRP_PEAK and plain.tobytes() == peaks.tobytes()
    assert main.srp_positions_device(scene_frames, *args, W=Z.SCENE_W, K=2, R=3, engine=engine).tobytes() == peaks.tobytes()
    one_peaks, one_zoomed, rec = main.srp_positions_device(scene_frames[0], *args, W=Z.SCENE_W, refine=True, engine=engine,
                                                           zoom=(Z.SCENE_Z, Z.SCENE_LEVELS))
    assert one_peaks.shape == (1,) and one_zoomed.shape == (1,) and one_zoomed[0].tobytes() == zoomed[0, 0].tobytes()
    print(f"[srp zoom] refined position of the one-source scene: {np.linalg.norm(rec['position'] - S.SCENE_SOURCES[0]):.4f} m from the source")
    assert np.all(np.isfinite(rec["position"]))
