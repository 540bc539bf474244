"""Engine.separate (k_separate in csrc/beamform.hip, csrc/separate_math.h) against its specification beamform.separate, at the shapes
where the kernels change path.

Tolerance: tol[b][s] = 1e-11 * |T[b]|_2 / delta[b], T[b,t] = sum_m |g[b,t,m]| max|frames[b,m]|, delta[b] = loading max_s sum_m g^2 -
steer's device bound 1e-11 sum_m |w| max|x| on the delay-and-sum spectra, which the solve amplifies by at most 1 / delta.  The bound
is loose (it holds in the 2-norm by Parseval; a sample's error lies orders of magnitude below it).  Every parity test prints the
worst error / tol it saw; a ratio above 1 is a finding about the kernel."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

from pyaudiolocalization_amd import Engine, _ffi, beamform
from pyaudiolocalization_amd._ffi import PalError
from pyaudiolocalization_amd.main import beamform_device, separate_device, srp_positions_device

import beamform_cases as BC
import separate_cases as SC

pytestmark = pytest.mark.gpu


def _parity(engine, frames, delays, gains, loading, want, tag, rel=1e-11):
    got = engine.separate(frames, SC.FS, delays, gains, loading)
    assert got.shape == want.shape
    ratio = BC.worst_ratio(got, want, SC.tolerance(frames, gains, loading, rel))
    print("separate %s loading=%g: worst error / tol = %.3g" % (tag, loading, ratio))
    assert ratio <= 1.0, (tag, loading, ratio)
    return got


def _still_works(engine):
    """after a refusal the engine computes as before"""
    frames, delays, gains, want = SC.random_case(200, 2, 2, 1, 0.01)
    got = engine.separate(frames, SC.FS, delays, gains, 0.01)
    assert BC.worst_ratio(got, want, SC.tolerance(frames, gains, 0.01, 1e-11)) <= 1.0


@contextlib.contextmanager
def _device(engine, *hosts):
    """device copies of the host arrays (an int: that many doubles of sentinel); freed on the way out"""
    ptrs = []
    try:
        for h in hosts:
            arr = np.full(h, BC.SENTINEL) if isinstance(h, int) else np.ascontiguousarray(h, dtype=np.float64)
            ptrs.append(engine.alloc(max(8, arr.nbytes)))
            engine.upload(ptrs[-1], arr)
        yield ptrs
    finally:
        for p in ptrs:
            engine.free(p)


@pytest.mark.parametrize("length", SC.GPU_LENGTHS)
def test_fade_classes_and_bin_tile_borders(engine, length):
    """int(0.01 L) = 1, 2, >= 3 and H = L + 1 around the multiples of the 256-bin tile; 5 microphones, 3 sources (the tile of 4 with
    three live), 3 frames: 9 beam rows, the last transform holds one.  Signed delays and gains, every loading."""
    for loading in SC.LOADINGS:
        frames, delays, gains, want = SC.signed_case(length, 5, 3, 3, loading)
        got = _parity(engine, frames, delays, gains, loading, want, "L=%d" % length)
        assert not got[:, :, 0].any()                                            # the fade window starts at 0


@pytest.mark.parametrize("m,s,b", SC.GPU_SHAPES)
def test_microphone_and_source_counts(engine, m, s, b):
    """every tile (1, 2, 4, 8 unknowns) full and partial, more sources than microphones, one and two LDS tiles' worth of microphones,
    odd B S; signed delays and gains, every loading"""
    for loading in SC.LOADINGS:
        frames, delays, gains, want = SC.signed_case(300, m, s, b, loading)
        _parity(engine, frames, delays, gains, loading, want, "M=%d S=%d B=%d" % (m, s, b))


def test_one_source_without_loading_is_steer(engine):
    """S = 1, loading 0: Engine.steer at weights gains / q, within steer's own tolerance"""
    frames, delays, gains, _ = SC.signed_case(300, 5, 1, 3, 0.01)
    w = gains / np.sum(gains * gains, axis=2, keepdims=True)
    got = engine.separate(frames, SC.FS, delays, gains, 0.0)
    want = engine.steer(frames, SC.FS, delays, w)
    ratio = BC.worst_ratio(got, want, BC.tolerance(frames, w, 1e-11))
    print("separate S=1 loading 0 vs Engine.steer: worst error / tol = %.3g" % ratio)
    assert ratio <= 1.0
    assert BC.worst_ratio(got, beamform.separate(frames, SC.FS, delays, gains, 0.0), BC.tolerance(frames, w, 1e-11)) <= 1.0
    ones = engine.separate(frames, SC.FS, delays)                                # gains None: every gain 1
    assert BC.worst_ratio(ones, beamform.separate(frames, SC.FS, delays, np.ones_like(delays), 0.01),
                          SC.tolerance(frames, np.ones_like(delays), 0.01, 1e-11)) <= 1.0


def test_exact_zero_cases(engine):
    frames, delays, gains, want = SC.signed_case(300, 5, 3, 3, 0.01)
    g = gains.copy()
    g[0, 1] = 0.0                                                                # a zero-gain source beside live ones
    g[2, 0] = 0.0
    got = _parity(engine, frames, delays, g, 0.01, beamform.separate(frames, SC.FS, delays, g, 0.01), "zero-gain sources")
    assert not got[0, 1].any() and not got[2, 0].any()
    assert got[0, 0].any() and got[0, 2].any() and got[1].any() and got[2, 1].any()
    silent = frames.copy()
    silent[1] = 0.0                                                              # a frame of zeros next to live ones
    got = _parity(engine, silent, delays, gains, 0.01, beamform.separate(silent, SC.FS, delays, gains, 0.01), "zero frame")
    assert not got[1].any() and got[0].any() and got[2].any()
    assert not engine.separate(frames, SC.FS, delays, np.zeros_like(gains), 0.01).any()   # no gains at all
    # NaN points and absent records through separate_device: gains of 0 there, the live rows as the specification has them
    mics = np.random.default_rng(5).uniform(-0.5, 0.5, (5, 3))
    points = np.array([[1.0, 2.0, 0.5], [np.nan, 0.0, 0.0], [-2.0, 0.7, 1.0]])
    got = separate_device(frames, mics, SC.FS, SC.C, points=points, engine=engine)
    d, valid = beamform.point_delays(np.broadcast_to(points, (3, 3, 3)), mics, SC.C)
    gn = np.where(valid[..., None], 1.0, 0.0) * np.ones(5)
    spec = beamform.separate(frames, SC.FS, d, gn, 0.01)
    ratio = BC.worst_ratio(got, spec, SC.tolerance(frames, gn, 0.01, 1e-11))
    print("separate_device with a NaN point: worst error / tol = %.3g" % ratio)
    assert ratio <= 1.0 and not got[:, 1].any() and got[:, 0].any() and got[:, 2].any()
    peaks = np.zeros((3, 2), dtype=_ffi.SRP_PEAK)
    peaks["x"], peaks["y"], peaks["z"] = [1.0, -2.0], [2.0, 0.7], [0.5, 1.0]
    peaks["index"] = [[4, -1], [4, -1], [4, 9]]
    rec = separate_device(frames, mics, SC.FS, SC.C, points=peaks, loading=0.1, engine=engine)
    assert not rec[0, 1].any() and not rec[1, 1].any() and rec[2, 1].any() and rec[:, 0].any()
    one = separate_device(frames[0], mics, SC.FS, SC.C, directions=np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0]]), engine=engine)
    assert one.shape == (2, 300) and np.all(np.isfinite(one)) and one.any()
    with pytest.raises(ValueError):
        separate_device(frames, mics, SC.FS, SC.C, engine=engine)
    with pytest.raises(ValueError):
        separate_device(frames, mics, SC.FS, SC.C, points=points, directions=points, engine=engine)


def test_identical_sources_and_extreme_amplitudes(engine):
    frames, delays, gains, _ = SC.signed_case(300, 5, 3, 2, 0.01)
    for loading in SC.LOADINGS:
        d, g = delays.copy(), gains.copy()
        d[:, 2], g[:, 2] = d[:, 0], g[:, 0]
        got = _parity(engine, frames, d, g, loading, beamform.separate(frames, SC.FS, d, g, loading), "sources 0 and 2 in one place")
        tol = SC.tolerance(frames, g, loading, 1e-11)
        assert np.all(np.max(np.abs(got[:, 0] - got[:, 2]), axis=1) <= tol[:, 0]) and got[:, 0].any()
    # S = 1: the beams of frames 0 and 1 share a transform; S = 3: frame 0's third beam shares one with frame 1's first
    for s in (1, 3):
        x, d, g, _ = SC.signed_case(300, 5, s, 2, 0.01)
        for scale in (2.0 ** 40, 2.0 ** -40):
            y = x.copy()
            y[0] *= scale
            _parity(engine, y, d, g, 0.01, beamform.separate(y, SC.FS, d, g, 0.01), "S=%d, frame 0 x %.3g" % (s, scale))


def test_grouping_slices_and_determinism(engine):
    frames, delays, gains, want = SC.signed_case(300, 5, 2, 3, 0.01)
    got = _parity(engine, frames, delays, gains, 0.01, want, "default grouping")
    assert engine.separate(frames, SC.FS, delays, gains, 0.01).tobytes() == got.tobytes()   # the same call twice
    try:
        engine.set_chunk(2)                                                      # 6 rows = 3 packed transforms: two launch groups
        again = engine.separate(frames, SC.FS, delays, gains, 0.01)
    finally:
        engine.set_chunk(0)
    assert again.tobytes() == got.tobytes()
    odd = SC.signed_case(300, 5, 3, 3, 0.01)
    before = os.environ.get("PAL_BEAM_SLICE")
    os.environ["PAL_BEAM_SLICE"] = "1"
    try:
        sliced = Engine(engine.device)                                           # the variable is read when the engine is made
    finally:
        if before is None:
            del os.environ["PAL_BEAM_SLICE"]
        else:
            os.environ["PAL_BEAM_SLICE"] = before
    try:
        assert sliced.separate(frames, SC.FS, delays, gains, 0.01).tobytes() == got.tobytes()   # S even: no beam changes partner
        _parity(sliced, odd[0], odd[1], odd[2], 0.01, odd[3], "slices of one frame, S odd")
    finally:
        sliced.close()


def test_dev_form_writes_its_rows_only(engine):
    frames, delays, gains, _ = SC.signed_case(255, 5, 3, 3, 0.01)
    b, m, length = frames.shape
    s = delays.shape[1]
    got = engine.separate(frames, SC.FS, delays, gains, 0.01)
    with _device(engine, frames, delays, gains, got.size + 64) as (d_x, d_d, d_g, d_out):
        engine.separate_dev(d_x, b, m, length, SC.FS, d_d, d_g, s, 0.01, d_out)
        engine.synchronize()
        back = engine.download(np.empty(got.size + 64), d_out)
        kept = [engine.download(np.empty(a.size), p) for a, p in ((frames, d_x), (delays, d_d), (gains, d_g))]
    assert back[: got.size].tobytes() == got.tobytes()
    assert np.all(back[got.size:].view(np.uint64) == np.float64(BC.SENTINEL).view(np.uint64))
    for a, k in zip((frames, delays, gains), kept):
        assert k.tobytes() == np.ascontiguousarray(a).tobytes()                  # the caller's arrays are not touched


def test_steer_is_unchanged_by_a_separate_call(engine):
    """the two share the scratch slot of the spectra, exponents and live marks"""
    frames, delays, weights, want = BC.random_case(300, 5, 3, 3)
    before = engine.steer(frames, BC.FS, delays, weights)
    x, d, g, _ = SC.signed_case(300, 64, 8, 3, 0.01)
    engine.separate(x, SC.FS, d, g, 0.01)
    after = engine.steer(frames, BC.FS, delays, weights)
    assert after.tobytes() == before.tobytes()
    assert BC.worst_ratio(after, want, BC.tolerance(frames, weights, 1e-11)) <= 1.0


def test_refusals(engine):
    frames, delays, gains, _ = SC.random_case(200, 2, 2, 1, 0.01)
    b, m, length = frames.shape
    with pytest.raises(ValueError):
        engine.separate(np.ones((1, 2, 99)), SC.FS, delays, gains)
    _still_works(engine)
    with pytest.raises(PalError):
        engine.separate(np.ones((1, 1, 2 ** 19 + 1)), SC.FS, np.zeros((1, 1, 1)), np.ones((1, 1, 1)))
    _still_works(engine)
    with pytest.raises(ValueError):
        engine.separate(np.ones((1, 0, 200)), SC.FS, np.zeros((1, 2, 0)))        # M = 0
    with pytest.raises(ValueError):
        engine.separate(frames, SC.FS, np.zeros((1, 0, 2)))                      # S = 0
    with pytest.raises(ValueError):
        engine.separate(frames, SC.FS, delays, gains[:, :1])
    with pytest.raises(ValueError):
        engine.separate(frames, 0.0, delays, gains)
    with pytest.raises(ValueError):
        engine.separate(frames, np.inf, delays, gains)
    _still_works(engine)
    # the three new refusals, in both forms
    nine_d, nine_g = np.zeros((1, 9, 2)), np.ones((1, 9, 2))
    with _device(engine, frames, nine_d, nine_g, b * 9 * length) as (d_x, d_d, d_g, d_out):
        for bad in (-0.01, np.nan, np.inf, -np.inf, 0.0):                        # 0 with S = 2: bin 0 of G is singular
            with pytest.raises(ValueError):
                engine.separate(frames, SC.FS, delays, gains, bad)
            with pytest.raises(ValueError):
                engine.separate_dev(d_x, b, m, length, SC.FS, d_d, d_g, 2, bad, d_out)
        with pytest.raises(PalError) as unsupported:
            engine.separate(frames, SC.FS, nine_d, nine_g, 0.01)                 # S = 9: one solve cannot be split
        assert not isinstance(unsupported.value, ValueError)
        with pytest.raises(PalError):
            engine.separate_dev(d_x, b, m, length, SC.FS, d_d, d_g, 9, 0.01, d_out)
        engine.separate_dev(d_x, b, m, length, SC.FS, d_d, d_g, 1, 0.0, d_out)   # loading 0 with one source is allowed
        engine.synchronize()
        engine.separate_dev(d_x, b, m, length, SC.FS, d_d, d_g, 8, 0.01, d_out)  # S = 8 is the most
        engine.synchronize()
    _still_works(engine)
    for which, value in ((0, np.nan), (0, np.inf), (1, np.nan), (1, -np.inf), (0, (length + 1) / SC.FS), (0, -(length + 1) / SC.FS)):
        tabs = [delays.copy(), gains.copy()]
        tabs[which][0, 1, 1] = value
        with pytest.raises(ValueError):
            engine.separate(frames, SC.FS, tabs[0], tabs[1])
        _still_works(engine)
        with _device(engine, frames, tabs[0], tabs[1], b * 2 * length) as (d_x, d_d, d_g, d_out):
            engine.separate_dev(d_x, b, m, length, SC.FS, d_d, d_g, 2, 0.01, d_out)
            with pytest.raises(ValueError):
                engine.synchronize()
        _still_works(engine)
    edge = delays.copy()
    edge[0, 0, 0] = length / SC.FS                                               # |d| fs = L exactly is still allowed
    engine.separate(frames, SC.FS, edge, gains)
    bad = frames.copy()
    bad[0, 1, 17] = np.nan
    with pytest.raises(ValueError):
        engine.separate(bad, SC.FS, delays, gains)
    _still_works(engine)
    with _device(engine, bad, delays, gains, b * 2 * length) as (d_x, d_d, d_g, d_out):
        engine.separate_dev(d_x, b, m, length, SC.FS, d_d, d_g, 2, 0.01, d_out)
        with pytest.raises(ValueError):
            engine.synchronize()
    _still_works(engine)
    # NULL pointers and bad counts through the raw ABI
    lib, h = engine._lib, engine._h
    x, d, g, out = frames.copy(), delays.copy(), gains.copy(), np.empty((1, 2, length))
    ptrs = [x.ctypes.data, d.ctypes.data, g.ctypes.data, out.ctypes.data]
    for hole in range(4):
        p = [None if q == hole else v for q, v in enumerate(ptrs)]
        assert lib.pal_separate(h, p[0], b, m, length, SC.FS, p[1], p[2], 2, 0.01, p[3]) == _ffi.ERR_INVALID
        assert lib.pal_separate_dev(h, ctypes.c_void_p(p[0]), b, m, length, SC.FS, ctypes.c_void_p(p[1]), ctypes.c_void_p(p[2]), 2, 0.01,
                                    ctypes.c_void_p(p[3])) == _ffi.ERR_INVALID
    for bb, mm, ss in ((0, m, 2), (b, 0, 2), (b, m, 0)):
        assert lib.pal_separate(h, ptrs[0], bb, mm, length, SC.FS, ptrs[1], ptrs[2], ss, 0.01, ptrs[3]) == _ffi.ERR_INVALID
    assert lib.pal_separate(h, ptrs[0], b, m, length, SC.FS, ptrs[1], ptrs[2], 9, 0.01, ptrs[3]) == _ffi.ERR_UNSUPPORTED
    _still_works(engine)


def _engine_rows(engine):
    return lambda rows, delays: engine.fractional_delay(rows, delays, SC.FS)


@pytest.mark.parametrize("name", ("apart", "close"))
def test_null_steering_gains_3_db_at_the_true_positions(engine, name):
    """the scenes of tests/test_host_separate.py with rows from Engine.fractional_delay, both beamformers on the device"""
    sources = SC.SOURCES_APART if name == "apart" else SC.SOURCES_CLOSE
    mics, frames, bases = SC.scene(sources, _engine_rows(engine))
    das = beamform_device(frames, mics, SC.FS, SC.C, points=sources, engine=engine)
    nul = separate_device(frames, mics, SC.FS, SC.C, points=sources, loading=SC.SCENE_LOADING, engine=engine)
    fd = SC.scene_figures(mics, bases, sources, sources, das, "%s, delay-and-sum (device)" % name)
    fn = SC.scene_figures(mics, bases, sources, sources, nul, "%s, null steering (device)" % name)
    for q in range(2):
        assert fd[q][0] == q and fn[q][0] == q
        print("%s (device): beam %d gains %.2f dB" % (name, q, fn[q][3] - fd[q][3]))
        assert fn[q][3] - fd[q][3] >= 3.0
        if name == "close":
            assert fn[q][2] < fd[q][2] / 3.0


def test_two_sources_found_and_separated(engine):
    """srp_positions_device(K=2, zoom) on the 1.5 m scene, then separate_device at the zoomed records as they come: the conditions of
    beamform_cases.two_source_check, parity with the specification at the found points, and each beam's SNR at least 3 dB above
    beamform_device's at the same points"""
    mics, frames, bases = BC.two_source_scene(_engine_rows(engine))
    peaks, zoomed = srp_positions_device(frames, mics, BC.FS, BC.C, BC.TWO_LO, BC.TWO_HI, BC.TWO_COUNT, W=BC.TWO_W, K=2, R=BC.TWO_R,
                                         zoom=BC.TWO_ZOOM, engine=engine)
    assert np.all(peaks["index"] >= 0) and np.all(zoomed["seed"] >= 0) and np.all(zoomed["levels"] > 0)
    beams = separate_device(frames, mics, BC.FS, BC.C, points=zoomed, loading=SC.SCENE_LOADING, engine=engine)
    das = beamform_device(frames, mics, BC.FS, BC.C, points=zoomed, engine=engine)
    assert beams.shape == (2, BC.TWO_L)
    found = beamform.records_to_points(zoomed)
    d, valid = beamform.point_delays(found, mics, BC.C)
    ones = np.ones((1, 2, BC.TWO_M))
    spec = beamform.separate(frames[None], BC.FS, d[None], ones, SC.SCENE_LOADING)
    ratio = BC.worst_ratio(beams[None], spec, SC.tolerance(frames[None], ones, SC.SCENE_LOADING, 1e-11))
    print("null-steering beams at the found positions against the specification: worst error / tol = %.3g" % ratio)
    assert ratio <= 1.0
    BC.two_source_check(mics, frames, bases, found, beams, "device, null steering")
    fd = SC.scene_figures(mics, bases, BC.TWO_SOURCES, found, das, "found positions, delay-and-sum")
    fn = SC.scene_figures(mics, bases, BC.TWO_SOURCES, found, beams, "found positions, null steering")
    for q in range(2):
        assert fd[q][0] == fn[q][0]
        print("found positions: beam %d gains %.2f dB" % (q, fn[q][3] - fd[q][3]))
        assert fn[q][3] - fd[q][3] >= 3.0
