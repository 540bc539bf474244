"""Engine.steer (csrc/beamform.hip) against its specification beamform.steer, at the shapes where the kernels change path.

Tolerance: tol[b][s] = 1e-11 * sum_m |w[b,s,m]| * max|frames[b,m]| - the bound the suite uses for multipath synthesis (the same
loader / inverse / storer chain, tests/test_gpu_second_path.py), scaled by the row's magnitude.  Every parity test prints the worst
error / tol it saw."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

from pyaudiolocalization_amd import Engine, _ffi, beamform
from pyaudiolocalization_amd._ffi import PalError
from pyaudiolocalization_amd.main import beamform_device, srp_positions_device

import beamform_cases as BC

pytestmark = pytest.mark.gpu


def _parity(engine, frames, delays, weights, want, tag, rel=1e-11):
    got = engine.steer(frames, BC.FS, delays, weights)
    assert got.shape == want.shape
    ratio = BC.worst_ratio(got, want, BC.tolerance(frames, weights, rel))
    print("steer %s: worst error / tol = %.3g" % (tag, ratio))
    assert ratio <= 1.0, (tag, ratio)
    return got


def _still_works(engine):
    """after a refusal the engine computes as before"""
    frames, delays, weights, want = BC.random_case(200, 2, 2, 1)
    got = engine.steer(frames, BC.FS, delays, weights)
    assert BC.worst_ratio(got, want, BC.tolerance(frames, weights, 1e-11)) <= 1.0


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


@pytest.mark.parametrize("length", BC.GPU_LENGTHS)
def test_fade_classes_and_bin_tile_borders(engine, length):
    """int(0.01 L) = 1, 2, >= 3 (SimStorer::fade) and H = L + 1 around the multiples of the 256-bin tile; 5 microphones, 3 beams,
    3 frames: 9 beam rows, the last transform holds one"""
    frames, delays, weights, want = BC.random_case(length, 5, 3, 3)
    got = _parity(engine, frames, delays, weights, want, "L=%d" % length)
    assert not got[:, :, 0].any()                                                # the fade window starts at 0
    if int(0.01 * length) >= 2:
        assert not got[:, :, length - 1].any()


@pytest.mark.parametrize("m,s,b", BC.GPU_SHAPES)
def test_microphone_and_beam_counts(engine, m, s, b):
    """every beam tile (1, 2, 4, 8 accumulators), the second pass at S = 9, one and two LDS tiles' worth of microphones, odd B S"""
    for length in (300, 1501):
        frames, delays, weights, want = BC.random_case(length, m, s, b)
        _parity(engine, frames, delays, weights, want, "M=%d S=%d B=%d L=%d" % (m, s, b, length))


def test_more_microphones_than_one_table_tile(engine):
    """70 microphones: the second LDS tile of delays and weights holds six"""
    frames, delays, weights, want = BC.random_case(300, 70, 3, 1)
    _parity(engine, frames, delays, weights, want, "M=70")


def test_negative_and_zero_delays_and_fractional_delay(engine):
    """M = 1, w = 1 is Engine.fractional_delay of the row (1e-12 of the scale, that call's own bound); delays of both signs"""
    length = 300
    rng = np.random.default_rng(23)
    rows = rng.standard_normal((4, 1, length))
    d = np.array([0.0, -0.0011, 0.00173, -3.0 / BC.FS]).reshape(4, 1, 1)
    w = np.ones((4, 1, 1))
    want = beamform.steer(rows, BC.FS, d, w)
    got = _parity(engine, rows, d, w, want, "signed delays", rel=1e-12)
    for q in range(4):
        alone = engine.fractional_delay(rows[q, 0], float(d[q, 0, 0]), BC.FS)
        assert float(np.max(np.abs(alone - got[q, 0]))) <= 1e-12 * float(np.max(np.abs(rows[q]))), q
    frames, delays, weights, _ = BC.random_case(length, 5, 3, 3)
    signed = delays - 0.002                                                      # U(-2 ms, 2 ms)
    _parity(engine, frames, signed, -weights, beamform.steer(frames, BC.FS, signed, -weights), "negative delays and weights")


@pytest.mark.parametrize("length", (100, 200, 300))
def test_whole_sample_delays_are_shifts(engine, length):
    """held to max(4 x the specification's own error against the exact shift, 1e-14 of the scale), the rule of
    test_fractional_delay_fade_lengths"""
    rng = np.random.default_rng([24, length])
    rows = rng.standard_normal((1, 1, length))
    shifts = np.array([0, 1, 7, -1, -5])
    d = (shifts / BC.FS).reshape(1, 5, 1)
    w = np.ones((1, 5, 1))
    got = engine.steer(rows, BC.FS, d, w)
    spec = beamform.steer(rows, BC.FS, d, w)
    for q, k in enumerate(shifts):
        exact = BC.exact_shift(rows[0, 0], int(k))
        own = float(np.max(np.abs(spec[0, q] - exact)))
        err = float(np.max(np.abs(got[0, q] - exact)))
        print("steer L=%d shift %d: engine - exact %.3g, specification - exact %.3g" % (length, k, err, own))
        assert err <= max(4 * own, 1e-14 * float(np.max(np.abs(rows)))), (length, k, err, own)


def test_zero_rows(engine):
    frames, delays, weights, _ = BC.random_case(300, 5, 2, 3)
    w = weights.copy()
    w[0, 1] = 0.0                                                                # packed with the live beam (0, 0)
    w[2, 0] = 0.0                                                                # packed with the live beam (1, 1)
    got = _parity(engine, frames, delays, w, beamform.steer(frames, BC.FS, delays, w), "zero weights")
    assert not got[0, 1].any() and not got[2, 0].any()
    assert got[0, 0].any() and got[1, 1].any()
    silent = frames.copy()
    silent[1] = 0.0                                                              # an all-zero frame: its beams share transforms with live ones
    got = _parity(engine, silent, delays, weights, beamform.steer(silent, BC.FS, delays, weights), "zero frame")
    assert not got[1].any() and got[0].any() and got[2].any()


def test_nan_point_through_beamform_device(engine):
    mics = np.random.default_rng(5).uniform(-0.5, 0.5, (5, 3))
    frames = BC.random_case(300, 5, 3, 3)[0]
    points = np.array([[1.0, 2.0, 0.5], [np.nan, 0.0, 0.0], [-2.0, 0.7, 1.0]])
    got = beamform_device(frames, mics, BC.FS, BC.C, points=points, engine=engine)
    d, valid = beamform.point_delays(np.broadcast_to(points, (3, 3, 3)), mics, BC.C)
    w = beamform.uniform_weights(valid, 5)
    want = beamform.steer(frames, BC.FS, d, w)
    ratio = BC.worst_ratio(got, want, BC.tolerance(frames, w, 1e-11))
    print("beamform_device with a NaN point: worst error / tol = %.3g" % ratio)
    assert ratio <= 1.0 and not got[:, 1].any() and got[:, 0].any() and got[:, 2].any()
    peaks = np.zeros((3, 2), dtype=_ffi.SRP_PEAK)                                # records as they come from the SRP calls
    peaks["x"], peaks["y"], peaks["z"] = 1.0, 2.0, 0.5
    peaks["index"] = [[4, -1], [4, -1], [4, 9]]
    rec = beamform_device(frames, mics, BC.FS, BC.C, points=peaks, engine=engine)
    assert not rec[0, 1].any() and not rec[1, 1].any() and rec[2, 1].any()
    assert BC.worst_ratio(rec[:, :1], want[:, :1], BC.tolerance(frames, w[:, :1], 1e-11)) <= 1.0
    one = beamform_device(frames[0], mics, BC.FS, BC.C, directions=np.array([[0.0, 0.0, 1.0]]), engine=engine)
    assert one.shape == (1, 300)
    with pytest.raises(ValueError):
        beamform_device(frames, mics, BC.FS, BC.C, engine=engine)
    with pytest.raises(ValueError):
        beamform_device(frames, mics, BC.FS, BC.C, points=points, directions=points, engine=engine)


def test_amplitude_independence(engine):
    """a beam never sees the amplitude of the beam it shares a transform with, nor does a quiet microphone with a large weight drown"""
    frames, delays, weights, _ = BC.random_case(300, 5, 1, 2)
    for scale in (2.0 ** 40, 2.0 ** -40):
        x = frames.copy()
        x[0] *= scale                                                            # S = 1: the beams of frames 0 and 1 share a transform
        _parity(engine, x, delays, weights, beamform.steer(x, BC.FS, delays, weights), "frame 0 x %.3g" % scale)
    x, w = frames.copy(), weights.copy()
    x[:, 2] *= 2.0 ** -30
    w[:, :, 2] *= 2.0 ** 30
    _parity(engine, x, delays, w, beamform.steer(x, BC.FS, delays, w), "microphone 2 x 2^-30, weight x 2^30")


def test_grouping_slices_and_determinism(engine):
    frames, delays, weights, want = BC.random_case(300, 5, 2, 3)
    got = _parity(engine, frames, delays, weights, want, "default grouping")
    assert engine.steer(frames, BC.FS, delays, weights).tobytes() == got.tobytes()   # the same call twice
    try:
        engine.set_chunk(2)                                                      # 6 rows = 3 packed transforms: two launch groups
        again = engine.steer(frames, BC.FS, delays, weights)
    finally:
        engine.set_chunk(0)
    assert again.tobytes() == got.tobytes()
    odd = BC.random_case(300, 5, 3, 3)
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
        assert sliced.steer(frames, BC.FS, delays, weights).tobytes() == got.tobytes()   # S even: no beam changes partner
        _parity(sliced, odd[0], odd[1], odd[2], odd[3], "slices of one frame, S odd")
    finally:
        sliced.close()


def test_dev_form_writes_its_rows_only(engine):
    frames, delays, weights, want = BC.random_case(299, 5, 3, 3)
    b, m, length = frames.shape
    s = delays.shape[1]
    got = engine.steer(frames, BC.FS, delays, weights)
    with _device(engine, frames, delays, weights, got.size + 64) as (d_x, d_d, d_w, d_out):
        engine.steer_dev(d_x, b, m, length, BC.FS, d_d, d_w, s, d_out)
        engine.synchronize()
        back = engine.download(np.empty(got.size + 64), d_out)
        kept = [engine.download(np.empty(a.size), p) for a, p in ((frames, d_x), (delays, d_d), (weights, d_w))]
    assert back[: got.size].tobytes() == got.tobytes()
    assert np.all(back[got.size:].view(np.uint64) == np.float64(BC.SENTINEL).view(np.uint64))
    for a, k in zip((frames, delays, weights), kept):
        assert k.tobytes() == np.ascontiguousarray(a).tobytes()                  # the caller's arrays are not touched


def test_refusals(engine):
    frames, delays, weights, _ = BC.random_case(200, 2, 2, 1)
    with pytest.raises(ValueError):
        engine.steer(np.ones((1, 2, 99)), BC.FS, delays, weights)
    _still_works(engine)
    with pytest.raises(PalError):
        engine.steer(np.ones((1, 1, 2 ** 19 + 1)), BC.FS, np.zeros((1, 1, 1)), np.ones((1, 1, 1)))
    _still_works(engine)
    with pytest.raises(ValueError):
        engine.steer(np.ones((1, 0, 200)), BC.FS, np.zeros((1, 2, 0)))           # M = 0
    with pytest.raises(ValueError):
        engine.steer(frames, BC.FS, np.zeros((1, 0, 2)))                         # S = 0
    with pytest.raises(ValueError):
        engine.steer(frames, 0.0, delays, weights)
    with pytest.raises(ValueError):
        engine.steer(frames, np.inf, delays, weights)
    _still_works(engine)
    b, m, length = frames.shape
    for which, value in ((0, np.nan), (0, np.inf), (1, np.nan), (1, -np.inf), (0, (length + 1) / BC.FS), (0, -(length + 1) / BC.FS)):
        tabs = [delays.copy(), weights.copy()]
        tabs[which][0, 1, 1] = value
        with pytest.raises(ValueError):
            engine.steer(frames, BC.FS, tabs[0], tabs[1])
        _still_works(engine)
        with _device(engine, frames, tabs[0], tabs[1], b * 2 * length) as (d_x, d_d, d_w, d_out):
            engine.steer_dev(d_x, b, m, length, BC.FS, d_d, d_w, 2, d_out)
            with pytest.raises(ValueError):
                engine.synchronize()
        _still_works(engine)
    edge = delays.copy()
    edge[0, 0, 0] = length / BC.FS                                               # |d| fs = L exactly is still allowed
    engine.steer(frames, BC.FS, edge, weights)
    bad = frames.copy()
    bad[0, 1, 17] = np.nan
    with pytest.raises(ValueError):
        engine.steer(bad, BC.FS, delays, weights)
    _still_works(engine)
    with _device(engine, bad, delays, weights, b * 2 * length) as (d_x, d_d, d_w, d_out):
        engine.steer_dev(d_x, b, m, length, BC.FS, d_d, d_w, 2, d_out)
        with pytest.raises(ValueError):
            engine.synchronize()
    _still_works(engine)
    # NULL pointers and bad counts through the raw ABI
    lib, h = engine._lib, engine._h
    x, d, w, out = frames.copy(), delays.copy(), weights.copy(), np.empty((1, 2, length))
    ptrs = [x.ctypes.data, d.ctypes.data, w.ctypes.data, out.ctypes.data]
    for hole in range(4):
        p = [None if q == hole else v for q, v in enumerate(ptrs)]
        assert lib.pal_steer_sum(h, p[0], b, m, length, BC.FS, p[1], p[2], 2, p[3]) == _ffi.ERR_INVALID
        assert lib.pal_steer_sum_dev(h, ctypes.c_void_p(p[0]), b, m, length, BC.FS, ctypes.c_void_p(p[1]), ctypes.c_void_p(p[2]), 2,
                                     ctypes.c_void_p(p[3])) == _ffi.ERR_INVALID
    for bb, mm, ss in ((0, m, 2), (b, 0, 2), (b, m, 0)):
        assert lib.pal_steer_sum(h, ptrs[0], bb, mm, length, BC.FS, ptrs[1], ptrs[2], ss, ptrs[3]) == _ffi.ERR_INVALID
    _still_works(engine)


def _engine_rows(engine):
    return lambda rows, delays: engine.fractional_delay(rows, delays, BC.FS)


def test_array_gain_on_the_device(engine):
    """the scene of tests/test_host_beamform.py with rows from Engine.fractional_delay, steered on the device: the same two assertions"""
    mics, frames, ref = BC.gain_scene(_engine_rows(engine))
    single, at_source, elsewhere = BC.gain_figures(lambda x, d, w: engine.steer(x, BC.FS, d, w), mics, frames, ref)
    print("array gain (device): one microphone %.2f dB, beam at the source %.2f dB, beam elsewhere %.2f dB" % (single, at_source, elsewhere))
    assert at_source - single >= 10.0 * np.log10(BC.GAIN_M) - 1.0
    assert elsewhere < single


def test_two_sources_found_and_separated(engine):
    """srp_positions_device(K=2, zoom) on the two-source scene, then beamform_device at the zoomed records as they come: the two
    conditions of beamform_cases.two_source_check (tests/test_host_beamform.py holds the specifications to the same on the CPU).
    Steering at a found position loses gain at high frequencies with every centimetre of error: no 10 log10 M here."""
    mics, frames, bases = BC.two_source_scene(_engine_rows(engine))
    peaks, zoomed = srp_positions_device(frames, mics, BC.FS, BC.C, BC.TWO_LO, BC.TWO_HI, BC.TWO_COUNT, W=BC.TWO_W, K=2, R=BC.TWO_R,
                                         zoom=BC.TWO_ZOOM, engine=engine)
    assert np.all(peaks["index"] >= 0) and np.all(zoomed["seed"] >= 0) and np.all(zoomed["levels"] > 0)
    beams = beamform_device(frames, mics, BC.FS, BC.C, points=zoomed, engine=engine)
    assert beams.shape == (2, BC.TWO_L)
    found = beamform.records_to_points(zoomed)
    d, valid = beamform.point_delays(found, mics, BC.C)
    w = beamform.uniform_weights(valid, BC.TWO_M)
    spec = beamform.steer(frames[None], BC.FS, d[None], w[None])
    ratio = BC.worst_ratio(beams[None], spec, BC.tolerance(frames[None], w[None], 1e-11))
    print("beams at the found positions against the specification: worst error / tol = %.3g" % ratio)
    assert ratio <= 1.0
    BC.two_source_check(mics, frames, bases, found, beams, "device")


