"""Engine.mvdr (k_mvdr_cov, k_mvdr_weights, k_mvdr_apply in csrc/mvdr_kernels.h, Engine::mvdr_dev in csrc/beamform.hip) against its
specification beamform.mvdr, at the shapes where the kernels change path.

Tolerances (tests/mvdr_cases.py): the beams within 1e-13 (100 + kappa) sum_m wmax[m] max|frames[b,m]|, the weights in their own scale
within 1e-13 (100 + kappa) wmax, kappa = M / loading + 1.  Every parity test prints the worst error / tol it saw; a ratio above 1 is
a finding about the kernels, one above 0.1 about the tolerance."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

from pyaudiolocalization_amd import Engine, _ffi, beamform
from pyaudiolocalization_amd._ffi import PalError
from pyaudiolocalization_amd.main import beamform_device, mvdr_device

import beamform_cases as BC
import mvdr_cases as MC
import separate_cases as SC

pytestmark = pytest.mark.gpu

REL = 1e-13


def _parity(engine, case, loading, groups, tag):
    frames, delays, gains, w, want = case
    length = frames.shape[2]
    got, gw = engine.mvdr(frames, MC.FS, delays, gains, loading, groups, return_weights=True)
    assert got.shape == want.shape and gw.shape == w[..., :length + 1].shape
    ratio = BC.worst_ratio(got, want, MC.tolerance(frames, w, loading, REL))
    wratio = MC.weight_ratio(gw, w[..., :length + 1], frames.shape[1], loading, REL)
    print("mvdr %s loading=%g: worst error / tol = %.3g (beams), %.3g (weights)" % (tag, loading, ratio, wratio))
    assert ratio <= 1.0 and wratio <= 1.0, (tag, loading, ratio, wratio)
    return got


def _still_works(engine):
    """after a refusal the engine computes as before"""
    case = MC.random_case(200, 2, 2, 1, 2, 0.1)
    got = engine.mvdr(case[0], MC.FS, case[1], case[2], 0.1, 1)
    assert BC.worst_ratio(got, case[4], MC.tolerance(case[0], case[3], 0.1, REL)) <= 1.0


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


@contextlib.contextmanager
def _sliced_engine(engine, frames_per_slice):
    before = os.environ.get("PAL_BEAM_SLICE")
    os.environ["PAL_BEAM_SLICE"] = str(frames_per_slice)
    try:
        sliced = Engine(engine.device)                                           # the variable is read when the engine is made
    finally:
        if before is None:
            del os.environ["PAL_BEAM_SLICE"]
        else:
            os.environ["PAL_BEAM_SLICE"] = before
    try:
        yield sliced
    finally:
        sliced.close()


@pytest.mark.parametrize("length", MC.GPU_LENGTHS)
def test_fade_classes_and_bin_tile_borders(engine, length):
    """int(0.01 L) = 1, 2, >= 3 and H = L + 1 under, on and over the 256-bin tile; 5 microphones, 3 sources, 3 groups of 3 frames (9
    rows per group: the last transform of a slice holds one).  Signed delays and gains, every loading."""
    for loading in MC.GPU_LOADINGS:
        got = _parity(engine, MC.signed_case(length, 5, 3, 3, 3, loading), loading, 3, "L=%d" % length)
        assert not got[:, :, 0].any()                                            # the fade window starts at 0


@pytest.mark.parametrize("m,s,g,q", MC.GPU_SHAPES)
def test_microphone_source_group_and_snapshot_counts(engine, m, s, g, q):
    for loading in MC.GPU_LOADINGS:
        _parity(engine, MC.signed_case(100 if m * q > 2000 else 300, m, s, g, q, loading), loading, g, "M=%d S=%d G=%d Q=%d" % (m, s, g, q))


def test_slices_grouping_and_determinism(engine):
    case = MC.signed_case(300, 5, 2, 1, 3, 0.1)
    frames, delays, gains = case[:3]
    got = _parity(engine, case, 0.1, 1, "default grouping")
    out, w = engine.mvdr(frames, MC.FS, delays, gains, 0.1, 1, return_weights=True)
    assert out.tobytes() == got.tobytes()                                        # the same call twice; the weights output changes nothing
    try:
        engine.set_chunk(2)                                                      # 6 rows = 3 packed transforms: two launch groups
        again = engine.mvdr(frames, MC.FS, delays, gains, 0.1, 1)
    finally:
        engine.set_chunk(0)
    assert again.tobytes() == got.tobytes()
    two = MC.signed_case(300, 5, 2, 2, 3, 0.1)                                   # slices end at the group border
    plain = engine.mvdr(two[0], MC.FS, two[1], two[2], 0.1, 2, return_weights=True)
    odd = MC.signed_case(300, 5, 3, 2, 3, 0.1)
    for per in (1, 2):
        with _sliced_engine(engine, per) as sliced:
            so, sw = sliced.mvdr(frames, MC.FS, delays, gains, 0.1, 1, return_weights=True)
            assert so.tobytes() == got.tobytes() and sw.tobytes() == w.tobytes()   # S even: no row changes its transform partner
            so, sw = sliced.mvdr(two[0], MC.FS, two[1], two[2], 0.1, 2, return_weights=True)
            assert so.tobytes() == plain[0].tobytes() and sw.tobytes() == plain[1].tobytes()
            _parity(sliced, odd, 0.1, 2, "slices of %d, S odd" % per)


def test_covariance_tile_shapes_give_the_same_bytes(engine):
    """PAL_MVDR_TILE=44: 4 x 4 microphone pairs per workgroup of k_mvdr_cov instead of 8 x 4 - every pair keeps its owner's sum"""
    before = os.environ.get("PAL_MVDR_TILE")
    os.environ["PAL_MVDR_TILE"] = "44"
    try:
        small = Engine(engine.device)                                            # the variable is read when the engine is made
    finally:
        if before is None:
            del os.environ["PAL_MVDR_TILE"]
        else:
            os.environ["PAL_MVDR_TILE"] = before
    try:
        for m, s, g, q in ((5, 2, 1, 3), (9, 8, 1, 2), (33, 2, 1, 3), (64, 8, 1, 4)):
            frames, delays, gains, _, _ = MC.signed_case(300, m, s, g, q, 0.1)
            a = engine.mvdr(frames, MC.FS, delays, gains, 0.1, g, return_weights=True)
            b = small.mvdr(frames, MC.FS, delays, gains, 0.1, g, return_weights=True)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), (m, s, g, q)
    finally:
        small.close()


def test_dev_form_writes_its_rows_only(engine):
    frames, delays, gains, _, _ = MC.signed_case(255, 5, 3, 2, 3, 0.1)
    b, m, length = frames.shape
    g, s = delays.shape[:2]
    got, w = engine.mvdr(frames, MC.FS, delays, gains, 0.1, g, return_weights=True)
    nw = 2 * w.size
    sentinel = np.float64(BC.SENTINEL).view(np.uint64)
    with _device(engine, frames, delays, gains, got.size + 64, nw + 64) as (d_x, d_d, d_g, d_out, d_w):
        engine.mvdr_dev(d_x, b, m, length, MC.FS, d_d, d_g, g, s, 0.1, d_out, d_w)
        engine.synchronize()
        back = engine.download(np.empty(got.size + 64), d_out)
        wback = engine.download(np.empty(nw + 64), d_w)
        kept = [engine.download(np.empty(a.size), p) for a, p in ((frames, d_x), (delays, d_d), (gains, d_g))]
        assert back[: got.size].tobytes() == got.tobytes() and wback[:nw].tobytes() == w.tobytes()
        assert np.all(back[got.size:].view(np.uint64) == sentinel) and np.all(wback[nw:].view(np.uint64) == sentinel)
        for a, k in zip((frames, delays, gains), kept):
            assert k.tobytes() == np.ascontiguousarray(a).tobytes()              # the caller's arrays are not touched
        engine.upload(d_out, np.full(got.size + 64, BC.SENTINEL))
        engine.mvdr_dev(d_x, b, m, length, MC.FS, d_d, d_g, g, s, 0.1, d_out)    # no weights asked for: the same rows
        engine.synchronize()
        back = engine.download(np.empty(got.size + 64), d_out)
    assert back[: got.size].tobytes() == got.tobytes() and np.all(back[got.size:].view(np.uint64) == sentinel)


def test_groups_at_extreme_amplitudes(engine):
    """a group at 2^+40 beside one at 2^-40, Q S odd: the rows take their exponents from their own spectra"""
    for s in (1, 3):
        frames, delays, gains, _, _ = MC.signed_case(300, 5, s, 2, 3, 0.1)
        x = frames.copy()
        x[:3] *= 2.0 ** 40
        x[3:] *= 2.0 ** -40
        w = beamform.mvdr_weights(x, MC.FS, delays, gains, 0.1, 2)
        _parity(engine, (x, delays, gains, w, beamform.mvdr(x, MC.FS, delays, gains, 0.1, 2)), 0.1, 2, "S=%d, groups at 2^40 and 2^-40" % s)
    # inside one group: a frame at 2^-40 shares its transforms with its neighbours (S = 1: rows of frames 0 and 1 in one transform)
    frames, delays, gains, _, _ = MC.signed_case(300, 5, 1, 1, 3, 1.0)
    x = frames.copy()
    x[1] *= 2.0 ** -40
    w = beamform.mvdr_weights(x, MC.FS, delays, gains, 1.0, 1)
    _parity(engine, (x, delays, gains, w, beamform.mvdr(x, MC.FS, delays, gains, 1.0, 1)), 1.0, 1, "a frame at 2^-40 in a live group")


def test_exact_zero_cases(engine):
    frames, delays, gains, _, _ = MC.signed_case(300, 5, 3, 2, 3, 0.1)
    g = gains.copy()
    g[0, 1] = 0.0                                                                # a zero-gain source beside live ones
    g[1, 0] = 0.0
    w = beamform.mvdr_weights(frames, MC.FS, delays, g, 0.1, 2)
    got = _parity(engine, (frames, delays, g, w, beamform.mvdr(frames, MC.FS, delays, g, 0.1, 2)), 0.1, 2, "zero-gain sources")
    assert not got[:3, 1].any() and not got[3:, 0].any()
    assert got[:3, 0].any() and got[:3, 2].any() and got[3:, 1].any() and got[3:, 2].any()
    silent = frames.copy()
    silent[1] = 0.0                                                              # a zero frame in a live group
    silent[3:] = 0.0                                                             # and a silent group
    w = beamform.mvdr_weights(silent, MC.FS, delays, gains, 0.1, 2)
    got = _parity(engine, (silent, delays, gains, w, beamform.mvdr(silent, MC.FS, delays, gains, 0.1, 2)), 0.1, 2, "zero frame, silent group")
    assert not got[1].any() and not got[3:].any() and got[0].any() and got[2].any()
    assert not engine.mvdr(frames, MC.FS, delays, np.zeros_like(gains), 0.1, 2).any()   # no gains at all


def test_large_loading_is_delay_and_sum(engine):
    """loading 1e10 against Engine.steer at weights gains / q, within (2 M / loading + 2e-11) of steer's scale"""
    frames, delays, gains, _, _ = MC.signed_case(300, 5, 3, 2, 3, 1.0)
    got = engine.mvdr(frames, MC.FS, delays, gains, 1e10, 2)
    wt = np.repeat(gains / np.sum(gains * gains, axis=2, keepdims=True), 3, axis=0)
    want = engine.steer(frames, MC.FS, np.repeat(delays, 3, axis=0), wt)
    ratio = BC.worst_ratio(got, want, BC.tolerance(frames, wt, 2.0 * 5 / 1e10 + 2e-11))
    print("mvdr at loading 1e10 vs Engine.steer: worst deviation / bound = %.3g" % ratio)
    assert ratio <= 1.0


def test_steer_and_separate_are_unchanged_by_an_mvdr_call(engine):
    """the three share the scratch slot of the spectra, exponents and live marks"""
    frames, delays, weights, want = BC.random_case(300, 5, 3, 3)
    sx, sd, sg, swant = SC.signed_case(300, 5, 3, 3, 0.01)
    before = engine.steer(frames, BC.FS, delays, weights)
    sep = engine.separate(sx, SC.FS, sd, sg, 0.01)
    case = MC.signed_case(100, 64, 8, 1, 4, 0.1)
    engine.mvdr(case[0], MC.FS, case[1], case[2], 0.1, 1)
    assert engine.steer(frames, BC.FS, delays, weights).tobytes() == before.tobytes()
    assert engine.separate(sx, SC.FS, sd, sg, 0.01).tobytes() == sep.tobytes()
    assert BC.worst_ratio(before, want, BC.tolerance(frames, weights, 1e-11)) <= 1.0
    assert BC.worst_ratio(sep, swant, SC.tolerance(sx, sg, 0.01, 1e-11)) <= 1.0


def test_mvdr_device_is_engine_mvdr_at_point_delays(engine):
    frames = MC.signed_case(300, 5, 2, 2, 3, 0.1)[0]
    mics = np.random.default_rng(5).uniform(-0.5, 0.5, (5, 3))
    points = np.array([[1.0, 2.0, 0.5], [-2.0, 0.7, 1.0]])
    d, valid = beamform.point_delays(points, mics, MC.C)
    assert valid.all()
    tables = np.broadcast_to(d[None], (2, 2, 5))
    got = mvdr_device(frames, mics, MC.FS, MC.C, points=points, loading=0.1, groups=2, engine=engine)
    assert got.tobytes() == engine.mvdr(frames, MC.FS, tables, None, 0.1, 2).tobytes()
    per_group = np.stack([points, points[::-1]])                                 # [G][S][3]
    got = mvdr_device(frames, mics, MC.FS, MC.C, points=per_group, loading=0.1, groups=2, engine=engine)
    assert got[:3].tobytes() == engine.mvdr(frames[:3], MC.FS, d[None], None, 0.1, 1).tobytes()
    assert got[3:].tobytes() == engine.mvdr(frames[3:], MC.FS, d[None, ::-1], None, 0.1, 1).tobytes()
    bad = points.copy()
    bad[1, 0] = np.nan                                                           # a point nobody found: gains of 0, a row of zeros
    got = mvdr_device(frames, mics, MC.FS, MC.C, points=bad, groups=2, engine=engine)
    assert not got[:, 1].any() and got[:, 0].any()
    one = mvdr_device(frames[0], mics, MC.FS, MC.C, directions=np.array([[0.0, 0.0, 1.0]]), engine=engine)
    assert one.shape == (1, 300) and np.all(np.isfinite(one)) and one.any()
    with pytest.raises(ValueError):
        mvdr_device(frames, mics, MC.FS, MC.C, engine=engine)
    with pytest.raises(ValueError):
        mvdr_device(frames, mics, MC.FS, MC.C, points=points, groups=4, engine=engine)


def test_refusals(engine):
    frames, delays, gains, _, _ = MC.random_case(200, 2, 2, 1, 2, 0.1)
    b, m, length = frames.shape
    with pytest.raises(ValueError):
        engine.mvdr(np.ones((1, 2, 99)), MC.FS, delays, gains)
    with pytest.raises(PalError):
        engine.mvdr(np.ones((1, 1, 2 ** 19 + 1)), MC.FS, np.zeros((1, 1, 1)), np.ones((1, 1, 1)))
    _still_works(engine)
    with pytest.raises(ValueError):
        engine.mvdr(np.ones((1, 0, 200)), MC.FS, np.zeros((1, 2, 0)))            # M = 0
    with pytest.raises(ValueError):
        engine.mvdr(frames, MC.FS, np.zeros((1, 0, 2)))                          # S = 0
    with pytest.raises(ValueError):
        engine.mvdr(frames, MC.FS, delays, gains[:, :1])
    with pytest.raises(ValueError):
        engine.mvdr(frames, MC.FS, delays, gains, 0.1, 3)                        # 2 frames in 3 groups
    with pytest.raises(ValueError):
        engine.mvdr(frames, MC.FS, delays, gains, 0.1, 2)                        # one table for two groups
    with pytest.raises(ValueError):
        engine.mvdr(frames, 0.0, delays, gains)
    with pytest.raises(ValueError):
        engine.mvdr(frames, np.inf, delays, gains)
    _still_works(engine)
    with _device(engine, frames, delays, gains, b * 2 * length) as (d_x, d_d, d_g, d_out):
        for bad in (0.0, -0.01, np.nan, np.inf, -np.inf):
            with pytest.raises(ValueError):
                engine.mvdr(frames, MC.FS, delays, gains, bad)
            with pytest.raises(ValueError):
                engine.mvdr_dev(d_x, b, m, length, MC.FS, d_d, d_g, 1, 2, bad, d_out)
        for groups in (0, -1, 3):
            with pytest.raises(ValueError):
                engine.mvdr_dev(d_x, b, m, length, MC.FS, d_d, d_g, groups, 2, 0.1, d_out)
        with pytest.raises(PalError) as unsupported:                             # M = 65: one wavefront factors a bin
            engine.mvdr_dev(d_x, 1, 65, length, MC.FS, d_d, d_g, 1, 1, 0.1, d_out)
        assert not isinstance(unsupported.value, ValueError)
        with pytest.raises(PalError) as unsupported:                             # 64 microphones at 2^19 samples: a 17 GB triangle
            engine.mvdr_dev(d_x, 1, 64, 2 ** 19, MC.FS, d_d, d_g, 1, 1, 0.1, d_out)
        assert not isinstance(unsupported.value, ValueError)
    with pytest.raises(PalError) as unsupported:
        engine.mvdr(np.ones((1, 65, 100)), MC.FS, np.zeros((1, 1, 65)))
    assert not isinstance(unsupported.value, ValueError)
    _still_works(engine)
    for which, value in ((0, np.nan), (0, np.inf), (1, np.nan), (1, -np.inf), (0, (length + 1) / MC.FS), (0, -(length + 1) / MC.FS)):
        tabs = [delays.copy(), gains.copy()]
        tabs[which][0, 1, 1] = value
        with pytest.raises(ValueError):
            engine.mvdr(frames, MC.FS, tabs[0], tabs[1])
        _still_works(engine)
        with _device(engine, frames, tabs[0], tabs[1], b * 2 * length) as (d_x, d_d, d_g, d_out):
            engine.mvdr_dev(d_x, b, m, length, MC.FS, d_d, d_g, 1, 2, 0.1, d_out)
            with pytest.raises(ValueError):
                engine.synchronize()
        _still_works(engine)
    edge = delays.copy()
    edge[0, 0, 0] = length / MC.FS                                               # |d| fs = L exactly is still allowed
    engine.mvdr(frames, MC.FS, edge, gains)
    bad = frames.copy()
    bad[0, 1, 17] = np.nan
    with pytest.raises(ValueError):
        engine.mvdr(bad, MC.FS, delays, gains)
    _still_works(engine)
    with _device(engine, bad, delays, gains, b * 2 * length) as (d_x, d_d, d_g, d_out):
        engine.mvdr_dev(d_x, b, m, length, MC.FS, d_d, d_g, 1, 2, 0.1, d_out)
        with pytest.raises(ValueError):
            engine.synchronize()
    _still_works(engine)
    # NULL pointers and bad counts through the raw ABI
    lib, h = engine._lib, engine._h
    x, d, g, out = frames.copy(), delays.copy(), gains.copy(), np.empty((b, 2, length))
    ptrs = [x.ctypes.data, d.ctypes.data, g.ctypes.data, out.ctypes.data]
    for hole in range(4):
        p = [None if q == hole else v for q, v in enumerate(ptrs)]
        assert lib.pal_mvdr(h, p[0], b, m, length, MC.FS, p[1], p[2], 1, 2, 0.1, p[3], None) == _ffi.ERR_INVALID
        assert lib.pal_mvdr_dev(h, ctypes.c_void_p(p[0]), b, m, length, MC.FS, ctypes.c_void_p(p[1]), ctypes.c_void_p(p[2]), 1, 2, 0.1,
                                ctypes.c_void_p(p[3]), None) == _ffi.ERR_INVALID
    for bb, mm, ss, gg in ((0, m, 2, 1), (b, 0, 2, 1), (b, m, 0, 1), (b, m, 2, 0), (b, m, 2, 3)):
        assert lib.pal_mvdr(h, ptrs[0], bb, mm, length, MC.FS, ptrs[1], ptrs[2], gg, ss, 0.1, ptrs[3], None) == _ffi.ERR_INVALID
    assert lib.pal_mvdr(h, ptrs[0], 1, 65, length, MC.FS, ptrs[1], ptrs[2], 1, 1, 0.1, ptrs[3], None) == _ffi.ERR_UNSUPPORTED
    _still_works(engine)


def test_mvdr_gains_3_db_beside_an_unlisted_interferer(engine):
    """the scene of tests/test_host_mvdr.py with rows from Engine.fractional_delay, both beamformers on the device: the
    specification's figures to the digits printed (2.78 and 9.76 dB) and the 3 dB condition"""
    mics, frames, bases = MC.scene(lambda rows, delays: engine.fractional_delay(rows, delays, MC.FS))
    target = MC.SCENE_SOURCES[0:1]
    das = beamform_device(frames, mics, MC.FS, MC.C, points=target, engine=engine)[:, 0]
    adaptive = mvdr_device(frames, mics, MC.FS, MC.C, points=target, loading=MC.SCENE_LOADING, groups=1, engine=engine)[:, 0]
    s_das = MC.scene_snr(mics, bases, das, "delay-and-sum (device)")
    s_mvdr = MC.scene_snr(mics, bases, adaptive, "MVDR (device)")
    print("MVDR (device) gains %.2f dB" % (s_mvdr - s_das))
    assert "%.2f" % s_das == "2.78" and "%.2f" % s_mvdr == "9.76"
    assert s_mvdr - s_das >= 3.0
