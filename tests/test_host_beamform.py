"""The beamformer's specification (pyaudiolocalization_amd/beamform.py) on the CPU: steer against the plain sum of the oracle's
fractional_delay rows, the delay helpers against plain loops, and the array gain the feature exists for.

Tolerance of steer against the plain sum: 1e-13 * sum_m |w| max|x_m| - both sides are the same transforms in another order of
summation (the fade window after the sum instead of per row), a few ulps per term; the worst ratio is printed."""
import numpy as np
import pytest

from oracle import pal_oracle as O
from pyaudiolocalization_amd import _ffi, beamform, srp

import beamform_cases as BC


@pytest.mark.parametrize("length", BC.HOST_LENGTHS)
def test_steer_is_the_weighted_sum_of_fractional_delays(length):
    worst = 0.0
    for m in BC.HOST_MICS:
        frames, delays, weights, got = BC.random_case(length, m, 3, 1)
        want = BC.plain_sum(frames, delays, weights)
        ratio = BC.worst_ratio(got, want, BC.tolerance(frames, weights, 1e-13))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (length, m, ratio)
    print("steer vs plain sum, L=%d: worst error / (1e-13 scale) = %.3g" % (length, worst))


def test_fade_window_is_the_oracles():
    for n in (100, 199, 200, 299, 300, 1501):
        assert np.array_equal(beamform.fade_window(n), O.fade_window(n))
    with pytest.raises(ValueError):
        beamform.fade_window(99)


def test_steer_shape_errors():
    x = np.zeros((2, 3, 100))
    with pytest.raises(ValueError):
        beamform.steer(x[0], BC.FS, np.zeros((2, 1, 3)), np.zeros((2, 1, 3)))
    with pytest.raises(ValueError):
        beamform.steer(x, BC.FS, np.zeros((2, 1, 4)), np.zeros((2, 1, 4)))
    with pytest.raises(ValueError):
        beamform.steer(x, BC.FS, np.zeros((2, 1, 3)), np.zeros((2, 2, 3)))


def _mics(m=6, seed=3):
    return np.random.default_rng(seed).uniform(-0.5, 0.5, (m, 3))


def test_point_delays_against_a_loop():
    mics = _mics()
    rng = np.random.default_rng(4)
    points = rng.uniform(-3, 3, (2, 4, 3))
    points[1, 2, 1] = np.nan
    points[0, 3, 0] = np.inf
    calib = rng.uniform(0, 1e-3, 6)
    for cal in (None, calib):
        d, valid = beamform.point_delays(points, mics, BC.C, cal)
        assert d.shape == (2, 4, 6) and valid.shape == (2, 4)
        for b in range(2):
            for s in range(4):
                ok = bool(np.all(np.isfinite(points[b, s])))
                assert valid[b, s] == ok
                if not ok:
                    assert not d[b, s].any()
                    continue
                r = [float(np.sqrt(np.sum((points[b, s] - mics[m]) ** 2))) for m in range(6)]
                if cal is None:
                    want = np.array([(max(r) - r[m]) / BC.C for m in range(6)])
                else:
                    want = np.array([(max(r) / BC.C - r[m] / BC.C) + (max(cal) - cal[m]) for m in range(6)])
                    want = want - min(want)
                assert np.allclose(d[b, s], want, rtol=0, atol=1e-17), (b, s, cal is None)
                assert d[b, s].min() == 0.0 and np.all(d[b, s] >= 0)
                if cal is None:
                    assert int(np.argmin(d[b, s])) == int(np.argmax(r))          # the farthest microphone gets 0


def test_calibration_delays_line_the_rows_up():
    """a row that is late by calib[m] on top of its path needs exactly that much less delay: path + calib + delay is one constant"""
    mics = _mics()
    calib = np.array([0.0, 2e-4, 5e-4, 1e-4, 0.0, 3e-4])
    p = np.array([1.0, -2.0, 0.3])
    d, _ = beamform.point_delays(p, mics, BC.C, calib)
    arrival = np.linalg.norm(p - mics, axis=1) / BC.C + calib + d
    assert np.ptp(arrival) < 1e-15
    with pytest.raises(ValueError):
        beamform.point_delays(p, mics, BC.C, calib[:5])


def test_direction_delays_against_a_loop_and_a_plane_wave():
    mics = _mics(8, 6)
    az, el = np.deg2rad(35.0), np.deg2rad(20.0)
    u = np.array([[np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], [np.nan, 0.0, 1.0], [0.0, 0.0, -1.0]])
    calib = np.random.default_rng(8).uniform(0, 1e-3, 8)
    for cal in (None, calib):
        d, valid = beamform.direction_delays(u, mics, BC.C, cal)
        assert valid.tolist() == [True, False, True] and not d[1].any()
        for g in (0, 2):
            a = srp.doa_advances(u[g], mics)[0]
            want = np.array([(a[m] - min(a)) / BC.C for m in range(8)])
            if cal is not None:
                want = want + (max(cal) - cal)
                want = want - min(want)
            assert np.allclose(d[g], want, rtol=0, atol=1e-17)
            assert d[g].min() == 0.0 and np.all(d[g] >= 0)
    # a plane wave built with the same advances: microphone m hears base(t + a_m / c), i.e. the base delayed by (max a - a_m) / c
    length = 2048
    base = np.random.default_rng(9).standard_normal(length)
    a = srp.doa_advances(u[0], mics)[0]
    rows = np.array([O.fractional_delay(base, (np.max(a) - a[m]) / BC.C, BC.FS) for m in range(8)])
    d, valid = beamform.direction_delays(u[0], mics, BC.C)
    beam = beamform.steer(rows[None], BC.FS, d[None, None], beamform.uniform_weights(valid, 8)[None, None])[0, 0]
    ref = O.fractional_delay(base, (np.max(a) - np.min(a)) / BC.C, BC.FS)        # every row ends up beside the latest one
    core = slice(100, length - 100)                                             # (away from the fade windows applied twice)

    def corr(y):
        return float(np.dot(y[core], ref[core]) / np.sqrt(np.dot(y[core], y[core]) * np.dot(ref[core], ref[core])))

    # two fractional delays of a truncated white row are one delay up to the sinc tails of the cut ends (1e-3 of the row here):
    # aligned rows correlate with the reference to 0.999; under the opposite sign convention the eight white rows sit up to 90
    # samples apart and only the microphones whose advance is near the extreme still line up
    wrong, _ = beamform.direction_delays(-u[0], mics, BC.C)
    off = beamform.steer(rows[None], BC.FS, wrong[None, None], beamform.uniform_weights(valid, 8)[None, None])[0, 0]
    print("plane wave: correlation with the reference %.6f aligned, %.3f under the opposite sign" % (corr(beam), corr(off)))
    assert corr(beam) >= 0.999
    assert abs(corr(off)) < 0.5


def test_uniform_weights():
    w = beamform.uniform_weights(np.array([[True, False], [False, True]]), 4)
    assert w.shape == (2, 2, 4)
    assert np.array_equal(w[0, 0], np.full(4, 0.25)) and np.array_equal(w[1, 1], np.full(4, 0.25))
    assert not w[0, 1].any() and not w[1, 0].any()


def test_records_to_points():
    peaks = np.zeros((2, 2), dtype=_ffi.SRP_PEAK)
    peaks["x"], peaks["y"], peaks["z"] = 1.0, 2.0, 3.0
    peaks["index"] = [[5, -1], [0, 7]]
    p = beamform.records_to_points(peaks)
    assert p.shape == (2, 2, 3)
    assert np.array_equal(p[0, 0], [1.0, 2.0, 3.0]) and np.all(np.isnan(p[0, 1])) and np.array_equal(p[1, 0], [1.0, 2.0, 3.0])
    zoom = np.zeros(4, dtype=_ffi.SRP_ZOOM)
    zoom["x"], zoom["y"], zoom["z"] = -1.0, 0.5, 0.25
    zoom["seed"] = [0, -1, 3, 2]
    zoom["levels"] = [3, 3, 0, 1]
    q = beamform.records_to_points(zoom)
    assert [bool(np.all(np.isfinite(v))) for v in q] == [True, False, False, True]
    assert np.array_equal(q[3], [-1.0, 0.5, 0.25])
    with pytest.raises(ValueError):
        beamform.records_to_points(np.zeros(3))
    # an absent record steers to a row of zeros: no valid point, zero weights
    d, valid = beamform.point_delays(p, _mics(), BC.C)
    w = beamform.uniform_weights(valid, 6)
    assert not valid[0, 1] and not w[0, 1].any() and not d[0, 1].any()
    out = beamform.steer(np.ones((2, 6, 100)), BC.FS, d, w)
    assert not out[0, 1].any() and out[0, 0].any()


def test_array_gain_of_the_specification():
    """M microphones with independent unit noise: the beam at the source gains 10 log10(M) dB over one aligned microphone (the 1 dB
    covers one noise draw); a beam 3.3 m away lies below the single microphone.  Computed with this seed: -0.02 dB for one
    microphone, 9.04 dB at the source (10 log10 8 = 9.03), -19.3 dB at the other point."""
    mics, frames, ref = BC.gain_scene()
    single, at_source, elsewhere = BC.gain_figures(lambda x, d, w: beamform.steer(x, BC.FS, d, w), mics, frames, ref)
    print("array gain (specification): one microphone %.2f dB, beam at the source %.2f dB, beam elsewhere %.2f dB" % (single, at_source, elsewhere))
    assert at_source - single >= 10.0 * np.log10(BC.GAIN_M) - 1.0
    assert elsewhere < single


def test_two_sources_found_and_separated_by_the_specifications():
    """the chain of tests/test_gpu_beamform.py on the CPU: the oracle's correlation rows, srp.strips / srp_map / map_peaks / zoom, then
    beamform.steer at the two zoomed positions - the scene itself meets the two conditions the device is held to"""
    from pyaudiolocalization_amd.engine import pair_list
    mics, frames, bases = BC.two_source_scene()
    rows = np.stack([O.phat_correlation(frames[i], frames[j]) for i, j in pair_list(BC.TWO_M)])
    t = srp.half_width(mics, BC.FS, BC.C)
    st = srp.strips(rows, BC.TWO_L, t, BC.TWO_W)
    power, _ = srp.srp_map(st, t, mics, BC.FS, BC.C, BC.TWO_LO, BC.TWO_HI, BC.TWO_COUNT)
    peaks = srp.map_peaks(power.reshape(BC.TWO_COUNT), 2, BC.TWO_R, BC.TWO_LO, BC.TWO_HI)
    lo, hi, count = srp.check_grid(BC.TWO_LO, BC.TWO_HI, BC.TWO_COUNT)
    zoomed = srp.zoom(st, t, mics, BC.FS, BC.C, peaks, (hi - lo) / count, *BC.TWO_ZOOM)
    found = beamform.records_to_points(zoomed)
    d, valid = beamform.point_delays(found, mics, BC.C)
    beams = beamform.steer(frames[None], BC.FS, d[None], beamform.uniform_weights(valid, BC.TWO_M)[None])[0]
    BC.two_source_check(mics, frames, bases, found, beams, "specification")
