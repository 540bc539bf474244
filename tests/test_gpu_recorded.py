"""Recorded audio on the device: Engine.resample against signal_processing.resample_kaiser_best bit for bit, the device forms of
normalise / compress and of the frame cutter, and stream.recorded_tdoa_stream / recorded_position_stream against the staged
path (host arrays between the stages), frame by frame."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (rows, input samples, original rate, target rate).  One row: the cases of tests/test_host_recorded.py (the per-sample
# function on the CPU).  R = 3, N = 1000, 48000 -> 44100: 918 outputs = three full workgroups and a partial one, wings
# truncated at both ends of the row, the row index in the addressing.  R = 2, N = 700, 8000 -> 32000: ratio 4.
CASES = [(1, 2, 48000, 44100), (1, 97, 48000, 44100), (1, 300, 44100, 48000), (1, 257, 96000, 16000), (1, 411, 8000, 8000),
         (1, 130, 22050, 44100), (1, 600, 44100, 16000), (3, 1000, 48000, 44100), (2, 700, 8000, 32000)]
# the kernel's other path: at ratio 1/16 a workgroup's input span (255 * 16 + 2 * 1024 + 2 samples) is beyond the LDS budget and is
# read from global memory; below 1/512 the table step is 0 and there are no taps (the host function's `// 0`)
CASES += [(2, 5000, 48000, 3000), (1, 2100, 1024000, 1000)]


@pytest.fixture(scope="module", autouse=True)
def _engine(engine):
    import pyaudiolocalization_amd.engine as E
    E._default = engine
    yield
    E._default = None


@pytest.mark.parametrize("r,n,fs0,fs1", CASES)
def test_resample_equals_host_function(engine, r, n, fs0, fs1):
    from pyaudiolocalization_amd.signal_processing import resample_audio, resample_kaiser_best
    x = np.random.default_rng([r, n, fs0, fs1]).standard_normal((r, n))
    keep = x.copy()
    with np.errstate(divide="ignore"):
        want = resample_kaiser_best(x, float(fs0), float(fs1))
    got = engine.resample(x, float(fs0), float(fs1))
    assert got.shape == want.shape == (r, int(n * (fs1 / fs0)))
    assert np.array_equal(got, want), float(np.max(np.abs(got - want)))
    assert np.array_equal(x, keep)                                             # the input is left untouched
    # the same rows already in HBM: the same bytes, and the uploaded rows are still what was uploaded
    d_in, d_out = engine.alloc(x.nbytes), engine.alloc(want.nbytes)
    try:
        engine.upload(d_in, x)
        assert engine.resample_dev(d_in, r, n, float(fs0), float(fs1), d_out, want.shape[1]) == want.shape[1]
        engine.synchronize()
        dev, back = np.empty_like(want), np.empty_like(x)
        engine.download(dev, d_out)
        engine.download(back, d_in)
    finally:
        engine.free(d_in); engine.free(d_out)
    assert dev.tobytes() == want.tobytes()
    assert back.tobytes() == x.tobytes()
    if r == 1:                                                                 # the public switch, one-dimensional input
        assert np.array_equal(resample_audio(x[0], float(fs0), float(fs1), resampler="device"), want[0])


def test_resample_refuses_what_the_host_function_refuses(engine):
    from pyaudiolocalization_amd.signal_processing import resample_kaiser_best
    one = np.ones(1)
    with pytest.raises(ValueError) as host:
        resample_kaiser_best(one, 48000, 44100)
    with pytest.raises(ValueError) as dev:
        engine.resample(one, 48000, 44100)                                     # int(1 * 0.91875) = 0 output samples
    assert str(dev.value) == str(host.value)
    with pytest.raises(ValueError) as host:
        resample_kaiser_best(np.ones(50), 48000, -44100)
    with pytest.raises(ValueError) as dev:
        engine.resample(np.ones(50), 48000, -44100)
    assert str(dev.value) == str(host.value)
    d = engine.alloc(800)
    try:
        with pytest.raises(ValueError):                                        # the ABI's own checks: a rate of zero, a short buffer
            engine._check(engine._lib.pal_resample_dev(engine._h, d, 1, 100, 0.0, 44100.0, d, 100, ctypes.byref(ctypes.c_int())))
        with pytest.raises(ValueError):
            engine.resample_dev(d, 1, 50, 8000.0, 16000.0, d, 99)
    finally:
        engine.free(d)
    assert engine.resample(np.ones(50), 8000.0, 16000.0).shape == (100,)       # the engine is usable afterwards


def test_normalize_compress_dev_equals_host_form(engine):
    rows = np.random.default_rng(71).standard_normal((3, 777)) * np.array([[0.01], [1.0], [300.0]])
    rows[1] = 0.0
    d_in, d_out = engine.alloc(rows.nbytes), engine.alloc(rows.nbytes)
    try:
        engine.upload(d_in, rows)
        for only in (False, True):
            want = engine.normalize_compress(rows, normalize_only=only)
            engine.normalize_compress_dev(d_in, 3, 777, d_out, normalize_only=only)
            engine.synchronize()
            got = np.empty_like(rows)
            engine.download(got, d_out)
            assert got.tobytes() == want.tobytes(), only
            assert not got[1].any()
        engine.normalize_compress_dev(d_in, 3, 777, d_in)                      # in place
        engine.synchronize()
        engine.download(got, d_in)
        assert got.tobytes() == engine.normalize_compress(rows).tobytes()
    finally:
        engine.free(d_in); engine.free(d_out)


def test_frame_rows_dev_equals_numpy_slicing(engine):
    from pyaudiolocalization_amd.stream import frame_count, frame_rows
    m, t, frame_len = 3, 1000, 256
    rows = np.random.default_rng(72).standard_normal((m, t))
    d_rows, d_out = engine.alloc(rows.nbytes), engine.alloc(8 * m * frame_len * 8)
    try:
        engine.upload(d_rows, rows)
        for hop, count in ((100, 8), (256, 3), (300, 3)):                      # overlapping, abutting, with gaps
            assert frame_count(t, frame_len, hop) == count
            want = frame_rows(rows, frame_len, hop)
            for first in (0, 2):
                got = np.empty((count - first, m, frame_len))
                engine.frame_rows_dev(d_rows, m, t, frame_len, hop, first, count - first, d_out)
                engine.synchronize()
                engine.download(got, d_out)
                assert got.tobytes() == np.ascontiguousarray(want[first:]).tobytes(), (hop, first)
            with pytest.raises(ValueError):                                    # one frame more would read past the row
                engine.frame_rows_dev(d_rows, m, t, frame_len, hop, 0, count + 1, d_out)
            with pytest.raises(ValueError):
                engine.frame_rows_dev(d_rows, m, t, frame_len, hop, count, 1, d_out)
        with pytest.raises(ValueError):
            engine.frame_rows_dev(d_rows, m, t, frame_len, 0, 0, 1, d_out)
    finally:
        engine.free(d_rows); engine.free(d_out)


# ---------------------------------------------------------------- the recorded stream against the staged path
FS_IN, FS, FRAME_LEN, HOP, MED = 12000.0, 8000.0, 1500, 1000, 0.01


def _recording(m=4, t_in=6000, silence=True):
    """One common noise sequence per microphone, delayed by an integer lag that changes half-way through the recording, plus
    independent noise at 0.3.  Microphone 2 is digital silence from before frame 1 to after it: the resampler's wings span 96
    input samples at this ratio, frame 1 is samples 1000 .. 2499 at 8 kHz = 1500 .. 3749 at 12 kHz.  (Seed chosen on the CPU:
    the oracle's synchronize_signals gives the lengths 1513, 1508, 1509 for the three frames of the host-resampled rows.)"""
    rng = np.random.default_rng(0)
    common = rng.standard_normal(t_in + 64)
    lags = np.array([[0, 0], [5, 9], [-7, 3], [12, -4]])
    half = t_in // 2
    rows = np.empty((m, t_in))
    for i in range(m):
        for h, (a, b) in enumerate(((0, half), (half, t_in))):
            rows[i, a:b] = common[32 + lags[i, h] + a: 32 + lags[i, h] + b]
    rows += 0.3 * rng.standard_normal((m, t_in))
    if silence:
        rows[2, 1400:3850] = 0.0
    return rows


def _staged(engine, rows, fs_in, fs, filter_method, med):
    """Engine.resample on host arrays -> normalize_compress -> NumPy framing -> synchronize_signals_improved ->
    noise_reduction_rows -> main.tdoa_table, frame by frame."""
    from pyaudiolocalization_amd.main import tdoa_table
    from pyaudiolocalization_amd.signal_processing import noise_reduction_rows
    from pyaudiolocalization_amd.stream import frame_rows
    from pyaudiolocalization_amd.utils import synchronize_signals_improved
    rs = rows if fs_in == fs else engine.resample(rows, fs_in, fs)
    frames = frame_rows(engine.normalize_compress(rs), FRAME_LEN, HOP)
    tables, lengths = [], []
    for frame in frames:
        filt = noise_reduction_rows(np.array(synchronize_signals_improved(list(frame), fs)), fs, filter_method)
        tables.append(tdoa_table(filt, fs, med))
        lengths.append(filt.shape[1])
    return frames, tables, lengths


@pytest.fixture(scope="module")
def staged(engine):
    rows = _recording()
    return (rows,) + _staged(engine, rows, FS_IN, FS, "butterworth", MED)


def test_recorded_tdoa_stream_equals_staged_path(engine, staged):
    from pyaudiolocalization_amd.stream import recorded_tdoa_stream
    rows, frames, want, want_len = staged
    keep = rows.copy()
    assert frames.shape == (3, 4, FRAME_LEN) and not frames[1, 2].any() and frames[0, 2].any() and frames[2, 2].any()
    timings = {}
    tables, lengths = recorded_tdoa_stream(rows, FS_IN, FS, FRAME_LEN, HOP, "butterworth", MED, engine=engine, frames_per_batch=2,
                                           timings=timings)
    assert tables.shape == (3, 6) and lengths.shape == (3,)
    assert np.array_equal(rows, keep)
    for f in range(3):
        assert lengths[f] == want_len[f], f
        assert tables[f].tobytes() == want[f].tobytes(), f
    assert len(set(int(v) for v in lengths)) >= 2                              # the case does exercise the grouping by length
    assert {"upload", "resample", "normalize", "frames", "pairs"} <= set(timings)
    # one batch for all frames: the same tables
    again, len2 = recorded_tdoa_stream(rows, FS_IN, FS, FRAME_LEN, HOP, "butterworth", MED, engine=engine)
    assert again.tobytes() == tables.tobytes() and np.array_equal(len2, lengths)


def test_recorded_tdoa_stream_skips_the_resampler_at_equal_rates(engine):
    from pyaudiolocalization_amd.stream import recorded_tdoa_stream
    rows = _recording(silence=False)[:, :4000]                                 # (a silent stretch is 0 / 0 in the Wiener filter, as in SciPy's)
    _, want, want_len = _staged(engine, rows, FS, FS, "wiener", None)
    timings = {}
    tables, lengths = recorded_tdoa_stream(rows, FS, FS, FRAME_LEN, HOP, "wiener", None, engine=engine, frames_per_batch=2, timings=timings)
    assert "resample" not in timings
    assert tables.shape == (3, 6)
    for f in range(3):
        assert lengths[f] == want_len[f], f
        assert tables[f].tobytes() == want[f].tobytes(), f


def test_recorded_position_stream(engine, staged):
    from pyaudiolocalization_amd.stream import recorded_position_stream
    rows, _, want, want_len = staged
    mics = np.array([[0.0, 0.0, 0.0], [0.6, 0.0, 0.1], [0.0, 0.7, 0.0], [0.1, 0.1, 0.8]])
    positions, tables, lengths = recorded_position_stream(rows, FS_IN, FS, FRAME_LEN, HOP, mics, 343.0, "butterworth", MED, engine=engine,
                                                          frames_per_batch=2)
    assert [int(v) for v in lengths] == want_len
    for f in range(3):
        assert tables[f].tobytes() == want[f].tobytes(), f
    solved = engine.solve_positions(tables, lengths, mics, FS, 343.0)
    assert positions.tobytes() == solved.tobytes()
