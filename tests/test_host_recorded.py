"""The recorded-audio entrance on the host: csrc/resample_math.h compiled for the CPU (tests/host/test_resample_math.cpp, with
the address and undefined-behaviour sanitizers) against signal_processing.resample_kaiser_best bit for bit, the frame-count rule,
the input checks of stream.recorded_tdoa_stream / recorded_position_stream, and the unchanged default of resample_audio.  No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from pyaudiolocalization_amd import signal_processing as SP
from pyaudiolocalization_amd import stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (input samples, original rate, target rate): the shortest input that gives an output at all, both wings truncated at both
# ends, up- and downsampling with index steps that do not divide the table, a wing longer than the row (96000 -> 16000), the
# identity ratio and an integer one
CASES = [(2, 48000, 44100), (97, 48000, 44100), (300, 44100, 48000), (257, 96000, 16000), (411, 8000, 8000), (130, 22050, 44100),
         (600, 44100, 16000)]
# beyond the issue's list: a ratio whose workgroup span is read from global memory in the kernel (1/16), and one below 1/512,
# where int(scale * 512) = 0 and the host function's `// 0` gives no taps at all (all-zero output, NumPy warns)
CASES += [(500, 48000, 3000), (2100, 1024000, 1000)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    out = tmp_path_factory.mktemp("resample_math") / "test_resample_math"
    subprocess.run(["hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "pyaudiolocalization_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "test_resample_math.cpp"), "-o", str(out)], check=True)
    return str(out)


@pytest.fixture(scope="module")
def win_file(tmp_path_factory):
    win, num_table = SP._kaiser_best_filter()
    path = tmp_path_factory.mktemp("kaiser_best") / "win.bin"
    np.ascontiguousarray(win, dtype=np.float64).tofile(path)
    return str(path), num_table


@pytest.mark.parametrize("n,fs0,fs1", CASES)
def test_per_sample_header_equals_resample_kaiser_best(exe, win_file, tmp_path, n, fs0, fs1):
    """One scalar loop per output sample, the taps in the specification's order, multiply then add: the same bits as the
    vectorised host function (whose extra 0.0 * x terms for ended wings leave a finite sum unchanged)."""
    x = np.random.default_rng([n, fs0, fs1]).standard_normal(n)
    with np.errstate(divide="ignore"):
        want = SP.resample_kaiser_best(x, float(fs0), float(fs1))
    x.tofile(tmp_path / "x.bin")
    run = subprocess.run([exe, win_file[0], str(win_file[1]), str(tmp_path / "x.bin"), repr(float(fs0)), repr(float(fs1)),
                          str(tmp_path / "y.bin")], capture_output=True, text=True)
    assert run.returncode == 0 and "ALL OK" in run.stdout, run.stdout + run.stderr
    got = np.fromfile(tmp_path / "y.bin", dtype=np.float64)
    assert got.shape == want.shape
    assert np.array_equal(got, want), float(np.max(np.abs(got - want)))


@pytest.mark.parametrize("t,frame_len,hop,count", [(1000, 256, 100, 8), (1000, 256, 256, 3), (1000, 256, 300, 3), (1000, 1000, 1, 1),
                                                   (1000, 999, 1, 2), (4000, 1500, 1000, 3), (256, 256, 7, 1)])
def test_frame_count_rule(t, frame_len, hop, count):
    """F = (T - frame_len) // hop + 1: every frame lies inside the recording and one more would not."""
    assert stream.frame_count(t, frame_len, hop) == count
    rows = np.arange(3 * t, dtype=np.float64).reshape(3, t)
    frames = stream.frame_rows(rows, frame_len, hop)
    assert frames.shape == (count, 3, frame_len)
    for f in range(count):
        assert np.array_equal(frames[f], rows[:, f * hop: f * hop + frame_len])
    assert (count - 1) * hop + frame_len <= t < count * hop + frame_len


class _NoEngine:
    """Any use of the engine fails the test: the input checks come before GPU work."""
    def __getattr__(self, name):
        raise AssertionError(f"engine.{name} was reached before the input checks")


@pytest.mark.parametrize("entrance", ["tdoa", "position"])
def test_recorded_stream_input_checks(entrance):
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((3, 1200))
    mics = rng.uniform(-1, 1, (3, 3))

    def call(recordings, fs_in=12000.0, fs=8000.0, frame_len=400, hop=200, **kw):
        if entrance == "tdoa":
            return stream.recorded_tdoa_stream(recordings, fs_in, fs, frame_len, hop, engine=_NoEngine(), **kw)
        return stream.recorded_position_stream(recordings, fs_in, fs, frame_len, hop, mics, 343.0, engine=_NoEngine(), **kw)

    with pytest.raises(ValueError):
        call([rows[0], rows[1][:-1], rows[2]])                  # rows of unequal length
    with pytest.raises(ValueError):
        call(rows[:1])                                          # fewer than two microphones
    with pytest.raises(ValueError):
        call(rows, frame_len=801)                               # 1200 samples at 12 kHz are 800 at 8 kHz
    with pytest.raises(ValueError):
        call(rows, fs_in=8000.0, frame_len=1201)                # no resampling: T = T_in
    with pytest.raises(ValueError):
        call(rows, hop=0)
    with pytest.raises(ValueError):
        call(rows, filter_method="median-filter")
    with pytest.raises(AssertionError):                         # valid arguments do get as far as the engine
        call(rows, frame_len=800)


def test_resample_audio_default_is_the_host_path():
    x = np.random.default_rng(9).standard_normal((2, 200))
    want = SP.resample_audio(x, 48000.0, 44100.0)
    assert np.array_equal(SP.resample_audio(x, 48000.0, 44100.0, resampler="host"), want)
    with pytest.raises(ValueError):
        SP.resample_audio(x, 48000.0, 44100.0, resampler="fpga")
