"""The MVDR beamformer's specification (pyaudiolocalization_amd/beamform.py: mvdr_covariance, mvdr_weights, mvdr) on the CPU: against
the direct formulation with einsum and np.linalg.solve, the consequences its docstring states, the refusals of the Python layer,
csrc/mvdr_geometry.h compiled for the CPU with the sanitizers on, and the gain the feature exists for: a target beside an interferer
nobody listed.  Tolerances: tests/mvdr_cases.py; every parity test prints the worst error / tolerance it saw."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from pyaudiolocalization_amd import beamform

import beamform_cases as BC
import mvdr_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("loading", MC.LOADINGS)
@pytest.mark.parametrize("length,m,s,g,q", MC.HOST_CASES)
def test_mvdr_is_the_loaded_minimum_variance_solution(length, m, s, g, q, loading):
    frames, delays, gains, w, got = MC.random_case(length, m, s, g, q, loading)
    wd, want = MC.direct(frames, delays, gains, loading, g)
    ratio = BC.worst_ratio(got, want, MC.tolerance(frames, w, loading, 1e-15))
    wratio = MC.weight_ratio(w, wd, m, loading, 1e-15)
    print("mvdr vs np.linalg.solve, L=%d M=%d S=%d G=%d Q=%d loading=%g: worst error / tol = %.3g (beams), %.3g (weights)"
          % (length, m, s, g, q, loading, ratio, wratio))
    assert ratio <= 1.0 and wratio <= 1.0
    # the distortionless constraint: w^H a = 1 at every bin
    f = np.fft.fftfreq(2 * length, d=1.0 / MC.FS)
    a = gains[..., None] * np.exp(1j * 2 * np.pi * f * delays[..., None])
    assert np.allclose(np.sum(np.conj(w) * a, axis=2), 1.0, rtol=0, atol=1e-13 * MC.kappa(m, loading))


def test_covariance_is_the_lower_triangle_of_the_sample_covariance():
    frames = MC.random_case(100, 5, 2, 2, 3, 0.1)[0]
    r = beamform.mvdr_covariance(frames, 2)
    assert r.shape == (2, 5, 5, 200)
    spec = np.fft.fft(frames, n=200, axis=-1).reshape(2, 3, 5, 200)
    full = np.einsum("gqik,gqjk->gijk", spec, spec.conj())
    for i in range(5):
        assert not r[:, i, i].imag.any() and np.all(r[:, i, i].real >= 0)
        for j in range(5):
            if j <= i:
                assert np.allclose(r[:, i, j], full[:, i, j], rtol=0, atol=1e-12 * float(np.max(np.abs(full))))
            else:
                assert not r[:, i, j].any()


def test_weights_are_conjugate_symmetric():
    """w(-f) = conj(w(f)): L + 1 bins carry everything (to the rounding of the spectra, whose own symmetry NumPy keeps to an ulp)"""
    for length, m, s, g, q in ((100, 5, 2, 1, 3), (101, 2, 3, 2, 1), (128, 64, 3, 1, 4)):
        for loading in MC.LOADINGS:
            w = MC.random_case(length, m, s, g, q, loading)[3]
            ratio = MC.weight_ratio(np.conj(w[..., :length:-1]), w[..., 1:length], m, loading, 1e-15)
            print("w(-f) against conj(w(f)), L=%d M=%d loading=%g: worst difference / tol = %.3g" % (length, m, loading, ratio))
            assert ratio <= 1.0


def test_beams_and_groups_do_not_see_each_other():
    frames, delays, gains, w, want = MC.random_case(300, 5, 8, 2, 4, 0.01)
    for s in (0, 3, 7):                                                          # beam s of the S-source call is the one-source call
        alone = beamform.mvdr(frames, MC.FS, delays[:, s:s + 1], gains[:, s:s + 1], 0.01, 2)
        assert alone[:, 0].tobytes() == np.ascontiguousarray(want[:, s]).tobytes()
    for g in range(2):                                                           # a G-group call is G one-group calls
        part = beamform.mvdr(frames[4 * g:4 * g + 4], MC.FS, delays[g:g + 1], gains[g:g + 1], 0.01, 1)
        assert part.tobytes() == np.ascontiguousarray(want[4 * g:4 * g + 4]).tobytes()
        wpart = beamform.mvdr_weights(frames[4 * g:4 * g + 4], MC.FS, delays[g:g + 1], gains[g:g + 1], 0.01, 1)
        assert wpart.tobytes() == np.ascontiguousarray(w[g:g + 1]).tobytes()


@pytest.mark.parametrize("power", (40, -40))
def test_a_scaled_group_gives_scaled_output_byte_for_byte(power):
    frames, delays, gains, w, want = MC.random_case(300, 5, 3, 2, 3, 0.01)
    scaled = frames.copy()
    scaled[:3] *= 2.0 ** power
    got = beamform.mvdr(scaled, MC.FS, delays, gains, 0.01, 2)
    assert got[:3].tobytes() == (want[:3] * 2.0 ** power).tobytes()
    assert got[3:].tobytes() == np.ascontiguousarray(want[3:]).tobytes()         # the neighbouring group is untouched
    assert beamform.mvdr_weights(scaled, MC.FS, delays, gains, 0.01, 2).tobytes() == w.tobytes()   # the weights ignore the scale


def test_dead_sources_and_zero_frames_are_exact_zeros():
    frames, delays, gains, _, want = MC.random_case(300, 5, 3, 2, 3, 0.01)
    g = gains.copy()
    g[0, 1] = 0.0
    g[1, 0] = 0.0
    got = beamform.mvdr(frames, MC.FS, delays, g, 0.01, 2)
    assert not got[:3, 1].any() and not got[3:, 0].any()
    assert got[:3, 0].tobytes() == np.ascontiguousarray(want[:3, 0]).tobytes() and got[3:, 2].tobytes() == np.ascontiguousarray(want[3:, 2]).tobytes()
    assert not beamform.mvdr_weights(frames, MC.FS, delays, g, 0.01, 2)[0, 1].any()
    silent = frames.copy()
    silent[1] = 0.0                                                              # a zero frame in a live group
    got = beamform.mvdr(silent, MC.FS, delays, gains, 0.01, 2)
    assert not got[1].any() and got[0].any() and got[2].any() and np.all(np.isfinite(got))
    assert got[3:].tobytes() == np.ascontiguousarray(want[3:]).tobytes()
    silent[:3] = 0.0                                                             # a silent group: every bin's diagonal is 1
    got = beamform.mvdr(silent, MC.FS, delays, gains, 0.01, 2)
    assert not got[:3].any() and np.all(np.isfinite(beamform.mvdr_weights(silent, MC.FS, delays, gains, 0.01, 2)))


@pytest.mark.parametrize("loading", MC.LOADINGS)
def test_weight_norm_bound(loading):
    """|w|_2 <= kappa / |a|_2 with kappa = M / loading + 1"""
    for length, m, s, g, q in ((100, 5, 2, 1, 3), (100, 16, 2, 1, 5), (100, 64, 2, 1, 70), (100, 64, 8, 1, 1)):
        _, _, gains, w, _ = MC.random_case(length, m, s, g, q, loading)
        norm = np.sqrt(np.sum(np.abs(w) ** 2, axis=2))                          # [G][S][2L]
        a_norm = np.sqrt(np.sum(gains * gains, axis=2))[..., None]
        worst = float(np.max(norm * a_norm))
        print("|w|_2 |a|_2: worst %.4g, bound %.4g (M=%d Q=%d loading=%g)" % (worst, MC.kappa(m, loading), m, q, loading))
        assert worst <= MC.kappa(m, loading)


def test_large_loading_tends_to_delay_and_sum():
    """loading -> inf: the beam tends to steer(frames, fs, delays, gains / q), q = sum_m gains^2, within 2 M / loading of steer's scale"""
    for length, m, s, g, q, loading in ((100, 5, 2, 1, 3, 1e10), (300, 5, 3, 2, 3, 1e6), (100, 16, 2, 1, 5, 1e4)):
        frames, delays, gains, _, _ = MC.random_case(length, m, s, g, q, 1.0)
        got = beamform.mvdr(frames, MC.FS, delays, gains, loading, g)
        wt = np.repeat(gains / np.sum(gains * gains, axis=2, keepdims=True), q, axis=0)
        want = beamform.steer(frames, MC.FS, np.repeat(delays, q, axis=0), wt)
        ratio = BC.worst_ratio(got, want, BC.tolerance(frames, wt, 2.0 * m / loading + 1e-13))
        dev = BC.worst_ratio(got, want, BC.tolerance(frames, wt, 1.0))
        print("mvdr at loading %g vs steer, M=%d: deviation %.3g of steer's scale, %.3g of the bound" % (loading, m, dev, ratio))
        assert ratio <= 1.0


def test_refusals_of_the_specification():
    frames, delays, gains, _, _ = MC.random_case(100, 2, 3, 2, 1, 0.01)
    for bad in (0.0, -0.01, np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError):
            beamform.mvdr(frames, MC.FS, delays, gains, bad, 2)
        with pytest.raises(ValueError):
            beamform.mvdr_weights(frames, MC.FS, delays, gains, bad, 2)
    for groups in (0, -1, 3):
        with pytest.raises(ValueError):
            beamform.mvdr(np.concatenate([frames, frames]), MC.FS, delays, gains, 0.1, groups)
        with pytest.raises(ValueError):
            beamform.mvdr_covariance(np.concatenate([frames, frames]), groups)
    with pytest.raises(ValueError):
        beamform.mvdr(frames, MC.FS, delays, gains, 0.1, 1)                      # two tables, one group
    with pytest.raises(ValueError):
        beamform.mvdr(frames[0], MC.FS, delays, gains, 0.1, 2)
    with pytest.raises(ValueError):
        beamform.mvdr(frames, MC.FS, delays, gains[:, :2], 0.1, 2)
    with pytest.raises(ValueError):
        beamform.mvdr(np.zeros((2, 2, 99)), MC.FS, delays, gains, 0.1, 2)
    with pytest.raises(ValueError):
        beamform.mvdr(frames, MC.FS, delays[:, :, :1], gains[:, :, :1], 0.1, 2)


# ------------------------------------------------------------------------------------------------ csrc/mvdr_geometry.h on the CPU
def test_geometry_header_on_the_cpu(tmp_path):
    """every pair of the triangle owned once for M = 1 .. 64, the slices at group borders, the refusal bound (tests/host/test_mvdr_geometry.cpp)"""
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    exe = tmp_path / "test_mvdr_geometry"
    subprocess.run(["hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "pyaudiolocalization_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "test_mvdr_geometry.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and "ALL OK" in run.stdout, run.stdout + run.stderr


# ------------------------------------------------------------------------------------------------ the scene
def test_mvdr_gains_3_db_over_delay_and_sum_beside_an_unlisted_interferer():
    """8 microphones, 32 frames of 1024 samples, the target beside an interferer at twice its amplitude that the beamformer is never
    told about, noise variance 0.3; weights 1/M against gains 1, one group, loading 0.1, both at the target's delays.  Computed with
    these seeds: delay-and-sum 2.78 dB, MVDR 9.76 dB mean SNR."""
    mics, frames, bases = MC.scene()
    d = np.broadcast_to(MC.scene_delays(mics)[None], (MC.SCENE_Q, 1, MC.SCENE_M))
    das = beamform.steer(frames, MC.FS, d, np.full(d.shape, 1.0 / MC.SCENE_M))[:, 0]
    adaptive = beamform.mvdr(frames, MC.FS, d[:1], np.ones((1, 1, MC.SCENE_M)), MC.SCENE_LOADING, 1)[:, 0]
    s_das = MC.scene_snr(mics, bases, das, "delay-and-sum")
    s_mvdr = MC.scene_snr(mics, bases, adaptive, "MVDR")
    print("MVDR gains %.2f dB" % (s_mvdr - s_das))
    assert s_mvdr - s_das >= 3.0
