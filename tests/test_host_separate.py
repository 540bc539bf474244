"""The null-steering beamformer's specification (pyaudiolocalization_amd/beamform.py: separate, solve_loaded) on the CPU: against the
direct formulation with np.linalg.solve, its stated consequences (one source is steer, dead beams, silent frames, identical sources),
csrc/separate_math.h compiled for the CPU against solve_loaded bit for bit, and the gain the feature exists for on two scenes.

Tolerance against np.linalg.solve: tol[b][s] = 1e-13 * |T[b]|_2 / delta[b], T[b,t] = sum_m |g[b,t,m]| max|x[b,m]| - the scale of the
delay-and-sum spectra (steer's own 1e-13 bound), amplified by |(G + delta I)^-1| <= 1 / delta; the worst ratio is printed."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from pyaudiolocalization_amd import beamform

import beamform_cases as BC
import separate_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("loading", SC.LOADINGS)
@pytest.mark.parametrize("length", SC.HOST_LENGTHS)
def test_separate_is_the_loaded_least_squares_solution(length, loading):
    worst = 0.0
    for m, s in SC.HOST_SHAPES:
        frames, delays, gains, got = SC.random_case(length, m, s, 1, loading)
        want = SC.direct(frames, delays, gains, loading)
        ratio = BC.worst_ratio(got, want, SC.tolerance(frames, gains, loading, 1e-13))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (length, m, s, loading, ratio)
    print("separate vs np.linalg.solve, L=%d loading=%g: worst error / (1e-13 scale / delta) = %.3g" % (length, loading, worst))


def test_one_source_without_loading_is_steer():
    """S = 1, loading 0: Z = Y / q, which is steer at weights gains / q (held to steer's 1e-13 of sum |w| max|x|)"""
    for length, m in ((100, 1), (300, 5), (1024, 64)):
        frames, delays, gains, _ = SC.random_case(length, m, 1, 2, 0.01)
        w = gains / np.sum(gains * gains, axis=2, keepdims=True)
        got = beamform.separate(frames, SC.FS, delays, gains, 0.0)
        want = beamform.steer(frames, SC.FS, delays, w)
        ratio = BC.worst_ratio(got, want, BC.tolerance(frames, w, 1e-13))
        print("separate S=1 loading 0 vs steer, L=%d M=%d: worst error / (1e-13 scale) = %.3g" % (length, m, ratio))
        assert ratio <= 1.0


def test_dead_beams_and_silent_frames_are_exact_zeros():
    frames, delays, gains, want = SC.random_case(300, 5, 3, 3, 0.01)
    g = gains.copy()
    g[0, 1] = 0.0
    g[2, 0] = 0.0
    got = beamform.separate(frames, SC.FS, delays, g, 0.01)
    assert not got[0, 1].any() and not got[2, 0].any()
    assert np.array_equal(got[1], want[1])                                       # frame 1 does not notice
    # the live rows are what the specification gives without the dead source
    alone = beamform.separate(frames[0:1], SC.FS, delays[0:1, [0, 2]], g[0:1, [0, 2]], 0.01)
    assert np.array_equal(got[0, [0, 2]], alone[0])
    silent = frames.copy()
    silent[1] = 0.0
    got = beamform.separate(silent, SC.FS, delays, gains, 0.01)
    assert not got[1].any() and np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    # no gains at all: delta is 0 too, the output is still zeros and not NaN
    assert not beamform.separate(frames, SC.FS, delays, np.zeros_like(gains), 0.01).any()
    assert not beamform.separate(frames[:, :, :], SC.FS, delays[:, :1], np.zeros_like(gains[:, :1]), 0.0).any()


@pytest.mark.parametrize("loading", SC.LOADINGS)
def test_identical_sources_give_equal_rows(loading):
    frames, delays, gains, _ = SC.random_case(300, 5, 3, 2, loading)
    d, g = delays.copy(), gains.copy()
    d[:, 2], g[:, 2] = d[:, 0], g[:, 0]
    got = beamform.separate(frames, SC.FS, d, g, loading)
    assert np.all(np.isfinite(got)) and got[:, 0].any()
    assert np.allclose(got[:, 0], got[:, 2], rtol=0, atol=float(np.max(SC.tolerance(frames, g, loading, 1e-13))))
    both = np.concatenate([d[:, :1], d[:, :1]], axis=1), np.concatenate([g[:, :1], g[:, :1]], axis=1)
    two = beamform.separate(frames, SC.FS, both[0], both[1], loading)
    # G = q [[1, 1], [1, 1]] at every bin: each row is Y / (q (2 + loading)), the single beam under the loading 1 + loading
    one = beamform.separate(frames, SC.FS, d[:, :1], g[:, :1], 1.0 + loading)
    atol = float(np.max(SC.tolerance(frames, both[1], loading, 1e-13)))
    assert np.allclose(two[:, 0], two[:, 1], rtol=0, atol=atol) and np.allclose(two[:, 0], one[:, 0], rtol=0, atol=atol)


def test_condition_number_bound():
    """cond(G + delta I) <= (S + loading) / loading where q is equal across sources (unit gains: q = M)"""
    rng = np.random.default_rng(31)
    m, s, loading = 6, 4, 0.01
    f = np.fft.fftfreq(512, d=1.0 / SC.FS)
    d = rng.uniform(0, 0.004, (s, m))
    d[3] = d[0]                                                                  # the worst case: two sources in one place
    a = np.exp(-1j * 2 * np.pi * f[:, None, None] * d)                           # [bins][S][M]
    gram = np.einsum("ksm,ktm->kst", a, a.conj()) + loading * m * np.eye(s)
    worst = float(np.max(np.linalg.cond(gram)))
    print("cond(G + delta I): worst %.1f, bound %.1f" % (worst, (s + loading) / loading))
    assert worst <= (s + loading) / loading * (1 + 1e-12)


def test_refusals_of_the_specification():
    frames, delays, gains, _ = SC.random_case(100, 2, 3, 1, 0.01)
    for bad in (-0.01, np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError):
            beamform.separate(frames, SC.FS, delays, gains, bad)
    with pytest.raises(ValueError):
        beamform.separate(frames, SC.FS, delays, gains, 0.0)                     # loading 0 with S = 3
    beamform.separate(frames, SC.FS, delays[:, :1], gains[:, :1], 0.0)
    with pytest.raises(ValueError):
        beamform.separate(frames[0], SC.FS, delays, gains)
    with pytest.raises(ValueError):
        beamform.separate(frames, SC.FS, delays, gains[:, :2])
    with pytest.raises(ValueError):
        beamform.separate(np.zeros((1, 2, 99)), SC.FS, delays, gains)


# ------------------------------------------------------------------------------------------------ csrc/separate_math.h on the CPU
@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    out = tmp_path_factory.mktemp("separate_math") / "test_separate_math"
    subprocess.run(["hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "pyaudiolocalization_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "test_separate_math.cpp"), "-o", str(out)], check=True)
    return str(out)


def solve_spec(g, y):
    """The specification's factor-and-solve loops as a function of (G, Y): G[n][n][...] Hermitian with its loaded diagonal, Y[n][...]"""
    return beamform.solve_loaded(np.real(np.einsum("ii...->i...", g)), g, y)


@pytest.mark.parametrize("n", range(1, 9))
def test_separate_math_equals_the_specification_bit_for_bit(exe, tmp_path, n):
    diag, g, y, dead = SC.solve_systems(n)
    count = y.shape[-1]
    full = g.copy()
    for i in range(n):
        full[i, i] = diag[i]
    want = solve_spec(full, y)                                                   # [n][K]
    assert np.all(np.isfinite(want.view(np.float64)))
    residual = np.einsum("ijk,jk->ik", full, want) - y
    assert float(np.max(np.abs(residual))) <= 1e-9 * float(np.max(np.abs(y)))   # the loops do solve the systems
    assert want[dead, SC.DEAD_SYSTEM] == 0.0
    lower = [(i, j) for i in range(n) for j in range(i)]
    parts = [[float(n), float(count)]]
    for c in range(count):
        parts += [diag[:, c], [g[i, j, c].real for i, j in lower], [g[i, j, c].imag for i, j in lower], y[:, c].real, y[:, c].imag]
    np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1) for v in parts]).tofile(tmp_path / "in.bin")
    run = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert run.returncode == 0 and "ALL OK" in run.stdout, run.stdout + run.stderr
    tiles = [st for st in (1, 2, 4, 8) if st >= n]
    got = np.fromfile(tmp_path / "out.bin").reshape(len(tiles), count, 2, n)
    for t, st in enumerate(tiles):
        assert np.ascontiguousarray(got[t, :, 0].T).tobytes() == np.ascontiguousarray(want.real).tobytes(), (n, st)
        assert np.ascontiguousarray(got[t, :, 1].T).tobytes() == np.ascontiguousarray(want.imag).tobytes(), (n, st)


# ------------------------------------------------------------------------------------------------ the two scenes
def _scene_beams(sources):
    mics, frames, bases = SC.scene(sources)
    d, valid = beamform.point_delays(sources, mics, SC.C)
    assert valid.all()
    das = beamform.steer(frames[None], SC.FS, d[None], beamform.uniform_weights(valid, BC.TWO_M)[None])[0]
    nul = beamform.separate(frames[None], SC.FS, d[None], np.ones((1, 2, BC.TWO_M)), SC.SCENE_LOADING)[0]
    return mics, bases, das, nul


def test_scene_is_the_two_source_scene():
    for a, b in zip(SC.scene(SC.SOURCES_APART), BC.two_source_scene()):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", ("apart", "close"))
def test_null_steering_gains_3_db_over_delay_and_sum_at_the_true_positions(name):
    """Two white sources, 8 microphones, noise variance 0.3, beams at the true positions, loading 0.01.  Computed with these seeds
    (own / other correlation, SNR; beam 0 and beam 1): 1.5 m apart, delay-and-sum 0.928 / 0.026, 7.96 dB and 0.928 / 0.020, 7.93 dB,
    null steering 0.978 / 0.027, 13.34 dB and 0.978 / 0.037, 13.47 dB; 0.3 m apart, delay-and-sum 0.888 / 0.258, 5.72 dB and
    0.882 / 0.259, 5.43 dB, null steering 0.960 / 0.028, 10.68 dB and 0.958 / 0.026, 10.44 dB."""
    sources = SC.SOURCES_APART if name == "apart" else SC.SOURCES_CLOSE
    mics, bases, das, nul = _scene_beams(sources)
    fd = SC.scene_figures(mics, bases, sources, sources, das, "%s, delay-and-sum" % name)
    fn = SC.scene_figures(mics, bases, sources, sources, nul, "%s, null steering" % name)
    for q in range(2):
        assert fd[q][0] == q and fn[q][0] == q
        print("%s: beam %d gains %.2f dB" % (name, q, fn[q][3] - fd[q][3]))
        assert fn[q][3] - fd[q][3] >= 3.0
        if name == "close":
            assert fn[q][2] < fd[q][2] / 3.0
