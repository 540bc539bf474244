"""Seeded inputs of the MVDR beamformer's tests (tests/test_host_mvdr.py, tests/test_gpu_mvdr.py): random cases with their
specification weights and output computed once, the direct formulation with einsum and np.linalg.solve, the tolerance, and the scene
of one target and one unlisted interferer.  NumPy and the oracle only.

Tolerance: tol[b][s] = rel * (100 + kappa) * sum_m wmax[g,s,m] * max_t |frames[b,m,t]|, wmax the specification's max_k |w|, kappa =
M / loading + 1 the bound of cond(R~); rel is 1e-15 on the host and 1e-13 on the device.  At small kappa that is steer's 1e-13 / 1e-11
bound with the weights the data chose; the kappa term is the solve's sensitivity to the rounding of the spectra.  It is not scaled by
kappa / |a| alone: outputs fall to 1e-10 of that (an interferer cancelled), and a test would see nothing."""
import functools

import numpy as np

from oracle import pal_oracle as O
from pyaudiolocalization_amd import beamform

import beamform_cases as BC

FS = BC.FS
C = BC.C
LOADINGS = (1e-3, 1e-2, 1.0)
GPU_LOADINGS = (1e-3, 0.1, 1.0)
# (L, M, S, G, Q)
HOST_CASES = ((100, 1, 1, 1, 1), (101, 2, 3, 2, 1), (100, 5, 2, 1, 3), (300, 5, 8, 2, 4), (100, 16, 2, 1, 5), (128, 64, 3, 1, 4),
              (100, 64, 2, 1, 70), (100, 64, 8, 1, 1))
# fade classes int(0.01 L) = 1, 2, >= 3; H = L + 1 under, on and over the 256-bin tile
GPU_LENGTHS = (100, 101, 254, 255, 256, 300, 1024)
# (M, S, G, Q): M on and beside the edges of the 8 x 4 covariance tiles, S across the source tiles of 1, 2 and 4, Q S odd (the last
# transform of a slice holds one row), Q = 1, Q above and below M
GPU_SHAPES = ((1, 1, 1, 1), (2, 3, 2, 1), (5, 2, 1, 3), (5, 3, 3, 3), (7, 1, 1, 16), (8, 2, 2, 2), (9, 8, 1, 2), (17, 9, 1, 2), (33, 2, 1, 3),
              (63, 1, 1, 2), (64, 8, 1, 4), (64, 2, 2, 70))


def kappa(m, loading):
    return m / loading + 1.0


def tolerance(frames, weights, loading, rel):
    """tol[b][s] of the module's docstring; weights[G][S][M][bins] are the specification's"""
    b, m, _ = frames.shape
    groups = weights.shape[0]
    wmax = np.repeat(np.max(np.abs(weights), axis=-1), b // groups, axis=0)    # [B][S][M]
    top = np.max(np.abs(frames), axis=2)                                       # [B][M]
    return rel * (100.0 + kappa(m, loading)) * np.einsum("bsm,bm->bs", wmax, top)


def weight_tolerance(weights, m, loading, rel):
    """the weights in their own scale: tol[g][s][m] = rel * (100 + kappa) * max_k |w[g,s,m,k]|"""
    return rel * (100.0 + kappa(m, loading)) * np.max(np.abs(weights), axis=-1)


def weight_ratio(got, want, m, loading, rel):
    """max over (g, s, m) of max_k |got - want| / tol (0 / 0 = 0)"""
    err = np.max(np.abs(got - want), axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / weight_tolerance(want, m, loading, rel))
    return float(np.max(ratio))


@functools.lru_cache(maxsize=None)
def random_case(length, m, s, g, q, loading, seed=0, d_lo=0.0, d_hi=0.004):
    """frames[g q][m][length] N(0,1), delays U(d_lo, d_hi), gains U(-1, 1) -> frames, delays, gains, beamform.mvdr_weights, beamform.mvdr"""
    rng = np.random.default_rng([94, length, m, s, g, q, seed])
    frames = rng.standard_normal((g * q, m, length))
    delays = rng.uniform(d_lo, d_hi, (g, s, m))
    gains = rng.uniform(-1.0, 1.0, (g, s, m))
    weights = beamform.mvdr_weights(frames, FS, delays, gains, loading, g)
    want = beamform.mvdr(frames, FS, delays, gains, loading, g)
    for a in (frames, delays, gains, weights, want):
        a.setflags(write=False)
    return frames, delays, gains, weights, want


def signed_case(length, m, s, g, q, loading, seed=0):
    """delays U(-2 ms, 2 ms): both signs, like the gains"""
    return random_case(length, m, s, g, q, loading, seed, -0.002, 0.002)


def direct(frames, delays, gains, loading, groups):
    """The rule without its operation order: R by einsum, w = solve(R + delta I, a) / (a^H solve(R + delta I, a)) with np.linalg.solve
    per bin -> (w[G][S][M][2L], out[B][S][L])"""
    b, m, length = frames.shape
    q = b // groups
    spec = np.fft.fft(frames, n=2 * length, axis=-1).reshape(groups, q, m, 2 * length)
    r = np.einsum("gqik,gqjk->gkij", spec, spec.conj())
    tr = np.real(np.einsum("gkii->gk", r))
    r = r + (loading * tr / m)[:, :, None, None] * np.eye(m)
    f = np.fft.fftfreq(2 * length, d=1.0 / FS)
    a = np.moveaxis(gains[..., None] * np.exp(1j * 2 * np.pi * f * delays[..., None]), 3, 1)   # [G][2L][S][M]
    ria = np.linalg.solve(r[:, :, None], a[..., None])[..., 0]
    den = np.real(np.einsum("gksm,gksm->gks", a.conj(), ria))
    w = np.moveaxis(ria / den[..., None], 1, 3)                                 # [G][S][M][2L]
    y = np.einsum("gsmk,gqmk->gqsk", w.conj(), spec).reshape(b, -1, 2 * length)
    return w, np.fft.ifft(y, axis=-1).real[..., :length] * beamform.fade_window(length)


# ------------------------------------------------------------------------------------------------ the scene
SCENE_M, SCENE_Q, SCENE_L = 8, 32, 1024
SCENE_LOADING = 0.1
SCENE_SOURCES = BC.TWO_SOURCES                                                  # source 0 is the target, source 1 the interferer nobody lists


def scene(delay_rows=None):
    """8 microphones, 32 frames of 1024 samples: a target and an interferer at twice its amplitude, both where they are in every
    frame, fresh white signals and noise (variance 0.3) per frame.  ``delay_rows(rows, delays)``: what delays the rows (default:
    the oracle).  -> mics, frames[Q][M][L], bases[Q][2][L]"""
    mics = np.random.default_rng(17).uniform(-0.4, 0.4, (SCENE_M, 3))
    rng = np.random.default_rng(18)
    bases = rng.standard_normal((SCENE_Q, 2, SCENE_L))
    bases[:, 1] *= 2
    frames = np.sqrt(0.3) * rng.standard_normal((SCENE_Q, SCENE_M, SCENE_L))
    for src in range(2):
        r = np.linalg.norm(SCENE_SOURCES[src] - mics, axis=1)
        if delay_rows is None:
            frames = frames + np.array([[O.fractional_delay(bases[b, src], r[m] / C, FS) for m in range(SCENE_M)] for b in range(SCENE_Q)])
        else:
            rows = delay_rows(np.repeat(bases[:, src], SCENE_M, axis=0), np.tile(r / C, SCENE_Q))
            frames = frames + rows.reshape(SCENE_Q, SCENE_M, SCENE_L)
    return mics, frames, bases


def scene_delays(mics):
    d, valid = beamform.point_delays(SCENE_SOURCES[0:1], mics, C)
    assert valid.all()
    return d                                                                    # [1][M]


def scene_snr(mics, bases, beams, tag):
    """mean over the frames of the SNR of beams[Q][L] against the target's base after its paths and the beam's delays (their mean
    over the microphones).  Printed."""
    d = scene_delays(mics)[0]
    paths = np.linalg.norm(SCENE_SOURCES[0] - mics, axis=1) / C
    snrs = [BC.snr_db(beams[b], O.fractional_delay(bases[b, 0], float(np.mean(paths + d)), FS)) for b in range(SCENE_Q)]
    mean = float(np.mean(snrs))
    print("%s: mean SNR over %d frames %.2f dB" % (tag, SCENE_Q, mean))
    return mean
