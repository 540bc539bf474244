"""Seeded inputs of the null-steering beamformer's tests (tests/test_host_separate.py, tests/test_gpu_separate.py): random cases with
their specification output computed once, the direct formulation with np.linalg.solve, the small systems of the solve's bit-for-bit
test, and the two scenes of two white sources (1.5 m and 0.3 m apart) with their figures.  NumPy and the oracle only."""
import functools

import numpy as np

from oracle import pal_oracle as O
from pyaudiolocalization_amd import beamform

import beamform_cases as BC

FS = BC.FS
C = BC.C
LOADINGS = (1e-3, 1e-2, 1.0)
HOST_LENGTHS = (100, 101, 300, 1024)
HOST_SHAPES = ((1, 1), (1, 2), (2, 3), (5, 2), (5, 8), (64, 8))                # (M, S)
# fade classes int(0.01 L) = 1, 2, >= 3; H = L + 1 under, on and over a multiple of the 256-bin tile
GPU_LENGTHS = (100, 101, 254, 255, 256, 300, 511, 1024)
# (M, S, B): the tiles of 1, 2, 4 and 8 full (S = 1, 2, 8) and partial (3 in 4; 5 and 7 in 8), S > M, two LDS microphone tiles (70), B S odd
GPU_SHAPES = ((1, 1, 1), (1, 2, 3), (2, 2, 3), (2, 3, 1), (5, 3, 3), (5, 5, 1), (5, 8, 1), (64, 2, 1), (64, 8, 3), (70, 7, 1))


def deltas(gains, loading):
    """delta[b] = loading * max_s sum_m gains[b,s,m]^2"""
    return loading * np.max(np.sum(gains * gains, axis=2), axis=1)


def tolerance(frames, gains, loading, rel):
    """tol[b][s] = rel * |T[b]|_2 / delta[b], T[b,t] = sum_m |g[b,t,m]| max|frames[b,m]| (the same for every s of a frame): the bound
    of the delay-and-sum spectra, amplified by |(G + delta I)^-1| <= 1 / delta"""
    top = np.max(np.abs(frames), axis=2)                                       # [B][M]
    t = np.einsum("bsm,bm->bs", np.abs(gains), top)
    tol = rel * np.sqrt(np.sum(t * t, axis=1)) / deltas(gains, loading)
    return np.broadcast_to(tol[:, None], t.shape)


@functools.lru_cache(maxsize=None)
def random_case(length, m, s, b, loading, seed=0, d_lo=0.0, d_hi=0.004):
    """frames[b][m][length] N(0,1), delays U(d_lo, d_hi), gains U(-1, 1), and beamform.separate of them"""
    rng = np.random.default_rng([92, length, m, s, b, seed])
    frames = rng.standard_normal((b, m, length))
    delays = rng.uniform(d_lo, d_hi, (b, s, m))
    gains = rng.uniform(-1.0, 1.0, (b, s, m))
    want = beamform.separate(frames, FS, delays, gains, loading)
    for a in (frames, delays, gains, want):
        a.setflags(write=False)
    return frames, delays, gains, want


def signed_case(length, m, s, b, loading, seed=0):
    """delays U(-2 ms, 2 ms): both signs, like the gains"""
    return random_case(length, m, s, b, loading, seed, -0.002, 0.002)


def direct(frames, delays, gains, loading):
    """The rule without its operation order: solve(A^H A + delta I, A^H X) per bin with einsum and np.linalg.solve, A[m,s] = g conj(p)"""
    b, s, m = delays.shape
    length = frames.shape[2]
    spec = np.fft.fft(frames, n=2 * length, axis=-1)
    f = np.fft.fftfreq(2 * length, d=1.0 / FS)
    ah = gains[..., None] * np.exp(-1j * 2 * np.pi * f * delays[..., None])    # A^H: [B][S][M][2L]
    y = np.einsum("bsmk,bmk->bks", ah, spec)
    gram = np.einsum("bsmk,btmk->bkst", ah, ah.conj())
    gram = gram + deltas(gains, loading)[:, None, None, None] * np.eye(s)
    z = np.linalg.solve(gram, y[..., None])[..., 0]                            # [B][2L][S]
    return np.fft.ifft(np.moveaxis(z, 1, 2), axis=-1).real[..., :length] * beamform.fade_window(length)


# ------------------------------------------------------------------------------------------------ systems of the solve alone
DEAD_SYSTEM = 4                                                                 # which of solve_systems' K holds the zero row and column


def solve_systems(n, delta=1e-3):
    """-> diag[n][K], g[n][n][K] complex (Hermitian, zero diagonal: the diagonal travels in diag), y[n][K] complex, dead (the zero row
    of system DEAD_SYSTEM).  The K systems: three
    random Hermitian positive definite ones (A A^H of an n x (n + 2) matrix, plus delta), the all-ones matrix plus delta (two sources
    in one place, at every bin), one with a zero row and column (a source without gains: diagonal delta, y = 0 there) and a diagonal one."""
    rng = np.random.default_rng([93, n])
    diag, g, y = [], [], []

    def add(full, rhs):
        diag.append(np.real(np.diag(full)) + delta)
        g.append(full - np.diag(np.diag(full)))
        y.append(rhs)

    def rhs():
        return rng.standard_normal(n) + 1j * rng.standard_normal(n)

    for _ in range(3):
        a = rng.standard_normal((n, n + 2)) + 1j * rng.standard_normal((n, n + 2))
        add(a @ a.conj().T, rhs())
    add(np.ones((n, n), dtype=np.complex128), rhs())
    a = rng.standard_normal((n, n + 2)) + 1j * rng.standard_normal((n, n + 2))
    dead = n // 2
    a[dead] = 0.0
    v = rhs()
    v[dead] = 0.0
    add(a @ a.conj().T, v)
    add(np.diag(rng.uniform(0.5, 2.0, n)).astype(np.complex128), rhs())
    return np.stack(diag, axis=-1), np.stack(g, axis=-1), np.stack(y, axis=-1), dead


# ------------------------------------------------------------------------------------------------ the two scenes
SOURCES_APART = BC.TWO_SOURCES                                                  # 1.5 m apart
SOURCES_CLOSE = np.array([[0.7, 0.6, 0.2], [0.6, 0.35, 0.3]])                   # 0.3 m apart
SCENE_LOADING = 0.01


def scene(sources, delay_rows=None):
    """beamform_cases.two_source_scene with the sources where ``sources`` puts them: the same microphones, bases and noise"""
    mics = np.random.default_rng(17).uniform(-0.4, 0.4, (BC.TWO_M, 3))
    rng = np.random.default_rng(17)
    bases = rng.standard_normal((2, BC.TWO_L))
    frames = np.sqrt(BC.TWO_NOISE) * rng.standard_normal((BC.TWO_M, BC.TWO_L))
    for q in range(2):
        r = np.linalg.norm(sources[q] - mics, axis=1)
        if delay_rows is None:
            frames = frames + np.array([O.fractional_delay(bases[q], r[m] / C, FS) for m in range(BC.TWO_M)])
        else:
            frames = frames + delay_rows(np.tile(bases[q], (BC.TWO_M, 1)), r / C)
    return mics, frames, bases


def scene_figures(mics, bases, sources, steered_at, beams, tag):
    """Per beam q steered at steered_at[q]: (own, correlation with its own base, with the other base, SNR in dB against its own base),
    ``own`` the source it correlates with most, with the references of beamform_cases.two_source_check - base src after its paths and
    the beam's delays, their mean over the microphones.  Printed."""
    d, valid = beamform.point_delays(steered_at, mics, C)
    assert valid.all(), steered_at
    out = []
    for q in range(2):
        cors, snrs = [], []
        for src in range(2):
            paths = np.linalg.norm(sources[src] - mics, axis=1) / C
            ref = O.fractional_delay(bases[src], float(np.mean(paths + d[q])), FS)
            cors.append(abs(float(np.dot(beams[q], ref))) / float(np.sqrt(np.dot(beams[q], beams[q]) * np.dot(ref, ref))))
            snrs.append(BC.snr_db(beams[q], ref))
        own = int(np.argmax(cors))
        print("%s: beam %d -> source %d: correlation own %.3f / other %.3f, SNR %.2f dB" % (tag, q, own, cors[own], cors[1 - own], snrs[own]))
        out.append((own, cors[own], cors[1 - own], snrs[own]))
    return out
