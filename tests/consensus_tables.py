"""Inputs of the consensus tests (pal_tdoa_consensus*, pyaudiolocalization_amd/consensus.py): candidate tables around the geometry of
``robust_tables`` (microphones in a one-metre cube, the source at SRC, integer lags at 48 kHz, frames of LENGTH samples).

``random_candidates(m, seed, q, k, absent)``: draws, in this order, from ``default_rng(seed)``: the microphones; ``cand`` = uniform lags in
+-2400 samples for every (pair, slot); the slot of the true lag (with probability ``q`` a random slot 1 .. k-1, else slot 0); the pairs that
lose their true lag (probability ``absent``; their slot is redrawn from +-2400).
``two_sources(m, seed, p_true, k)``: every pair holds the lag of SRC and of the image source IMAGE in its first two slots, the true one
first with probability ``p_true``; noise lags follow.
``ragged(cand_k, seed)``: the same table with a random number of trailing candidates of every pair made absent.
``spec(...)``: the specification's (sel, summary), computed once per argument set and shared between the tests."""
import functools
import os

import numpy as np

import robust_tables as T
from pyaudiolocalization_amd import consensus as CN
from pyaudiolocalization_amd import solve as S

IMAGE = np.array([1.0, -6.0, 0.5])
CASES = [(4, 5, .3, 2, 0), (5, 1, .4, 3, 0), (8, 2, .5, 4, 0), (16, 3, .7, 8, 0), (16, 3, .5, 4, .1), (33, 7, .5, 4, .1)]   # (m, seed, q, K, absent)
TWO_SOURCE_CASES = [(8, 2, .7), (16, 3, .6), (33, 7, .6)]                                                                  # (m, seed, pT)


def true_lags(mics, src=T.SRC):
    pi, pj = S.pair_indices(mics.shape[0])
    d = np.linalg.norm(np.asarray(src) - mics, axis=1)
    return np.rint((d[pj] - d[pi]) / T.C_SOUND * T.FS).astype(np.int64)


@functools.lru_cache(maxsize=None)
def random_candidates(m, seed, q, k, absent=0.0):
    """-> dict: mics[m][3], cand_k[P][k] (int64 array indices), true_lag[P], slot[P] (of the true lag; -1 where the pair lost it)."""
    rng = np.random.default_rng(seed)
    mics = rng.uniform(-0.5, 0.5, (m, 3))
    p = m * (m - 1) // 2
    cand = rng.integers(-2400, 2401, (p, k))
    slot = np.where(rng.random(p) < q, rng.integers(1, k, p), 0) if k > 1 else np.zeros(p, dtype=np.int64)
    lost = rng.random(p) < absent
    true_lag = true_lags(mics)
    cand[np.arange(p), slot] = true_lag
    cand[lost, slot[lost]] = rng.integers(-2400, 2401, int(np.count_nonzero(lost)))
    return {"mics": mics, "cand_k": cand + T.LENGTH - 1, "true_lag": true_lag, "slot": np.where(lost, -1, slot)}


@functools.lru_cache(maxsize=None)
def two_sources(m, seed, p_true, k=4):
    """-> dict: mics, cand_k[P][k], true_lag[P], image_lag[P], first[P] (the true lag is candidate 0)."""
    rng = np.random.default_rng(seed)
    mics = rng.uniform(-0.5, 0.5, (m, 3))
    p = m * (m - 1) // 2
    cand = rng.integers(-2400, 2401, (p, k))
    first = rng.random(p) < p_true
    true_lag, image_lag = true_lags(mics), true_lags(mics, IMAGE)
    cand[:, 0] = np.where(first, true_lag, image_lag)
    cand[:, 1] = np.where(first, image_lag, true_lag)
    return {"mics": mics, "cand_k": cand + T.LENGTH - 1, "true_lag": true_lag, "image_lag": image_lag, "first": first}


def ragged(cand_k, seed):
    """cand_k[..][P][K] with a random number (0 .. K-1) of trailing candidates of every pair made absent."""
    ck = np.array(cand_k, dtype=np.int64, copy=True)
    k = ck.shape[-1]
    keep = np.random.default_rng([seed, k]).integers(1, k + 1, ck.shape[:-1])
    ck[np.arange(k) >= keep[..., None]] = CN.ABSENT
    return ck


# One 256-microphone frame with 8 candidate slots (the device's chunked-LDS path).  Stage 0 of the specification takes a quarter of a minute
# on it in NumPy, so its result is kept in tests/golden/consensus_m256.npz (``PYTHONPATH=. python tests/consensus_tables.py`` rewrites the file, with ``--check`` it compares every row instead;
# tests/test_host_consensus.py recomputes some of its rows); the rounds and the summary are computed by the specification from there.
BIG = dict(m=256, seed=9, q=.5, k=8, absent=.1, ragged_seed=1, tol=1)
BIG_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "consensus_m256.npz")


def big_frame():
    """cand_k[P][8] of the 256-microphone frame: BIG's random candidates with trailing candidates removed."""
    t = random_candidates(BIG["m"], BIG["seed"], BIG["q"], BIG["k"], BIG["absent"])
    return ragged(t["cand_k"], BIG["ragged_seed"])


@functools.lru_cache(maxsize=None)
def big_spec(rounds):
    """(sel[1][P], summary[1]) of the specification on big_frame(), stage 0 read from the golden file."""
    with np.load(BIG_GOLDEN) as z:
        sel0 = z["sel0"].astype(np.int32)
    sel, summ = CN.consensus_frame(big_frame(), T.LENGTH, BIG["m"], BIG["tol"], rounds, sel0=sel0)
    return sel[None], np.array([summ], dtype=CN.SUMMARY)


_SPEC, _STAGE0 = {}, {}


def spec(cand_k, lengths, m, tol=1, rounds=2):
    """consensus.tdoa_consensus, remembered per argument set (the array by its bytes; stage 0, which does not depend on ``rounds``, on
    its own); the caller leaves the result unchanged."""
    ck = np.ascontiguousarray(cand_k, dtype=np.int64)
    if ck.ndim == 2:
        ck = ck[None]
    ln = np.ascontiguousarray(np.broadcast_to(np.asarray(lengths, dtype=np.int64), (ck.shape[0],)))
    key = (ck.tobytes(), ck.shape, ln.tobytes(), m, tol)
    if key + (rounds,) not in _SPEC:
        CN.check_args(ck.shape[0], m, ck.shape[2], ln, tol, rounds)
        if key not in _STAGE0:
            _STAGE0[key] = [CN.stage0(CN.check_candidates(ck[b], ln[b]), int(ln[b]), m, tol) for b in range(ck.shape[0])]
        frames = [CN.consensus_frame(ck[b], int(ln[b]), m, tol, rounds, sel0=_STAGE0[key][b]) for b in range(ck.shape[0])]
        _SPEC[key + (rounds,)] = (np.stack([f[0] for f in frames]), np.array([f[1] for f in frames], dtype=CN.SUMMARY))
    return _SPEC[key + (rounds,)]


if __name__ == "__main__":
    import sys
    fresh = CN.stage0(big_frame(), T.LENGTH, BIG["m"], BIG["tol"]).astype(np.int8)
    if "--check" in sys.argv:                     # every row of the golden file against the specification (half a minute)
        with np.load(BIG_GOLDEN) as z:
            same = np.array_equal(z["sel0"], fresh)
        print("the golden file equals the specification" if same else "the golden file DIFFERS from the specification")
        sys.exit(0 if same else 1)
    np.savez_compressed(BIG_GOLDEN, sel0=fresh)
    print("wrote", BIG_GOLDEN)
