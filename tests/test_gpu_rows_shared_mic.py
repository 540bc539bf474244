"""Rader row pass (csrc/pfa_rader.h), first stage: a packed transform whose two pairs share their first microphone
(quad.x == quad.z, the usual case in the row-major i < j list) reads that microphone's spectrum row once; every other
transform keeps the four-row body.  The kernel exists for N2 = 991 only, so the frame length is 44100 (88199 = 89 x 991)
and the cases stay small through the microphone count.  One oracle table of ten pairs serves every case: the smaller
frames are subsets of the five microphones."""
import numpy as np
import pytest

from oracle import pal_oracle as O

pytestmark = pytest.mark.gpu

L, FS, MED = 44100, 44100.0, 0.05
INT_FIELDS = ("k_sel", "branch", "k_argmax")
METRICS = ("cmax", "cmin", "snr")
# index of pair (i, j) in the row-major i < j list of five microphones
IDX5 = {(i, j): k for k, (i, j) in enumerate((i, j) for i in range(5) for j in range(i + 1, 5))}


def _frames(seed):
    rng = np.random.default_rng(seed)
    common = rng.standard_normal(L + 64)
    return np.stack([common[d:d + L] for d in (0, 17, 5, 40, 23)]) + 0.5 * rng.standard_normal((5, L))


@pytest.fixture(scope="module")
def five():
    """frames[5][L] and the oracle's ten records (read-only for the tests)."""
    frames = _frames(991)
    frames.setflags(write=False)
    return frames, O.all_pairs(frames, FS, max_expected_delay=MED)


@pytest.fixture(scope="module")
def five_silent(five):
    """The same frames with microphone 0 - the shared one of the first two transforms - silent."""
    frames = five[0].copy()
    frames[0] = 0.0
    frames.setflags(write=False)
    return frames, O.all_pairs(frames, FS, max_expected_delay=MED)


def _check(got, want, pick, tag):
    """The project's bar: selected indices equal, metrics to 1e-9."""
    pick = np.asarray(pick)
    for f in INT_FIELDS:
        assert np.array_equal(got[f], want[f][pick]), (tag, f, got[f], want[f][pick])
    for f in METRICS:
        assert np.allclose(got[f], want[f][pick], rtol=1e-9, atol=0), (tag, f, got[f], want[f][pick])


def _subset(mics):
    return [IDX5[(mics[a], mics[b])] for a in range(len(mics)) for b in range(a + 1, len(mics))]


def test_five_mics_run_both_first_stage_bodies(engine, five):
    """Ten pairs pack as (01,02) (03,04) (12,13) - shared first microphone - then (14,23) (24,34): both bodies in one launch."""
    frames, want = five
    assert engine.plan_info(L)["tile_len"] == 990
    engine.profile_begin()
    got = engine.gcc_phat_all_pairs(frames, FS, max_expected_delay=MED)
    engine.profile_end()
    assert engine.profile_entries()["k_pfa_rows_rader<11,9,10>"][1] >= 1
    _check(got, want, np.arange(10), "M=5")


def test_half_empty_transform_and_second_frame(engine, five):
    """M = 3: one shared transform (01,02) and one without a second pair (12,-).  B = 2, M = 4: six pairs per frame, so
    frame 1's transforms point at rows offset by M, the shared ones included."""
    frames, want = five
    got = engine.gcc_phat_all_pairs(frames[:3], FS, max_expected_delay=MED)
    _check(got, want, _subset((0, 1, 2)), "M=3")
    two = np.stack([frames[:4], frames[1:]])
    got = engine.gcc_phat_all_pairs(two, FS, max_expected_delay=MED)
    _check(got[0], want, _subset((0, 1, 2, 3)), "B=2 frame 0")
    _check(got[1], want, _subset((1, 2, 3, 4)), "B=2 frame 1")


@pytest.mark.parametrize("pairs", [((0, 2), (1, 2)), ((0, 1), (1, 2)), ((1, 2), (0, 1)), ((0, 1), (0, 1))],
                         ids=["y==w", "y==z", "x==w", "x==z,y==w"])
def test_explicit_pair_lists(engine, five, pairs):
    """Lists whose packed partners coincide in the positions the kernel does NOT test (second rows equal, first row of one
    = second row of the other, either way round) keep the four-row body; the same pair twice has quad.x == quad.z like
    an all-pairs transform and must be right too."""
    frames, want = five
    got = engine.gcc_phat_pairs(frames[:3], np.array(pairs, dtype=np.int32), FS, max_expected_delay=MED)
    _check(got, want, [IDX5[p] for p in pairs], pairs)


def test_silent_shared_microphone_gives_exact_zero_rows(engine, five_silent):
    """Microphone 0 silent: R = 0 / (0 + 1e-10) = 0 in every bin of its four pairs, which sit in the two shared
    transforms (01,02) (03,04).  Their rows are exact zeros, the other six pairs are untouched."""
    frames, want = five_silent
    got, corr = engine.gcc_phat_all_pairs(frames, FS, max_expected_delay=MED, want_corr=True)
    _check(got, want, np.arange(10), "silent, rows stored")
    assert np.array_equal(corr[:4], np.zeros((4, 2 * L - 1)))
    assert np.all(np.max(np.abs(corr[4:]), axis=1) > 0.01)
    _check(engine.gcc_phat_all_pairs(frames, FS, max_expected_delay=MED), want, np.arange(10), "silent")


def test_shared_and_four_row_bodies_are_bit_identical(engine, five, five_silent, monkeypatch):
    """PAL_ROWS_SHARED=0 never takes the shared body.  The loaded values are the same doubles and the arithmetic behind
    them is unchanged, so every field of every record - and every stored sample - is bit-identical."""
    from pyaudiolocalization_amd import Engine
    monkeypatch.setenv("PAL_ROWS_SHARED", "0")
    plain = Engine(engine.device)
    monkeypatch.delenv("PAL_ROWS_SHARED")
    try:
        for frames in (five[0], five_silent[0]):
            for med in (MED, None):
                a = engine.gcc_phat_all_pairs(frames, FS, max_expected_delay=med)
                b = plain.gcc_phat_all_pairs(frames, FS, max_expected_delay=med)
                assert a.tobytes() == b.tobytes(), med
            a, ca = engine.gcc_phat_all_pairs(frames, FS, max_expected_delay=MED, want_corr=True)
            b, cb = plain.gcc_phat_all_pairs(frames, FS, max_expected_delay=MED, want_corr=True)
            assert a.tobytes() == b.tobytes() and ca.tobytes() == cb.tobytes()
    finally:
        plain.close()
