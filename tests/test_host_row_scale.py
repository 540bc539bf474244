"""Preconditions of tests/test_gpu_row_scale.py, checked without a GPU, so that a failure there can only be the engine's.

* The reference property: the oracle transforms every row on its own and a power of two is exact, so a pair without the
  scaled microphone is bit-identical with and without the scaling, ``O.xcorr_full`` / ``O.fractional_delay`` of a row
  scaled by 2^e are 2^e x the unscaled result bit for bit, and ``O.simulate_from_base`` (normalised) does not change.
* Peak margins: every oracle peak the GPU test compares exactly leads its runner-up by more than 1e-9 (PHAT: absolute,
  the rows are of unit scale; xcorr: relative to the row's own peak).  These are conditions on the seeded inputs of
  tests/row_scale.py, not tolerances: a seed that fails one is replaced.  No case is skipped or filtered.
* The quiet pair: at 2^-40 per microphone the margin cannot hold (printed below); ``row_scale.QUIET_EXP`` holds, per
  shape, the largest negative exponent of -40, -38, ... at which it does (-32 at L = 496, -38 at L = 44 100).
"""
import numpy as np
import pytest

from oracle import pal_oracle as O

import row_scale as RS


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", sorted(RS.PHAT_SHAPES))
def test_oracle_pairs_without_the_scaled_microphone_do_not_change(name):
    _, m, _, _ = RS.PHAT_SHAPES[name]
    for tag, nframes, mic in RS.phat_positions(name):
        for e in RS.EXPS:
            fr = RS.scaled_frames(name, nframes, mic, e)
            plain = RS.phat_frames(name)
            assert _same_bits(fr[0, mic], plain[0, mic] * 2.0 ** e)
            for p, (i, j) in enumerate(RS.pairs_of(m)):
                got = O.phat_correlation(fr[0, i], fr[0, j])
                if mic in (i, j):
                    assert _same_bits(got, RS.oracle_corr(name, 0, i, j, e if i == mic else 0, e if j == mic else 0))
                else:
                    assert _same_bits(got, RS.oracle_corr(name, 0, i, j)), (name, tag, e, i, j)


@pytest.mark.parametrize("name", sorted(RS.PHAT_SHAPES))
def test_phat_peak_margins(name):
    b, m, _, _ = RS.PHAT_SHAPES[name]
    worst = np.inf
    for f in range(b):                                               # the unscaled frames
        for i, j in RS.pairs_of(m):
            for med in RS.MEDS:
                for method in RS.METHODS:
                    mg = RS.peak_margin(name, f, i, j, 0, 0, med, method)
                    assert mg > RS.MARGIN, (name, f, i, j, med, method, mg)
                    worst = min(worst, mg)
    for mic in sorted({mic for _, _, mic in RS.phat_positions(name)}):
        for e in RS.EXPS:
            for i, j in RS.pairs_of(m):
                if mic not in (i, j):
                    continue
                for med in RS.MEDS:
                    for method in RS.METHODS:
                        mg = RS.peak_margin(name, 0, i, j, e if i == mic else 0, e if j == mic else 0, med, method)
                        assert mg > RS.MARGIN, (name, mic, e, i, j, med, method, mg)
                        worst = min(worst, mg)
    print("%s: smallest peak margin %.3g" % (name, worst))


def test_quiet_pair_margin_and_exponent():
    for name in RS.QUIET_SHAPES:
        for e in (-40, RS.QUIET_EXP[name] - 2, RS.QUIET_EXP[name]):
            print("%s: quiet pair at 2^%d, margin %.3g" % (name, e, RS.quiet_margin(name, e)))
        assert RS.quiet_margin(name, RS.QUIET_EXP[name]) > RS.MARGIN
        assert RS.quiet_margin(name, -40) <= RS.MARGIN               # why 2^-40 is not used
        assert RS.quiet_exponent_search(name) == RS.QUIET_EXP[name]


@pytest.mark.parametrize("r", RS.XCORR_R)
def test_xcorr_is_covariant_and_peaks_lead(r):
    rows = RS.xcorr_rows(r)
    for ref in RS.xcorr_refs(r):
        plain = RS.xcorr_exact(rows, ref)
        for q, seq in enumerate(plain):
            assert RS.xcorr_margin(seq) > RS.MARGIN, (r, ref, q, RS.xcorr_margin(seq))
        for at in RS.xcorr_positions(r, ref):
            for e in RS.EXPS:
                x = np.array(rows)
                x[at] *= 2.0 ** e
                for q, seq in enumerate(RS.xcorr_exact(x, ref)):
                    k = (e if q == at else 0) + (e if ref == at else 0)
                    assert _same_bits(seq, plain[q] * 2.0 ** k), (r, ref, at, e, q)
    frames = RS.sync_frames()
    assert [RS.numpy_ref(fr) for fr in frames] == list(RS.SYNC_LOUD)
    for f, fr in enumerate(frames):
        for q, seq in enumerate(RS.xcorr_exact(fr, RS.SYNC_LOUD[f])):
            assert RS.xcorr_margin(seq) > RS.MARGIN, (f, q)
    for f, q in RS.SYNC_SCALED:                                      # with the scaled row as the reference
        for seq in RS.xcorr_exact(frames[f], q):
            assert RS.xcorr_margin(seq) > RS.MARGIN, (f, q)


def test_fractional_delay_is_covariant():
    rows = RS.fd_rows()
    for q in range(RS.FD_R):
        plain = O.fractional_delay(rows[q], RS.FD_DELAYS[q], RS.FD_FS)
        for e in RS.EXPS:
            assert _same_bits(O.fractional_delay(rows[q] * 2.0 ** e, RS.FD_DELAYS[q], RS.FD_FS), plain * 2.0 ** e), (q, e)


def test_simulate_from_base_ignores_the_scale_of_the_base():
    base, delays, gains = RS.sim_tables()
    for f in range(RS.SIM_B):
        for e in RS.SIM_EXPS:
            got = O.simulate_from_base(base[f] * 2.0 ** e, delays[f], gains[f], RS.SIM_FS, RS.SIM_TOTAL, None)
            assert _same_bits(got, RS.sim_want(f)), (f, e)
        assert np.all(np.max(np.abs(RS.sim_want(f)), axis=1) == 1.0)
