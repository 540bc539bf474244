"""Strip form of the finishing column pass (csrc/pfa_cols_fin.h, csrc/pfa_fin_lean.h fin_rows_wave): wavefronts 0 and 1 of a
transform's last block finish one row each.  The cases here are the ones where the two finishers do not have the same work: a call
with an odd number of rows (the last transform carries one row, its second finisher has none), a single pair, and waits that give
up (each finisher hands on its own row, the report counts every pair once).

Inputs and helpers are those of test_gpu_fin_strip.py and peak_positions.py, the same three lengths (Rader-89 columns in four
wavefronts, dense columns in two, strips in four).  Compared with the polling form (PAL_FIN_STRIP=0, one finishing wavefront: every
field byte-identical but `snr`, which the strip sums in another order - rtol 1e-11 as in test_gpu_fin_strip.py), with the stored-row
path (PAL_FIN=0) and with the NumPy oracle."""
import numpy as np
import pytest

import peak_positions as P
import test_gpu_fin_strip as S

pytestmark = pytest.mark.gpu

LENGTHS = S.LENGTHS
MICS = (2, 3, 6)                                                  # 1, 3 and 15 rows: a lone row, a lone row behind a full transform, eight transforms


def _frames(L, mics, seed):
    """one frame, an impulse of sqrt(L) per microphone (peak_positions.py): the rows' maxima at the lags between them"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((1, mics, L))
    x[0, np.arange(mics), rng.choice(40, mics, replace=False) + 100] += np.sqrt(L)
    return x


@pytest.mark.parametrize("L,n1,n2", LENGTHS, ids=[f"L{c[0]}" for c in LENGTHS])
def test_odd_row_counts(engine, L, n1, n2, monkeypatch, capfd):
    fs, med = P.rates(L)
    info = engine.plan_info(L)
    assert (info["n1"], info["n2"]) == (n1, n2), info
    polling = S._engine(engine.device, monkeypatch, {"PAL_FIN_STRIP": "0"})
    try:
        for mics in MICS:
            frames = _frames(L, mics, 31 * L + mics)
            spec = P.spectra(frames[0])
            pairs = [(i, j) for i in range(mics) for j in range(i + 1, mics)]
            for method, mult in S.MODES:
                tag = (L, mics, method)
                got, _ = S._call(engine, frames, fs, method, mult, med, capfd)
                assert got.shape == (1, len(pairs)), tag
                ref, _ = S._call(polling, frames, fs, method, mult, med, capfd)
                S._same_as_polling(got, ref, tag)
                again, _ = S._call(engine, frames, fs, method, mult, med, capfd)
                assert again.tobytes() == got.tobytes(), tag
                for p, (i, j) in enumerate(pairs):
                    corr = P.corr_from_spectra(spec[i], spec[j])
                    want = P.record(corr, L, fs, method, mult, med)
                    if P.decided(corr, L, fs, method, mult, med, want):      # (a row that rounding decides is the oracle's matter)
                        S._compare(got[0][p], want, tag + (i, j))
    finally:
        polling.close()


@pytest.mark.parametrize("L,n1,n2", LENGTHS, ids=[f"L{c[0]}" for c in LENGTHS])
def test_given_up_waits_hand_on_every_row_once(engine, L, n1, n2, monkeypatch, capfd):
    """PAL_DEBUG_FIN_GIVEUP=1 in the strip form: every pair is flagged exactly once, by its own finisher, and resolved from stored
    rows - records byte-identical to PAL_FIN=0"""
    fs, med = P.rates(L)
    monkeypatch.setenv("PAL_DEBUG_FALLBACK", "1")                  # (read at every report, not at creation)
    gave = S._engine(engine.device, monkeypatch, {"PAL_DEBUG_FIN_GIVEUP": "1"})
    stored = S._engine(engine.device, monkeypatch, {"PAL_FIN": "0"})
    try:
        for mics in MICS:
            frames = _frames(L, mics, 31 * L + mics)
            npairs = mics * (mics - 1) // 2
            got, rep = S._call(gave, frames, fs, "median", 1.0, med, capfd)
            assert rep["flagged"] == npairs and rep["waits given up"] == npairs, (L, mics, rep)
            ref = stored.gcc_phat_all_pairs(frames, fs, 1, "median", 1.0, med)
            assert got.tobytes() == ref.tobytes(), (L, mics)
    finally:
        gave.close()
        stored.close()
