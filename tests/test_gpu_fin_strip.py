"""The strip form of the finishing column pass (csrc/pfa_fin_lean.h, csrc/pair_route.h fin_strip): windowed calls store the samples
of three pieces of the row to a strip - the centre piece [win_lo - snr_w, win_hi + snr_w - 1] and the row's two ends, where lags of
up to max_expected_delay sit in a circular correlation - no wavefront polls its siblings, and the finishing wavefront sums the SNR
window from the strip or, where the row's argmax lies outside all three, evaluates it from the grid.

Inputs: the star frames of tests/peak_positions.py (an impulse of sqrt(L) per microphone: the maximum of pair (0, j) sits at a
designed array index).  Three lengths, one per column source: Rader-89 columns (89 x 257, five column blocks), dense columns in two
chunks (25 x 683), strips (5 x 3277).  Designed indices: the lag centre and the window's two ends (the SNR window reaches the centre
piece's first and last sample), one sample outside either end (the first rows of the direct path), the row's ends (clipped windows,
from the end pieces) and the end pieces' last index inside and first outside, a column-block border and the grid's last column
inside the lag window (where the length has such an index) and away from every piece, and one frame with a silent microphone.

Against the NumPy oracle with the tolerances of test_gpu_peak_positions.py, and against an engine created with PAL_FIN_STRIP=0:
integer fields, cmax, cmin and the selected height byte-identical (their code is untouched), snr to rtol 1e-11 (only the summation
order of the window changed)."""
import re
from collections import namedtuple

import numpy as np
import pytest

import peak_positions as P

pytestmark = pytest.mark.gpu

LENGTHS = [(11437, 89, 257), (8538, 25, 683), (8193, 5, 3277)]
MODES = (("median", 1.0), ("adaptive", 1.0))                      # the per-wavefront body: through the bound on the median, 'adaptive'
SAME_FIELDS = ("k_sel", "branch", "k_argmax", "n_sel", "cmax", "cmin", "sel_height")
FLAGGED_SHARE = 0.10                                              # of a call's rows, the window-edge rule apart
_REPORT = re.compile(r"\[pal\] (\d+) row\(s\) of the finishing column pass went through the stored-row path \(no maximum / abandoned (\d+), "
                     r"tie (\d+), tie in window (\d+), SNR window energy (\d+), histogram windows (\d+), threshold interval (\d+), "
                     r"window interval (\d+), window edge (\d+); waits given up (\d+)\)")
_REASONS = ("flagged", "no maximum / abandoned", "tie", "tie in window", "SNR window energy", "histogram windows", "threshold interval",
            "window interval", "window edge", "waits given up")


def _engine(device, monkeypatch, env):
    """An engine created under `env` (read at creation); the variables are what they were again behind it."""
    from pyaudiolocalization_amd import Engine
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        return Engine(device)


Geo = namedtuple("Geo", "n c D win_lo win_hi snr_w pieces")


def _geometry(L, fs, med):
    """the lag window, the SNR half width and the strip's three pieces (csrc/pair_route.h fin_strip) of a frame length"""
    n, c = 2 * L - 1, L - 1
    D = P.window_half_width(fs, med)
    win_lo, win_hi = max(1, c - D), min(n - 2, c + D)
    w = max(1, int(0.01 * n))
    pieces = ((0, D + w - 1), (win_lo - w, win_hi + w - 1), (n - D - w, n - 1))
    assert 0 < pieces[0][1] + 1 < pieces[1][0] and pieces[1][1] + 1 < pieces[2][0] < n     # (three pieces, apart)
    return Geo(n, c, D, win_lo, win_hi, w, pieces)


def _border_columns(n1, n2):
    """first columns of the column strips behind the first: the grid's columns are dealt evenly to ceil(N2 / 62) blocks, four strips
    per block where the column transforms are short (one chunk, N1 <= 23)"""
    strips = -(-n2 // 248) * 4 if n1 <= 23 else -(-n2 // 62)
    return {k * n2 // strips for k in range(1, strips)}


def _designed(L, n1, n2, fs, med):
    """{name: index}: a row's maximum at each of them"""
    g = _geometry(L, fs, med)
    n, win_lo, win_hi, snr_w = g.n, g.win_lo, g.win_hi, g.snr_w
    out = {"centre": g.c, "win_lo": win_lo, "win_hi": win_hi, "win_lo - 1": win_lo - 1, "win_hi + 1": win_hi + 1,
           "0": 0, "snr_w - 1": snr_w - 1, "snr_w": snr_w, "n - 1 - snr_w": n - 1 - snr_w, "n - 1": n - 1,
           # the end pieces: the last argmax whose window they hold (lags +D and -D) and the first one on the direct path
           "D": g.D, "D + 1": g.D + 1, "n - D": n - g.D, "n - D - 1": n - g.D - 1}
    apart = lambda m: all(m < lo - 2 * snr_w or m > hi + 2 * snr_w for lo, hi in g.pieces)
    for name, cols in (("block border", _border_columns(n1, n2)), ("last column", {n2 - 1})):
        inside = [m for m in range(win_lo, win_hi + 1) if m % n2 in cols]
        outside = [m for m in range(n) if m % n2 in cols and apart(m)]
        if inside:
            out[name + " inside"] = inside[len(inside) // 2]
        out[name + " outside"] = outside[len(outside) // 3]
    return out


def _flag_report(err):
    found = _REPORT.findall(err)
    assert len(found) <= 1, err
    if not found:
        assert "finishing column pass" not in err and "stored-row path" not in err, err
    return dict(zip(_REASONS, (int(x) for x in found[0]))) if found else dict.fromkeys(_REASONS, 0)


def _call(eng, frames, fs, method, mult, med, capfd):
    eng.synchronize()
    capfd.readouterr()
    eng.profile_begin()
    got = eng.gcc_phat_all_pairs(frames, fs, 1, method, mult, med)
    eng.profile_end()
    rep = _flag_report(capfd.readouterr().err)
    assert any(k.startswith("k_pfa_cols_fin") and v[1] > 0 for k, v in eng.profile_entries().items()), sorted(eng.profile_entries())
    return got, rep


def _same_as_polling(got, ref, tag):
    for f in SAME_FIELDS:
        assert got[f].tobytes() == ref[f].tobytes(), (tag, f)
    assert np.allclose(got["snr"], ref["snr"], rtol=1e-11, atol=0, equal_nan=True), (tag, "snr", float(np.nanmax(np.abs(got["snr"] / ref["snr"] - 1))))


def _compare(rec, want, tag):
    for f in P.INT_FIELDS:
        assert int(rec[f]) == want[f], (tag, f, int(rec[f]), want[f])
    assert int(rec["n_sel"]) == 1, tag
    assert np.isclose(rec["cmax"], want["cmax"], rtol=1e-11, atol=0), (tag, "cmax", float(rec["cmax"]), want["cmax"])
    for f in ("cmin", "sel_height"):
        assert np.isclose(rec[f], want[f], rtol=1e-10, atol=1e-14), (tag, f, float(rec[f]), want[f])
    assert np.isclose(rec["snr"], want["snr"], rtol=1e-9, atol=0, equal_nan=True), (tag, "snr", float(rec["snr"]), want["snr"])


@pytest.fixture(scope="module")
def cases():
    """per length: the designed indices, their star frames and the oracle's records of the designed rows - built once, never changed"""
    out = {}
    for L, n1, n2 in LENGTHS:
        fs, med = P.rates(L)
        designed = _designed(L, n1, n2, fs, med)
        star = P.star_frames(L, sorted(set(designed.values())), 4000 + L)
        wants = {}
        for f, frame in enumerate(star.frames):
            spec = P.spectra(frame)
            for j, k in sorted(star.designed[f].items()):
                corr = P.corr_from_spectra(spec[0], spec[j])
                assert int(np.argmax(corr)) == k, (L, f, j, k)
                for method, mult in MODES:
                    want = P.record(corr, L, fs, method, mult, med)
                    assert P.decided(corr, L, fs, method, mult, med, want), (L, f, j, k, method)   # (test_host_peak_positions.py)
                    wants[(f, j, method)] = want
        out[L] = (designed, star, wants)
    return out


@pytest.mark.parametrize("L,n1,n2", LENGTHS, ids=[f"L{c[0]}" for c in LENGTHS])
def test_strip_form_against_oracle_and_polling_form(engine, cases, L, n1, n2, monkeypatch, capfd):
    """every designed index: records against the oracle; the whole table against PAL_FIN_STRIP=0; handed-on rows within 10 %;
    the same call twice and once through a one-stream engine byte-identical"""
    fs, med = P.rates(L)
    info = engine.plan_info(L)
    assert (info["n1"], info["n2"]) == (n1, n2), info
    g = _geometry(L, fs, med)
    assert sum(hi - lo + 1 for lo, hi in g.pieces) <= 0.12 * g.n   # (the strip's share of the row: these calls take the strip form)
    designed, star, wants = cases[L]
    assert "block border inside" in designed and (n1 != 89 or "last column inside" in designed), designed
    mics = star.frames.shape[1]
    pair_index = {p: q for q, p in enumerate((i, j) for i in range(mics) for j in range(i + 1, mics))}
    monkeypatch.setenv("PAL_DEBUG_FALLBACK", "1")                  # (read at every report, not at creation)
    polling = _engine(engine.device, monkeypatch, {"PAL_FIN_STRIP": "0"})
    one = _engine(engine.device, monkeypatch, {"PAL_OVERLAP": "0"})
    try:
        for method, mult in MODES:
            tag = (L, method, mult)
            got, rep = _call(engine, star.frames, fs, method, mult, med, capfd)
            counted = rep["flagged"] - rep["window edge"]
            assert counted <= FLAGGED_SHARE * got.size, (tag, got.size, {k: v for k, v in rep.items() if v})
            for (f, j, me), want in wants.items():
                if me == method:
                    _compare(got[f][pair_index[(0, j)]], want, tag + (f, j, star.designed[f][j]))
            ref, _ = _call(polling, star.frames, fs, method, mult, med, capfd)
            _same_as_polling(got, ref, tag)
            again, _ = _call(engine, star.frames, fs, method, mult, med, capfd)
            assert again.tobytes() == got.tobytes(), tag
            single, _ = _call(one, star.frames, fs, method, mult, med, capfd)
            assert single.tobytes() == got.tobytes(), tag
    finally:
        polling.close()
        one.close()


@pytest.mark.parametrize("L,n1,n2", LENGTHS, ids=[f"L{c[0]}" for c in LENGTHS])
def test_silent_microphone(engine, cases, L, n1, n2, monkeypatch, capfd):
    """a frame with a silent microphone: its rows are exact zeros in the strip and on the direct path; the table against
    PAL_FIN_STRIP=0 and the silent pairs' partners against the oracle"""
    fs, med = P.rates(L)
    _, star, _ = cases[L]
    frames = star.frames[:1].copy()
    frames[0, 1] = 0.0
    polling = _engine(engine.device, monkeypatch, {"PAL_FIN_STRIP": "0"})
    try:
        for method, mult in MODES:
            got, _ = _call(engine, frames, fs, method, mult, med, capfd)
            ref, _ = _call(polling, frames, fs, method, mult, med, capfd)
            _same_as_polling(got, ref, (L, "silent", method))
            spec = P.spectra(frames[0])
            for p, (i, j) in ((1, (0, 2)), (2, (0, 3))):           # pair (0, 1) is silent; (0, 2) shares its transform
                want = P.record(P.corr_from_spectra(spec[i], spec[j]), L, fs, method, mult, med)
                _compare(got[0][p], want, (L, "silent", method, i, j))
    finally:
        polling.close()


@pytest.mark.parametrize("L,n1,n2", LENGTHS, ids=[f"L{c[0]}" for c in LENGTHS])
def test_calls_without_a_strip_keep_the_polling_form(engine, cases, L, n1, n2, monkeypatch, capfd):
    """a call without a lag window, and one whose window is 60 % of the row (above any share cap): byte-identical to PAL_FIN_STRIP=0"""
    fs, _ = P.rates(L)
    _, star, _ = cases[L]
    polling = _engine(engine.device, monkeypatch, {"PAL_FIN_STRIP": "0"})
    try:
        for med in (None, 0.6 * L / fs):
            got, _ = _call(engine, star.frames, fs, "median", 1.0, med, capfd)
            ref, _ = _call(polling, star.frames, fs, "median", 1.0, med, capfd)
            assert got.tobytes() == ref.tobytes(), (L, med)
    finally:
        polling.close()
