"""A row's peak ON the layout borders of every statistics pass behind Engine.gcc_phat_all_pairs, against the NumPy oracle.
Inputs: tests/peak_positions.py (impulse "star" frames: the maximum of pair (0, j) sits exactly at a designed array index; two-
arrival rows at the lag window's edges).  Designed indices: the row's ends, the lag-window centre, the window's edges and its
`distance - 1` margins, the grid's edge columns, the 62-column block and 248-column strip borders in the first, middle and last
output index, and for the passes over stored rows the 64-sample chunk and wavefront-span borders.

One parametrised test per route of csrc/pair_route.h; every case asserts the plan, that the kernel under test really ran
(profile entries), and the records of every designed pair and of a seeded sample of the other pairs: integer fields exact, float
fields to the tolerances test_gpu_fin_exchange.py and test_all_pairs_small_batches hold against the oracle.  Rows whose oracle
record is not decided (peak_positions.decided) are left out, at most 2 % of a case's designed rows.  For the finishing forms the
stderr report (PAL_DEBUG_FALLBACK=1) bounds the rows that were handed to the stored-row path: a handed-on row tests the repair,
not the pass."""
import re
from collections import namedtuple

import numpy as np
import pytest

import peak_positions as P

pytestmark = pytest.mark.gpu

Route = namedtuple("Route", "L n1 n2 kind env want_corr stored r2 others")


def _route(L, n1, n2, kind, env=None, want_corr=False, stored=False, r2=None, others=None):
    # (the oracle is the cost of a case: fewer of the other pairs on long rows, every designed index everywhere)
    return Route(L, n1, n2, kind, env or {}, want_corr, stored, r2, (P.OTHERS if L < 16000 else 12) if others is None else others)


# Plans as pal_plan_factors reports them on the device (asserted in every case).
FIN = [_route(11437, 89, 257, "fin"),                               # Rader-89 columns
       _route(8193, 5, 3277, "fin"),                                # strips
       _route(8538, 25, 683, "fin"),                                # two chunks of output indices
       _route(16051, 47, 683, "fin"),                               # three chunks
       _route(23564, 69, 683, "fin"),                               # four chunks
       _route(44100, 89, 991, "fin", r2=(0, 1, 989, 990, 62))]      # the headline length: row-level indices and five column residues
STORE = [_route(8193, 5, 3277, "store", want_corr=True), _route(8538, 25, 683, "store", want_corr=True)]
FUSED = [_route(1008, 5, 403, "fused"), _route(11962, 47, 509, "fused")]
LEAN_ENV = {"PAL_ROWS_LEAN_MIN": "1", "PAL_ROWS_LEAN": "1"}
ROWS_LEAN = [_route(12000, 103, 233, "rows_lean", LEAN_ENV, stored=True), _route(6007, 0, 0, "rows_lean", LEAN_ENV, stored=True),
             _route(2500, 0, 0, "rows_lean", LEAN_ENV, stored=True)]
THREE = [_route(12000, 103, 233, "three", {"PAL_ROWS_LEAN": "0"}, stored=True), _route(1000, 0, 0, "three", stored=True)]

_REPORT = re.compile(r"\[pal\] (\d+) row\(s\) of the finishing column pass went through the stored-row path \(no maximum / abandoned (\d+), "
                     r"tie (\d+), tie in window (\d+), SNR window energy (\d+), histogram windows (\d+), threshold interval (\d+), "
                     r"window interval (\d+), window edge (\d+); waits given up (\d+)\)")
_REASONS = ("flagged", "no maximum / abandoned", "tie", "tie in window", "SNR window energy", "histogram windows", "threshold interval",
            "window interval", "window edge", "waits given up")
FLAGGED_SHARE = 0.10             # of a call's rows, the window-edge rule apart: room for given-up waits only


def _ids(routes):
    return [f"L{r.L}" for r in routes]


def _engine(device, monkeypatch, env):
    """An engine created under `env` (read at creation); the variables are removed again behind it."""
    from pyaudiolocalization_amd import Engine
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return Engine(device)
    finally:
        for k in env:
            monkeypatch.delenv(k)


def _no_hist(method, mult):
    return method == "adaptive" or 0 <= mult <= 2.0


def _kernel_ran(kind, method, mult, entries):
    """the kernel class under test, from the profile entries of one call"""
    ran = lambda name: any(k.startswith(name) and v[1] > 0 for k, v in entries.items())
    if kind == "fin":
        return ran("k_pfa_cols_fin")                                # both bodies: per-wavefront statistics, histograms (multiplier 4.2)
    if kind == "store":                                             # (a threshold that needs histograms keeps the fused pass)
        return ran("k_pfa_cols_lean") if _no_hist(method, mult) else ran("k_pfa_cols_stats") and not ran("k_pfa_cols_lean")
    if kind == "fused":
        return ran("k_pfa_cols_stats") and ran("k_peak_finish") and not ran("k_peak_stream")
    if kind == "rows_lean" and _no_hist(method, mult):
        return ran("k_rows_lean")
    return ran("k_peak_pivots") and ran("k_peak_stream") and ran("k_peak_finish") and not ran("k_rows_lean")


def _flag_report(err):
    found = _REPORT.findall(err)
    assert len(found) <= 1, err
    if not found:                                                   # (a report in other words must not read as "none handed on")
        assert "finishing column pass" not in err and "stored-row path" not in err, err
    return dict(zip(_REASONS, (int(x) for x in found[0]))) if found else dict.fromkeys(_REASONS, 0)


def _check_flags(rep, rows, windowed, tag, method, mult):
    """The share of a call's rows that the finishing forms handed to the stored-row path.  The two bodies of k_pfa_cols_fin share
    their profile name; what tells them apart from outside is one-sided: only the histogram body can miss the median with its
    histogram windows, so a call that must take the per-wavefront body reports none.  That multiplier 4.2 takes the histogram
    body rests on the engine's own choice (csrc/pfa.hip, pfa_pair_group_fin); nothing it leaves behind is certain to show it."""
    if _no_hist(method, mult):
        assert rep["histogram windows"] == 0, (tag, rep)
    counted = rep["flagged"] - (rep["window edge"] if windowed else 0)
    assert counted <= FLAGGED_SHARE * rows, f"{tag}: {rows} rows, " + ", ".join(f"{k} {v}" for k, v in rep.items() if v)


def _compare(rec, want, tag):
    for f in P.INT_FIELDS:
        assert int(rec[f]) == want[f], (tag, f, int(rec[f]), want[f])
    assert int(rec["n_sel"]) == 1, tag
    assert np.isclose(rec["cmax"], want["cmax"], rtol=1e-11, atol=0), (tag, "cmax", float(rec["cmax"]), want["cmax"])
    for f in ("cmin", "sel_height"):
        assert np.isclose(rec[f], want[f], rtol=1e-10, atol=1e-14), (tag, f, float(rec[f]), want[f])
    assert np.isclose(rec["snr"], want["snr"], rtol=1e-9, atol=0), (tag, "snr", float(rec["snr"]), want["snr"])


def _call(eng, frames, fs, method, mult, med, want_corr, capfd):
    eng.synchronize()                                               # (reports and clears what earlier calls of the session's engine left
    capfd.readouterr()                                              #  in the status words: they are only cleared when they are reported)
    eng.profile_begin()
    got = eng.gcc_phat_all_pairs(frames, fs, 1, method, mult, med, want_corr=want_corr)
    eng.profile_end()
    return got, _flag_report(capfd.readouterr().err), eng.profile_entries()


def _run(engine, route, monkeypatch, capfd):
    L, fs, med = route.L, *P.rates(route.L)
    info = engine.plan_info(L)
    assert (info["n1"], info["n2"]) == (route.n1, route.n2), info
    c = P.case(L, route.n1, route.n2, fs, med, route.stored, route.r2, route.others)
    ta = P.two_arrival_frames(L, fs, med, L)
    monkeypatch.setenv("PAL_DEBUG_FALLBACK", "1")                   # (read at every report, not at creation)
    eng = _engine(engine.device, monkeypatch, route.env) if route.env else engine
    finishing = route.kind in ("fin", "store")
    undecided = compared = others = two = 0
    flagged = []
    nframes = c.star.frames.shape[0]
    try:
        for method, mult, m in P.param_sets(med):
            tag = (route.kind, L, method, mult, m)
            got, rep, entries = _call(eng, c.star.frames, fs, method, mult, m, route.want_corr, capfd)
            table, rows = (got if route.want_corr else (got, None))
            assert _kernel_ran(route.kind, method, mult, entries), (tag, sorted(entries))
            if finishing:
                _check_flags(rep, table.size, m is not None, tag, method, mult)
                flagged.append((method, mult, m, table.size, {k: v for k, v in rep.items() if v}))
            for f, i, j, k in c.rows:
                want = c.want(f, i, j, method, mult, m)
                if not want["decided"]:
                    undecided += k is not None
                    continue
                compared += k is not None
                others += k is None
                p = c.pair_index[(i, j)]
                _compare(table[f][p], want, tag + (f, i, j, k))
                if rows is not None and k is not None and m is None and (method, mult) == P.MODES[0]:
                    # (the rows do not depend on the selection's parameters: once per case)
                    assert np.max(np.abs(rows[f][p] - c.corr(f, i, j))) <= 1e-13, tag + (f, i, j, k)
        assert undecided <= P.UNDECIDED_SHARE * 6 * len(c.designed_rows), (route.kind, L, undecided)
        # ---- two arrivals at the window's edges (windowed calls): per four-microphone frame the three designed pairs (0, j)
        #      and one of the other three pairs (seeded); the call's handed-on rows are bounded like any other windowed call's
        pairs = [(i, j) for i in range(4) for j in range(i + 1, 4)]
        pick = np.random.default_rng(L + 1).integers(3, 6, ta.frames.shape[0])
        wants = {}
        for f, frame in enumerate(ta.frames):
            spec = P.spectra(frame)
            for p in (0, 1, 2, int(pick[f])):
                i, j = pairs[p]
                corr = P.corr_from_spectra(spec[i], spec[j])
                for method, mult in P.MODES:
                    want = P.record(corr, L, fs, method, mult, med)
                    want["decided"] = P.decided(corr, L, fs, method, mult, med, want)
                    assert want["decided"] or i > 0, (L, f, i, j, method, mult)   # (the designed rows are decided: test_host_peak_positions.py)
                    wants[(f, p, method, mult)] = want
        for method, mult in P.MODES:
            tag = (route.kind, L, "two arrivals", method, mult)
            got, rep, entries = _call(eng, ta.frames, fs, method, mult, med, route.want_corr, capfd)
            table = got[0] if route.want_corr else got
            assert _kernel_ran(route.kind, method, mult, entries), (tag, sorted(entries))
            if finishing:
                _check_flags(rep, table.size, True, tag, method, mult)
                flagged.append((method, mult, "two arrivals", table.size, {k: v for k, v in rep.items() if v}))
            for (f, p, me, mu), want in wants.items():
                if (me, mu) == (method, mult) and want["decided"]:
                    _compare(table[f][p], want, tag + (f,) + pairs[p])
                    two += 1
    finally:
        if eng is not engine:
            eng.close()
        c.release()
    with capfd.disabled():
        print(f"\n[peak positions] {route.kind} L={L} plan=({route.n1}, {route.n2}) frames={nframes}x{c.mics} mics: "
              f"{len(c.indices)} designed indices, {compared} designed records compared, {undecided} left out as undecided, "
              f"{others} records of other pairs, {two} two-arrival records; flagged per call {flagged}")


@pytest.mark.parametrize("route", FIN, ids=_ids(FIN))
def test_finishing_pass(engine, route, monkeypatch, capfd):
    """k_pfa_cols_fin (rows never stored), lean body (multiplier 1, 'adaptive') and histogram body (4.2): Rader-89 columns,
    strips, two / three / four chunks of output indices, partial last column blocks, and the headline length."""
    _run(engine, route, monkeypatch, capfd)


@pytest.mark.parametrize("route", STORE, ids=_ids(STORE))
def test_finishing_pass_storing_rows(engine, route, monkeypatch, capfd):
    """k_pfa_cols_lean (the caller wants the rows): records as above, and every designed row against O.phat_correlation."""
    _run(engine, route, monkeypatch, capfd)


@pytest.mark.parametrize("route", FUSED, ids=_ids(FUSED))
def test_fused_pass(engine, route, monkeypatch, capfd):
    """k_pfa_cols_stats + k_peak_finish on grids with fewer than twelve column blocks."""
    _run(engine, route, monkeypatch, capfd)


@pytest.mark.parametrize("route", ROWS_LEAN, ids=_ids(ROWS_LEAN))
def test_rows_lean(engine, route, monkeypatch, capfd):
    """k_rows_lean over stored rows of the prime-factor and the four-step route (PAL_ROWS_LEAN_MIN=1 lets a small call through)."""
    _run(engine, route, monkeypatch, capfd)


@pytest.mark.parametrize("route", THREE, ids=_ids(THREE))
def test_three_launches(engine, route, monkeypatch, capfd):
    """k_peak_pivots + k_peak_stream + k_peak_finish: PAL_ROWS_LEAN=0 on the 103 x 233 plan, the default on a prime n = 1999."""
    _run(engine, route, monkeypatch, capfd)
