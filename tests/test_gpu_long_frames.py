"""Frames above 98 304 samples on the device: every rung of the LDS-tile chirp convolution (conv_kernels.h k_cols_* / k_cols3_* with
1024- and 2048-point rows, k_rows<10 | 11>) at its first and its last frame length, the five long prime-factor cuts, and
``xcorr_vs_ref`` up to the ABI's 2^20 samples.  The inputs and their references come from tests/long_frames.py;
tests/test_host_long_frames.py holds the conditions on them and tests/host/test_plan_geometry.cpp pins the same geometry.

Every case asserts the plan it exists for (``plan_info``) and the kernel instances it launched (``profile_entries``), so a later
change to the plan chooser fails here instead of moving the case off its rung.

Bounds: impulse rows against their exact values and stored rows against ``O.phat_correlation`` 1e-13 absolute (rows with a
unit peak: the bound the suite holds the register geometries to; the oracle itself is within 4e-16 of the exact rows);
cmax / cmin / snr rtol 1e-11, atol 1e-15 as in tests/test_gpu_fullsize.py; integer fields equal.  Every test prints the
figures it asserts.
"""
import numpy as np
import pytest

from oracle import pal_oracle as O
from pyaudiolocalization_amd import _ffi
from pyaudiolocalization_amd._ffi import PalError

import long_frames as LF
import peak_positions as PP
import second_path as S

pytestmark = pytest.mark.gpu
INT_FIELDS = PP.INT_FIELDS


@pytest.fixture(scope="module")
def engines():
    """(default switches, PAL_PFA=0): the switches are read when an engine is created.  Launch groups of four transforms keep the
    workspaces of a 2^22-point convolution small; results do not depend on the group size."""
    from pyaudiolocalization_amd import Engine
    default = Engine(0)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("PAL_PFA", "0")
        plain = Engine(0)
    default.set_chunk(4)
    plain.set_chunk(4)
    yield default, plain
    default.close()
    plain.close()


def _profiled(eng, call):
    eng.profile_begin()
    try:
        out = call()
    finally:
        eng.profile_end()
    return out, {name: v for name, v in eng.profile_entries().items() if v[1] >= 1}   # (names of earlier brackets stay, with no launches)


def _transform_instances(length, pfa):
    """prefixes of the kernel instances a first call at this length launches: the setup of both convolutions, the forward
    transform, and the PHAT inverse as the convolution or as the cut's row and column pass"""
    inv, fwd = LF.geometry(length)
    cut = LF.CUTS.get(length) if pfa else None
    want = LF.setup_instances(fwd) + LF.setup_instances(inv)
    want += LF.conv_instances(fwd, "FrameLoader", "PermSpectrumStorer" if cut else "SpectrumStorer")
    if cut:
        want += ["k_pfa_rows_big<%d>" % cut[2], "k_pfa_cols"]
    else:
        want += LF.conv_instances(inv, "PairLoader", "CorrStorer")
    return want


def _assert_instances(entries, length, pfa, tag):
    missing = LF.missing_instances(entries, _transform_instances(length, pfa))
    assert not missing, (tag, missing, sorted(entries))
    cut = LF.CUTS.get(length) if pfa else None
    if cut:                                                         # nothing of the inverse convolution but its setup
        inv, _ = LF.geometry(length)
        assert not any(name.startswith(p) for name in entries for p in LF.conv_instances(inv, "PairLoader", "CorrStorer")[::2]), (tag, sorted(entries))
        if cut[3] > 4:                                              # more than four chunks: the plain column pass, never the fused ones
            assert entries["k_pfa_cols"][1] >= 1 and not any(name.startswith("k_pfa_cols_") for name in entries), (tag, sorted(entries))
        else:
            assert any(name.startswith("k_pfa_cols_") for name in entries) and "k_pfa_cols" not in entries, (tag, sorted(entries))
    else:
        assert not any(name.startswith("k_pfa_") for name in entries), (tag, sorted(entries))


def _engines_of(engines, length):
    default, plain = engines
    return [("default", default, True)] + ([("PAL_PFA=0", plain, False)] if length in LF.CUTS else [])


def _check_impulse_row(row, rec, n, index, value, tag):
    err = np.abs(row)
    err[index] = abs(row[index] - value)
    worst = float(np.max(err))
    print(tag, "index", index, "value %.17g" % value, "max |row - exact| %.3g" % worst)
    assert worst <= LF.ROW_BOUND, (tag, worst, int(np.argmax(err)))
    if rec is None:
        return worst
    if value > 0:
        assert int(rec["k_argmax"]) == index, (tag, int(rec["k_argmax"]))
        assert abs(float(rec["cmax"]) - value) <= LF.ROW_BOUND and abs(float(rec["cmin"])) <= LF.ROW_BOUND, (tag, rec)
        # (scipy's find_peaks never returns a row's end points: with the maximum on index 0 or n - 1 the selected index is one of
        #  the row's rounding residues, in the oracle as here, so k_sel is asserted on interior indices)
        if 0 < index < n - 1:
            assert int(rec["k_sel"]) == index and int(rec["branch"]) == 0, (tag, int(rec["k_sel"]), int(rec["branch"]))
    else:
        assert abs(float(rec["cmin"]) - value) <= LF.ROW_BOUND and abs(float(rec["cmax"])) <= LF.ROW_BOUND, (tag, rec)
    return worst


@pytest.mark.parametrize("length", LF.IMPULSE_LENGTHS)
def test_impulse_rows_are_exact_on_every_rung(engines, length):
    """Three microphones with one impulse each: the row of pair (i, j) is a_i a_j / (|a_i a_j| + 1e-10) at (p_i - p_j) mod n and 0
    elsewhere.  Peaks on 0, n - 1, L - 2, L - 1, beside a row wrap of the inverse convolution (M2 - 1, M2) and beside a 4096-point
    tile border (4095, 4096); mixed signs; 2^-20 against 2^+20.  Both engines at the cut lengths."""
    n = 2 * length - 1
    frames = LF.impulse_frames(length)
    for name, eng, pfa in _engines_of(engines, length):
        try:
            assert eng.plan_info(length) == LF.plan_pin(length, pfa), (name, eng.plan_info(length))
            eng.clear_plans()                                       # the plan's setup kernels run inside the profiled call
            for q, f in enumerate(frames):
                (table, corr), entries = _profiled(eng, lambda: eng.gcc_phat_all_pairs(f.frame, LF.FS, want_corr=True))
                if q == 0:
                    _assert_instances(entries, length, pfa, (length, name))
                assert corr.shape == (3, n)
                for p, (i, j, index, value) in enumerate(f.peaks):
                    _check_impulse_row(corr[p], table[p], n, index, value, (length, name, f.name, i, j))
                if f.name == "wrap":                                # the pair with its peak on n - 1 alone in a transform
                    i, j, index, value = f.peaks[0]
                    single = eng.phat_correlation(f.frame[i], f.frame[j])
                    _check_impulse_row(single, None, n, index, value, (length, name, f.name, "phat_correlation"))
        finally:
            eng.clear_plans()


def _check_noise(table, corr, case, length, med, tag):
    want = case.records[med]
    for key in INT_FIELDS:
        assert [int(v) for v in table[key]] == [w[key] for w in want], (tag, key, table[key])
    for key in ("cmax", "cmin", "snr"):
        ref = np.array([w[key] for w in want])
        print(tag, key, "max relative difference %.3g" % float(np.max(np.abs(table[key] - ref) / np.abs(ref))))
        assert np.allclose(table[key], ref, rtol=1e-11, atol=1e-15), (tag, key, table[key], ref)
    if corr is not None:
        worst = float(np.max(np.abs(corr - case.corr)))
        print(tag, "max |row - oracle| %.3g" % worst)
        assert worst <= LF.ROW_BOUND, (tag, worst)


@pytest.mark.parametrize("length", LF.NOISE_LENGTHS)
def test_noise_rows_match_the_oracle(engines, length):
    """One frame of three microphones whose rows share a component (rolled by 37 and by -1234) at the first length of every
    rung and at 2^20: records and stored rows against the oracle; both engines against each other at the cut length."""
    case = LF.noise_case(length)
    got = {}
    for name, eng, pfa in _engines_of(engines, length):
        try:
            assert eng.plan_info(length) == LF.plan_pin(length, pfa), (name, eng.plan_info(length))
            eng.clear_plans()
            for q, med in enumerate(LF.noise_windows(length)):
                (table, corr), entries = _profiled(eng, lambda: eng.gcc_phat_all_pairs(case.frame, LF.FS, max_expected_delay=med, want_corr=True))
                if q == 0:
                    _assert_instances(entries, length, pfa, (length, name))
                _check_noise(table, corr, case, length, med, (length, name, med))
                rows_free = eng.gcc_phat_all_pairs(case.frame, LF.FS, max_expected_delay=med)   # the call that does not store the rows
                _check_noise(rows_free, None, case, length, med, (length, name, med, "table only"))
                got[(name, med)] = (table, corr)
        finally:
            eng.clear_plans()
    if length in LF.CUTS:
        for med in LF.noise_windows(length):
            (t1, c1), (t0, c0) = got[("default", med)], got[("PAL_PFA=0", med)]
            for key in INT_FIELDS:
                assert np.array_equal(t1[key], t0[key]), (length, med, key)
            assert float(np.max(np.abs(c1 - c0))) <= LF.ROW_BOUND, (length, med)


@pytest.mark.parametrize("length", sorted(LF.CUTS))
@pytest.mark.parametrize("method", LF.CUT_METHODS)
def test_long_cuts_match_the_oracle_and_the_convolution(engines, length, method):
    """The five long cuts (8192- and 16384-point register tiles, N1 up to 127, three to six accumulator chunks) with a row's
    maximum on the first, middle and last column class at the first and last tile point: records and rows against the oracle,
    and the default engine against the PAL_PFA=0 engine."""
    default, plain = engines
    case = LF.cut_case(length)
    n = 2 * length - 1
    try:
        assert default.plan_info(length) == LF.plan_pin(length, True) and plain.plan_info(length) == LF.plan_pin(length, False)
        default.clear_plans()
        for f, frame in enumerate(case.frames):
            mics = frame.shape[0]
            pair_of = {(i, j): q for q, (i, j) in enumerate((i, j) for i in range(mics) for j in range(i + 1, mics))}
            call = dict(max_expected_delay=LF.CUT_MED, threshold_method=method)
            (t1, c1), entries = _profiled(default, lambda: default.gcc_phat_all_pairs(frame, LF.FS, want_corr=True, **call))
            if f == 0:
                _assert_instances(entries, length, True, (length, method))
            t0, c0 = plain.gcc_phat_all_pairs(frame, LF.FS, want_corr=True, **call)
            free = default.gcc_phat_all_pairs(frame, LF.FS, **call)                   # rows not stored: the finishing pass where it applies
            worst = float(np.max(np.abs(c1 - c0)))
            print((length, method, f), "max |cut - convolution| %.3g" % worst)
            assert worst <= LF.ROW_BOUND and c1.shape == (len(pair_of), n)
            for key in INT_FIELDS:
                assert np.array_equal(t1[key], t0[key]) and np.array_equal(free[key], t1[key]), (length, method, f, key)
            for ff, j, k in case.rows:
                if ff != f:
                    continue
                p = pair_of[(0, j)]
                want = case.records[method][(f, j)]
                err = float(np.max(np.abs(c1[p] - case.corr[(f, j)])))
                print((length, method, f, j, k), "max |row - oracle| %.3g" % err)
                assert err <= LF.ROW_BOUND, (length, method, f, j, err)
                assert int(t1[p]["k_argmax"]) == k == want["k_argmax"], (length, method, f, j)
                for got in (t1[p], t0[p], free[p]):
                    for key in INT_FIELDS:
                        assert int(got[key]) == want[key], (length, method, f, j, key, int(got[key]), want[key])
                    for key in ("cmax", "cmin", "snr"):
                        assert np.isclose(float(got[key]), want[key], rtol=1e-11, atol=1e-15), (length, method, f, j, key, float(got[key]), want[key])
    finally:
        default.clear_plans()
        plain.clear_plans()


@pytest.mark.parametrize("n", LF.SPARSE_N)
def test_xcorr_vs_ref_sparse_integer_rows(engines, n):
    """Three rows of 64 non-zero integers, samples 0 and N - 1 among them, the reference row in the middle, at the first N of
    five rungs of the 2N - 1-point convolution: against the exact 64 x 64 sums."""
    default, _ = engines
    case = LF.sparse_case(n)
    g = LF.SPARSE_GEOM[n]
    try:
        measured, entries = _profiled(default, lambda: default.xcorr_vs_ref(case.rows, LF.SPARSE_REF))
        want = [LF.conv_instances(g, "RefLoader")[0], ("k_rowsreg<%d,fwd>" if g.kind == "reg2" else "k_rows<%d,fwd>") % g.l2]
        want += LF.conv_instances(g, "RowPairLoader", "PlainStorer")
        missing = LF.missing_instances(entries, want)
        assert not missing, (n, missing, sorted(entries))
        print(n, "kpk", measured[0], "pkabs", measured[2], "refpk", measured[3])
        S.check_xcorr(measured, case.exact[LF.SPARSE_REF], LF.SPARSE_REF, n, case.name)
    finally:
        default.clear_plans()


def test_frames_past_the_longest_are_refused_and_the_engine_goes_on(engines):
    """2^20 + 1 samples: PAL_ERR_UNSUPPORTED from the all-pairs call, the pair list, phat_correlation (either argument) and
    xcorr_vs_ref; the next call of the same engine at L = 1000 is still right."""
    default, _ = engines
    long_rows = np.zeros((2, LF.MAX_FRAME + 1))
    long_rows[:, 5] = 1.0
    short = np.ones(1000)
    rng = np.random.default_rng(1000)
    frame = rng.standard_normal((3, 1000))
    frame[1:] += 0.6 * np.roll(frame[:1], 37, axis=1)
    want = O.all_pairs(frame, LF.FS, max_expected_delay=0.01)
    refused = (lambda: default.gcc_phat_all_pairs(long_rows, LF.FS),
               lambda: default.gcc_phat_pairs(long_rows, [[0, 1]], LF.FS),
               lambda: default.phat_correlation(long_rows[0], short),
               lambda: default.phat_correlation(short, long_rows[0]),
               lambda: default.xcorr_vs_ref(long_rows, 0))
    try:
        for q, call in enumerate(refused):
            with pytest.raises(PalError) as exc:
                call()
            assert exc.value.code == _ffi.ERR_UNSUPPORTED, (q, exc.value)
            table, corr = default.gcc_phat_all_pairs(frame, LF.FS, max_expected_delay=0.01, want_corr=True)
            for key in INT_FIELDS:
                assert np.array_equal(table[key], want[key]), (q, key)
            assert np.max(np.abs(corr[0] - O.phat_correlation(frame[0], frame[1]))) <= LF.ROW_BOUND, q
    finally:
        default.clear_plans()
