"""What the column blocks of the finishing pass (csrc/pfa_cols_fin.h, pfa_fin_lean.h) hand to each other through the per-stream
scratch block (csrc/fin_scratch.h): one engine that alternates layouts against engines that only ever see one, the epoch wrap, the
given-up waits and the serialised launches.  64 microphones = 2016 pairs: nine launch groups at 240 transforms, all three stream
slots.  "Exact" is the FIN_CASES rule of test_gpu_parity.py: integer fields bit-exact, float fields to rtol 1e-11."""
import re

import numpy as np
import pytest

from oracle import pal_oracle as O

pytestmark = pytest.mark.gpu

FS = 44100.0
MICS = 64
INT_FIELDS = ("k_sel", "branch", "k_argmax", "n_sel")
FLOAT_FIELDS = ("cmax", "cmin", "snr", "sel_height")
# (method, multiplier): the lean form (per-wavefront statistics, pw 4), the histogram form (pw 1), 'adaptive'
MODES = [("median", 1.0), ("median", 4.2), ("adaptive", 1.0)]
FIN_NAME = "k_pfa_cols_fin"

# the forms of the walk: (name, frame length, fixed group size or None).  The five default forms of FIN_CASES, a length the pass
# does not take (2 x 44106 - 1 = 88211 is prime: the four-step route, whose rows are always stored) and the Rader-89 form under
# pal_set_chunk(64), set back with pal_set_chunk(0) behind the call
FORMS = [("rader89", 44100, None), ("dense2", 44113, None), ("dense3", 44110, None), ("dense4", 44254, None),
         ("strips", 44103, None), ("nofin", 44106, None), ("chunk64", 44100, 64)]


def _walk(m):
    """A sequence of form indices in which every ordered pair (a, b), a != b, follows each other once (Euler circuit)."""
    out_edges = {a: [b for b in range(m) if b != a] for a in range(m)}
    stack, seq = [0], []
    while stack:
        v = stack[-1]
        if out_edges[v]:
            stack.append(out_edges[v].pop())
        else:
            seq.append(stack.pop())
    return seq[::-1]


def _frames(call, length):
    """Delayed copies of one source plus noise, a different seed for every call (stale partials would give other records)."""
    rng = np.random.default_rng(7000 + call)
    base = rng.standard_normal(length + 64)
    delays = rng.integers(0, 64, MICS)
    return np.stack([base[d:d + length] for d in delays]) + 0.5 * rng.standard_normal((MICS, length))


def _mode(call):
    method, mult = MODES[call % 3]
    return method, mult, (0.05 if (call // 3) % 2 == 0 else None)


def _exact(got, want, tag):
    for f in INT_FIELDS:
        assert np.array_equal(got[f], want[f]), (tag, f)
    for f in FLOAT_FIELDS:
        assert np.allclose(got[f], want[f], rtol=1e-11, atol=1e-300), (tag, f)


def _oracle_rows(table, frames, length, call, method, mult, med, count):
    """A seeded sample of rows against the NumPy oracle: integer fields exact, cmax to 1e-11, snr to 1e-9."""
    pairs = [(i, j) for i in range(MICS) for j in range(i + 1, MICS)]
    for k in np.random.default_rng(call).choice(len(pairs), count, replace=False):
        i, j = pairs[k]
        want = O.pair_record(O.phat_correlation(frames[i], frames[j]), length, FS, method, mult, med)
        tag = (call, length, method, mult, med, int(k))
        for f in ("k_sel", "branch", "k_argmax"):
            assert int(table[f][k]) == want[f], (tag, f)
        assert np.isclose(table["cmax"][k], want["cmax"], rtol=1e-11, atol=0), tag
        assert np.isclose(table["snr"][k], want["snr"], rtol=1e-9, atol=0), tag


def _engine(device, monkeypatch, env, chunk=None):
    """An engine created under `env` (read at creation); the variables are removed again behind it."""
    from pyaudiolocalization_amd import Engine
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        eng = Engine(device)
    finally:
        for k in env:
            monkeypatch.delenv(k)
    if chunk:
        eng.set_chunk(chunk)
    return eng


def _per_form(device, monkeypatch, forms, seq, env):
    """Tables of engines that each see one form only (created one at a time), and the stored-row tables (PAL_FIN=0)."""
    alone, stored = {}, {}
    for f, (_, length, chunk) in enumerate(forms):
        eng = _engine(device, monkeypatch, env, chunk)
        try:
            for call, g in enumerate(seq):
                if g == f:
                    method, mult, med = _mode(call)
                    alone[call] = eng.gcc_phat_all_pairs(_frames(call, length), FS, 1, method, mult, med)
        finally:
            eng.close()
    eng = _engine(device, monkeypatch, dict(env, PAL_FIN="0"))
    try:
        for call, g in enumerate(seq):
            _, length, chunk = forms[g]
            eng.set_chunk(chunk or 0)
            method, mult, med = _mode(call)
            stored[call] = eng.gcc_phat_all_pairs(_frames(call, length), FS, 1, method, mult, med)
    finally:
        eng.close()
    return alone, stored


def _run_walk(eng, forms, seq, alone, stored=None, oracle_rows=0, profile=False):
    for call, g in enumerate(seq):
        name, length, chunk = forms[g]
        method, mult, med = _mode(call)
        frames = _frames(call, length)
        if chunk:
            eng.set_chunk(chunk)
        if profile:
            eng.profile_begin()
        t = eng.gcc_phat_all_pairs(frames, FS, 1, method, mult, med)
        if profile:
            eng.profile_end()
            ran = any(k.startswith(FIN_NAME) and v[1] > 0 for k, v in eng.profile_entries().items())
            assert ran == (name != "nofin"), (name, method, mult)   # (the length without a finishing form never runs it)
        if chunk:
            eng.set_chunk(0)
        tag = (call, name, method, mult, med)
        # the same form on an engine that never saw another layout: the same launches, the same partners, the same bytes
        assert t.tobytes() == alone[call].tobytes(), tag
        if stored is not None:
            _exact(t, stored[call], tag)
        if oracle_rows:
            _oracle_rows(t, frames, length, call, method, mult, med, oracle_rows)


@pytest.fixture(scope="module")
def walk_refs(engine):
    return {}


def test_mixed_layouts_on_one_engine(engine, monkeypatch, walk_refs):
    """Every ordered pair of the seven forms follows each other on ONE engine (43 calls, three modes in turn, windowed and not):
    each table byte-identical to an engine that only ever saw its form, exact against the stored rows, 16 rows per call against
    the oracle."""
    seq = _walk(len(FORMS))
    assert len(seq) == len(FORMS) * (len(FORMS) - 1) + 1
    alone, stored = _per_form(engine.device, monkeypatch, FORMS, seq, {})
    walk_refs["plain"] = (seq, alone)
    eng = _engine(engine.device, monkeypatch, {})
    try:
        _run_walk(eng, FORMS, seq, alone, stored, oracle_rows=16, profile=True)
    finally:
        eng.close()


def test_epoch_wrap_across_layouts(engine, monkeypatch, walk_refs):
    """PAL_DEBUG_FIN_WRAP=3: the launch number restarts every second or third launch of a slot, between layouts of either size
    order; every table still byte-identical to the engines that saw one form."""
    if "plain" not in walk_refs:
        seq = _walk(len(FORMS))
        walk_refs["plain"] = (seq, _per_form(engine.device, monkeypatch, FORMS, seq, {})[0])
    seq, alone = walk_refs["plain"]
    eng = _engine(engine.device, monkeypatch, {"PAL_DEBUG_FIN_WRAP": "3"})
    try:
        _run_walk(eng, FORMS, seq, alone)
    finally:
        eng.close()


GIVEUP_LENGTHS = [44100, 44113, 44110, 44254, 44103]
_REPORT = re.compile(r"\[pal\] (\d+) row\(s\) of the finishing column pass went through the stored-row path .*waits given up (\d+)\)")


@pytest.mark.parametrize("length", GIVEUP_LENGTHS, ids=[f"L{c}" for c in GIVEUP_LENGTHS])
def test_given_up_waits_take_the_stored_row_path(engine, length, monkeypatch, capfd):
    """PAL_DEBUG_FIN_GIVEUP=1: every bounded wait of the pass gives up, every pair is flagged and resolved from stored rows at
    the end of the call.  Records byte-identical to PAL_FIN=0 (a repaired row keeps its partner); the finishing kernel and the
    repair's statistics kernels both ran; the report names as many flagged rows as the call has pairs."""
    rng = np.random.default_rng(length + 5)
    mics = 5
    base = rng.standard_normal(length + 64)
    silent = rng.standard_normal((1, mics, length))
    silent[0, 1] = 0.0
    cases = {"noise": rng.standard_normal((1, mics, length)),
             "delayed": (np.stack([base[d:d + length] for d in rng.integers(0, 64, mics)]) + 0.3 * rng.standard_normal((mics, length)))[None],
             "tone": (np.sin(0.05 * np.arange(length))[None, :] + 0.3 * rng.standard_normal((mics, length)))[None],
             "silent": silent,
             "64 mics": _frames(length, length)[None]}
    monkeypatch.setenv("PAL_DEBUG_FALLBACK", "1")                # (read at every report, not at creation)
    gave = _engine(engine.device, monkeypatch, {"PAL_FIN": "1", "PAL_DEBUG_FIN_GIVEUP": "1"})
    stored = _engine(engine.device, monkeypatch, {"PAL_FIN": "0"})
    try:
        for k, (name, fr) in enumerate(cases.items()):
            method, mult = MODES[k % 3]
            med = 0.05 if k % 2 == 0 else None
            tag = (name, method, med)
            npairs = fr.shape[1] * (fr.shape[1] - 1) // 2
            capfd.readouterr()
            gave.profile_begin()
            ta = gave.gcc_phat_all_pairs(fr, FS, 1, method, mult, med)
            gave.profile_end()
            err = capfd.readouterr().err
            ent = gave.profile_entries()
            assert any(e.startswith(FIN_NAME) for e in ent), (tag, sorted(ent))
            assert "k_peak_finish" in ent, (tag, sorted(ent))           # the stored-row pass of the repair
            found = _REPORT.findall(err)
            assert len(found) == 1, (tag, err)
            assert int(found[0][0]) == npairs and int(found[0][1]) > 0, (tag, err)
            tb = stored.gcc_phat_all_pairs(fr, FS, 1, method, mult, med)
            _exact(ta, tb, tag)
            assert ta.tobytes() == tb.tobytes(), tag
    finally:
        gave.close()
        stored.close()


@pytest.mark.parametrize("length", [44100, 44254, 44103])
def test_serialised_launches_equal_default_at_full_size(engine, length, monkeypatch):
    """2 frames x 64 microphones: the finishing launches of the three streams one at a time (PAL_FIN_SERIAL=1) against the
    default (byte-identical), and both against the stored rows (exact)."""
    frames = np.stack([_frames(length + b, length) for b in range(2)])
    engines = {name: _engine(engine.device, monkeypatch, env) for name, env in
               (("default", {}), ("serial", {"PAL_FIN_SERIAL": "1"}), ("stored", {"PAL_FIN": "0"}))}
    try:
        for method, mult, med in (("median", 1.0, 0.05), ("median", 4.2, None), ("adaptive", 1.0, 0.05)):
            t = {name: eng.gcc_phat_all_pairs(frames, FS, 1, method, mult, med) for name, eng in engines.items()}
            tag = (length, method, mult, med)
            assert t["default"].tobytes() == t["serial"].tobytes(), tag
            _exact(t["default"], t["stored"], tag)
            _exact(t["serial"], t["stored"], tag)
    finally:
        for eng in engines.values():
            eng.close()
