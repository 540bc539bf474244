#!/usr/bin/env python3
"""Record the rounding error of the transforms of frames above 98 304 samples (needs an MI355X).

    python tools/long_frame_errors.py [out.json]        (default: profiles/long_frames.json)

Per frame length of tests/long_frames.py and per engine (default switches; PAL_PFA=0 where the default plan takes a prime-factor
cut) it prints and records
    impulse   the largest |row - exact| over the impulse frames' rows (exact: one non-zero sample per row),
    noise     the largest |row - O.phat_correlation| over the three rows of the noise frame (the rung bottoms and 2^20),
and per N of the sparse integer rows the largest |value - exact| / max(1, peak) of what xcorr_vs_ref reports.
These are the values behind the 1e-13 bound of tests/test_gpu_long_frames.py; DESIGN.md section 4.1 carries the table.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import long_frames as LF  # noqa: E402


def kind_name(g):
    return "%s %s,%d" % (g.kind, g.m1 if g.kind == "reg2" else g.l1, g.l2)


def measure(eng, length, pfa):
    n = 2 * length - 1
    worst_peak = worst_off = 0.0
    for f in LF.impulse_frames(length):
        _, corr = eng.gcc_phat_all_pairs(f.frame, LF.FS, want_corr=True)
        for p, (_, _, index, value) in enumerate(f.peaks):
            row = np.abs(corr[p])
            worst_peak = max(worst_peak, abs(float(corr[p][index]) - value))
            row[index] = 0.0
            worst_off = max(worst_off, float(np.max(row)))
    out = {"impulse_peak": worst_peak, "impulse_off_peak": worst_off, "impulse": max(worst_peak, worst_off)}
    if length in LF.NOISE_LENGTHS:
        case = LF.noise_case(length)
        _, corr = eng.gcc_phat_all_pairs(case.frame, LF.FS, want_corr=True)
        out["noise"] = float(np.max(np.abs(corr - case.corr)))
    info = eng.plan_info(length)
    assert info == LF.plan_pin(length, pfa), (length, pfa, info)
    out["plan"] = "%d x %d" % (info["n1"], info["n2"]) if info["n1"] else "%d x %d" % (info["m1"], info["m2"])
    eng.clear_plans()
    assert n == info["n"]
    return out


def main():
    from pyaudiolocalization_amd import Engine
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "long_frames.json")
    default = Engine(0)
    os.environ["PAL_PFA"] = "0"
    try:
        plain = Engine(0)
    finally:
        del os.environ["PAL_PFA"]
    default.set_chunk(4)
    plain.set_chunk(4)
    result = {"bound": LF.ROW_BOUND, "lengths": {}, "xcorr": {}}
    for length in LF.IMPULSE_LENGTHS:
        inv, fwd = LF.geometry(length)
        row = {"inverse": kind_name(inv), "forward": kind_name(fwd)}
        row["default"] = measure(default, length, True)
        if length in LF.CUTS:
            row["PAL_PFA=0"] = measure(plain, length, False)
        result["lengths"][str(length)] = row
        for name in ("default", "PAL_PFA=0"):
            if name in row:
                m = row[name]
                print("L %8d  %-10s %-14s impulse %.3g (peak %.3g, off peak %.3g)%s" % (
                    length, name, m["plan"], m["impulse"], m["impulse_peak"], m["impulse_off_peak"],
                    "  noise %.3g" % m["noise"] if "noise" in m else ""), flush=True)
    for n in LF.SPARSE_N:
        case = LF.sparse_case(n)
        kpk, win, pk, _ = default.xcorr_vs_ref(case.rows, LF.SPARSE_REF)
        worst = 0.0
        for q, seq in enumerate(case.exact[LF.SPARSE_REF]):
            at = int(np.argmax(np.abs(seq)))
            assert int(kpk[q]) == at, (n, q, int(kpk[q]), at)
            scale = max(1.0, abs(float(seq[at])))
            worst = max(worst, abs(float(pk[q]) - abs(float(seq[at]))) / scale,
                        max(abs(float(win[q, j]) - float(seq[at + j - 2])) / scale for j in range(5)))
        result["xcorr"][str(n)] = {"geometry": kind_name(LF.SPARSE_GEOM[n]), "relative_error": worst}
        print("xcorr N %8d  %-12s relative error %.3g" % (n, kind_name(LF.SPARSE_GEOM[n]), worst), flush=True)
        default.clear_plans()
    default.close()
    plain.close()
    with open(out_path, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
