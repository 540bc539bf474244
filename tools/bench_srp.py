#!/usr/bin/env python3
"""SRP-PHAT map on ONE GPU (csrc/srp.hip): 128 frames x 64 microphones on bench_solve.py's sphere of 0.5 m, L = 12 000 samples at 48 kHz
(the frame shape of configuration C5), a 64^3 grid over a 6 m box, W = 8.

    python tools/bench_srp.py [frames=128] [mics=64] [grid=64] [repeats=5] [spec_grid=16]

Writes one JSON to profiles/srp_bench.json and prints it.  Every time is the best of `repeats` calls that end in synchronize, after a
warm-up call, on buffers resident in HBM; kernel times are pal_profile's.
- the strips call beside the one-peak call and the K = 4 call on the same frames (pairs/s);
- the map (K = 1 peak per frame) in lag evaluations per second (G * P per frame) and in strip bytes read per second (8 B per
  evaluation), with its square roots per cell beside its lags per cell;
- the NumPy specification (srp.srp_map) per frame on a `spec_grid`^3 grid of the same box, and whether the device's map of that grid
  equals it within the rounding bound and its peak index exactly.
Frames: per frame one source inside the box, a common noise sequence delayed per microphone by the rounded path difference, plus
independent noise of half its amplitude - host work, not timed."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import cases  # noqa: E402
from pyaudiolocalization_amd import RECORD, Engine, _ffi, make_params, srp  # noqa: E402

arg = [int(a) for a in sys.argv[1:]]
frames, mics_n, grid_n, repeats, spec_n = (arg + [128, 64, 64, 5, 16][len(arg):])[:5]
fs, L, c, W, K_PEAKS = 48000.0, 12000, cases.C_SOUND, 8, 4
lo, hi = (-3.0, -3.0, -1.5), (3.0, 3.0, 4.5)
count = (grid_n,) * 3
mics = cases.fibonacci_sphere(mics_n, 0.5)
T = srp.half_width(mics, fs, c)
P, G = mics_n * (mics_n - 1) // 2, grid_n ** 3

rng = np.random.default_rng(11)
sources = rng.uniform(-2.5, 2.5, (frames, 3)) + np.array([0, 0, 1.5])
x = np.empty((frames, mics_n, L))
for f in range(frames):
    d = np.rint(np.linalg.norm(mics - sources[f], axis=1) * fs / c).astype(np.int64)
    d -= d.min()
    common = rng.standard_normal(L + int(d.max()))
    for m in range(mics_n):
        x[f, m] = common[d.max() - d[m]: d.max() - d[m] + L]                  # a larger distance hears the sequence later
    x[f] += 0.5 * rng.standard_normal((mics_n, L))

eng = Engine(0)


def best_of(call):
    call()
    best = None
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        el = time.perf_counter() - t0
        best = el if best is None else min(best, el)
    eng.profile_begin()
    call()
    eng.profile_end()
    return best, {k: {"ms": round(v[0], 4), "launches": v[1]} for k, v in eng.profile_entries().items()}


width = 2 * T + 1
sizes = {"x": x.nbytes, "table": frames * P * RECORD.itemsize, "cand_k": frames * P * K_PEAKS * 4, "cand_h": frames * P * K_PEAKS * 8,
         "strips": frames * P * width * 8, "power": frames * G * 8, "peaks": frames * _ffi.SRP_PEAK.itemsize, "summary": frames * _ffi.SRP_FRAME.itemsize}
dev = {k: eng.alloc(v) for k, v in sizes.items()}
eng.upload(dev["x"], x)
one, many = make_params(fs, 1), make_params(fs, K_PEAKS)
t_one, _ = best_of(lambda: (eng.gcc_phat_all_pairs_dev(dev["x"], frames, mics_n, L, one, dev["table"]), eng.synchronize()))
t_many, _ = best_of(lambda: (eng.gcc_phat_all_pairs_peaks_dev(dev["x"], frames, mics_n, L, many, dev["table"], dev["cand_k"], dev["cand_h"]),
                             eng.synchronize()))
t_strips, k_strips = best_of(lambda: (eng.gcc_phat_all_pairs_strips_dev(dev["x"], frames, mics_n, L, one, T, W, dev["strips"], dev["table"]),
                                      eng.synchronize()))
t_map, k_map = best_of(lambda: (eng.srp_map_dev(dev["strips"], frames, T, mics, fs, c, lo, hi, count, 0, 1, 1, dev["power"], dev["peaks"],
                                                dev["summary"]), eng.synchronize()))
peaks = eng.download(np.zeros((frames, 1), dtype=_ffi.SRP_PEAK), dev["peaks"])
summ = eng.download(np.zeros(frames, dtype=_ffi.SRP_FRAME), dev["summary"])
pos = np.stack([peaks["x"][:, 0], peaks["y"][:, 0], peaks["z"][:, 0]], axis=1)
dist = np.linalg.norm(pos - sources, axis=1)

# the specification on a grid small enough to time, against the device's map of that grid
strips0 = eng.download(np.zeros((P, width)), dev["strips"])                           # frame 0
t0 = time.perf_counter()
want, clipped, total = srp.srp_map(strips0, T, mics, fs, c, lo, hi, (spec_n,) * 3, return_abs=True)
t_spec = time.perf_counter() - t0
got, got_peaks, _ = eng.srp_map(strips0, mics, fs, c, lo, hi, (spec_n,) * 3, K=1, R=1)
within = bool(np.all(np.abs(got[0] - want) <= (P + 1) * 2.0 ** -53 * total))
same_peak = bool(got_peaks[0, 0]["index"] == srp.map_peaks(want.reshape((spec_n,) * 3), 1, 1)["index"][0])
for d in dev.values():
    eng.free(d)

tiles = (mics_n + 15) // 16
t_kernel = k_map.get("k_srp_map", {"ms": 0})["ms"] / 1e3
out = {
    "workload": {"frames": frames, "mics": mics_n, "pairs": P, "length": L, "fs": fs, "half_width_T": T, "smoothing_W": W, "grid": list(count),
                 "cells": G, "box_lo": lo, "box_hi": hi, "repeats": repeats},
    "pair_calls": {"one_peak_seconds": round(t_one, 6), "one_peak_pairs_per_s": round(frames * P / t_one, 1),
                   "peaks4_seconds": round(t_many, 6), "peaks4_pairs_per_s": round(frames * P / t_many, 1),
                   "strips_seconds": round(t_strips, 6), "strips_pairs_per_s": round(frames * P / t_strips, 1),
                   "strips_kernels": {k: v for k, v in k_strips.items() if v["ms"] >= 0.01 * sum(e["ms"] for e in k_strips.values())}},
    "map": {"seconds_per_call": round(t_map, 6), "frames_per_s": round(frames / t_map, 2),
            "lag_evaluations_per_s": round(frames * G * P / t_map, 1), "strip_bytes_read_per_s": round(8.0 * frames * G * P / t_map, 1),
            "kernels": {k: v for k, v in k_map.items() if k.startswith("k_srp")},
            "k_srp_map_lag_evaluations_per_s": round(frames * G * P / t_kernel, 1) if t_kernel else None,
            "square_roots_per_cell": 16 * (tiles + tiles * (tiles + 1) // 2), "lags_per_cell": P,
            "clipped_terms": int(summ["clipped"].sum()), "strips_bytes_per_frame": P * width * 8,
            "first_peak_to_source_m": {"median": round(float(np.median(dist)), 3), "max": round(float(dist.max()), 3),
                                       "cell_m": round((hi[0] - lo[0]) / grid_n, 4)}},
    "specification": {"grid": [spec_n] * 3, "seconds_per_frame": round(t_spec, 3), "lag_evaluations_per_s": round(spec_n ** 3 * P / t_spec, 1),
                      "device_map_within_rounding_bound": within, "device_peak_equals_specification": same_peak},
}
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "srp_bench.json"), "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print(json.dumps(out))
eng.close()
