#!/usr/bin/env python3
"""SRP-PHAT map on ONE GPU (csrc/srp.hip): 128 frames x 64 microphones on bench_solve.py's sphere of 0.5 m, L = 12 000 samples at 48 kHz
(the frame shape of configuration C5), a 64^3 grid over a 6 m box, W = 8.

    python tools/bench_srp.py [frames=128] [mics=64] [grid=64] [repeats=5] [spec_grid=16]

Writes one JSON to profiles/srp_bench.json, the zoom's to profiles/srp_zoom_bench.json, the direction map's to
profiles/srp_doa_bench.json, and prints all three.  Every time is the best of `repeats` calls that end in synchronize, after a
warm-up call, on buffers resident in HBM; kernel times are pal_profile's.
- the strips call beside the one-peak call and the K = 4 call on the same frames (pairs/s);
- the map (K = 1 peak per frame) in lag evaluations per second (G * P per frame) and in strip bytes read per second (8 B per
  evaluation), with its square roots per cell beside its lags per cell;
- the NumPy specification (srp.srp_map) per frame on a `spec_grid`^3 grid of the same box, and whether the device's map of that grid
  equals it within the rounding bound and its peak index exactly.
- the zoom (pal_srp_zoom_dev, Z = 8, three levels, the first box one map cell on each side of the seed) alone at K = 1 and K = 2 on the
  peaks of the `grid`^3 map, and the `grid`^3 map alone against a (`grid` / 2)^3 map plus the zoom on the same strips: seconds, and the
  median and worst distance of the answer from the frame's source.
- the direction map (pal_srp_doa_dev, K = 1) on a 72 x 36 and a 360 x 90 sphere and the direction zoom (pal_srp_doa_zoom_dev, Z = 8,
  three levels, the first one cell of elevation) on each one's peaks, on the same strips: seconds, and the median and worst angle
  between the answer and the source's direction from the array's centre, beside the same angle for the `grid`^3 map's peak.
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

# the zoom: alone on the fine map's peaks, and behind a map of half the resolution
ZOOM_Z, ZOOM_LEVELS = 8, 3
coarse = (max(grid_n // 2, 1),) * 3
cell = lambda cnt: (np.asarray(hi) - np.asarray(lo)) / np.asarray(cnt, dtype=np.float64)  # noqa: E731
dev_z = {"peaks2": eng.alloc(frames * 2 * _ffi.SRP_PEAK.itemsize), "zoom": eng.alloc(frames * 2 * _ffi.SRP_ZOOM.itemsize)}


def zoom_distances(k):
    z = eng.download(np.zeros((frames, k), dtype=_ffi.SRP_ZOOM), dev_z["zoom"])
    d = np.linalg.norm(np.stack([z["x"], z["y"], z["z"]], axis=2) - sources[:, None, :], axis=2)
    d = np.where(z["seed"] >= 0, d, np.inf).min(axis=1)                                # the seed that ends nearest the source
    return {"median": round(float(np.median(d)), 4), "max": round(float(d.max()), 4)}, z


zoom_rows = {}
for k in (1, 2):
    eng.srp_map_dev(dev["strips"], frames, T, mics, fs, c, lo, hi, count, 0, k, 1, dev["power"], dev_z["peaks2"], 0)
    eng.synchronize()
    t_z, k_z = best_of(lambda: (eng.srp_zoom_dev(dev["strips"], frames, T, mics, fs, c, dev_z["peaks2"], k, cell(count), ZOOM_Z, ZOOM_LEVELS,
                                                 dev_z["zoom"]), eng.synchronize()))
    dz, rec = zoom_distances(k)
    zoom_rows[f"K{k}"] = {"seconds_per_call": round(t_z, 6), "kernels": {n: v for n, v in k_z.items() if n.startswith("k_srp")},
                          "seeds": int(np.count_nonzero(rec["seed"] >= 0)), "clipped_terms": int(rec["clipped"].sum()),
                          "levels_completed_min": int(rec["levels"][rec["seed"] >= 0].min()), "nearest_zoomed_to_source_m": dz}


def coarse_then_zoom():
    eng.srp_map_dev(dev["strips"], frames, T, mics, fs, c, lo, hi, coarse, 0, 1, 1, dev["power"], dev_z["peaks2"], 0)
    eng.srp_zoom_dev(dev["strips"], frames, T, mics, fs, c, dev_z["peaks2"], 1, cell(coarse), ZOOM_Z, ZOOM_LEVELS, dev_z["zoom"])
    eng.synchronize()


t_cz, k_cz = best_of(coarse_then_zoom)
d_cz, _ = zoom_distances(1)
coarse_peaks = eng.download(np.zeros((frames, 1), dtype=_ffi.SRP_PEAK), dev_z["peaks2"])
d_coarse = np.linalg.norm(np.stack([coarse_peaks["x"][:, 0], coarse_peaks["y"][:, 0], coarse_peaks["z"][:, 0]], axis=1) - sources, axis=1)
for d in dev_z.values():
    eng.free(d)
zoom_out = {
    "workload": {"frames": frames, "mics": mics_n, "pairs": P, "fs": fs, "half_width_T": T, "smoothing_W": W, "box_lo": lo, "box_hi": hi,
                 "repeats": repeats, "Z": ZOOM_Z, "levels": ZOOM_LEVELS, "cells_per_seed": ZOOM_LEVELS * ZOOM_Z ** 3,
                 "first_half_extent": "one cell of the map that gave the seeds"},
    "zoom_alone_on_fine_map_peaks": zoom_rows,
    "fine_map_alone": {"grid": list(count), "seconds_per_call": round(t_map, 6), "cell_m": round((hi[0] - lo[0]) / grid_n, 4),
                       "first_peak_to_source_m": {"median": round(float(np.median(dist)), 4), "max": round(float(dist.max()), 4)}},
    "coarse_map_plus_zoom": {"grid": list(coarse), "seconds_per_call": round(t_cz, 6), "cell_m": round((hi[0] - lo[0]) / coarse[0], 4),
                             "kernels": {n: v for n, v in k_cz.items() if n.startswith("k_srp")},
                             "coarse_first_peak_to_source_m": {"median": round(float(np.median(d_coarse)), 4), "max": round(float(d_coarse.max()), 4)},
                             "zoomed_to_source_m": d_cz},
}

# the direction map (csrc/srp.hip) on the same strips: two spheres and the zoom on each one's peaks, against the `grid`^3 map
src_dir = sources / np.linalg.norm(sources, axis=1, keepdims=True)                   # the array's centre is the origin


def angle_stats(u):
    """Median and worst angle, in degrees, between the rows of u[frames][3] and the sources' directions from the array's centre."""
    u = u / np.linalg.norm(u, axis=1, keepdims=True)
    ang = np.degrees(np.arccos(np.clip(np.sum(u * src_dir, axis=1), -1.0, 1.0)))
    return {"median": round(float(np.median(ang)), 3), "max": round(float(ang.max()), 3)}


d_dzoom = eng.alloc(frames * _ffi.SRP_ZOOM.itemsize)
doa_rows = {}
for n_az, n_el in ((72, 36), (360, 90)):
    az, el, wrap = srp.doa_axes(n_az, n_el)
    t_d, k_d = best_of(lambda: (eng.srp_doa_dev(dev["strips"], frames, T, mics, fs, c, az, el, wrap, 0, 1, 1, dev["power"], dev["peaks"],
                                                dev["summary"]), eng.synchronize()))
    dpk = eng.download(np.zeros((frames, 1), dtype=_ffi.SRP_PEAK), dev["peaks"])
    dsum = eng.download(np.zeros(frames, dtype=_ffi.SRP_FRAME), dev["summary"])
    t_dz, k_dz = best_of(lambda: (eng.srp_doa_zoom_dev(dev["strips"], frames, T, mics, fs, c, dev["peaks"], 1, np.pi / n_el, ZOOM_Z, ZOOM_LEVELS,
                                                       d_dzoom), eng.synchronize()))
    dz = eng.download(np.zeros((frames, 1), dtype=_ffi.SRP_ZOOM), d_dzoom)
    t_kd = k_d.get("k_srp_doa", {"ms": 0})["ms"] / 1e3
    doa_rows[f"{n_az}x{n_el}"] = {
        "cells": n_az * n_el, "cell_deg": round(180.0 / n_el, 3), "map_seconds_per_call": round(t_d, 6),
        "map_kernels": {n: v for n, v in k_d.items() if n.startswith("k_srp") and v["launches"]},
        "k_srp_doa_lag_evaluations_per_s": round(frames * n_az * n_el * P / t_kd, 1) if t_kd else None,
        "clipped_terms": int(dsum["clipped"].sum()), "first_peak_to_source_deg": angle_stats(np.stack([dpk["x"][:, 0], dpk["y"][:, 0], dpk["z"][:, 0]], axis=1)),
        "zoom_seconds_per_call": round(t_dz, 6), "zoom_kernels": {n: v for n, v in k_dz.items() if n.startswith("k_srp") and v["launches"]},
        "zoom_clipped_terms": int(dz["clipped"].sum()), "zoom_levels_completed_min": int(dz["levels"].min()),
        "zoomed_to_source_deg": angle_stats(np.stack([dz["x"][:, 0], dz["y"][:, 0], dz["z"][:, 0]], axis=1))}
eng.free(d_dzoom)
doa_out = {
    "workload": {"frames": frames, "mics": mics_n, "pairs": P, "fs": fs, "half_width_T": T, "smoothing_W": W, "repeats": repeats,
                 "array_radius_m": 0.5, "source_range_m": {"min": round(float(np.linalg.norm(sources, axis=1).min()), 3),
                                                           "median": round(float(np.median(np.linalg.norm(sources, axis=1))), 3),
                                                           "max": round(float(np.linalg.norm(sources, axis=1).max()), 3)},
                 "zoom": {"Z": ZOOM_Z, "levels": ZOOM_LEVELS, "cells_per_seed": ZOOM_LEVELS * ZOOM_Z ** 2, "half0": "one cell of elevation"}},
    "direction_maps": doa_rows,
    "position_map": {"grid": list(count), "cells": G, "seconds_per_call": round(t_map, 6), "first_peak_to_source_deg": angle_stats(pos)},
}

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
with open(os.path.join(ROOT, "profiles", "srp_zoom_bench.json"), "w") as fh:
    json.dump(zoom_out, fh, indent=1)
    fh.write("\n")
with open(os.path.join(ROOT, "profiles", "srp_doa_bench.json"), "w") as fh:
    json.dump(doa_out, fh, indent=1)
    fh.write("\n")
print(json.dumps(out))
print(json.dumps(zoom_out))
print(json.dumps(doa_out))
eng.close()
