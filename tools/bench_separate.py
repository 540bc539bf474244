#!/usr/bin/env python3
"""Null-steering beamformer on ONE GPU (k_separate in csrc/beamform.hip): the shapes of tools/bench_beamform.py - 128 frames x 64
microphones x 12 000 samples at 48 kHz and 16 x 64 x 44 100 at 44.1 kHz - each separated into S = 2, 4 and 8 sources per frame.

    python tools/bench_separate.py [window_seconds=1] [rounds=2]

Writes one JSON to profiles/separate_bench.json and prints it.  Per shape and S, on buffers resident in HBM:
- pal_separate_dev and, in the same run and alternated with it window by window, pal_steer_sum_dev at the same S (the delay-and-sum
  beams the engine offered before: the yardstick): after a warm-up call of each, `rounds` times one window of each, as many calls as
  fill `window_seconds`, the device synchronised before and after a window; every window's ms per call is kept, the best is the figure;
- pal_profile's times of the three parts of one call of each - the forward spectra, k_separate or k_steer_sum, the inverse transforms;
- the ratios separate / steer of the call and of the kernel."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import cases  # noqa: E402
from pyaudiolocalization_amd import Engine, beamform  # noqa: E402

window = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 2
SHAPES = ((128, 64, 12000, 48000.0), (16, 64, 44100, 44100.0))
SOURCES = (2, 4, 8)
LOADING = 0.01
c = cases.C_SOUND

eng = Engine(0)
rng = np.random.default_rng(12)


def one_window(call):
    eng.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        call()
        n += 1
        if n % 4 == 0 or n == 1:
            eng.synchronize()
            if time.perf_counter() - t0 >= window:
                break
    eng.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def parts_of(call, kernel):
    eng.profile_begin()
    call()
    eng.synchronize()
    eng.profile_end()
    prof = eng.profile_entries()
    return {k: round(prof.get(k, (0.0, 0))[0], 4) for k in ("steer_forward_spectra", kernel, "steer_inverse")}


rows_out = []
for B, M, L, fs in SHAPES:
    mics = cases.fibonacci_sphere(M, 0.5)
    x = rng.standard_normal((B, M, L))
    d_x = eng.alloc(x.nbytes)
    eng.upload(d_x, x)
    for S in SOURCES:
        points = rng.uniform(-2.5, 2.5, (B, S, 3)) + np.array([0, 0, 1.5])
        delays, valid = beamform.point_delays(points, mics, c)
        weights = beamform.uniform_weights(valid, M)
        gains = np.ones_like(delays)
        d_d, d_w, d_g, d_out = eng.alloc(delays.nbytes), eng.alloc(weights.nbytes), eng.alloc(gains.nbytes), eng.alloc(B * S * L * 8)
        eng.upload(d_d, delays)
        eng.upload(d_w, weights)
        eng.upload(d_g, gains)

        def separate():
            eng.separate_dev(d_x, B, M, L, fs, d_d, d_g, S, LOADING, d_out)

        def steer():
            eng.steer_dev(d_x, B, M, L, fs, d_d, d_w, S, d_out)

        separate()
        steer()
        eng.synchronize()
        t_sep, t_steer = [], []
        for _ in range(rounds):
            t_sep.append(round(one_window(separate), 4))
            t_steer.append(round(one_window(steer), 4))
        p_sep, p_steer = parts_of(separate, "k_separate"), parts_of(steer, "k_steer_sum")
        rows_out.append({
            "frames": B, "mics": M, "length": L, "fs": fs, "sources_per_frame": S, "loading": LOADING,
            "separate_ms_per_call": min(t_sep), "steer_ms_per_call": min(t_steer), "separate_windows_ms": t_sep, "steer_windows_ms": t_steer,
            "separate_over_steer_call": round(min(t_sep) / min(t_steer), 4),
            "separate_parts_ms": p_sep, "steer_parts_ms": p_steer,
            "k_separate_over_k_steer_sum": round(p_sep["k_separate"] / p_steer["k_steer_sum"], 4) if p_steer["k_steer_sum"] else None,
            "sincos_evaluations": B * M * S * (L + 1),
            "k_separate_sincos_per_s": round(B * M * S * (L + 1) / (p_sep["k_separate"] / 1e3), 1) if p_sep["k_separate"] else None})
        for p in (d_d, d_w, d_g, d_out):
            eng.free(p)
    eng.free(d_x)

out = {"window_seconds": window, "rounds": rounds, "rows": rows_out}
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "separate_bench.json"), "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print(json.dumps(out))
eng.close()
