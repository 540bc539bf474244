#!/usr/bin/env python3
"""MVDR beamformer on ONE GPU (k_mvdr_cov, k_mvdr_weights, k_mvdr_apply in csrc/mvdr_kernels.h): 128 frames x 64 microphones x 12 000
samples at 48 kHz as one group and as 8 groups of 16, and 16 x 64 x 44 100 at 44.1 kHz as one group, each at S = 1, 4 and 8 sources.

    python tools/bench_mvdr.py [window_seconds=1] [rounds=2]

Writes one JSON to profiles/mvdr_bench.json and prints it.  Per shape and S, on buffers resident in HBM:
- pal_mvdr_dev and, in the same run and alternated with it window by window, pal_separate_dev at the same S (the beamformer the engine
  offered before: the yardstick): after a warm-up call of each, `rounds` times one window of each, as many calls as fill
  `window_seconds`, the device synchronised before and after a window; every window's ms per call is kept, the best is the figure;
- pal_profile's times of the parts of one call: the forward spectra of each sweep, k_mvdr_cov, k_mvdr_weights, k_mvdr_apply, the inverse;
- per kernel the bytes it moves by its loop counts and what they would take at 4.2 TB/s (DESIGN 7's figure for mixed streams);
- for the first shape at S = 4, k_mvdr_cov with 4 x 4 tiles (PAL_MVDR_TILE=44) beside the default 8 x 4."""
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
SHAPES = ((128, 64, 12000, 48000.0, 1), (128, 64, 12000, 48000.0, 8), (16, 64, 44100, 44100.0, 1))   # B, M, L, fs, G
SOURCES = (1, 4, 8)
LOADING = 0.1
SEP_LOADING = 0.01
RATE = 4.2e12                                                                   # bytes / s
PARTS = ("mvdr_forward_spectra_1", "k_mvdr_cov", "k_mvdr_weights", "mvdr_forward_spectra_2", "k_mvdr_apply", "mvdr_inverse")
c = cases.C_SOUND

eng = Engine(0)
rng = np.random.default_rng(13)


def one_window(engine, call):
    engine.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        call()
        n += 1
        if n % 4 == 0 or n == 1:
            engine.synchronize()
            if time.perf_counter() - t0 >= window:
                break
    engine.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def parts_of(engine, call, names):
    engine.profile_begin()
    call()
    engine.synchronize()
    engine.profile_end()
    prof = engine.profile_entries()
    return {k: round(prof.get(k, (0.0, 0))[0], 4) for k in names}


def byte_counts(B, M, L, G, S, ti=8, tj=4):
    """bytes each kernel moves over the call by its loop counts (16 bytes per complex value), slices as the engine cuts them"""
    H, Q, T = L + 1, B // G, M * (M + 1) // 2
    per = max(1, min(Q, (1 << 30) // (M * H * 16)))
    slices = -(-Q // per)
    tiles = sum(min((bi + 1) * ti, M) // tj + (1 if min((bi + 1) * ti, M) % tj else 0) for bi in range(-(-M // ti)))
    cov = G * (tiles * (ti + tj) * Q * H + T * H * (2 * slices - 1)) * 16
    weights = G * (T * H + S * M * H) * 16
    ts, tf = (1, 8) if S == 1 else ((2, 4) if S == 2 else (4, 4))
    apply_ = G * (-(-S // ts) * Q * M * H + sum(-(-min(per, Q - s0) // tf) for s0 in range(0, Q, per)) * S * M * H + Q * S * H) * 16
    return {"k_mvdr_cov": cov, "k_mvdr_weights": weights, "k_mvdr_apply": apply_}


rows_out = []
for B, M, L, fs, G in SHAPES:
    mics = cases.fibonacci_sphere(M, 0.5)
    x = rng.standard_normal((B, M, L))
    d_x = eng.alloc(x.nbytes)
    eng.upload(d_x, x)
    for S in SOURCES:
        points = rng.uniform(-2.5, 2.5, (B, S, 3)) + np.array([0, 0, 1.5])
        delays, valid = beamform.point_delays(points, mics, c)
        gains = np.ones_like(delays)
        d_d, d_g, d_out = eng.alloc(delays.nbytes), eng.alloc(gains.nbytes), eng.alloc(B * S * L * 8)
        eng.upload(d_d, delays)                                                 # the first G tables are the groups'
        eng.upload(d_g, gains)

        def mvdr(engine=eng):
            engine.mvdr_dev(d_x, B, M, L, fs, d_d, d_g, G, S, LOADING, d_out)

        def separate():
            eng.separate_dev(d_x, B, M, L, fs, d_d, d_g, S, SEP_LOADING, d_out)

        mvdr()
        separate()
        eng.synchronize()
        t_mvdr, t_sep = [], []
        for _ in range(rounds):
            t_mvdr.append(round(one_window(eng, mvdr), 4))
            t_sep.append(round(one_window(eng, separate), 4))
        parts = parts_of(eng, mvdr, PARTS)
        p_sep = parts_of(eng, separate, ("steer_forward_spectra", "k_separate", "steer_inverse"))
        nbytes = byte_counts(B, M, L, G, S)
        row = {
            "frames": B, "mics": M, "length": L, "fs": fs, "groups": G, "sources": S, "loading": LOADING,
            "mvdr_ms_per_call": min(t_mvdr), "separate_ms_per_call": min(t_sep), "mvdr_windows_ms": t_mvdr, "separate_windows_ms": t_sep,
            "mvdr_over_separate_call": round(min(t_mvdr) / min(t_sep), 4), "mvdr_parts_ms": parts, "separate_parts_ms": p_sep,
            "kernel_bytes": nbytes, "kernel_ms_at_4.2_TB_s": {k: round(v / RATE * 1e3, 4) for k, v in nbytes.items()},
            "kernel_over_byte_estimate": {k: round(parts[k] / (v / RATE * 1e3), 3) if v else None for k, v in nbytes.items()},
            "covariance_flop": 8 * (M * (M + 1) // 2) * (B // G) * (L + 1) * G}
        if (B, G, S) == (SHAPES[0][0], SHAPES[0][4], 4):                        # the other tile of k_mvdr_cov, the same buffers
            os.environ["PAL_MVDR_TILE"] = "44"
            small = Engine(0)
            del os.environ["PAL_MVDR_TILE"]
            mvdr(small)
            small.synchronize()
            cov44 = [parts_of(small, lambda: mvdr(small), ("k_mvdr_cov",))["k_mvdr_cov"] for _ in range(3)]
            cov84 = [parts_of(eng, mvdr, ("k_mvdr_cov",))["k_mvdr_cov"] for _ in range(3)]
            small.close()
            b44 = byte_counts(B, M, L, G, S, 4, 4)["k_mvdr_cov"]
            row["k_mvdr_cov_tiles_ms"] = {"8x4": cov84, "4x4": cov44, "4x4_bytes": b44, "4x4_ms_at_4.2_TB_s": round(b44 / RATE * 1e3, 4)}
        rows_out.append(row)
        for p in (d_d, d_g, d_out):
            eng.free(p)
    eng.free(d_x)

result = {"tool": "tools/bench_mvdr.py", "window_seconds": window, "rounds": rounds, "rate_bytes_per_s": RATE, "rows": rows_out}
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "mvdr_bench.json"), "w") as fh:
    json.dump(result, fh, indent=1)
    fh.write("\n")
print(json.dumps(result))
eng.close()
