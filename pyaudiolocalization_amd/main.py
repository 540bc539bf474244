"""Drop-in for the reference's main.py: same ``config`` dict, ``simulate_signals_with_multipath`` and
``localize_sound_source`` signatures and result dict (main.py:26-64, :66-79, :126, :326-333).

What changed underneath: the per-(mic, path) fractional-delay loop (main.py:104-118) is one batched
HIP launch group, and the i<j pair loop around get_time_delays_phat (main.py:202-228) is one call
that returns the whole TDOA table.  The 3-unknown position solve runs on the host with the same
SciPy / scikit-learn calls as the reference by default; ``localization["solver"] = "device"`` and
``solve_positions_device`` take the batched device solve instead (solve.py).
"""
from __future__ import annotations

import logging
from typing import Any, Dict, Optional, Sequence

import numpy as np

from . import _ffi
from .engine import default_engine, pair_list
from .materials import material_properties  # module-level table, used regardless of config
from .signal_processing import generate_signal, noise_reduction_rows
from .utils import (bootstrap_significance, bootstrap_thresholds, calculate_attenuation, compute_weights, distance, dynamic_bounds_extended,
                    equations, equations_jacobian, generate_image_sources_iterative, residuals, heuristic_initialization_adaptive, read_audio_files,
                    speed_of_sound, synchronize_signals_improved)

log = logging.getLogger(__name__)

config = {
    "fs": 44100,
    "duration": 1.0,
    "celsius": 20,
    "humidity": 50,
    "mic_positions": [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]],
    "source_position": [0.5, 0.5, 0.5],
    "signal_type": "sine",
    "freq": 1000,
    "reflective_planes": [
        {"plane": [1, 0, 0, -5], "material": "wood"},
        {"plane": [0, 1, 0, -5], "material": "metal"},
        {"plane": [0, 0, 1, -5], "material": "wood"},
    ],
    "calibration": {"signal_type": "chirp", "freq_start": 500, "freq_end": 5000, "attenuation_factor": 1.0,
                    "noise_level": 0.01},
    "localization": {"max_reflections": 3, "filter_method": "butterworth", "absorption_threshold": 0.01,
                     "analyze_correlation": True, "visualize_correlation": True, "clustering_method": "kmeans",
                     "clustering_eps": 0.001, "clustering_min_samples": 2, "max_expected_delay": 0.05},
}


def multipath_geometry(source_pos, mic_positions, c, freq, reflective_planes, material_properties, max_reflections,
                       absorption_threshold):
    """Per-mic path table: delays[M][1+I] seconds and gains[M][1+I], direct path first with material
    'air' (main.py:106-108) then the image sources in discovery order (main.py:111-116), and the
    longest delay over all mics and paths (main.py:93-101)."""
    images = generate_image_sources_iterative(source=source_pos, planes=reflective_planes, max_order=max_reflections,
                                              frequency=freq, material_properties=material_properties,
                                              mic_positions=mic_positions, absorption_threshold=absorption_threshold)
    mics = np.asarray(mic_positions, dtype=np.float64)
    delays = np.zeros((mics.shape[0], 1 + len(images)))
    gains = np.zeros_like(delays)
    longest = 0
    for m, mic in enumerate(mics):
        dists = [distance(source_pos, mic)] + [distance(img["source"], mic) for img in images]
        mats = ["air"] + [img["material"] for img in images]
        for p, (d, mat) in enumerate(zip(dists, mats)):
            delays[m, p] = d / c
            gains[m, p] = calculate_attenuation(d, mat, freq, material_properties)
        longest = max(longest, max(dists) / c)
    return delays, gains, longest


def simulate_signals_with_multipath(source_pos, mic_positions, fs, c, duration=1.0, signal_type="sine", freq=1000,
                                    reflective_planes=None, material_properties=None, max_reflections=2,
                                    absorption_threshold=0.01, trim_to_duration=True):
    """Image-source multipath simulation (main.py:66-124): list of M signals of int(duration*fs) samples,
    each normalised and compressed.  Geometry on the host, synthesis on the HIP engine."""
    base = generate_signal(signal_type, fs, duration, freq)
    delays, gains, longest = multipath_geometry(source_pos, mic_positions, c, freq, reflective_planes,
                                                material_properties, max_reflections, absorption_threshold)
    total = int((duration + longest) * fs)                                    # main.py:102
    trim = int(duration * fs) if trim_to_duration else 0                      # main.py:119-120
    out = default_engine().simulate_multipath(base[None], fs, total, delays[None], gains[None], trim)
    return [row.copy() for row in out[0]]


def tdoa_table(frames: np.ndarray, fs: float, max_expected_delay: Optional[float] = None, threshold_method="median",
               threshold_multiplier=1.0, want_corr=False):
    """The pair loop of main.py:202-228 as one engine call: frames[M][L] or [B][M][L] ->
    structured table[(B,) P] in row-major i<j order (fields of _ffi.RECORD) [+ corr]."""
    return default_engine().gcc_phat_all_pairs(frames, fs, 1, threshold_method, threshold_multiplier,
                                               max_expected_delay, want_corr)


def _warn_branches(table) -> None:
    for bit, text in ((_ffi.BR_ALT_THRESHOLD, "primary threshold found no peaks"),
                      (_ffi.BR_ARGMAX_NO_PEAKS, "no peaks at all, correlation maximum used"),
                      (_ffi.BR_WINDOW_RETRY, "no peak inside the expected delay range"),
                      (_ffi.BR_ARGMAX_WINDOW, "no valid peak after alternative filtering, correlation maximum used")):
        hit = int(np.count_nonzero(table["branch"] & bit))
        if hit:
            log.warning("%s for %d microphone pair(s)", text, hit)


def solve_position(mic_positions, mic_pairs, td_diffs, c, weights=None, clustering_method="kmeans", clustering_eps=0.001,
                   clustering_min_samples=2, jacobian="2-point") -> np.ndarray:
    """TDOA table -> source position exactly as main.py:233-298: clustered start points, extended bounds,
    bounded trust-region least squares from every start (best successful cost wins), differential
    evolution when none succeeds, first start as the last resort.  Host side (3 unknowns, SciPy / scikit-learn
    like the reference); kept separate so that it can be pinned against the reference's fixtures without a GPU."""
    from scipy.optimize import differential_evolution, least_squares
    if weights is None:
        weights = np.ones(len(mic_pairs))
    guesses = heuristic_initialization_adaptive(mic_positions, mic_pairs, td_diffs, c, clustering_method=clustering_method,
                                                eps=clustering_eps, min_samples=clustering_min_samples)
    bounds = dynamic_bounds_extended(mic_positions, td_diffs, c, buffer=5.0)
    lower = [b[0] for b in bounds]
    upper = [b[1] for b in bounds]
    guesses = [np.array([np.clip(g[k], lower[k], upper[k]) for k in range(len(g))]) for g in guesses]
    best = None
    pair_arr = np.asarray(mic_pairs, dtype=np.int64).reshape(-1, 2)      # (converted once: 32 640 tuples cost 10 ms per evaluation)
    td_arr = np.asarray(td_diffs, dtype=np.float64)
    # Same solver, bounds, tolerances and - by default - the same forward-differenced Jacobian as main.py:259-274.  The
    # reference stops at ftol = xtol = gtol = 1e-6, which on ill-conditioned tables (C3: planar array) is
    # millimetres short of the optimum and depends on the path taken: with the analytic Jacobian
    # (jacobian="analytic", utils.equations_jacobian) the C3 fixture lands 4.6 mm from the reference's answer, so the 1e-3 m
    # parity bar keeps the differenced one.  Its cost is no longer the reference's (three extra passes of a Python loop
    # over the pairs per step): the residuals are one vectorised evaluation, 0.5 ms at 32 640 pairs.
    jac = equations_jacobian if jacobian == "analytic" else "2-point"
    for guess in guesses:
        fit = least_squares(residuals, guess, jac=jac, args=(mic_positions, pair_arr, td_arr, c, weights),
                            bounds=(lower, upper), method="trf", ftol=1e-6, xtol=1e-6, gtol=1e-6)
        if fit.success and (best is None or fit.cost < best.cost):
            best = fit
    if best is not None:
        return np.array(best.x)
    log.warning("least squares failed for every start, trying differential evolution")
    de = differential_evolution(lambda v: np.sum(np.square(equations(v, mic_positions, mic_pairs, td_diffs, c, weights))),
                                bounds=list(zip(lower, upper)), strategy="best1bin", maxiter=1000, popsize=15, tol=1e-6,
                                mutation=(0.5, 1), recombination=0.7, polish=True, init="latinhypercube")
    return np.array(de.x) if de.success else np.array(guesses[0])


def host_position(table, length, mic_positions, fs, c, calib_delays, weights, clustering=("kmeans", 0.001, 2)) -> np.ndarray:
    """One frame through the host tail (solve_position) from its record table."""
    m = len(mic_positions)
    pairs = pair_list(m)
    td = (table["k_sel"].astype(np.int64) - (int(length) - 1)) / fs
    if calib_delays is not None:
        cal = np.asarray(calib_delays, dtype=float)
        td = td - (cal[pairs[:, 1]] - cal[pairs[:, 0]])
    mic_pairs = [(int(i), int(j)) for i, j in pairs]
    if isinstance(weights, str):
        w = np.ones(len(mic_pairs)) if weights == "ones" else compute_weights({p: {"snr": float(s)} for p, s in zip(mic_pairs, table["snr"])},
                                                                             mic_pairs)
    else:
        w = np.asarray(weights, dtype=float)
    return solve_position(mic_positions, mic_pairs, list(td), c, w, *clustering)


def solve_positions_device(tables, lengths, mic_positions, fs, c, calib_delays=None, weights=None, buffer=5.0, grid=4, max_iter=200,
                           extra_starts=None, engine=None, return_records=False, clustering=("kmeans", 0.001, 2), loss="linear",
                           f_scale=1.0, closure_tol=1, closure_min_votes=1, closure_mode="soft", candidates=None, consensus_tol=1,
                           consensus_rounds=2):
    """TDOA tables[B][P] (or [P]) -> positions[B][3] by the batched device solve (Engine.solve_positions; algorithm: solve.py).
    ``weights``: None / 'ones', 'snr' (the records' SNR as compute_weights weighs it) or an array [B][P].  A frame the device does
    not solve - a weight that is not finite (an infinite SNR), or no start that ended inside a stop rule - goes through the host
    tail (solve_position) instead, as the reference would have solved it.  ``return_records``: also the solve.POSITION records.
    ``loss`` / ``f_scale``: a robust loss of solve.LOSSES for tables with outlier pairs (the host tail knows the linear one only).
    ``weights='closure'``: the loop-closure weights of the tables (Engine.tdoa_closure with ``closure_tol``, ``closure_min_votes``,
    ``closure_mode``; closure.py), computed on the device and used as the array, in the host tail too.  A frame that keeps fewer than
    four pairs is solved like any other: its position means nothing, and ``kept_pairs`` of Engine.tdoa_closure's summary says so.
    ``candidates=(cand_k, cand_h)``: K candidate peaks per pair ([B][P][K]; cand_h may be None): the loop-closure consensus
    (Engine.tdoa_consensus with ``consensus_tol`` and ``consensus_rounds``; consensus.py) first replaces every pair's first peak by the
    candidate the other pairs agree with, and the solve - and the closure weights, if asked for - see the repaired tables.
    Precondition, as for ``weights='closure'``: CENTRED indices, whose lag k - (L - 1) is the true delay.  The tables and candidates of
    the GCC-PHAT calls keep the reference's index mapping, under which no triangle closes and the consensus moves nothing:
    map ``tables['k_sel']`` and ``cand_k`` with ``consensus.centred`` first (tests/test_gpu_pairs_peaks.py does)."""
    from . import solve as S
    S.check_loss(loss, f_scale)
    eng = engine or default_engine()
    tab = np.ascontiguousarray(tables, dtype=_ffi.RECORD)
    one = tab.ndim == 1
    if one:
        tab = tab[None]
    w = "ones" if weights is None else weights
    ln = np.broadcast_to(np.asarray(lengths, dtype=np.int64), (tab.shape[0],))
    if candidates is not None:
        cand_k, cand_h = candidates
        tab = eng.tdoa_consensus(cand_k, ln, len(mic_positions), consensus_tol, consensus_rounds, tables=tab, cand_h=cand_h,
                                 outputs=("table_out",))[1]
    if isinstance(w, str) and w == "closure":
        w = eng.tdoa_closure(tab, ln, len(mic_positions), closure_tol, closure_min_votes, closure_mode, outputs=("weights",))[2]
    robust = {} if loss == "linear" else {"loss": loss, "f_scale": f_scale}
    rec = eng.solve_positions(tab, ln, mic_positions, fs, c, calib_delays, w, buffer, grid, max_iter, extra_starts, **robust)
    pos = rec["position"].copy()
    for f in np.flatnonzero((rec["status"] & S.ST_CONVERGED) == 0):
        log.warning("frame %d: the device solve has no converged start (status %d), using the host solve", f, int(rec["status"][f]))
        wf = w if isinstance(w, str) else np.asarray(w, dtype=float).reshape(tab.shape[0], -1)[f]
        pos[f] = host_position(tab[f], ln[f], np.asarray(mic_positions), fs, c, calib_delays, wf, clustering)
    if one:
        pos, rec = pos[0], rec[0]
    return (pos, rec) if return_records else pos


def srp_positions_device(frames, mic_positions, fs, c, lo, hi, count, W=8, K=1, R=1, refine=False, T=None, pair_weights=None, engine=None,
                         threshold_method="median", threshold_multiplier=1.0, max_expected_delay=None, zoom=None, **solve_args):
    """frames[B][M][L] (or [M][L]) -> peaks[B][K] of _ffi.SRP_PEAK: the first ``K`` maxima (neighbourhood radius ``R`` cells) of every
    frame's steered-response power map over the grid of ``count`` cells in the box ``lo .. hi`` (Engine.gcc_phat_all_pairs_strips with
    smoothing ``W``, then Engine.srp_map; rules: srp.py).  ``T``: the strips' half-width, by default srp.half_width, for which no lag
    is clipped.  The map reads the rows at the true delay, so the table's index mapping plays no part, and a second source shows as a
    second peak.  ``refine=True`` -> (peaks, records of solve.POSITION): every frame's first peak goes to Engine.solve_positions as one
    more start (``extra_starts``), on the one-peak table of the same rows with ``consensus.centred`` applied to ``k_sel`` (the
    precondition solve_positions_device documents); the solve's winner rule is unchanged, ``solve_args`` go to it.
    ``zoom=(Z, levels)`` or ``(Z, levels, span)``: Engine.srp_zoom refines the K peaks on the same strips, the first level over each
    peak -+ ``span`` (default 1.0) cells of the map -> (peaks, zoomed[B][K] of _ffi.SRP_ZOOM), with ``refine=True`` -> (peaks, zoomed,
    records) and the zoomed position, where present, as the solve's start.  The zoom is a local search: it finds the maximum of the
    interpolated power that the first box holds."""
    from . import consensus, srp
    eng = engine or default_engine()
    x = np.ascontiguousarray(frames, dtype=np.float64)
    one = x.ndim == 2
    if one:
        x = x[None]
    if x.ndim != 3:
        raise ValueError("frames must be [M][L] or [B][M][L]")
    mics = np.ascontiguousarray(mic_positions, dtype=np.float64)
    length = x.shape[2]
    half = srp.half_width(mics, fs, c) if T is None else int(T)
    strips, table = eng.gcc_phat_all_pairs_strips(x, fs, half, W, threshold_method, threshold_multiplier, max_expected_delay,
                                                  want_table=bool(refine))
    peaks = eng.srp_map(strips, mics, fs, c, lo, hi, count, pair_weights, K, R, outputs=("peaks",))[1]
    zoomed = None
    if zoom is not None:
        if len(zoom) not in (2, 3):
            raise ValueError("zoom is (Z, levels) or (Z, levels, span)")
        span = float(zoom[2]) if len(zoom) == 3 else 1.0
        lo_, hi_, count_ = srp.check_grid(lo, hi, count)
        zoomed = eng.srp_zoom(strips, mics, fs, c, peaks, span * ((hi_ - lo_) / count_), int(zoom[0]), int(zoom[1]), pair_weights)
    if not refine:
        if zoomed is None:
            return peaks[0] if one else peaks
        return (peaks[0], zoomed[0]) if one else (peaks, zoomed)
    tab = table.copy()
    tab["k_sel"] = consensus.centred(tab["k_sel"], length)
    first = peaks[:, 0]
    centre = 0.5 * (np.asarray(lo, dtype=np.float64) + np.asarray(hi, dtype=np.float64))
    starts = np.where((first["index"] >= 0)[:, None], np.stack([first["x"], first["y"], first["z"]], axis=1), centre[None, :])
    if zoomed is not None:
        zf = zoomed[:, 0]
        starts = np.where(((zf["seed"] >= 0) & (zf["levels"] > 0))[:, None], np.stack([zf["x"], zf["y"], zf["z"]], axis=1), starts)
    rec = eng.solve_positions(tab, length, mics, fs, c, extra_starts=starts[:, None, :], **solve_args)
    if zoomed is not None:
        return (peaks[0], zoomed[0], rec[0]) if one else (peaks, zoomed, rec)
    return (peaks[0], rec[0]) if one else (peaks, rec)


def srp_directions_device(frames, mic_positions, fs, c, n_az=72, n_el=36, W=2, K=1, R=1, T=None, pair_weights=None, zoom=None, engine=None,
                          threshold_method="median", threshold_multiplier=1.0, max_expected_delay=None):
    """frames[B][M][L] (or [M][L]) -> peaks[B][K] of _ffi.SRP_PEAK with directions in x, y, z: the first ``K`` maxima (neighbourhood
    radius ``R`` cells, azimuth wrapped) of every frame's direction map over ``n_az`` x ``n_el`` cells
    of azimuth and elevation (Engine.gcc_phat_all_pairs_strips with smoothing ``W``, then Engine.srp_doa; rules: srp.py, doa_*).  For
    arrays that resolve direction and not range: a source far from the array lies on a two-dimensional set of directions, and a
    5-degree sphere is 2592 cells.  ``T``: the strips' half-width, by default srp.half_width, for which no lag is clipped.
    ``zoom=(Z, levels)`` or ``(Z, levels, span)``: Engine.srp_doa_zoom refines the K directions on the same strips, the first level
    over each peak -+ ``span`` (default 1.0) cells of elevation in its tangent plane -> (peaks, zoomed[B][K] of _ffi.SRP_ZOOM).
    srp.doa_angles turns either into degrees."""
    from . import srp
    eng = engine or default_engine()
    x = np.ascontiguousarray(frames, dtype=np.float64)
    one = x.ndim == 2
    if one:
        x = x[None]
    if x.ndim != 3:
        raise ValueError("frames must be [M][L] or [B][M][L]")
    mics = np.ascontiguousarray(mic_positions, dtype=np.float64)
    az, el, wrap = srp.doa_axes(n_az, n_el)                                             # the full sphere: azimuth wraps
    half = srp.half_width(mics, fs, c) if T is None else int(T)
    strips, _ = eng.gcc_phat_all_pairs_strips(x, fs, half, W, threshold_method, threshold_multiplier, max_expected_delay, want_table=False)
    peaks = eng.srp_doa(strips, mics, fs, c, az, el, wrap, pair_weights, K, R, outputs=("peaks",))[1]
    if zoom is None:
        return peaks[0] if one else peaks
    if len(zoom) not in (2, 3):
        raise ValueError("zoom is (Z, levels) or (Z, levels, span)")
    span = float(zoom[2]) if len(zoom) == 3 else 1.0
    zoomed = eng.srp_doa_zoom(strips, mics, fs, c, peaks, span * (np.pi / int(n_el)), int(zoom[0]), int(zoom[1]), pair_weights)
    return (peaks[0], zoomed[0]) if one else (peaks, zoomed)


def _beam_tables(frames, mic_positions, c, points, directions, weights, calib_delays, default):
    """The input handling beamform_device and separate_device share: -> x[B][M][L], delays[B][S][M], w[B][S][M], one.  ``points`` or
    ``directions`` (exactly one) is [B][S][3], or [S][3] for every frame, or SRP records; ``weights`` is what broadcasts to [B][S][M], or
    None for ``default`` everywhere (None: 1/M); a point that is not valid (absent record, non-finite coordinate) gets weights of 0."""
    from . import beamform
    if (points is None) == (directions is None):
        raise ValueError("give exactly one of points and directions")
    x = np.ascontiguousarray(frames, dtype=np.float64)
    one = x.ndim == 2
    if one:
        x = x[None]
    if x.ndim != 3:
        raise ValueError("frames must be [M][L] or [B][M][L]")
    mics = np.ascontiguousarray(mic_positions, dtype=np.float64)
    if mics.shape != (x.shape[1], 3):
        raise ValueError("one microphone position per row of a frame")
    where = np.asarray(points if points is not None else directions)
    if where.dtype.names:
        where = beamform.records_to_points(where)
    else:
        where = np.asarray(where, dtype=np.float64)
    if one and where.ndim == 3 and where.shape[0] == 1:
        where = where[0]
    if where.ndim == 2:
        where = np.broadcast_to(where[None], (x.shape[0],) + where.shape)
    if where.ndim != 3 or where.shape[0] != x.shape[0] or where.shape[2] != 3:
        raise ValueError("points / directions must be [B][S][3], [S][3] or SRP records [B][S]")
    to_delays = beamform.point_delays if points is not None else beamform.direction_delays
    delays, valid = to_delays(where, mics, c, calib_delays)
    if weights is None:
        w = beamform.uniform_weights(valid, x.shape[1])
        if default is not None:
            w = np.where(valid[..., None], float(default), 0.0) * np.ones(x.shape[1])
    else:
        w = np.where(valid[..., None], np.broadcast_to(np.asarray(weights, dtype=np.float64), delays.shape), 0.0)
    return x, delays, w, one


def beamform_device(frames, mic_positions, fs, c, points=None, directions=None, weights=None, calib_delays=None, engine=None):
    """frames[B][M][L] (or [M][L]) -> out[B][S][L] (or [S][L]): every frame's delay-and-sum beams at ``points`` or ``directions``
    (exactly one of them; Engine.steer, rule: beamform.py).  Either is [B][S][3], or [S][3] for every frame, or an array of
    _ffi.SRP_PEAK / _ffi.SRP_ZOOM records, so the peaks or the zoom results of srp_positions_device and srp_directions_device go in as
    they are.  An absent record or a point with a non-finite coordinate gives a row of zeros.  ``weights``: [B][S][M] (or what
    broadcasts to it), by default 1/M.  ``calib_delays``: the per-microphone calibration delays localize_sound_source corrects the
    pair delays with.  A beam at source 0 still holds source 1 at the level of the array's side lobes: separate_device cancels it."""
    x, delays, w, one = _beam_tables(frames, mic_positions, c, points, directions, weights, calib_delays, None)
    out = (engine or default_engine()).steer(x, fs, delays, w)
    return out[0] if one else out


def separate_device(frames, mic_positions, fs, c, points=None, directions=None, gains=None, loading=0.01, calib_delays=None, engine=None):
    """frames[B][M][L] (or [M][L]) -> out[B][S][L] (or [S][L]): every frame's null-steering beams at ``points`` or ``directions``, the
    inputs of beamform_device (Engine.separate, rule: beamform.separate): beam s holds source s with the other S - 1 cancelled, which
    is what separates the sources srp_positions_device(K=2, zoom=...) finds.  ``gains``: [B][S][M] (or what broadcasts to it), by
    default 1; an absent record or a point with a non-finite coordinate gets gains of 0, a row of zeros that the other beams do not
    notice.  ``loading``: the diagonal loading relative to the largest sum_m gains^2 (> 0 where S > 1).  S <= 8."""
    x, delays, g, one = _beam_tables(frames, mic_positions, c, points, directions, gains, calib_delays, 1.0)
    out = (engine or default_engine()).separate(x, fs, delays, g, loading)
    return out[0] if one else out


def mvdr_device(frames, mic_positions, fs, c, points=None, directions=None, gains=None, loading=0.1, groups=1, calib_delays=None,
                engine=None):
    """frames[B][M][L] -> out[B][S][L]: the MVDR beams at ``points`` or ``directions`` (Engine.mvdr, rule: beamform.mvdr).  The frames
    are ``groups`` groups of B / groups consecutive frames; a group's frames are the snapshots of one covariance and share one
    steering table, so ``points`` / ``directions`` are [G][S][3], or [S][3] for every group, or SRP records [G][S].  ``gains``:
    [G][S][M] (or what broadcasts to it), by default 1; an absent record or a point with a non-finite coordinate gets gains of 0, a
    row of zeros.  ``loading``: the diagonal loading relative to tr(R) / M (> 0).  Unlike separate_device the beam is told nothing
    about the other sources: what is stationary over a group's frames and does not arrive with the target's delays is cancelled from
    the data.  M <= 64.  frames[M][L] is one group of one frame and gives out[S][L]."""
    x = np.ascontiguousarray(frames, dtype=np.float64)
    one = x.ndim == 2
    if one:
        x = x[None]
    groups = int(groups)
    if x.ndim != 3 or groups < 1 or x.shape[0] % groups:
        raise ValueError("frames must be [B][M][L] in groups that divide B")
    _, delays, g, _ = _beam_tables(x[:groups], mic_positions, c, points, directions, gains, calib_delays, 1.0)
    out = (engine or default_engine()).mvdr(x, fs, delays, g, loading, groups)
    return out[0] if one else out


def localize_sound_source(config, calibration_data=None, audio_files=None, use_simulation=True, show_plots=True):
    fs = config["fs"]
    duration = config["duration"]
    mic_positions = np.array(config["mic_positions"])
    source_position = config["source_position"]
    signal_type = config["signal_type"]
    freq = config["freq"]
    reflective_planes = config.get("reflective_planes", [])
    loc = config.get("localization", {})
    filter_method = loc.get("filter_method", "butterworth")
    max_reflections = loc.get("max_reflections", 2)
    absorption_threshold = loc.get("absorption_threshold", 0.01)
    analyze_correlation = loc.get("analyze_correlation", False)
    visualize_correlation = loc.get("visualize_correlation", False)
    clustering_method = loc.get("clustering_method", "kmeans")
    clustering_eps = loc.get("clustering_eps", 0.001)
    clustering_min_samples = loc.get("clustering_min_samples", 2)
    max_expected_delay = loc.get("max_expected_delay", None)
    bootstrap_rng = loc.get("bootstrap_rng", "numpy")        # "device": counter-based shuffles, all pairs in one call
    bootstrap_seed = loc.get("bootstrap_seed", 0)
    solver = loc.get("solver", "host")                       # "device": the batched Levenberg-Marquardt solve (solve.py)
    if solver not in ("host", "device"):
        raise ValueError("localization.solver must be 'host' or 'device'")
    solver_loss = {}                                         # a robust loss of the device solve (solve.LOSSES)
    if solver == "device":
        solver_loss = {"loss": loc.get("solver_loss", "linear"), "f_scale": loc.get("solver_f_scale", 1.0)}
        from . import solve as S
        S.check_loss(**solver_loss)

    calib_delays = None
    if calibration_data is not None:                                           # main.py:147-157
        if len(calibration_data) != len(mic_positions):
            log.warning("calibration entries do not match the microphone count, ignoring calibration")
        else:
            try:
                calib_delays = np.array([d.get("delay", 0.0) for d in calibration_data], dtype=float)
                log.info("calibration correction enabled")
            except Exception as exc:
                log.warning("cannot use calibration data (%s), ignoring calibration", exc)
                calib_delays = None

    c = speed_of_sound(config["celsius"], config["humidity"])
    log.info("speed of sound: %.2f m/s", c)

    if use_simulation:
        if source_position is None:
            raise ValueError("source_position is required when use_simulation=True")
        signals = simulate_signals_with_multipath(source_pos=source_position, mic_positions=mic_positions, fs=fs, c=c,
                                                  duration=duration, signal_type=signal_type, freq=freq,
                                                  reflective_planes=reflective_planes,
                                                  material_properties=material_properties,
                                                  max_reflections=max_reflections,
                                                  absorption_threshold=absorption_threshold, trim_to_duration=True)
    else:
        if audio_files is None:
            raise ValueError("audio_files are required when use_simulation=False")
        if len(audio_files) != len(mic_positions):
            raise ValueError("the number of audio files must equal the number of microphones")
        signals = read_audio_files(audio_files, fs)

    signals = synchronize_signals_improved(signals, fs)                       # main.py:188
    filtered = noise_reduction_rows(np.asarray(signals), fs, method=filter_method)   # main.py:191, one launch

    # ---- main.py:195-228 as one table -------------------------------------------------------
    m = len(mic_positions)
    pairs = pair_list(m)
    res = tdoa_table(filtered, fs, max_expected_delay, want_corr=visualize_correlation)
    table, corr_rows = res if visualize_correlation else (res, None)
    if len(table) == 0:
        raise RuntimeError("no microphone pairs with an estimated time delay")   # main.py:230-231
    _warn_branches(table)
    n2 = filtered.shape[1]
    td_diffs, mic_pairs = [], []
    corr_matrix = np.zeros((m, m))
    correlation_metrics: Dict[Any, Any] = {}
    thresholds = None
    if analyze_correlation and bootstrap_rng == "device":
        thresholds = bootstrap_thresholds(filtered, pairs, fs, alpha=0.05, seed=bootstrap_seed)
    for p, (row, (i, j)) in enumerate(zip(table, pairs)):
        i, j = int(i), int(j)
        td = (np.int64(row["k_sel"]) - (n2 - 1)) / fs                          # time_lags[k] (utils.py:141-142)
        if calib_delays is not None:
            td = td - (calib_delays[j] - calib_delays[i])                     # main.py:209-212
        td_diffs.append(td)
        mic_pairs.append((i, j))
        if analyze_correlation:                                                # main.py:219-222, utils.py:261-271
            ratio = np.inf if row["cmin"] == 0 else row["cmax"] / abs(row["cmin"])
            limit = thresholds[p] if thresholds is not None else \
                bootstrap_significance(filtered[i], filtered[j], fs, alpha=0.05, rng=bootstrap_rng)
            snr = float(row["snr"])
            correlation_metrics[(i, j)] = {"peak_to_peak_ratio": ratio, "snr": snr,
                                           "significant": bool(row["cmax"] > limit) and snr > 2.0}
        corr_matrix[i, j] = corr_matrix[j, i] = row["cmax"]                   # main.py:223-225

    # ---- host tail: main.py:233-298 ---------------------------------------------------------------
    weights = compute_weights(correlation_metrics, mic_pairs) if analyze_correlation and correlation_metrics \
        else np.ones(len(mic_pairs))
    if solver == "device":
        position = solve_positions_device(table, n2, mic_positions, fs, c, calib_delays, weights,
                                          clustering=(clustering_method, clustering_eps, clustering_min_samples), **solver_loss)
    else:
        position = solve_position(mic_positions, mic_pairs, td_diffs, c, weights, clustering_method, clustering_eps,
                                  clustering_min_samples)
    log.info("estimated source: (%.3f, %.3f, %.3f) m", *position)

    # ---- plots: main.py:300-319 (files are written when show_plots is False) ------------
    if use_simulation:
        import matplotlib.pyplot as plt
        fig = plt.figure()
        ax = fig.add_subplot(111, projection="3d")
        ax.scatter(mic_positions[:, 0], mic_positions[:, 1], mic_positions[:, 2], c="r", marker="o", label="microphones")
        ax.scatter(*source_position, c="g", marker="*", s=100, label="actual source")
        ax.scatter(*position, c="b", marker="x", s=100, label="estimated source")
        ax.set_xlabel("X (m)"); ax.set_ylabel("Y (m)"); ax.set_zlabel("Z (m)")
        ax.legend()
        plt.title("Sound Source Localization")
        plt.show() if show_plots else plt.savefig("localization_result.png")
        plt.close(fig)
    if visualize_correlation:
        from .plotting import plot_correlation_3d, plot_correlation_heatmap
        plot_correlation_heatmap(corr_matrix, mic_positions, show_plot=show_plots, save_path="heatmap.png")
        plot_correlation_3d(list(corr_rows), mic_pairs, fs, show_plot=show_plots, save_path="correlation_3d.png")

    return {
        "estimated_position": position,
        "actual_position": source_position if use_simulation else None,
        "mic_positions": mic_positions,
        "correlation_metrics": correlation_metrics if analyze_correlation else None,
        "correlation_matrix": corr_matrix if visualize_correlation else None,
        "calibration_data": calibration_data,
    }
