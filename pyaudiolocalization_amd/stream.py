"""Device-resident stage chain of localize_sound_source for many frames (main.py:165-204): simulate -> synchronise ->
prefilter -> all pairs with every waveform staying in HBM.  A second entrance takes recorded audio instead of the simulation
(recorded_tdoa_stream / recorded_position_stream: resample -> normalise -> cut frames, then the same tail).  This is the streaming configuration of BASELINE.json
(64 microphones x 1024 frames of 0.25 s, multipath simulation on): the host supplies the base signals, the per-frame
path tables and the filter design, reads back five numbers per row for the synchronisation (the 5-point spline and the
integer pads of utils.py:428-451 are host scalar work) and receives the TDOA tables.

Frame lengths follow the reference: the simulated length int((duration + longest path delay) * fs) (main.py:102) and the
synchronised length N + (max shift - min shift) (utils.py:448-456) differ from frame to frame, and with them
the exact DFT lengths.  Frames are therefore grouped by those lengths and every group runs as one batched engine call;
the results are the staged host path's (simulate_signals_with_multipath -> synchronize_signals_improved ->
noise_reduction -> pair table), bit for bit - tests/test_gpu_stream.py."""
from __future__ import annotations

from collections import defaultdict
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import closure, solve
from ._ffi import RECORD
from .engine import Engine, default_engine, make_params
from .signal_processing import _filter_design
from .utils import sync_shifts_batch


def tdoa_stream(bases: Sequence[np.ndarray], delays: Sequence[np.ndarray], gains: Sequence[np.ndarray], fs: float,
                totals: Sequence[int], trim_len: int, filter_method: str = "butterworth",
                max_expected_delay: Optional[float] = None, engine: Optional[Engine] = None,
                frames_per_batch: int = 128, timings: Optional[Dict[str, float]] = None) -> Tuple[np.ndarray, np.ndarray]:
    """bases[F][nbase], delays / gains[F][M][K], totals[F] (main.py:102) -> (tables[F][P], lengths[F]); see _chain."""
    tables, lengths, _ = _chain(bases, delays, gains, fs, totals, trim_len, filter_method, max_expected_delay, engine, frames_per_batch,
                                timings, None)
    return tables, lengths


def position_stream(bases: Sequence[np.ndarray], delays: Sequence[np.ndarray], gains: Sequence[np.ndarray], fs: float,
                    totals: Sequence[int], trim_len: int, mic_positions, c: float, filter_method: str = "butterworth",
                    max_expected_delay: Optional[float] = None, engine: Optional[Engine] = None, frames_per_batch: int = 128,
                    timings: Optional[Dict[str, float]] = None, calib_delays=None, weights: str = "ones", buffer: float = 5.0,
                    grid: int = solve.GRID, max_iter: int = solve.MAX_ITER, loss: str = "linear",
                    f_scale: float = 1.0, closure_tol: int = 1, closure_min_votes: int = 1,
                    closure_mode: str = "soft") -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The chain of tdoa_stream with the position solve (solve.py) run on the table buffer while it is still in HBM:
    -> (positions[F] of solve.POSITION records, tables[F][P], lengths[F]).  Tables and lengths are tdoa_stream's; the positions are
    what Engine.solve_positions returns for those tables (``weights``: 'ones', 'snr' or 'closure'; ``loss`` / ``f_scale``: a robust loss for
    tables with outlier pairs).  ``weights='closure'``: the loop-closure check (closure.py; ``closure_tol``, ``closure_min_votes``,
    ``closure_mode``) runs on the table buffer in HBM and only its weights come down, to go into the solve as an array; a frame that
    keeps fewer than four pairs is solved like any other and its record means nothing (Engine.tdoa_closure's ``kept_pairs`` tells).
    A frame without the converged bit in ``positions["status"]`` is the caller's to hand to main.solve_positions_device / solve_position."""
    args = _solve_keywords(mic_positions, fs, c, calib_delays, weights, buffer, grid, max_iter, loss, f_scale, closure_tol, closure_min_votes,
                           closure_mode)
    tables, lengths, positions = _chain(bases, delays, gains, fs, totals, trim_len, filter_method, max_expected_delay, engine,
                                        frames_per_batch, timings, args)
    return positions, tables, lengths


def _solve_keywords(mic_positions, fs, c, calib_delays, weights, buffer, grid, max_iter, loss, f_scale, closure_tol=1, closure_min_votes=1,
                    closure_mode="soft"):
    """Keywords of Engine.solve_positions_dev for a stream, checked before any GPU work; the linear loss passes none of its own, and
    only the closure weights pass theirs."""
    if not isinstance(weights, str) or weights not in ("ones", "snr", "closure"):
        raise ValueError("weights: 'ones', 'snr' or 'closure'")
    solve.check_loss(loss, f_scale)
    args = dict(mic_positions=mic_positions, fs=fs, c=c, calib_delays=calib_delays, weights=weights, buffer=buffer, grid=grid, max_iter=max_iter)
    if weights == "closure":
        closure.check_args(1, np.asarray(mic_positions).shape[0], 1, closure_tol, closure_min_votes, closure_mode)
        args.update(closure_tol=closure_tol, closure_min_votes=closure_min_votes, closure_mode=closure_mode)
    if loss != "linear":
        args.update(loss=loss, f_scale=f_scale)
    return args


def _laps(eng, timings):
    """lap(stage): adds the seconds since the previous lap to timings[stage] (the device synchronised), nothing without timings."""
    import time
    clock = [time.perf_counter()]

    def lap(stage: str) -> None:
        if timings is None:
            return
        eng.synchronize()
        now = time.perf_counter()
        timings[stage] = timings.get(stage, 0.0) + now - clock[0]
        clock[0] = now

    return lap


def _prefilter_design(fs, filter_method):
    """(b, a, zi) of the band-pass, None for the Wiener filter (main.py:191); ValueError for an unknown method."""
    if filter_method in ("butterworth", "fir"):
        return _filter_design(fs, filter_method, 300, 3400, 101)
    if filter_method == "wiener":
        return None
    raise ValueError("Unknown filter method. Available methods: 'butterworth', 'fir', 'wiener'")


def _tail(eng, d_frames, b, m, out_len, fs, design, prm, solve_args, lap):
    """The chain behind its entrances: d_frames[b][m][out_len] in HBM -> synchronise -> align -> prefilter -> pairs [-> solve]
    -> (tables[b][P], lengths[b], positions[b] or None) on the host, in the order of the frames."""
    npairs = m * (m - 1) // 2
    ref, kpk, win, pk, refpk = eng.sync_measure_dev(d_frames, b, m, out_len)                       # utils.py:413-427
    lap("sync_measure")
    shifts = sync_shifts_batch(kpk, win, pk, refpk, ref, out_len, fs)                             # utils.py:428-446
    pads = np.maximum(0, np.rint(shifts - shifts.min(axis=1, keepdims=True))).astype(np.int32)    # utils.py:448-451
    lap("host_spline")
    # one buffer for the whole batch: the frames of one synchronised length L sit together ([frames][M][L]) so
    # that each length is one pair-table call, and ALL rows go through the prefilter in ONE launch (one lane
    # per row: a launch takes as long for 64 rows as for 65 536)
    by_len: Dict[int, List[int]] = defaultdict(list)
    for q in range(b):
        by_len[out_len + int(pads[q].max())].append(q)
    region, at_d = {}, 0
    for length, local in by_len.items():
        region[length] = at_d
        at_d += len(local) * m * length
    d_al, d_flt = eng.alloc(at_d * 8), eng.alloc(at_d * 8)
    d_tab = eng.alloc(b * npairs * RECORD.itemsize)
    tables = np.zeros((b, npairs), dtype=RECORD)
    lengths = np.zeros(b, dtype=np.int64)
    positions = np.zeros(b, dtype=solve.POSITION) if solve_args is not None else None
    try:
        offs, lens = [], []
        for length, local in by_len.items():
            base_d = region[length]
            nb = len(local)
            if local == list(range(local[0], local[0] + nb)):
                eng.align_rows_dev(d_frames + local[0] * m * out_len * 8, nb * m, out_len, pads[local].reshape(-1), length,
                                   d_al + base_d * 8)
            else:
                for i, q in enumerate(local):
                    eng.align_rows_dev(d_frames + q * m * out_len * 8, m, out_len, pads[q], length,
                                       d_al + (base_d + i * m * length) * 8)
            offs.extend(base_d + k * length for k in range(nb * m))
            lens.extend([length] * (nb * m))
        lap("align")
        if design is None:                                                                         # main.py:191
            for length, local in by_len.items():
                eng.wiener3_dev(d_al + region[length] * 8, len(local) * m, length, d_flt + region[length] * 8)
        else:
            eng.filtfilt_ragged_dev(design[0], design[1], design[2], d_al, d_flt, offs, offs, lens)
        lap("prefilter")
        row0 = 0
        for length, local in by_len.items():                                                       # main.py:202-228
            eng.gcc_phat_all_pairs_dev(d_flt + region[length] * 8, len(local), m, length, prm, d_tab + row0 * npairs * RECORD.itemsize)
            row0 += len(local)
        eng.synchronize()
        lap("pairs")
        if solve_args is not None:                                                                 # main.py:233-298
            order = [q for local in by_len.values() for q in local]
            lens_b = [length for length, local in by_len.items() for _ in local]
            positions[order] = eng.solve_positions_dev(d_tab, b, lens_b, **solve_args)
            lap("solve")
        got = np.zeros((b, npairs), dtype=RECORD)
        eng.download(got, d_tab)
        row0 = 0
        for length, local in by_len.items():
            for i, q in enumerate(local):
                tables[q] = got[row0 + i]
                lengths[q] = length
            row0 += len(local)
        lap("download")
    finally:
        eng.free(d_al); eng.free(d_flt); eng.free(d_tab)
    return tables, lengths, positions


def _chain(bases, delays, gains, fs, totals, trim_len, filter_method, max_expected_delay, engine, frames_per_batch, timings, solve_args):
    """bases[F][nbase], delays / gains[F][M][K], totals[F] (main.py:102) -> (tables[F][P], lengths[F]): the simulation in front
    of _tail.

    ``trim_len`` = int(duration * fs) (main.py:119-120).  ``frames_per_batch`` bounds the HBM held by one batch
    (waveforms of a batch: 3 buffers of frames x M x L doubles).  ``timings`` (diagnostics): a dict that receives the
    seconds spent per stage; the device is synchronised at every stage boundary while it is given."""
    eng = engine or default_engine()
    lap = _laps(eng, timings)
    nf = len(bases)
    if not (len(delays) == len(gains) == len(totals) == nf) or nf == 0:
        raise ValueError("one base, path table and total length per frame")
    m, k = np.asarray(delays[0]).shape
    npairs = m * (m - 1) // 2
    prm = make_params(fs, 1, "median", 1.0, max_expected_delay)
    design = _prefilter_design(fs, filter_method)
    tables = np.zeros((nf, npairs), dtype=RECORD)
    lengths = np.zeros(nf, dtype=np.int64)
    positions = np.zeros(nf, dtype=solve.POSITION) if solve_args is not None else None

    def out_len_of(total: int) -> int:
        return trim_len if 0 < trim_len < total else total

    by_out: Dict[int, List[int]] = defaultdict(list)                       # frames whose simulated rows have one length
    for f in range(nf):
        by_out[out_len_of(int(totals[f]))].append(f)
    # Every distinct simulated length and every synchronised length is a transform plan (8-16 MB each), and the batches visit them in
    # the same order again and again - the worst case for a least-recently-used cache that is smaller than the working set.
    # The bound follows the workload: simulated lengths + as many synchronised lengths + the correlations of the
    # synchronisation, with room to spare.
    eng.set_max_plans(min(4096, max(64, 3 * len(set(int(t) for t in totals)) + 32)))
    for out_len, members in by_out.items():
        for at in range(0, len(members), frames_per_batch):
            group = members[at: at + frames_per_batch]
            b = len(group)
            d_sim = eng.alloc(b * m * out_len * 8)
            try:
                # ---- simulate (main.py:165): frames that share the transform length 2 * total go through one call
                by_total: Dict[Tuple[int, int], List[int]] = defaultdict(list)
                for q, f in enumerate(group):
                    by_total[(int(totals[f]), len(bases[f]))].append(q)
                for (total, nbase), local in by_total.items():
                    base = np.ascontiguousarray([bases[group[q]] for q in local], dtype=np.float64)
                    dl = np.ascontiguousarray([delays[group[q]] for q in local], dtype=np.float64)
                    gn = np.ascontiguousarray([gains[group[q]] for q in local], dtype=np.float64)
                    d_base, d_dl, d_gn = eng.alloc(base.nbytes), eng.alloc(dl.nbytes), eng.alloc(gn.nbytes)
                    contiguous = local == list(range(local[0], local[0] + len(local)))
                    d_part = d_sim + local[0] * m * out_len * 8 if contiguous else eng.alloc(len(local) * m * out_len * 8)
                    try:
                        eng.upload(d_base, base); eng.upload(d_dl, dl); eng.upload(d_gn, gn)
                        eng.simulate_multipath_dev(d_base, len(local), nbase, fs, total, d_dl, d_gn, m, k, trim_len, d_part)
                        if not contiguous:                    # frames of this length are scattered over the batch: move them home
                            zero = np.zeros(m, dtype=np.int32)
                            for i, q in enumerate(local):
                                eng.align_rows_dev(d_part + i * m * out_len * 8, m, out_len, zero, out_len, d_sim + q * m * out_len * 8)
                        eng.synchronize()
                    finally:
                        eng.free(d_base); eng.free(d_dl); eng.free(d_gn)
                        if not contiguous:
                            eng.free(d_part)
                lap("simulate")
                got, lens, pos = _tail(eng, d_sim, b, m, out_len, fs, design, prm, solve_args, lap)
                tables[group], lengths[group] = got, lens
                if pos is not None:
                    positions[group] = pos
            finally:
                eng.free(d_sim)
    return tables, lengths, positions


# ---------------------------------------------------------------- recorded audio
def frame_count(t: int, frame_len: int, hop: int) -> int:
    """Frames of frame_len samples every hop samples that lie wholly inside t samples."""
    return (int(t) - int(frame_len)) // int(hop) + 1


def frame_rows(rows: np.ndarray, frame_len: int, hop: int) -> np.ndarray:
    """rows[M][T] -> frames[F][M][frame_len], frames[f][m] = rows[m][f * hop : f * hop + frame_len] (what frame_rows_dev gathers)."""
    rows = np.asarray(rows)
    count = frame_count(rows.shape[1], frame_len, hop)
    return np.stack([rows[:, f * hop: f * hop + frame_len] for f in range(count)])


def _check_recorded(recordings, fs_in, fs, frame_len, hop, filter_method):
    """Input checks of the recorded entrances (before any GPU work) -> (rows[M][T_in] float64, T after resampling, design)."""
    rows = [np.asarray(r, dtype=np.float64) for r in recordings]
    if len(rows) < 2:
        raise ValueError("a recording needs at least two microphones")
    if any(r.ndim != 1 for r in rows) or len({r.shape[0] for r in rows}) != 1:
        raise ValueError("every microphone row must be one-dimensional and of the same length")
    if int(hop) < 1:
        raise ValueError("hop must be at least one sample")
    if int(frame_len) < 1:
        raise ValueError("frame_len must be at least one sample")
    design = _prefilter_design(fs, filter_method)
    t_in = rows[0].shape[0]
    if fs_in == fs:
        t = t_in
    else:
        ratio = float(fs) / float(fs_in)
        if ratio <= 0:
            raise ValueError("Invalid sample rates")
        t = int(t_in * ratio)
    if int(frame_len) > t:
        raise ValueError(f"frame_len={frame_len} is longer than the recording ({t} samples at {fs} Hz)")
    return np.ascontiguousarray(rows), t, design


def _recorded(recordings, fs_in, fs, frame_len, hop, filter_method, max_expected_delay, engine, frames_per_batch, timings, solve_args):
    """recordings[M][T_in] at fs_in -> upload once -> resample to fs (skipped when fs_in == fs) -> normalise and compress each
    microphone row over the whole recording (as read_audio_files does per file) -> frames of frame_len every hop -> _tail."""
    rows, t, design = _check_recorded(recordings, fs_in, fs, frame_len, hop, filter_method)
    frame_len, hop, frames_per_batch = int(frame_len), int(hop), max(1, int(frames_per_batch))
    m, t_in = rows.shape
    nf = frame_count(t, frame_len, hop)
    npairs = m * (m - 1) // 2
    eng = engine or default_engine()
    lap = _laps(eng, timings)
    prm = make_params(fs, 1, "median", 1.0, max_expected_delay)
    tables = np.zeros((nf, npairs), dtype=RECORD)
    lengths = np.zeros(nf, dtype=np.int64)
    positions = np.zeros(nf, dtype=solve.POSITION) if solve_args is not None else None
    eng.set_max_plans(min(1024, max(64, nf + 32)))             # one plan per synchronised length: at most one per frame (see _chain)
    held = [eng.alloc(rows.nbytes)]
    try:
        eng.upload(held[0], rows)
        lap("upload")
        if fs_in != fs:
            held.append(eng.alloc(m * t * 8))
            eng.resample_dev(held[0], m, t_in, fs_in, fs, held[1], t)
            lap("resample")
        d_rows = held[-1]
        eng.normalize_compress_dev(d_rows, m, t, d_rows)                                            # utils.py:476
        lap("normalize")
        for at in range(0, nf, frames_per_batch):
            b = min(frames_per_batch, nf - at)
            d_fr = eng.alloc(b * m * frame_len * 8)
            try:
                eng.frame_rows_dev(d_rows, m, t, frame_len, hop, at, b, d_fr)
                lap("frames")
                got, lens, pos = _tail(eng, d_fr, b, m, frame_len, fs, design, prm, solve_args, lap)
                tables[at: at + b], lengths[at: at + b] = got, lens
                if pos is not None:
                    positions[at: at + b] = pos
            finally:
                eng.free(d_fr)
    finally:
        for d in held:
            eng.free(d)
    return tables, lengths, positions


def recorded_tdoa_stream(recordings, fs_in: float, fs: float, frame_len: int, hop: int, filter_method: str = "butterworth",
                         max_expected_delay: Optional[float] = None, engine: Optional[Engine] = None, frames_per_batch: int = 128,
                         timings: Optional[Dict[str, float]] = None) -> Tuple[np.ndarray, np.ndarray]:
    """A multi-microphone recording recordings[M][T_in] sampled at fs_in -> (tables[F][P], lengths[F]) for the
    F = (T - frame_len) // hop + 1 frames of frame_len samples every hop samples at fs (T = int(T_in * fs / fs_in)); see _recorded.
    The result is the staged path's (Engine.resample -> normalize_compress -> NumPy framing -> synchronize_signals_improved ->
    noise_reduction_rows -> main.tdoa_table per frame), bit for bit - tests/test_gpu_recorded.py."""
    tables, lengths, _ = _recorded(recordings, fs_in, fs, frame_len, hop, filter_method, max_expected_delay, engine, frames_per_batch,
                                   timings, None)
    return tables, lengths


def recorded_position_stream(recordings, fs_in: float, fs: float, frame_len: int, hop: int, mic_positions, c: float,
                             filter_method: str = "butterworth", max_expected_delay: Optional[float] = None,
                             engine: Optional[Engine] = None, frames_per_batch: int = 128, timings: Optional[Dict[str, float]] = None,
                             calib_delays=None, weights: str = "ones", buffer: float = 5.0, grid: int = solve.GRID,
                             max_iter: int = solve.MAX_ITER, loss: str = "linear",
                             f_scale: float = 1.0, closure_tol: int = 1, closure_min_votes: int = 1,
                             closure_mode: str = "soft") -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """recorded_tdoa_stream with the position solve of position_stream on each batch's tables while they are in HBM:
    -> (positions[F] of solve.POSITION records, tables[F][P], lengths[F]).  ``weights='closure'`` and its keywords: as position_stream
    (a frame that keeps fewer than four pairs is solved like any other and its record means nothing)."""
    args = _solve_keywords(mic_positions, fs, c, calib_delays, weights, buffer, grid, max_iter, loss, f_scale, closure_tol, closure_min_votes,
                           closure_mode)
    tables, lengths, positions = _recorded(recordings, fs_in, fs, frame_len, hop, filter_method, max_expected_delay, engine,
                                           frames_per_batch, timings, args)
    return positions, tables, lengths
