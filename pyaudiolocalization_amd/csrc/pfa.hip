// pfa.hip - prime-factor route of the inverse PHAT transform (gfx950, fp64).
//
// numpy.fft.ifft at the exact length n = n1 + n2 - 1 (utils.py:118) is where the reference spends its time.
// The four-step chirp convolution of bluestein.hip works for every n but moves a 2n-point workspace through
// HBM three times.  When n = N1 x N2 with coprime odd factors, N1 <= 127 and N2 <= 2048 (the headline length
// 2 * 44100 - 1 = 88199 = 89 x 991 is such an n), the Chinese-remainder map k <-> (k mod N1, k mod N2) on the
// frequency side turns the length-n DFT into independent short DFTs:
//
//   c[m2 + N2 t] = 1/n  sum_k1 e^(2 pi i k1 t / N1) * e^(2 pi i u1 k1 m2 / N1) * sum_k2 e^(2 pi i u2 k2 m2 / N2) x[k1, k2]
//                       '------ k_pfa_cols: dense N1-point DFT ------'   '------ k_pfa_rows: N2-point DFT + twiddle ------'
//
// (u1 = N2^-1 mod N1, u2 = N1^-1 mod N2).  The N2-point DFTs are convolutions that live entirely in LDS - Rader's cyclic
// convolution of N2 - 1 points where N2 = 991 (pfa_rader.h: 990 = 9 x 10 x 11, twiddle-free prime-factor stages), else a
// chirp convolution of length M = 2^lm >= 2 N2 - 1 (pfa_kernels.h: forward FFT, multiply by the chirp spectrum, inverse
// FFT, two tiles per workgroup) - and the N1-point DFTs are real cos / sin contractions whose coefficients are wave-uniform and
// come through the scalar cache.  A transform touches HBM twice (16 B/point each way) instead of three times
// at twice the points, and the output index m = m2 + N2 t is the natural one, so the correlation rows are
// written in coalesced runs.
//
// As in bluestein.hip one complex transform carries two mic pairs (real part = pair p, imaginary part = pair q)
// and the whitened cross spectrum R = S_a conj(S_b) / (|.| + 1e-10) (utils.py:116-117) is built inside the
// first FFT stage.  The mic spectra arrive in the permuted layout SP[mic][k1][k2], k1 <= (N1-1)/2 (written by the
// forward transform: pfa_forward.h for Rader rows - the same cut, transposed - or the storer of the four-step route,
// bluestein.hip PermSpectrumStorer): row N1-k1
// is row k1 reversed and conjugated (Hermitian symmetry), so one workgroup serves both rows from the same
// loads - tile 0 transforms x[k1, e], tile 1 the reversed row z[e] = x[N1-k1, -e], whose DFT is the reversed DFT.
#include <cmath>
#include <cstdlib>
#include <vector>

#include "pfa_kernels.h"
#include "pfa_rader.h"
#include "pfa_cols_stats.h"
#include "pfa_cols_fin.h"
#include "pfa_forward.h"
#include "pfa_big.h"

namespace pal {

// points per lane of the register-resident row tiles (pfa_big.h); the build can override them for A/B runs
#ifndef PAL_BIG13_PTS
#define PAL_BIG13_PTS 32
#endif
#ifndef PAL_BIG14_PTS
#define PAL_BIG14_PTS 32
#endif
constexpr int kBig13 = PAL_BIG13_PTS, kBig14 = PAL_BIG14_PTS;

// ------------------------------------------------------------------ plan
// plan_geometry.h is host-only and restates what it needs of the kernels' constants and types
static_assert(kColChunk == kPfaTC && kColUnroll == kPfaUnr && kRader89 == kR89, "plan_geometry.h against the column pass's constants");
static_assert(sizeof(RowStep) == sizeof(int2) && sizeof(Cplx) == sizeof(cd), "plan_geometry.h tables are uploaded as they are");

void Engine::free_pfa(Pfa& f) {
  if (f.b) (void)hipFree(f.b);
  if (f.hhat) (void)hipFree(f.hhat);
  if (f.r1) (void)hipFree(f.r1);
  if (f.T) (void)hipFree(f.T);
  if (f.rowtab) (void)hipFree(f.rowtab);
  if (f.r89_tab) (void)hipFree(f.r89_tab);
  for (void* p : {(void*)f.rd_bhat, (void*)f.rd_bhat_f, (void*)f.rd_qidx,
                  (void*)f.rd_ridx})
    if (p) (void)hipFree(p);
  f = Pfa();
}

#define PAL_SWITCH_LM(lm, ...)                                     \
  switch (lm) {                                                    \
    case 9: { constexpr int LM = 9; __VA_ARGS__; } break;          \
    case 10: { constexpr int LM = 10; __VA_ARGS__; } break;        \
    case 11: { constexpr int LM = 11; __VA_ARGS__; } break;        \
    case 12: { constexpr int LM = 12; __VA_ARGS__; } break;        \
    default: return fail(PAL_ERR_INTERNAL, "prime-factor plan with log2 M = %d", lm); \
  }

// host table -> a device allocation of its own
template <class T, class D> static int upload_table(Engine* e, const std::vector<T>& host, D** dev) {
  static_assert(sizeof(T) == sizeof(D), "uploaded as it is");
  if (hipMalloc(dev, host.size() * sizeof(T)) != hipSuccess) return e->fail(PAL_ERR_NOMEM, "prime-factor tables");
  return e->check(hipMemcpy(*dev, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice), "prime-factor tables");
}

// split (plan_geometry.h) -> allocations and uploads -> setup launches, all into pl.pfa: a failure on the way leaves what exists of
// the cut where get_plan's cleanup frees it
int Engine::build_pfa(Plan& pl) {
  Pfa& f = pl.pfa;
  f = Pfa();
  static_cast<PfaSplit&>(f) = pfa_split(pl.n, pl.nout, pl.inv.g, plan_sw);
  if (!f.on()) return PAL_OK;
  const cd* tws = stage_table(f.lm, f.lm == 11 || f.lm == 12);
  if (!tws || !stage_table(f.lm)) return fail(PAL_ERR_NOMEM, "twiddle tables");   // (the full table feeds the register twiddles)
  PAL_HIP(hipMalloc(&f.b, sizeof(cd) * f.n2));
  PAL_HIP(hipMalloc(&f.hhat, sizeof(cd) << f.lm));
  PAL_HIP(hipMalloc(&f.r1, sizeof(cd) * f.n1));
  k_make_chirp<<<dim3((f.n2 + 255) / 256), dim3(256), 0, stream>>>(f.b, f.n2, int(f.u2));
  k_make_roots<<<dim3((f.n1 + 255) / 256), dim3(256), 0, stream>>>(f.r1, f.n1, double(f.n1));
  const double scale = 1.0 / (double(1 << f.lm) * double(pl.n));   // inverse FFT_M and numpy.fft.ifft's 1/n
  if (f.lm == 13) k_pfa_hhat_big<13, kBig13><<<dim3(1), dim3(BigTile<13, kBig13>::kLanes), 0, stream>>>(f.b, f.n2, f.hhat, scale, tws);
  else if (f.lm == 14) k_pfa_hhat_big<14, kBig14><<<dim3(1), dim3(BigTile<14, kBig14>::kLanes), 0, stream>>>(f.b, f.n2, f.hhat, scale, tws);
  else PAL_SWITCH_LM(f.lm, k_pfa_hhat<LM><<<dim3(1), dim3(PfaLds<LM>::kLanes), 0, stream>>>(f.b, f.n2, f.hhat, scale, tws));
  PAL_HIP(hipGetLastError());
  PAL_TRY(upload_table(this, pfa_row_table(f.n1, f.u1, stage_tw_last(f.lm)), &f.rowtab));
  PAL_TRY(upload_table(this, pfa_col_table(f.n1, f.nch), &f.T));
  if (f.rader) PAL_TRY(build_rader(f, pl.n, f.u2 % f.n2));
  if (f.r89) {                                                 // the 89-point column DFT as Rader's 8 x 11 convolution (pfa_rader89.h)
    Rader89Tab tab;
    make_rader89_tab(tab);
    PAL_HIP(hipMalloc(&f.r89_tab, sizeof tab));
    PAL_HIP(hipMemcpy(f.r89_tab, &tab, sizeof tab, hipMemcpyHostToDevice));
  }
  return PAL_OK;
}

// Rader tables of the prime N2 = f.n2 (pfa_rader.h): generator re-indexing into prime-factor positions (mixed_radix.h) and the 3-D
// spectra of the kernel sequences w^(g^s), w = exp(+/- 2 pi i u2 / N2)
int Engine::build_rader(Pfa& f, long long n, long long u2) {
  const RaderIndex ix = rader_index(f.n2, [](int s) { return Axes<kRaderR1, kRaderR2, kRaderR3>::pos(s); });
  if (!ix.g) return fail(PAL_ERR_INTERNAL, "no primitive root of %d", f.n2);
  const RaderSpectra sp = rader_spectra(f.n2, n, u2, ix.gpow);
  PAL_TRY(upload_table(this, sp.inv, &f.rd_bhat));
  PAL_TRY(upload_table(this, sp.fwd, &f.rd_bhat_f));
  PAL_TRY(upload_table(this, ix.qidx, &f.rd_qidx));
  PAL_TRY(upload_table(this, ix.ridx, &f.rd_ridx));
  return PAL_OK;
}

int Engine::pfa_rows(const Plan& pl, const cd* permuted, const int4* quads, int G, cd* Y, hipStream_t on) {
  const Pfa& f = pl.pfa;
  const cd* tws = stage_table(f.lm, f.lm >= 11);
  if (f.rader) {
    ProfScope ps(this, "k_pfa_rows_rader<11,9,10>", on);
    PfaRaderArgs a{permuted, quads, Y, f.rd_bhat, f.r1, f.rd_ridx, f.rowtab,
                   f.n1, f.n2, f.rows(), G, 1.0f / float(f.n1), 1.0 / double(pl.n), nullptr, xcd_rows, rows_shared};
    k_pfa_rows_rader<11, 9, 10><<<dim3(row_work_grid(G, f.rows(), xcd_rows)), dim3(256), 0, on>>>(a);
    PAL_HIP(hipGetLastError());
  } else if (f.lm >= 13) {
    char name[48];
    snprintf(name, sizeof name, "k_pfa_rows_big<%d>", f.lm);
    ProfScope ps(this, name, on);
    PfaRowsArgs a{permuted, quads, Y, f.b, f.hhat, f.r1, stage_table(f.lm), stage_table(f.lm), f.rowtab, f.n1, f.n2, f.rows(), G, f.u1, 1.0f / float(f.n1), nullptr, xcd_rows};
    const unsigned grid = row_work_grid(G, f.n1, xcd_rows);    // one workgroup per row of Y
    if (f.lm == 13) k_pfa_rows_big<13, kBig13><<<dim3(grid), dim3(BigTile<13, kBig13>::kLanes), 0, on>>>(a);
    else k_pfa_rows_big<14, kBig14><<<dim3(grid), dim3(BigTile<14, kBig14>::kLanes), 0, on>>>(a);
    PAL_HIP(hipGetLastError());
  } else {
    char name[48];
    snprintf(name, sizeof name, "k_pfa_rows<%d>", f.lm);
    ProfScope ps(this, name, on);
    PfaRowsArgs a{permuted, quads, Y, f.b, f.hhat, f.r1, tws, stage_table(f.lm), f.rowtab, f.n1, f.n2, f.rows(), G, f.u1, 1.0f / float(f.n1), nullptr, xcd_rows};
    const unsigned grid = row_work_grid(G, f.rows(), xcd_rows);
    PAL_SWITCH_LM(f.lm, k_pfa_rows<LM><<<dim3(grid), dim3(PfaLds<LM>::kLanes), 0, on>>>(a));
    PAL_HIP(hipGetLastError());
  }
  return PAL_OK;
}

int Engine::pfa_pair_group(const Plan& pl, const cd* permuted, const int4* quads, int G, cd* Y, double* corr, size_t stride,
                           const int* zero_rows, hipStream_t on) {
  const Pfa& f = pl.pfa;
  PAL_TRY(pfa_rows(pl, permuted, quads, G, Y, on));
  {
    ProfScope ps(this, "k_pfa_cols", on);
    const unsigned nblk = unsigned(f.n2 + 63) / 64;
    k_pfa_cols<kPfaTC, kPfaUnr><<<dim3(unsigned(G) * nblk, unsigned(f.nch + 3) / 4), dim3(256), 0, on>>>(Y, corr, stride, f.n1,
                                                                                                     f.n2, G, f.nch, f.T, zero_rows);
    PAL_HIP(hipGetLastError());
  }
  return PAL_OK;
}

// Forward spectra of `rows` real frames through the prime-factor cut (pfa_forward.h): two frames per transform, column
// DFTs into the workspace, Rader rows into the SP layout.  Applies to plans with Rader rows and frames that leave the
// upper half of the n points empty (len <= N2 (h + 1)).
bool Engine::pfa_forward_applies(const Plan& pl, int len) const {
  const Pfa& f = pl.pfa;
  return pfa_forward && f.on() && f.rader && f.nch >= 1 && (len - 1) / f.n2 <= (f.n1 - 1) / 2;
}

// `flags` (optional): the flag words k_row_nonzero wrote for these frames; they carry the exponents of the row rescale.
int Engine::pfa_forward_spectra(Plan& pl, const double* frames, size_t frame_stride, int rows, int len, cd* spectra, const int* flags) {
  const Pfa& f = pl.pfa;
  cd* Y = nullptr;
  PAL_TRY(scratch(kWsWork, size_t(chunk) * size_t(pl.n) * sizeof(cd), &Y));
  for (int r0 = 0; r0 < rows; r0 += 2 * chunk) {
    const int R = rows - r0 < 2 * chunk ? rows - r0 : 2 * chunk;   // frames of this group, two per transform
    const int G = (R + 1) / 2;
    {
      ProfScope ps(this, "k_pfa_fwd_cols", stream);
      const PfaFwdColsArgs a{frames + size_t(r0) * frame_stride, frame_stride, len, R, Y, f.T, f.n1, f.n2, G, f.nch,
                             flags ? flags + r0 : nullptr};
      const unsigned nblk = unsigned(f.n2 + 63) / 64;
      k_pfa_fwd_cols<kPfaTC, kPfaUnr><<<dim3(unsigned(G) * nblk, unsigned(f.nch + 3) / 4), dim3(256), 0, stream>>>(a);
      PAL_HIP(hipGetLastError());
    }
    {
      ProfScope ps(this, "k_pfa_fwd_rows_rader<11,9,10>", stream);
      const PfaFwdRowsArgs a{Y, spectra + size_t(r0) * pl.spec_stride(), f.rd_bhat_f, f.r1,
                             f.rd_qidx, f.rowtab, f.n1, f.n2, f.rows(), G, R, 1.0f / float(f.n1), flags ? flags + r0 : nullptr};
      k_pfa_fwd_rows_rader<11, 9, 10><<<dim3(unsigned(G) * unsigned(f.rows())), dim3(256), 0, stream>>>(a);
      PAL_HIP(hipGetLastError());
    }
  }
  return PAL_OK;
}

// row pass, column pass + streaming statistics (every column block publishes a histogram window around its median),
// finish: the peak selection of one launch group without a pivot launch, without bracket lists and without the separate
// read of its correlation rows (pfa_cols_stats.h)
int Engine::pfa_pair_group_fused(const Plan& pl, const cd* permuted, const int4* quads, int G, int rows, cd* Y, double* corr, size_t stride,
                                 const int* zero_rows, const pal_phat_params& prm, int n2, pal_pair_record* table, int32_t* ksel_multi,
                                 int slot, double* hsel_multi) {
  const Pfa& f = pl.pfa;
  const hipStream_t on = stream_of(slot);
  // short column DFTs (one chunk: N1 <= 23): the four wavefronts of a workgroup take four neighbouring strips
  const bool shortcols = f.nch <= 1;
  const int nblk = fin_blocks(f.n2, f.nch);
  PeakArgs a;
  PAL_TRY(peaks_setup(corr, stride, rows, pl.n, n2, prm, nblk, f.n2, slot, a));
  PAL_TRY(pfa_rows(pl, permuted, quads, G, Y, on));
  {
    ProfScope ps(this, "k_pfa_cols_stats", on);
    const dim3 grid(unsigned(G) * unsigned(nblk));
    const bool full = (f.n1 - 1) / 2 == f.nch * kPfaTC;          // every chunk index exists (N1 = 89: 44 = 4 x 11)
    const bool adaptive = a.method > 0;
    const int nw = f.nch == 2 ? 2 : 4;                         // wavefronts per workgroup = chunks (three chunks: the fourth wavefront idles) or strips
#define PAL_COLS_STATS(AD, FU, NW, ST) k_pfa_cols_stats<kPfaTC, kPfaUnr, AD, FU, NW, ST><<<grid, dim3(64 * NW), 0, on>>>(Y, corr, stride, f.n1, f.n2, G, f.nch, f.T, zero_rows, a, rows)
#define PAL_COLS_STATS_NW(AD, FU) do { if (shortcols) PAL_COLS_STATS(AD, false, 4, true); else if (nw == 2) PAL_COLS_STATS(AD, FU, 2, false); else PAL_COLS_STATS(AD, FU, 4, false); } while (0)
    if (f.r89 && full && nw == 4 && !shortcols) {
      const Rader89Tab* tab = static_cast<const Rader89Tab*>(f.r89_tab);
      if (adaptive) k_pfa_cols_stats<kPfaTC, kPfaUnr, true, true, 4, false, true><<<grid, dim3(256), 0, on>>>(Y, corr, stride, f.n1, f.n2, G, f.nch, f.T, zero_rows, a, rows, tab);
      else k_pfa_cols_stats<kPfaTC, kPfaUnr, false, true, 4, false, true><<<grid, dim3(256), 0, on>>>(Y, corr, stride, f.n1, f.n2, G, f.nch, f.T, zero_rows, a, rows, tab);
    } else if (adaptive) { if (full) PAL_COLS_STATS_NW(true, true); else PAL_COLS_STATS_NW(true, false); }
    else { if (full) PAL_COLS_STATS_NW(false, true); else PAL_COLS_STATS_NW(false, false); }
#undef PAL_COLS_STATS_NW
#undef PAL_COLS_STATS
    PAL_HIP(hipGetLastError());
  }
  return peaks_finish(a, rows, table, ksel_multi, slot, hsel_multi);
}

// ---- the column pass that finishes the rows itself (pfa_cols_fin.h, pfa_fin_lean.h): no correlation rows in HBM, no finish launch ----

// The blocks of a finishing pass wait for their siblings (pfa_cols_fin.h).  ONE such launch is deadlock-free (its workgroups are
// dispatched in order and siblings are adjacent), but two of them on different streams can fill every workgroup slot of the
// device with blocks that wait for siblings which then find no slot (seen with 34 blocks per transform, two per CU, three
// streams).  The kernel's waits are bounded and a block that gives up only sends its rows through the
// stored-row path, so this costs time, never correctness.  PAL_FIN_SERIAL=1 runs the finishing launches one at a time
// instead (each waits for the previous one's end, wherever that ran): no such stall can happen, 10 % slower on the metric run.
int Engine::fin_serialize(hipStream_t on) {
  if (fin_serial && fin_pending) PAL_HIP(hipStreamWaitEvent(on, ev_fin, 0));
  return PAL_OK;
}
int Engine::fin_done(hipStream_t on) {
  if (!fin_serial) return PAL_OK;
  PAL_HIP(hipEventRecord(ev_fin, on));
  fin_pending = true;
  return PAL_OK;
}

// arguments and scratch of one launch of the finishing pass, nblk blocks per transform; `grid_rows`: the rows of the grid whose first
// and last columns go to the finishing wavefront (the prime-factor grid's N1; k_rows_lean has no such columns: 1)
int Engine::fin_setup(const Plan& pl, int rows, int nblk, int grid_rows, const pal_phat_params& prm, int n2, pal_pair_record* table,
                      int* need, int slot, PeakArgs& a, FinArgs& fa, unsigned& nwg, int G) {
  const int n = pl.n;
  PAL_TRY(peaks_setup(nullptr, 0, rows, n, n2, prm, nblk, 0, slot, a));
  // per-stream scratch of the finishing pass: [done words G x blocks | emax | parts | edge] (fin_scratch.h)
  // (`done` words and FinPartial entries: room for one per WAVEFRONT of a block, pfa_fin_lean.h)
  const FinLayout lay = fin_layout(pair_group(n), nblk, grid_rows);
  char* base = nullptr;
  PAL_TRY(scratch(fin_scratch_slot(slot), lay.total, &base));
  PAL_TRY(status_words(&fa.status));
  fa.table = table;
  fa.need = need;
  fa.done = reinterpret_cast<unsigned*>(base);
  // launch number of this stream's scratch: entries of earlier launches of the same layout fail the comparison.  Another layout
  // (or a block that grew), or a number that would outgrow a double's integers, zeroes the whole block and starts again at 1
  FinKey key;
  key.gmax = pair_group(n);
  key.nblk = nblk;
  key.grid_rows = grid_rows;
  key.block = ws_bytes[fin_scratch_slot(slot)];
  if (fin_must_zero(fin_key[slot], key, fin_epoch[slot], fin_wrap)) {
    PAL_HIP(hipMemsetAsync(base, 0, key.block, stream_of(slot)));
    fin_key[slot] = key;
    fin_epoch[slot] = 0;
  }
  fa.epoch = ++fin_epoch[slot];
  fa.emax = reinterpret_cast<double*>(base + lay.off_emax);
  fa.parts = reinterpret_cast<FinPartial*>(base + lay.off_parts);
  fa.edge = reinterpret_cast<double*>(base + lay.off_edge);
  fa.giveup = fin_giveup;
  // the lag window |m - (n2 - 1)| / fs <= max_expected_delay (utils.py:163) as sample indices, with the reference's arithmetic
  fa.pw = 1;
  fa.corr = nullptr;
  fa.stride = 0;
  fa.store_rows = 0;
  fa.strip = nullptr;                                          // (the strip form is pfa_pair_group_fin's choice)
  fa.st = fin_no_strip();
  fa.grid = nullptr;
  fa.roots = nullptr;
  fa.zero_rows = nullptr;
  fa.windowed = std::isnan(prm.max_expected_delay) ? 0 : 1;
  fa.win_lo = 1;
  fa.win_hi = n - 2;
  if (fa.windowed) {
    const double med = prm.max_expected_delay, fs = prm.fs;
    long long k = -1;
    if (med >= 0) {
      const double est = med * fs;
      k = est < double(n) ? (long long)est + 2 : (long long)n;
      while (k >= 0 && !(std::fabs(double(k) / fs) <= med)) --k;
    }
    if (k < 0) { fa.win_lo = 1; fa.win_hi = 0; }
    else {
      const long long lo = (long long)(n2 - 1) - k, hi = (long long)(n2 - 1) + k;
      fa.win_lo = int(lo < 1 ? 1 : lo);
      fa.win_hi = int(hi > n - 2 ? n - 2 : hi);
    }
  }
  fa.cheb = a.method == 0 && nohist(prm.threshold_method, prm.threshold_multiplier) ? 1 : 0;
  nwg = 8u * unsigned((G + 7) / 8) * unsigned(nblk);
  return PAL_OK;
}

// Statistics of rows that are already in HBM, any route (k_rows_lean, RouteStats::kRowsLean of pair_route.h)
int Engine::rows_lean_group(const Plan& pl, const double* corr, size_t stride, int G, int rows, const pal_phat_params& prm, int n2,
                            pal_pair_record* table, int* need, int slot) {
  constexpr int NS = 22;
  const hipStream_t on = stream_of(slot);
  const int chunks = (pl.n + kColsOwn - 1) / kColsOwn;
  const int nblk = (chunks + 4 * NS - 1) / (4 * NS);
  PeakArgs a;
  FinArgs fa;
  unsigned nwg = 0;
  PAL_TRY(fin_setup(pl, rows, nblk, 1, prm, n2, table, need, slot, a, fa, nwg, G));
  fa.pw = 4;
  fa.corr = const_cast<double*>(corr);
  fa.stride = stride;
  ProfScope ps(this, "k_rows_lean", on);
  k_rows_lean<NS><<<dim3(nwg), dim3(256), 0, on>>>(corr, stride, G, nblk, a, fa, rows);
  PAL_HIP(hipGetLastError());
  return PAL_OK;
}

// The finishing column pass (RouteTransform::kFinish), and the same pass with the correlation rows stored as well (kLeanStore: `corr`)
int Engine::pfa_pair_group_fin(const Plan& pl, const cd* permuted, const int4* quads, int G, int rows, cd* Y, const int* zero_rows,
                               const pal_phat_params& prm, int n2, pal_pair_record* table, int* need, int slot,
                               double* corr, size_t stride) {
  const Pfa& f = pl.pfa;
  const hipStream_t on = stream_of(slot);
  const bool shortcols = f.nch <= 1;                           // short column DFTs (N1 <= 23): the four wavefronts of a block are four strips
  const int nblk = fin_blocks(f.n2, f.nch);
  PeakArgs a;
  FinArgs fa;
  unsigned nwg = 0;
  PAL_TRY(fin_setup(pl, rows, nblk, f.n1, prm, n2, table, need, slot, a, fa, nwg, G));
  fa.corr = corr;
  fa.stride = stride;
  fa.store_rows = corr ? 1 : 0;
  PAL_TRY(pfa_rows(pl, permuted, quads, G, Y, on));
  {
    ProfScope ps(this, corr ? "k_pfa_cols_lean" : "k_pfa_cols_fin", on);
    const dim3 grid(nwg);
    const bool full = (f.n1 - 1) / 2 == f.nch * kPfaTC;
    // histograms only where fin_decide's bound on the median (from sum x^2, the maximum set apart) cannot decide: multipliers above 2 (or negative)
    const bool hist = !(a.method > 0 || fa.cheb);
    const int nw = f.nch == 2 ? 2 : (f.nch == 3 && !hist ? 3 : 4);   // (three chunks: three wavefronts where the statistics are per wavefront)
    FinSrc src{Y, f.T, static_cast<const Rader89Tab*>(f.r89_tab)};
    // Strip form of the per-wavefront statistics (pair_route.h fin_strip): one strip buffer per launch-group slot, [2 x pair_group(n)]
    // [strip_len] doubles.  It is written in full by every launch that reads it and read only behind that launch's `done` words, so it
    // carries no epoch, is never zeroed and has no place in FinKey.
    const FinStrip st = fin_strip(pl.n, fa.windowed != 0, fa.win_lo, fa.win_hi, a.snr_w, !corr && !hist, fin_strip_on);
    if (st.on()) {
      PAL_TRY(scratch(fin_strip_slot(slot), size_t(2 * pair_group(pl.n)) * size_t(st.len) * sizeof(double), &fa.strip));
      fa.st = st;
      fa.grid = Y;
      fa.roots = f.r1;
      fa.zero_rows = zero_rows;
    }
    const bool strip = fa.strip != nullptr;
    PAL_TRY(fin_serialize(on));
    // (HI = false: the per-wavefront statistics, in the polling or the strip form)
#define PAL_COLS_FIN(MODE, HI, FU, NW) do { \
      if (!HI && strip) k_pfa_cols_fin<MODE, kPfaTC, kPfaUnr, HI, FU, NW, !HI><<<grid, dim3(64 * NW), 0, on>>>(src, f.n1, f.n2, G, f.nch, nblk, zero_rows, a, fa, rows); \
      else k_pfa_cols_fin<MODE, kPfaTC, kPfaUnr, HI, FU, NW, false><<<grid, dim3(64 * NW), 0, on>>>(src, f.n1, f.n2, G, f.nch, nblk, zero_rows, a, fa, rows); } while (0)
#define PAL_COLS_FIN_FU(MODE, HI, NW) do { if (full) PAL_COLS_FIN(MODE, HI, true, NW); else PAL_COLS_FIN(MODE, HI, false, NW); } while (0)
    if (!hist) fa.pw = shortcols ? 4 : nw;                    // one FinPartial / `done` word per wavefront (pfa_fin_lean.h)
    if (shortcols) { if (hist) PAL_COLS_FIN(kColsStrips, true, false, 4); else PAL_COLS_FIN(kColsStrips, false, false, 4); }
    else if (f.r89 && full && nw == 4) { if (hist) PAL_COLS_FIN(kColsRader89, true, true, 4); else PAL_COLS_FIN(kColsRader89, false, true, 4); }
    else if (nw == 3) PAL_COLS_FIN_FU(kColsDense, false, 3);  // (per-wavefront statistics only)
    else if (nw == 2) { if (hist) PAL_COLS_FIN_FU(kColsDense, true, 2); else PAL_COLS_FIN_FU(kColsDense, false, 2); }
    else { if (hist) PAL_COLS_FIN_FU(kColsDense, true, 4); else PAL_COLS_FIN_FU(kColsDense, false, 4); }
#undef PAL_COLS_FIN_FU
#undef PAL_COLS_FIN
    PAL_HIP(hipGetLastError());
    PAL_TRY(fin_done(on));
  }
  return PAL_OK;
}

}  // namespace pal
