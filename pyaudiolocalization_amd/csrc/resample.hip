// resample.hip - recorded-audio ingest on the device: the kaiser_best resampler and the frame cutter.
//
//   resample : signal_processing.resample_kaiser_best (the project's statement of resampy's `kaiser_best`: Smith's band-limited
//              interpolation over a Kaiser-windowed sinc table with linear interpolation between table entries).  One lane per
//              output sample, 256 consecutive outputs of one row per workgroup; every lane walks its left wing, then its right
//              wing, in the specification's tap order (resample_math.h).  This translation unit is built with
//              -ffp-contract=off: each product is rounded before it is added, as NumPy does, so the result is the
//              specification's bit for bit.
//              The table (32 769 entries of (win, delta): 512 KB) stays in global memory - it is far beyond LDS, every lane
//              reads its own entries (offset + i * index_step), and it is shared by all workgroups, so it lives in L2.
//              The input span of a workgroup (256 / ratio + 2 wings + 2 samples) is staged in LDS when it fits kStageMax doubles;
//              longer spans (ratios below about 1/11) are read from global memory.
//   frames   : out[f][m][i] = rows[m][(first_frame + f) * hop + i]: a gather.
#include "engine.h"

namespace pal {

namespace {

constexpr int kRsBlock = 256;      // outputs per workgroup
constexpr int kStageMax = 4096;    // doubles of LDS a workgroup may stage (32 KB: five workgroups per CU)

struct GlobalRow {
  const double* x;
  __device__ double operator()(int64_t i) const { return x[i]; }
};
struct StagedRow {
  const double* xs;    // LDS copy of x[lo ..]
  int64_t lo;
  __device__ double operator()(int64_t i) const { return xs[i - lo]; }
};

// grid: rows x ceil(n_out / 256) workgroups, flattened; stage_cap: doubles of dynamic LDS (0: no staging)
__global__ __launch_bounds__(kRsBlock) void k_resample(const double* __restrict__ x, int64_t n_orig, double* __restrict__ y, int64_t n_out,
                                                        int blocks_per_row, ResampleFilter f, int stage_cap) {
  extern __shared__ double xs[];
  const int64_t row = blockIdx.x / unsigned(blocks_per_row);
  const int64_t t0 = int64_t(blockIdx.x % unsigned(blocks_per_row)) * kRsBlock;
  const int64_t t1 = t0 + kRsBlock - 1 < n_out - 1 ? t0 + kRsBlock - 1 : n_out - 1;
  const double* xr = x + row * n_orig;
  const int64_t t = t0 + threadIdx.x;
  // the samples this workgroup can touch: n(t) does not decrease with t, a wing has at most `wing` taps
  const int64_t wing = resample_wing_taps(f);
  int64_t lo = int64_t(double(t0) * f.inv_ratio) - wing + 1;
  int64_t hi = int64_t(double(t1) * f.inv_ratio) + wing;
  lo = lo < 0 ? 0 : lo;
  hi = hi > n_orig - 1 ? n_orig - 1 : hi;
  const int64_t span = hi - lo + 1;
  if (span > 0 && span <= stage_cap) {                      // (uniform over the workgroup)
    for (int64_t i = threadIdx.x; i < span; i += kRsBlock) xs[i] = xr[lo + i];
    __syncthreads();
    if (t < n_out) y[row * n_out + t] = resample_sample(f, StagedRow{xs, lo}, n_orig, t);
  } else if (t < n_out) {
    y[row * n_out + t] = resample_sample(f, GlobalRow{xr}, n_orig, t);
  }
}

__global__ __launch_bounds__(256) void k_frame_rows(const double* __restrict__ rows, int M, int64_t T, int frame_len, int64_t hop,
                                                    int64_t first_frame, double* __restrict__ out) {
  const int64_t fm = blockIdx.x;                            // f * M + m
  const int64_t fr = fm / M, m = fm % M;
  const double* src = rows + m * T + (first_frame + fr) * hop;
  double* dst = out + fm * int64_t(frame_len);
  for (int i = threadIdx.x; i < frame_len; i += 256) dst[i] = src[i];
}

}  // namespace

// the filter of `ratio` on the device; rebuilt (and the stream drained) only when the ratio changes
static int resample_filter(Engine* e, double ratio, ResampleFilter* f) {
  const int nwin = int(e->rs_win.size());
  if (nwin < 2 || e->rs_num_table < 1) return e->fail(PAL_ERR_INVALID, "no interpolation filter: call pal_resample_set_filter first");
  void* d_tab = nullptr;
  PAL_TRY(e->scratch(kWsResample, size_t(nwin) * sizeof(ResampleTap), &d_tab));
  if (e->rs_ratio != ratio) {
    PAL_TRY(e->check(hipStreamSynchronize(e->stream), "resample table sync"));   // an earlier launch may still read the old table
    e->rs_host.resize(size_t(nwin));
    resample_fill_table(e->rs_win.data(), nwin, ratio, e->rs_host.data());
    PAL_TRY(e->check(hipMemcpyAsync(d_tab, e->rs_host.data(), size_t(nwin) * sizeof(ResampleTap), hipMemcpyHostToDevice, e->stream), "upload"));
    PAL_TRY(e->check(hipStreamSynchronize(e->stream), "resample table upload"));
    e->rs_ratio = ratio;
  }
  *f = resample_make_filter(static_cast<const ResampleTap*>(d_tab), nwin, e->rs_num_table, ratio);
  return PAL_OK;
}

// ratio and output length of resample_kaiser_best; PAL_ERR_INVALID as the host function's ValueError
static int resample_geometry(Engine* e, int R, int N, double original_fs, double target_fs, double* ratio, int* n_out) {
  if (R < 1 || N < 1 || !n_out) return e->fail(PAL_ERR_INVALID, "bad resample arguments");
  if (!(original_fs > 0) || !(target_fs > 0)) return e->fail(PAL_ERR_INVALID, "Invalid sample rates");
  *ratio = target_fs / original_fs;
  const double len = double(N) * *ratio;
  if (!(len < 2147483647.0)) return e->fail(PAL_ERR_UNSUPPORTED, "resampled length %.0f is beyond 2^31 - 1", len);
  *n_out = int(len);
  if (*n_out < 1) return e->fail(PAL_ERR_INVALID, "Input signal length=%d is too small to resample from %g->%g", N, original_fs, target_fs);
  return PAL_OK;
}

static int resample_dev(Engine* e, const double* d_rows, int R, int N, double ratio, double* d_out, int n_out) {
  ResampleFilter f;
  PAL_TRY(resample_filter(e, ratio, &f));
  const int64_t bpr = (int64_t(n_out) + kRsBlock - 1) / kRsBlock;
  if (bpr * R > 2147483647ll) return e->fail(PAL_ERR_UNSUPPORTED, "%d rows of %d outputs are more workgroups than one launch holds", R, n_out);
  // longest span of a workgroup: n(t0 + 255) - n(t0) <= 255 / ratio + 1, plus both wings
  const double need = 255.0 * f.inv_ratio + 2.0 + 2.0 * double(resample_wing_taps(f));
  const int cap = need <= double(kStageMax) ? (int(need) < N ? int(need) : N) : 0;
  {
    ProfScope ps(e, "k_resample");
    k_resample<<<dim3(unsigned(bpr * R)), dim3(kRsBlock), size_t(cap) * sizeof(double), e->stream>>>(d_rows, int64_t(N), d_out, int64_t(n_out),
                                                                                                   int(bpr), f, cap);
  }
  return e->check(hipGetLastError(), "k_resample");
}

}  // namespace pal

using namespace pal;

#define ENGINE(h)                                   \
  if (!(h)) return PAL_ERR_INVALID;                 \
  Engine* e = reinterpret_cast<Engine*>(h);         \
  if (hipSetDevice(e->device) != hipSuccess) return e->fail(PAL_ERR_HIP, "hipSetDevice(%d) failed", e->device)

extern "C" {

int pal_resample_set_filter(pal_handle h, const double* win, int nwin, int num_table) {
  ENGINE(h);
  if (!win || nwin < 2 || num_table < 1) return e->fail(PAL_ERR_INVALID, "bad interpolation filter");
  PAL_TRY(e->check(hipStreamSynchronize(e->stream), "resample table sync"));
  e->rs_win.assign(win, win + nwin);
  e->rs_num_table = num_table;
  e->rs_ratio = 0;
  return PAL_OK;
}

int pal_resample_dev(pal_handle h, const double* d_rows, int R, int N, double original_fs, double target_fs, double* d_out,
                     int n_out_capacity, int* n_out) {
  ENGINE(h);
  double ratio = 0;
  PAL_TRY(resample_geometry(e, R, N, original_fs, target_fs, &ratio, n_out));
  if (!d_out) return PAL_OK;                                                      // length query
  if (!d_rows) return e->fail(PAL_ERR_INVALID, "NULL buffer");
  if (*n_out > n_out_capacity) return e->fail(PAL_ERR_INVALID, "%d output samples per row do not fit the capacity %d", *n_out, n_out_capacity);
  return resample_dev(e, d_rows, R, N, ratio, d_out, *n_out);
}

int pal_resample(pal_handle h, const double* rows, int R, int N, double original_fs, double target_fs, double* out, int n_out_capacity,
                 int* n_out) {
  ENGINE(h);
  double ratio = 0;
  PAL_TRY(resample_geometry(e, R, N, original_fs, target_fs, &ratio, n_out));
  if (!out) return PAL_OK;
  if (!rows) return e->fail(PAL_ERR_INVALID, "NULL buffer");
  if (*n_out > n_out_capacity) return e->fail(PAL_ERR_INVALID, "%d output samples per row do not fit the capacity %d", *n_out, n_out_capacity);
  void *dx = nullptr, *dy = nullptr;
  PAL_TRY(e->scratch(kWsStageIn, size_t(R) * N * sizeof(double), &dx));
  PAL_TRY(e->scratch(kWsStageOut, size_t(R) * *n_out * sizeof(double), &dy));
  PAL_TRY(e->check(hipMemcpyAsync(dx, rows, size_t(R) * N * sizeof(double), hipMemcpyHostToDevice, e->stream), "upload"));
  PAL_TRY(resample_dev(e, static_cast<const double*>(dx), R, N, ratio, static_cast<double*>(dy), *n_out));
  PAL_TRY(e->check(hipMemcpyAsync(out, dy, size_t(R) * *n_out * sizeof(double), hipMemcpyDeviceToHost, e->stream), "download"));
  return pal_synchronize(h);
}

int pal_frame_rows_dev(pal_handle h, const double* d_rows, int M, int T, int frame_len, int hop, int first_frame, int F, double* d_out) {
  ENGINE(h);
  if (!d_rows || !d_out || M < 1 || T < 1 || frame_len < 1 || hop < 1 || first_frame < 0 || F < 1)
    return e->fail(PAL_ERR_INVALID, "bad framing arguments");
  const int64_t end = (int64_t(first_frame) + F - 1) * hop + frame_len;
  if (end > T) return e->fail(PAL_ERR_INVALID, "frame %d ends at sample %lld of %d", first_frame + F - 1, static_cast<long long>(end), T);
  if (int64_t(F) * M > 2147483647ll) return e->fail(PAL_ERR_UNSUPPORTED, "%d frames of %d rows are more workgroups than one launch holds", F, M);
  {
    ProfScope ps(e, "k_frame_rows");
    k_frame_rows<<<dim3(unsigned(int64_t(F) * M)), dim3(256), 0, e->stream>>>(d_rows, M, int64_t(T), frame_len, int64_t(hop), int64_t(first_frame), d_out);
  }
  return e->check(hipGetLastError(), "k_frame_rows");
}

}  // extern "C"
