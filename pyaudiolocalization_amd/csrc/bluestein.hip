// bluestein.hip - exact-length DFTs for GCC-PHAT on gfx950 (fp64, no MFMA: the work is
// butterflies and streaming, not a dense contraction).
//
// Replaces numpy.fft.fft(sig, n) / numpy.fft.ifft(R) of utils.py:114-118 at the exact length
// n = n1 + n2 - 1 (zero-padding to a smooth length changes the selected peaks).
//
//   DFT_n(x)[k] = conj(w_k) * sum_j (x_j conj(w_j)) w_{k-j},   w_j = exp(i pi j^2 / n)
//
// i.e. one circular convolution of power-of-two length M = M1 x M2 with a fixed chirp.  It runs as
// three launches over a resident HBM workspace W[g][M] (g = transform within a launch group):
//
//   cols_fwd : build the input on the fly (loader functor), M1-point column FFTs in LDS,
//              four-step twiddle, write W                         (read: source, write: 16 B/pt)
//   rows_conv: M2-point row FFT, multiply by the chirp spectrum (L2/Infinity-Cache resident,
//              shared by every transform), M2-point inverse row FFT, in place   (16 B r + 16 B w)
//   cols_inv : conj twiddle, M1-point inverse column FFTs, hand y[j] to a storer functor
//
// The inverse PHAT transform packs two mic pairs into one complex transform (real part = pair p,
// imaginary part = pair q) and whitens R = S_a conj(S_b) / (|.| + 1e-10) inside the loader, so the
// whitened cross spectrum never exists in memory.
#include <cmath>

#include "conv_kernels.h"
#include "reduce.h"

namespace pal {

// ------------------------------------------------------------------ table generators
// w[j] = exp(i pi mult j^2 / n)
__global__ void k_make_chirp(cd* w, int n, int mult) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  unsigned long long r = (unsigned long long)j * (unsigned long long)j % (2ull * (unsigned long long)n);
  r = r * (unsigned long long)mult % (2ull * (unsigned long long)n);
  double sgn = 1.0;
  if (r >= (unsigned long long)n) { r -= n; sgn = -1.0; }
  double s, c;
  sincospi(double(r) / double(n), &s, &c);
  w[j] = mk(sgn * c, sgn * s);
}

// out[q] = exp(-2 pi i q / denom)
__global__ void k_make_roots(cd* out, int count, double denom) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= count) return;
  double s, c;
  sincospi(-2.0 * double(q) / denom, &s, &c);
  out[q] = mk(c, s);
}

__global__ void k_make_stage_tw(cd* out, int ln, bool compact) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  for (int lp = stage_log2r(ln, 0); lp < ln; lp += stage_log2r(ln, lp)) {
    const int R = stage_radix(ln, lp), P = 1 << lp, off = stage_tw_offset(ln, lp);
    if (compact && stage_is_last(ln, lp)) {          // rows r = 1, 2, 4 (, 8) only
      if (idx >= off && idx < off + stage_log2r(ln, lp) * P) {
        const int r = 1 << ((idx - off) / P), k = (idx - off) % P;
        double s, c;
        sincospi(-2.0 * double(k * r) / double(P * R), &s, &c);
        out[idx] = mk(c, s);
      }
    } else if (idx >= off && idx < off + (R - 1) * P) {
      const int r = (idx - off) / P + 1, k = (idx - off) % P;
      double s, c;
      sincospi(-2.0 * double(k * r) / double(P * R), &s, &c);
      out[idx] = mk(c, s);
    }
  }
}

// ------------------------------------------------------------------ loader / storer functors
// chirp kernel of the convolution: c[m mod M] = w_|m| (or its conjugate) for -neg < m < pos
struct ChirpLoader {
  static constexpr const char* kName = "ChirpLoader";
  const cd* w;
  int neg, pos;
  unsigned M;
  bool conj_kernel;
  __device__ cd operator()(int, unsigned j) const {
    unsigned a;
    if (j < (unsigned)pos) a = j;
    else if (M - j < (unsigned)neg) a = M - j;
    else return mk(0, 0);
    cd v = w[a];
    return conj_kernel ? cconj(v) : v;
  }
};

// forward transform input: x_j conj(w_j)
struct FrameLoader {
  static constexpr const char* kName = "FrameLoader";
  const double* x;
  size_t stride;
  int len;
  const cd* w;
  __device__ cd operator()(int g, unsigned j) const {
    if (j >= (unsigned)len) return mk(0, 0);
    const double v = x[size_t(g) * stride + j];
    const cd c = w[j];
    return mk(v * c.x, -v * c.y);
  }
};

// forward transform output: X_k = conj(w_k) y_k, k < H
struct SpectrumStorer {
  static constexpr const char* kName = "SpectrumStorer";
  cd* S;
  int H;
  const cd* w;
  __device__ void operator()(int g, unsigned j, cd y) const {
    if (j < (unsigned)H) S[size_t(g) * H + j] = cmulc(y, w[j]);
  }
};

// forward transform output straight into the layout of the prime-factor route (pfa.hip): SP[row][k1][k2] holds the
// Hermitian-extended spectrum at k = CRT(k1, k2) for k1 < NR = (N1+1)/2.  Bin j < H lands at (j mod N1, j mod N2) when
// that row is kept; its mirror n - j has the residues (N1 - k1, N2 - k2) and takes the conjugate when THAT row is
// kept (row 0 pairs with itself and takes both).
struct PermSpectrumStorer {
  static constexpr const char* kName = "PermSpectrumStorer";
  cd* SP;
  int H, N1, N2, NR;
  float inv1, inv2;
  const cd* w;
  const int* slot;   // column k2 -> position inside a row (Rader rows keep generator order, pfa_rader.h); null: k2 itself
  __device__ void operator()(int g, unsigned j, cd y) const {
    if (j >= (unsigned)H) return;
    const cd v = cmulc(y, w[j]);
    int k1 = int(j) - int(unsigned(float(j) * inv1)) * N1;      // j < 2^24: the float quotient is off by at most one
    k1 = k1 < 0 ? k1 + N1 : (k1 >= N1 ? k1 - N1 : k1);
    int k2 = int(j) - int(unsigned(float(j) * inv2)) * N2;
    k2 = k2 < 0 ? k2 + N2 : (k2 >= N2 ? k2 - N2 : k2);
    cd* base = SP + size_t(g) * NR * N2;
    const int km = k2 ? N2 - k2 : 0;
    if (k1 < NR) base[size_t(k1) * N2 + (slot ? slot[k2] : k2)] = v;
    if (k1 == 0 ? j != 0 : k1 >= NR) base[size_t(k1 ? N1 - k1 : 0) * N2 + (slot ? slot[km] : km)] = cconj(v);
  }
};

// inverse transform input: (R^p_k + i R^q_k) w_k over the full Hermitian-extended grid k < n
struct PairLoader {
  static constexpr const char* kName = "PairLoader";
  const cd* S;       // spectra[row][H]
  const int4* quad;  // rows (a, b) of pair p and (c, d) of pair q; c < 0: no second pair
  int n, H;
  const cd* w;
  __device__ cd operator()(int g, unsigned j) const {
    if (j >= (unsigned)n) return mk(0, 0);
    const bool mirror = j >= (unsigned)H;
    const unsigned jj = mirror ? n - j : j;
    const int4 q = quad[g];
    const cd sa = S[size_t(q.x) * H + jj];
    cd r1 = whiten(sa, S[size_t(q.y) * H + jj]);
    cd r2 = mk(0, 0);
    // consecutive pairs of the i<j order share their first mic: reuse its spectrum bin (a quarter of the reads)
    if (q.z >= 0) r2 = whiten(q.z == q.x ? sa : S[size_t(q.z) * H + jj], S[size_t(q.w) * H + jj]);
    if (mirror) { r1.y = -r1.y; r2.y = -r2.y; }
    return cmul(mk(r1.x - r2.y, r1.y + r2.x), w[j]);
  }
};

// inverse transform output: z_m = w_m y_m; real part -> row 2g, imaginary part -> row 2g+1
struct CorrStorer {
  static constexpr const char* kName = "CorrStorer";
  double* corr;
  size_t stride;
  int n;
  const cd* w;
  const int* zero_rows;   // per row: 1 = a microphone of the pair is silent and the row is exactly zero (k_pair_zero); or null
  __device__ void operator()(int g, unsigned j, cd y) const {
    if (j >= (unsigned)n) return;
    const cd z = cmul(y, w[j]);
    corr[size_t(2 * g) * stride + j] = zero_rows && zero_rows[2 * g] ? 0.0 : z.x;
    corr[size_t(2 * g + 1) * stride + j] = zero_rows && zero_rows[2 * g + 1] ? 0.0 : z.y;
  }
};

// Silent channels.  A frame of zeros has a zero spectrum, R = 0 / (0 + 1e-10) = 0 in every bin, and the reference's
// correlation row is exactly zero (argmax 0, no peaks).  Here two pairs share one complex transform, whose rounding
// leaves 1e-17 of the OTHER pair in that row: the rows of pairs with a silent microphone are therefore forced to zero.
// The same pass looks for non-finite samples.  The reference confines a NaN to the pairs of its own microphone; here the
// pair packed into the same complex transform would be poisoned as well, so a non-finite frame sets kStInputNonFinite in the
// engine's status word kStInput and the call is reported as PAL_ERR_INVALID by pal_synchronize (never silently wrong rows).
// The flag of a live row also carries its power-of-two exponent (reduce.h: kRowExpBias + ilogb(max |x|)): the packed forward
// transform (pfa_forward.h) scales both of its frames to [1, 2) with it, so a quiet frame does not drown in a loud partner.
__global__ __launch_bounds__(256) void k_row_nonzero(const double* __restrict__ frames, size_t frame_stride, int len, int* __restrict__ flags,
                                                     int* __restrict__ status) {
  const double* x = frames + size_t(blockIdx.x) * frame_stride;
  __shared__ double rd[4];
  bool any = false, bad = false;
  double top = 0.0;
  for (int i = threadIdx.x; i < len; i += 256) {
    const double v = x[i];
    any = any || v != 0.0;
    bad = bad || !(v - v == 0.0);                             // NaN or infinity
    top = fmax(top, fabs(v));
  }
  const int all = __syncthreads_or(any ? 1 : 0);
  const int nonfinite = __syncthreads_or(bad ? 1 : 0);
  top = block_max(top, rd, threadIdx.x);
  if (threadIdx.x == 0) {
    flags[blockIdx.x] = all ? kRowExpBias + (nonfinite ? 0 : row_exponent(top)) : 0;
    if (nonfinite && status) atomicOr(status + kStInput, kStInputNonFinite);
  }
}

// explicit pair list (row indices, two per pair) -> the packed table of the pair pipeline: two pairs per complex
// transform, (c, d) = (-1, -1) when the count is odd.  A row index outside 0..R-1 sets kStInputBadRow in status word kStInput and the
// pair is redirected to row 0 (no out-of-range read; pal_synchronize reports PAL_ERR_INVALID).
__global__ __launch_bounds__(256) void k_pairs_to_quads(const int32_t* __restrict__ pairs, int64_t P, int R, int4* __restrict__ quads,
                                                        int* __restrict__ status) {
  const int64_t g = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (g >= (P + 1) / 2) return;
  int v[4];
  bool bad = false;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t at = 4 * g + q;
    v[q] = at < 2 * P ? pairs[at] : -1;
    if (at < 2 * P && (v[q] < 0 || v[q] >= R)) { bad = true; v[q] = 0; }
  }
  quads[g] = make_int4(v[0], v[1], v[2], v[3]);
  if (bad && status) atomicOr(status + kStInput, kStInputBadRow);
}

__global__ __launch_bounds__(256) void k_pair_zero(const int4* __restrict__ quads, const int* __restrict__ nonzero, int64_t ntr,
                                                   int* __restrict__ zero_rows) {
  const int64_t g = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (g >= ntr) return;
  const int4 q = quads[g];
  zero_rows[2 * g] = !nonzero[q.x] || !nonzero[q.y];
  zero_rows[2 * g + 1] = q.z >= 0 && (!nonzero[q.z] || !nonzero[q.w]);
}

// ---- the pairs the finishing column pass flagged (pfa_cols_fin.h): their TRANSFORMS, in order, with their original packing
// (a flagged pair is resolved beside the same partner pair as in the first pass, so its record does not depend on which other
// pairs of the call were flagged - the last bits of cmax / cmin / snr depend on the partner) ----
// one workgroup walks the transforms in tiles of 1024 (a stable compaction)
__global__ __launch_bounds__(1024) void k_flag_list(const int* __restrict__ need, int64_t npairs, int* __restrict__ list, int* __restrict__ count) {
  __shared__ int wsum[16];
  __shared__ int base;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t ntr = (npairs + 1) / 2;
  if (tid == 0) base = 0;
  __syncthreads();
  for (int64_t g0 = 0; g0 < ntr; g0 += 1024) {
    const int64_t g = g0 + tid;
    const bool f = g < ntr && (need[2 * g] != 0 || (2 * g + 1 < npairs && need[2 * g + 1] != 0));
    const unsigned long long mask = __ballot(f);
    if (lane == 0) wsum[wave] = __popcll(mask);
    __syncthreads();
    int before = base;
    for (int w = 0; w < wave; ++w) before += wsum[w];
    if (f) list[before + __popcll(mask & ((1ull << lane) - 1ull))] = int(g);
    __syncthreads();
    if (tid == 0) { int t = 0; for (int w = 0; w < 16; ++w) t += wsum[w]; base += t; }
    __syncthreads();
  }
  if (tid == 0) *count = base;
}

__global__ __launch_bounds__(256) void k_flag_quads(const int4* __restrict__ quads, const int* __restrict__ list, int count, int4* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < count) out[i] = quads[list[i]];
}

__global__ __launch_bounds__(256) void k_flag_scatter(const pal_pair_record* __restrict__ src, const int* __restrict__ list, int count,
                                                      const int* __restrict__ need, int64_t npairs, pal_pair_record* __restrict__ table) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * count) return;
  const int64_t p = 2 * int64_t(list[i >> 1]) + (i & 1);
  if (p < npairs && need[p]) table[p] = src[i];
}

// ------------------------------------------------------------------ plans
const cd* Engine::stage_table(int ln, bool compact) {
  cd*& slot = compact ? stage_twc[ln] : stage_tw[ln];
  if (!slot) {
    cd* p = nullptr;
    if (hipMalloc(&p, sizeof(cd) << ln) != hipSuccess) return nullptr;
    (void)hipMemsetAsync(p, 0, sizeof(cd) << ln, stream);
    k_make_stage_tw<<<dim3(((1 << ln) + 255) / 256), dim3(256), 0, stream>>>(p, ln, compact);
    slot = p;
  }
  return slot;
}

// geometry (plan_geometry.h) -> twiddle tables -> storage of the chirp spectrum and the four-step twiddles
int Engine::alloc_conv(Conv& c, size_t needed) {
  if (!conv_geometry(needed, plan_sw, &c.g)) return fail(PAL_ERR_UNSUPPORTED, "convolution of %zu points exceeds 2^22", needed);
  if ((!c.g.reg() && !stage_table(c.g.l1)) || !stage_table(c.g.l2)) return fail(PAL_ERR_NOMEM, "twiddle tables");
  PAL_HIP(hipMalloc(&c.chat, c.M() * sizeof(cd)));
  PAL_HIP(hipMalloc(&c.twA, sizeof(cd) * c.M1()));
  PAL_HIP(hipMalloc(&c.twB, sizeof(cd) * c.M2()));
  k_make_roots<<<dim3((c.M1() + 255) / 256), dim3(256), 0, stream>>>(c.twA, c.M1(), double(c.M1()));
  k_make_roots<<<dim3((c.M2() + 255) / 256), dim3(256), 0, stream>>>(c.twB, c.M2(), double(c.M()));
  return check(hipGetLastError(), "k_make_roots");
}

void Engine::free_conv(Conv& c) {
  if (c.chat) (void)hipFree(c.chat);
  if (c.twA) (void)hipFree(c.twA);
  if (c.twB) (void)hipFree(c.twB);
  c = Conv();
}

int Engine::build_conv(Conv& c, const cd* w, int n, int neg_count, int pos_count, bool conj_kernel,
                       double extra_scale) {
  Engine* e = this;
  PAL_TRY(alloc_conv(c, size_t(neg_count) + size_t(pos_count) - 1));
  // chirp spectrum: column FFTs + twiddle, then forward row FFTs, scaled, in [k1][k2] order
  ChirpLoader ld{w, neg_count, pos_count, unsigned(c.M()), conj_kernel};
  PAL_TRY(launch_cols_fwd(e, c, 1, ld, c.chat));
  PAL_TRY(launch_rows(e, c, 1, c.chat, false, extra_scale / double(c.M())));
  return PAL_OK;
}

void Engine::free_plan(Plan& pl) {
  if (pl.w) (void)hipFree(pl.w);
  free_conv(pl.fwd);
  free_conv(pl.inv);
  free_pfa(pl.pfa);
  pl = Plan();
}

// every plan and the cached synchronisation convolutions; the streams are drained first
int Engine::clear_plans() {
  PAL_HIP(hipStreamSynchronize(stream));
  PAL_HIP(hipStreamSynchronize(stream2));
  PAL_HIP(hipStreamSynchronize(stream3));
  for (auto& kv : plans) free_plan(kv.second);
  plans.clear();
  for (auto& kv : xconvs) free_conv(kv.second.conv);
  xconvs.clear();
  return PAL_OK;
}

// convolution geometry of the plain cross-correlation of pal_xcorr_vs_ref for sequences of `len` points, kept per
// length (at most max_plans of them, least recently used out first)
int Engine::xcorr_conv(size_t len, Conv** out) {
  auto it = xconvs.find(len);
  if (it == xconvs.end()) {
    if (int(xconvs.size()) >= max_plans) {
      auto old = xconvs.begin();
      for (auto k = xconvs.begin(); k != xconvs.end(); ++k)
        if (k->second.used < old->second.used) old = k;
      PAL_HIP(hipStreamSynchronize(stream));
      free_conv(old->second.conv);
      xconvs.erase(old);
    }
    XConv x;
    const int rc = alloc_conv(x.conv, len);
    if (rc != PAL_OK) { free_conv(x.conv); return rc; }
    it = xconvs.emplace(len, x).first;
  }
  it->second.used = ++plan_clock;
  *out = &it->second.conv;
  return PAL_OK;
}

int Engine::get_plan(int n, int lin, int nout, Plan** out) {
  auto key = std::make_tuple(n, lin, nout);
  auto it = plans.find(key);
  if (it != plans.end()) {
    it->second.used = ++plan_clock;
    *out = &it->second;
    return PAL_OK;
  }
  if (n < 1 || lin < 1 || lin > n || nout < 1 || nout > n)
    return fail(PAL_ERR_INVALID, "bad transform geometry n=%d lin=%d nout=%d", n, lin, nout);
  // The cache is bounded (recordings of many different lengths, ragged pairs, per-frame lengths behind the
  // synchronisation): the least recently used plan goes once every stream has drained (PAL_MAX_PLANS, default 32).
  while (int(plans.size()) >= max_plans) {
    auto old = plans.begin();
    for (auto k = plans.begin(); k != plans.end(); ++k)
      if (k->second.used < old->second.used) old = k;
    PAL_HIP(hipStreamSynchronize(stream));
    PAL_HIP(hipStreamSynchronize(stream2));
    PAL_HIP(hipStreamSynchronize(stream3));
    free_plan(old->second);
    plans.erase(old);
    ++plans_evicted;
  }
  Plan pl;
  pl.n = n;
  pl.H = n / 2 + 1;
  pl.lin = lin;
  pl.nout = nout;
  int rc = PAL_OK;
  do {
    if ((rc = check(hipMalloc(&pl.w, size_t(n) * sizeof(cd)), "chirp alloc")) != PAL_OK) break;
    k_make_chirp<<<dim3((n + 255) / 256), dim3(256), 0, stream>>>(pl.w, n, 1);
    if ((rc = check(hipGetLastError(), "k_make_chirp")) != PAL_OK) break;
    // forward: j < lin inputs, k < H outputs, kernel w_{k-j}
    if ((rc = build_conv(pl.fwd, pl.w, n, lin, pl.H, false, 1.0)) != PAL_OK) break;
    // inverse: k < n inputs, m < nout outputs, kernel conj(w_{m-k}); 1/n of numpy.fft.ifft folded in
    if ((rc = build_conv(pl.inv, pl.w, n, n, nout, true, 1.0 / double(n))) != PAL_OK) break;
    if ((rc = build_pfa(pl)) != PAL_OK) break;   // prime-factor route of the PHAT inverse, when n splits
    rc = check(hipStreamSynchronize(stream), "plan setup");
  } while (0);
  if (rc != PAL_OK) {                            // nothing of a half-built plan stays behind
    const std::string keep = err;
    (void)hipStreamSynchronize(stream);
    free_plan(pl);
    err = keep;
    return rc;
  }
  pl.used = ++plan_clock;
  ++plans_built;
  auto ins = plans.emplace(key, pl);
  *out = &ins.first->second;
  return PAL_OK;
}

// ------------------------------------------------------------------ pipelines
int Engine::forward_spectra(Plan& pl, const double* frames, size_t frame_stride, int rows, int len, cd* spectra, int* nonzero) {
  Engine* e = this;
  if (len > pl.lin) return fail(PAL_ERR_INVALID, "frame length %d exceeds plan input length %d", len, pl.lin);
  if (nonzero && rows > 0) {
    int* status = nullptr;
    PAL_TRY(status_words(&status));
    k_row_nonzero<<<dim3(rows), dim3(256), 0, stream>>>(frames, frame_stride, len, nonzero, status);
    PAL_HIP(hipGetLastError());
  }
  if (pfa_forward_applies(pl, len)) return pfa_forward_spectra(pl, frames, frame_stride, rows, len, spectra, nonzero);
  const Conv& c = pl.fwd;
  cd* W = nullptr;
  PAL_TRY(scratch(kWsWork, size_t(chunk) * c.M() * sizeof(cd), &W));
  for (int r0 = 0; r0 < rows; r0 += chunk) {
    const int G = rows - r0 < chunk ? rows - r0 : chunk;
    FrameLoader ld{frames + size_t(r0) * frame_stride, frame_stride, len, pl.w};
    PAL_TRY(launch_cols_fwd(e, c, G, ld, W));
    PAL_TRY(launch_rows(e, c, G, W, true, 1.0));
    if (pl.pfa.on()) {   // the prime-factor inverse reads the permuted layout (spec_stride() elements per row)
      const Pfa& f = pl.pfa;
      PermSpectrumStorer st{spectra + size_t(r0) * pl.spec_stride(), pl.H, f.n1, f.n2, f.rows(), 1.0f / float(f.n1),
                            1.0f / float(f.n2), pl.w, f.rader ? f.rd_qidx : nullptr};
      PAL_TRY(launch_cols_inv(e, c, G, W, st));
    } else {
      SpectrumStorer st{spectra + size_t(r0) * pl.H, pl.H, pl.w};
      PAL_TRY(launch_cols_inv(e, c, G, W, st));
    }
  }
  return PAL_OK;
}

// explicit pair list over R equal-length rows, everything in HBM: one-vs-many bootstrap batches, sparse pair sets, and
// the contiguous pair blocks a rank owns when ONE large frame is split over the GPUs (spectra recomputed locally)
int Engine::pairs_dev(const double* d_rows, int R, int L, const int32_t* d_pairs, int64_t P, const pal_phat_params& prm,
                      pal_pair_record* d_table, const CandOut* cands) {
  if (R < 1 || L < 1 || P < 1) return fail(PAL_ERR_INVALID, "need R >= 1, L >= 1, P >= 1");
  if (L > (1 << 20)) return fail(PAL_ERR_UNSUPPORTED, "frame length %d exceeds 2^20", L);
  Plan* pl = nullptr;
  PAL_TRY(get_plan(2 * L - 1, L, 2 * L - 1, &pl));
  cd* sp = nullptr;
  int4* dq = nullptr;
  int* status = nullptr;
  PAL_TRY(scratch(kWsSpectra, size_t(R) * pl->spec_stride() * sizeof(cd) + size_t(R) * sizeof(int), &sp));
  int* nonzero = reinterpret_cast<int*>(sp + size_t(R) * pl->spec_stride());
  const int64_t ntr = (P + 1) / 2;
  PAL_TRY(scratch(kWsQuads, size_t(ntr) * sizeof(int4), &dq));
  PAL_TRY(status_words(&status));
  k_pairs_to_quads<<<dim3(unsigned((ntr + 255) / 256)), dim3(256), 0, stream>>>(d_pairs, P, R, dq, status);
  PAL_HIP(hipGetLastError());
  PAL_TRY(forward_spectra(*pl, d_rows, size_t(L), R, L, sp, nonzero));
  return pair_correlations(*pl, sp, R, dq, P, L, prm, d_table, nullptr, nullptr, nonzero, false, cands);
}

// the first K of a launch group's PAL_MAX_PEAKS-wide selection rows -> the caller's K columns (indices -1, heights +0.0 past n_sel)
__global__ __launch_bounds__(256) void k_compact_cands(const int32_t* __restrict__ ksel, const double* __restrict__ hsel, int rows, int K,
                                                       int32_t* __restrict__ cand_k, double* __restrict__ cand_h) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= rows * K) return;
  const int r = t / K, c = t % K;
  const int32_t k = ksel[size_t(r) * PAL_MAX_PEAKS + c];
  cand_k[size_t(r) * K + c] = k;
  if (cand_h) cand_h[size_t(r) * K + c] = k >= 0 ? hsel[size_t(r) * PAL_MAX_PEAKS + c] : 0.0;
}

int Engine::pair_correlations(Plan& pl, const cd* spectra, int nspec, const int4* quads, int64_t npairs, int n2,
                              const pal_phat_params& prm, pal_pair_record* table, int32_t* ksel_multi,
                              double* corr_out, const int* nonzero, bool stored_only, const CandOut* cands) {
  const Conv& c = pl.inv;
  const int n = pl.n;
  const bool pfa = pl.pfa.on();
  const int chunk = pair_group(n);   // (shadows the engine-wide group size: larger groups amortise launch tails and the peak kernels' fixed costs)
  // Launch groups rotate over three HIP streams, each with its own workspace and correlation buffer: the
  // memory-bound head and tail of one group's kernels overlap the LDS/VALU-bound middle of the others', and the
  // peak kernels of group g run beside the FFT passes of group g+1.  Same-slot reuse is ordered by the stream.
  const int nslot = !one_stream && table != nullptr ? 3 : 1;
  const size_t wpoints = size_t(chunk) * (pfa ? size_t(n) : c.M());
  cd* W = nullptr;
  PAL_TRY(scratch(kWsWork, size_t(nslot) * wpoints * sizeof(cd), &W));
  const size_t stride = corr_out ? size_t(n) : (size_t(n) + 1) & ~size_t(1);
  const size_t buf_doubles = size_t(2 * chunk) * stride;
  double* cbuf = nullptr;
  PAL_TRY(scratch(kWsCorr, size_t(nslot) * buf_doubles * sizeof(double), &cbuf));
  const int64_t ntr = (npairs + 1) / 2;
  int* zero_rows = nullptr;
  if (nonzero && ntr > 0) {
    PAL_TRY(scratch(kWsZeroRows, size_t(2 * ntr) * sizeof(int), &zero_rows));
    k_pair_zero<<<dim3(unsigned((ntr + 255) / 256)), dim3(256), 0, stream>>>(quads, nonzero, ntr, zero_rows);
    PAL_HIP(hipGetLastError());
  }
  // who transforms a launch group and who computes its rows' statistics: one decision per call (pair_route.h)
  const Pfa& f = pl.pfa;
  const PairRoute route = pair_route(RouteIn{n, pl.nout, pfa, f.n1, f.n2, f.nch, f.lm, f.r89, table != nullptr, corr_out != nullptr,
                                             ksel_multi != nullptr || cands != nullptr, npairs, stored_only, prm.num_peaks, prm.threshold_method, prm.threshold_multiplier,
                                             fin_cols, fuse_peaks, lean_store, rows_lean, rows_lean_min});
  // the finishing passes and k_rows_lean write one flag per pair: 1 = resolved at the end of this call from stored rows
  int* need = nullptr;
  if (route.flags_pairs()) PAL_TRY(scratch(kWsFlags, (size_t(2 * npairs) + 64) * sizeof(int), &need));     // [flags | list | count]
  // candidates: the PAL_MAX_PEAKS-wide selection rows of a launch group stay in scratch per stream slot (reuse ordered by the slot's
  // stream) and k_compact_cands, on that stream, writes their first K columns at the group's place in the caller's buffers
  const size_t cand_rows = size_t(2 * chunk) * PAL_MAX_PEAKS;
  int32_t* cand_kbuf = nullptr;
  double* cand_hbuf = nullptr;
  if (cands) {
    if (!table || !cands->k || prm.num_peaks > PAL_MAX_CANDIDATES) return fail(PAL_ERR_INVALID, "candidates need a table, a buffer and num_peaks <= %d", PAL_MAX_CANDIDATES);
    PAL_TRY(scratch(kWsCandK, size_t(nslot) * cand_rows * sizeof(int32_t), &cand_kbuf));
    PAL_TRY(scratch(kWsCandH, size_t(nslot) * cand_rows * sizeof(double), &cand_hbuf));
  }
  if (nslot == 3) {   // the other streams start after everything already queued on `stream` (spectra, pair table)
    PAL_HIP(hipEventRecord(ev_fork, stream));
    PAL_HIP(hipStreamWaitEvent(stream2, ev_fork, 0));
    PAL_HIP(hipStreamWaitEvent(stream3, ev_fork, 0));
  }
  // one launch group; a failure leaves through the common exit below (side streams joined, sampling gate restored)
  auto run_group = [&](int64_t t0, int64_t group) -> int {
    const int G = int(ntr - t0 < chunk ? ntr - t0 : chunk);
    const int64_t p0 = 2 * t0;
    const int rows = int(npairs - p0 < 2 * G ? npairs - p0 : 2 * G);
    const int slot = int(group % nslot);
    const hipStream_t on = stream_of(slot);
    prof_gate = prof_every <= 1 || (prof_tick++ % prof_every) == 0;
    cd* Wg = W + size_t(slot) * wpoints;
    // odd tail with a caller buffer: the imaginary half of the last transform has no destination row there
    const bool via_scratch = !corr_out || rows < 2 * G;
    double* crow = via_scratch ? cbuf + size_t(slot) * buf_doubles : corr_out + size_t(p0) * stride;
    const int* zrows = zero_rows ? zero_rows + p0 : nullptr;
    int32_t* ksel = cands ? cand_kbuf + size_t(slot) * cand_rows : (ksel_multi ? ksel_multi + p0 * PAL_MAX_PEAKS : nullptr);
    double* hsel = cands ? cand_hbuf + size_t(slot) * cand_rows : nullptr;
    switch (route.transform) {   // (forward_spectra wrote the (k mod N1, k mod N2) layout when the plan has the split)
      case RouteTransform::kFinish:      // nobody reads the correlation rows: the column pass finishes them without storing them (pfa_cols_fin.h)
        PAL_TRY(pfa_pair_group_fin(pl, spectra, quads + t0, G, rows, Wg, zrows, prm, n2, table + p0, need + p0, slot)); break;
      case RouteTransform::kLeanStore:   // stored rows + per-wavefront statistics (pfa_fin_lean.h with FinArgs.corr)
        PAL_TRY(pfa_pair_group_fin(pl, spectra, quads + t0, G, rows, Wg, zrows, prm, n2, table + p0, need + p0, slot, crow, stride)); break;
      case RouteTransform::kFused:
        PAL_TRY(pfa_pair_group_fused(pl, spectra, quads + t0, G, rows, Wg, crow, stride, zrows, prm, n2, table + p0, ksel, slot, hsel)); break;
      case RouteTransform::kPfa:
        PAL_TRY(pfa_pair_group(pl, spectra, quads + t0, G, Wg, crow, stride, zrows, on)); break;
      case RouteTransform::kFourStep: {
        PairLoader ld{spectra, quads + t0, n, pl.H, pl.w};
        PAL_TRY(launch_cols_fwd(this, c, G, ld, Wg, on));
        PAL_TRY(launch_rows(this, c, G, Wg, true, 1.0, on));
        CorrStorer st{crow, stride, n, pl.w, zrows};
        PAL_TRY(launch_cols_inv(this, c, G, Wg, st, on));
        break;
      }
    }
    if (corr_out && via_scratch)
      PAL_HIP(hipMemcpyAsync(corr_out + size_t(p0) * stride, crow, size_t(rows) * stride * sizeof(double),
                             hipMemcpyDeviceToDevice, on));
    // rows of the plain routes: their statistics in one launch over the stored rows, or in three
    if (route.stats == RouteStats::kRowsLean) PAL_TRY(rows_lean_group(pl, crow, stride, G, rows, prm, n2, table + p0, need + p0, slot));
    else if (route.stats == RouteStats::kThreeLaunches) PAL_TRY(peaks(crow, stride, rows, n, n2, prm, table + p0, ksel, slot, hsel));
    if (cands) {
      const int K = prm.num_peaks;
      k_compact_cands<<<dim3(unsigned((rows * K + 255) / 256)), dim3(256), 0, on>>>(ksel, hsel, rows, K, cands->k + p0 * K, cands->h ? cands->h + p0 * K : nullptr);
      PAL_HIP(hipGetLastError());
    }
    return PAL_OK;
  };
  int64_t group = 0;
  for (int64_t t0 = 0; t0 < ntr; t0 += chunk, ++group) {
    const int rc = run_group(t0, group);
    if (rc != PAL_OK) {
      // work may still be running on the side streams: nothing that follows (frees, reuse of the workspaces, the
      // caller's next call) may overtake it
      prof_gate = true;
      const std::string keep = err;
      (void)hipStreamSynchronize(stream);
      (void)hipStreamSynchronize(stream2);
      (void)hipStreamSynchronize(stream3);
      err = keep;
      return rc;
    }
  }
  prof_gate = true;
  if (nslot == 3) {   // whatever follows on `stream` (downloads, the RCCL gather) sees the finished table
    PAL_HIP(hipEventRecord(ev_join2, stream2));
    PAL_HIP(hipStreamWaitEvent(stream, ev_join2, 0));
    PAL_HIP(hipEventRecord(ev_join3, stream3));
    PAL_HIP(hipStreamWaitEvent(stream, ev_join3, 0));
  }
  if (route.flags_pairs()) {
    // The pairs the finishing blocks flagged (a threshold comparison inside the median's interval, a tie, a window peak next to
    // the window's edge, ...) go through the stored-row path now, packed in pair order.  The count comes to the host: this
    // is the one synchronisation of the call (its launch groups above never waited for the host).
    int* list = need + npairs;
    int* dcount = need + 2 * npairs;
    k_flag_list<<<dim3(1), dim3(1024), 0, stream>>>(need, npairs, list, dcount);
    PAL_HIP(hipGetLastError());
    int count = 0;
    PAL_HIP(hipMemcpyAsync(&count, dcount, sizeof count, hipMemcpyDeviceToHost, stream));
    PAL_HIP(hipStreamSynchronize(stream));
    if (count > 0) {                                           // `count` transforms hold a flagged pair
      int4* qp = nullptr;
      pal_pair_record* tp = nullptr;
      PAL_TRY(scratch(kWsFlagQuads, size_t(count) * sizeof(int4), &qp));
      PAL_TRY(scratch(kWsFlagTable, size_t(2 * count) * sizeof(pal_pair_record), &tp));
      k_flag_quads<<<dim3(unsigned((count + 255) / 256)), dim3(256), 0, stream>>>(quads, list, count, qp);
      PAL_HIP(hipGetLastError());
      PAL_TRY(pair_correlations(pl, spectra, nspec, qp, int64_t(2) * count, n2, prm, tp, nullptr, nullptr, nonzero, true));   // stored rows only: nothing that flags again
      k_flag_scatter<<<dim3(unsigned((2 * count + 255) / 256)), dim3(256), 0, stream>>>(tp, list, count, need, npairs, table);
      PAL_HIP(hipGetLastError());
    }
  }
  return PAL_OK;
}

}  // namespace pal
