// beamform.hip - delay-and-sum beamformer: frames[B][M][L] steered at S points per frame (specification: beamform.py).
//
//   out[b,s] = ifft(sum_m w[b,s,m] X[b,m] exp(-j 2 pi f d[b,s,m])).real[:L] * fade_window(L),   X = fft(frames[b,m], 2L)
//
// the transpose of sim.hip's multipath synthesis (one base, many paths): many microphones, one output row.  Per slice of whole
// frames: the forward spectra of the slice's rows (Engine::forward_spectra at the plan of fractional_delay), k_steer_sum forms the
// S beam spectra of every frame while it reads each microphone spectrum once per tile of up to 8 beams, and the beams go through the
// exact-length inverse DFT(2L) two rows per complex transform (BeamLoader -> launch_cols_fwd / launch_rows / launch_cols_inv ->
// SimStorer: fade window, exponent put back).  Built with -ffp-contract=off: the operation order below is what runs.
// The null-steering beamformer (beamform.py, separate) is the same path with k_separate_frame and k_separate in k_steer_sum's place:
// the S beam spectra of a bin are solved against the Gram matrix of the S steering vectors, so each beam cancels the other sources.
// The MVDR beamformer (beamform.py, mvdr; Engine::mvdr_dev below, kernels in mvdr_kernels.h) takes its weights from the covariance of
// a group of frames: two sweeps over the group's slices with the Cholesky factor of every bin between them, the same inverse.
#include <climits>
#include <cmath>

#include "conv_kernels.h"
#include "mvdr_geometry.h"
#include "reduce.h"
#include "separate_math.h"
#include "sim_rows.h"

namespace pal {

namespace {

constexpr int kSteerBins = 256;    // bins per workgroup: one per lane
constexpr int kSteerMics = 64;     // microphones per LDS tile of the frame's delays and weights
constexpr int kSteerMaxTile = 8;   // beams per pass: their accumulators live in registers

// a delay or weight that is not finite, or a delay that leaves nothing of the row (the circular transform would wrap)
__global__ __launch_bounds__(256) void k_steer_check(const double* __restrict__ delays, const double* __restrict__ weights, size_t n,
                                                     double fs, double L, int* __restrict__ status) {
  const size_t i = size_t(blockIdx.x) * 256 + threadIdx.x;
  bool bad = false;
  if (i < n) {
    const double d = delays[i], w = weights[i];
    bad = !(d - d == 0.0) || !(w - w == 0.0) || fabs(d) * fs > L;
  }
  if (__syncthreads_or(bad ? 1 : 0) && threadIdx.x == 0) atomicOr(status + kStInput, kStInputBadSteer);
}

// Y[f,s,k] = sum_m w[f,s,m] X[f,m,k] exp(j theta), theta = (-6.283185307179586 f_k) d[f,s,m], m = 0 .. M-1 in this order, for the
// beams s0 .. s0 + ns - 1 (ns <= ST) of every frame of the slice; f_k = k val, and -N val at the Nyquist bin k = N
// (SimLoader::term's operation order).  One lane owns one bin, a workgroup 256 consecutive bins of one frame: every step of the
// loop over m is one coalesced 16-byte load per lane (the next one is issued before this one is used) that serves all ns beams.
// The frame's delays and weights are uniform over the workgroup and come through LDS, 64 microphones at a time.
// Exponents: a frame row's is in its flag word (k_row_nonzero); a beam's is e = ilogb(sum_m |w_m| 2^e_m) over the live rows, Y leaves
// times 2^-e and SimStorer multiplies 2^e back, so a beam never sees the amplitude of the beam it shares a transform with.  A beam
// without a live weighted row (all weights zero, or only silent rows) is marked dead: zero spectrum here, zero row in k_steer_silence.
template <int ST>
__global__ __launch_bounds__(256) void k_steer_sum(const cd* __restrict__ X, const int* __restrict__ flags, const double* __restrict__ delays,
                                                   const double* __restrict__ weights, int M, int N, int S, int s0, int ns, double val,
                                                   cd* __restrict__ Y, int* __restrict__ beam_exp, int* __restrict__ beam_live) {
  __shared__ double sd[ST][kSteerMics], sw[ST][kSteerMics], samp[kSteerMics];
  const int H = N + 1, f = blockIdx.y, tid = threadIdx.x;
  const int k = blockIdx.x * kSteerBins + tid;
  const bool in_row = k < H;
  const int kk = in_row ? k : H - 1;                          // lanes past the row compute bin N again and store nothing
  const double fk = kk == N ? -double(N) * val : double(kk) * val;   // fftfreq: bin N carries -fs/2
  const double a = -6.283185307179586 * fk;
  const cd* x = X + size_t(f) * size_t(M) * size_t(H) + size_t(kk);
  double ax[ST], ay[ST], top[ST];
#pragma unroll
  for (int q = 0; q < ST; ++q) ax[q] = ay[q] = top[q] = 0.0;
  for (int m0 = 0; m0 < M; m0 += kSteerMics) {
    const int mt = M - m0 < kSteerMics ? M - m0 : kSteerMics;
    __syncthreads();                                          // the previous tile has been read
    for (int i = tid; i < ST * kSteerMics; i += kSteerBins) {
      const int q = i / kSteerMics, m = i % kSteerMics;
      const bool on = q < ns && m < mt;
      const size_t at = (size_t(f) * size_t(S) + size_t(s0 + (on ? q : 0))) * size_t(M) + size_t(m0 + (on ? m : 0));
      sd[q][m] = on ? delays[at] : 0.0;
      sw[q][m] = on ? weights[at] : 0.0;
    }
    if (tid < kSteerMics) {
      const int fl = tid < mt ? flags[size_t(f) * size_t(M) + size_t(m0 + tid)] : 0;
      samp[tid] = fl ? ldexp(1.0, flag_exponent(fl)) : 0.0;   // 2^e_m of a live row
    }
    __syncthreads();
    cd nxt = x[size_t(m0) * size_t(H)];
    for (int m = 0; m < mt; ++m) {
      const cd xv = nxt;
      if (m + 1 < mt) nxt = x[size_t(m0 + m + 1) * size_t(H)];   // (two and three loads ahead measured no faster: DESIGN 6j)
      const double amp = samp[m];
#pragma unroll
      for (int q = 0; q < ST; ++q) {
        if (q < ns) {                                         // (uniform)
          double s, c;
          sincos(a * sd[q][m], &s, &c);
          const cd t = cmul(xv, mk(c, s));
          const double w = sw[q][m];
          ax[q] = ax[q] + w * t.x;
          ay[q] = ay[q] + w * t.y;
          top[q] = top[q] + fabs(w) * amp;
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < ST; ++q) {
    if (q < ns) {
      const bool live = top[q] > 0.0;
      const int e = row_exponent(top[q]);
      const size_t row = size_t(f) * size_t(S) + size_t(s0 + q);
      if (in_row) Y[row * size_t(H) + size_t(k)] = live ? mk(ldexp(ax[q], -e), ldexp(ay[q], -e)) : mk(0, 0);
      if (blockIdx.x == 0 && tid == 0) {
        beam_exp[row] = e;
        beam_live[row] = live ? 1 : 0;
      }
    }
  }
}

// What the null-steering beams of one frame share and no bin changes: q[s] = sum_m g[s,m]^2 (the real diagonal of G), top[s] = sum_m
// |g[s,m]| 2^e_m over the live rows as in k_steer_sum, both m ascending; delta = loading max_s q[s]; the loaded diagonal q[s] + delta (1
// where that is 0: a source without gains under loading 0, whose row and column of G are zeros).
// Exponents: the rows of a frame are coupled by the solve, so one exponent serves them all, e = ilogb((sum_t top_t) / delta), t
// ascending (|(G + delta I)^-1| <= 1 / delta; with loading 0, one source, the divisor is q[0]); it goes into each of the frame's S
// entries of beam_exp.  A frame without a live weighted row is S dead beams; a source without gains is a dead beam beside live ones.
// One workgroup of one wavefront per frame, lane s sums source s.
__global__ __launch_bounds__(64) void k_separate_frame(const int* __restrict__ flags, const double* __restrict__ gains, int M, int S,
                                                       double loading, double* __restrict__ diag, int* __restrict__ beam_exp,
                                                       int* __restrict__ beam_live) {
  __shared__ double stop[kSeparateMax], sq[kSeparateMax];
  const int f = blockIdx.x, q = threadIdx.x;
  if (q < S) {
    const double* g = gains + (size_t(f) * size_t(S) + size_t(q)) * size_t(M);
    const int* fl = flags + size_t(f) * size_t(M);
    double top = 0.0, qq = 0.0;
    for (int m = 0; m < M; ++m) {
      const double w = g[m];
      const double amp = fl[m] ? ldexp(1.0, flag_exponent(fl[m])) : 0.0;   // 2^e_m of a live row
      top = top + fabs(w) * amp;
      qq = qq + w * w;
    }
    stop[q] = top;
    sq[q] = qq;
  }
  __syncthreads();
  if (q < S) {
    double sumtop = 0.0, qmax = 0.0;
    for (int t = 0; t < S; ++t) {
      sumtop = sumtop + stop[t];
      qmax = sq[t] > qmax ? sq[t] : qmax;
    }
    const bool alive = sumtop > 0.0;
    const double delta = loading * qmax;
    const double dg = sq[q] + delta;
    const size_t row = size_t(f) * size_t(S) + size_t(q);
    diag[row] = dg == 0.0 ? 1.0 : dg;
    beam_exp[row] = alive ? row_exponent(sumtop / (delta > 0.0 ? delta : qmax)) : 0;
    beam_live[row] = alive && sq[q] > 0.0 ? 1 : 0;
  }
}

// The null-steering beams (beamform.py, separate): Z[f,:,k] = (G + delta I)^-1 Y with Y as k_steer_sum forms it (weights = gains, the
// same operations in the same order, all S <= ST beams in one pass) and G[s,t] = sum_m (g[s,m] g[t,m]) p[s,m] conj(p[t,m]), t < s, the
// Gram matrix of the steering vectors.  The launch shape, the LDS tiles and the load ahead are k_steer_sum's; every (s, m) phase is
// evaluated once and updates Y[s] and the row and column s of G's lower triangle, all in registers: ST (ST - 1) / 2 + ST complex
// accumulators per lane.  After the loop the lane factors and solves in registers (separate_math.h holds the operation order) with
// the frame's loaded diagonal, exponent and live marks from k_separate_frame: they are uniform over the grid's row, so they cost the
// lanes no registers and no work per microphone.
template <int ST>
__global__ __launch_bounds__(256) void k_separate(const cd* __restrict__ X, const double* __restrict__ delays, const double* __restrict__ gains,
                                                  int M, int N, int S, double val, const double* __restrict__ diag,
                                                  const int* __restrict__ beam_exp, const int* __restrict__ beam_live, cd* __restrict__ Z) {
  constexpr int NT = sep_tri_count(ST);
  __shared__ double sd[ST][kSteerMics], sw[ST][kSteerMics];
  const int H = N + 1, f = blockIdx.y, tid = threadIdx.x, ns = S;
  const int k = blockIdx.x * kSteerBins + tid;
  const bool in_row = k < H;
  const int kk = in_row ? k : H - 1;                          // lanes past the row compute bin N again and store nothing
  const double fk = kk == N ? -double(N) * val : double(kk) * val;   // fftfreq: bin N carries -fs/2
  const double a = -6.283185307179586 * fk;
  const cd* x = X + size_t(f) * size_t(M) * size_t(H) + size_t(kk);
  double ax[ST], ay[ST], gre[NT + 1], gim[NT + 1];
#pragma unroll
  for (int q = 0; q < ST; ++q) ax[q] = ay[q] = 0.0;
#pragma unroll
  for (int q = 0; q < NT + 1; ++q) gre[q] = gim[q] = 0.0;
  for (int m0 = 0; m0 < M; m0 += kSteerMics) {
    const int mt = M - m0 < kSteerMics ? M - m0 : kSteerMics;
    __syncthreads();                                          // the previous tile has been read
    for (int i = tid; i < ST * kSteerMics; i += kSteerBins) {
      const int q = i / kSteerMics, m = i % kSteerMics;
      const bool on = q < ns && m < mt;
      const size_t at = (size_t(f) * size_t(S) + size_t(on ? q : 0)) * size_t(M) + size_t(m0 + (on ? m : 0));
      sd[q][m] = on ? delays[at] : 0.0;
      sw[q][m] = on ? gains[at] : 0.0;
    }
    __syncthreads();
    cd nxt = x[size_t(m0) * size_t(H)];
    for (int m = 0; m < mt; ++m) {
      const cd xv = nxt;
      if (m + 1 < mt) nxt = x[size_t(m0 + m + 1) * size_t(H)];
      cd ph[ST];
#pragma unroll
      for (int q = 0; q < ST; ++q) {
        if (q < ns) {                                         // (uniform)
          double s, c;
          sincos(a * sd[q][m], &s, &c);
          ph[q] = mk(c, s);
          const cd t = cmul(xv, ph[q]);
          const double w = sw[q][m];
          ax[q] = ax[q] + w * t.x;
          ay[q] = ay[q] + w * t.y;
        }
      }
#pragma unroll
      for (int s = 1; s < ST; ++s) {
        if (s < ns) {
#pragma unroll
          for (int t = 0; t < s; ++t) {
            const double gg = sw[s][m] * sw[t][m];
            const cd c = cmulc(ph[s], ph[t]);
            gre[sep_tri(s, t)] = gre[sep_tri(s, t)] + gg * c.x;
            gim[sep_tri(s, t)] = gim[sep_tri(s, t)] + gg * c.y;
          }
        }
      }
    }
  }
  const size_t row0 = size_t(f) * size_t(S);
  const int e = beam_exp[row0];
  bool alive = false;                                         // (uniform: the marks are the frame's)
#pragma unroll
  for (int q = 0; q < ST; ++q)
    if (q < ns && beam_live[row0 + size_t(q)]) alive = true;
  if (alive) {
    double dg[ST];
#pragma unroll
    for (int q = 0; q < ST; ++q) dg[q] = q < ns ? diag[row0 + size_t(q)] : 1.0;
    separate_solve<ST>(ns, dg, gre, gim, ax, ay);
  }
  if (in_row) {
#pragma unroll
    for (int q = 0; q < ST; ++q) {
      if (q < ns) {
        const size_t row = row0 + size_t(q);
        Z[row * size_t(H) + size_t(k)] = beam_live[row] ? mk(ldexp(ax[q], -e), ldexp(ay[q], -e)) : mk(0, 0);
      }
    }
  }
}

// the half spectra of two beams -> one complex transform of 2N points (SimLoader::operator()'s mirror and Nyquist rules)
struct BeamLoader {
  static constexpr const char* kName = "BeamLoader";
  const cd* Y;            // beam spectra [rows][N + 1], each times 2^-e of its beam
  int rows, N, row0;      // row0: first row of this launch group
  const cd* w;
  __device__ cd term(int r, unsigned kk, bool nyquist, bool mirror) const {
    r += row0;
    if (r >= rows) return mk(0, 0);
    cd z = Y[size_t(r) * size_t(N + 1) + kk];
    if (nyquist) z.y = 0;                                   // only the real part of bin N survives .real
    if (mirror) z.y = -z.y;
    return z;
  }
  __device__ cd operator()(int g, unsigned j) const {
    const unsigned n = 2u * unsigned(N);
    if (j >= n) return mk(0, 0);
    const bool mirror = j > unsigned(N), nyq = j == unsigned(N);
    const unsigned kk = mirror ? n - j : j;
    const cd z1 = term(2 * g, kk, nyq, mirror);
    const cd z2 = term(2 * g + 1, kk, nyq, mirror);
    return cmul(mk(z1.x - z2.y, z1.y + z2.x), w[j]);
  }
};

// a dead beam (k_steer_sum) shares its transform with a live one and carries that one's rounding noise: written as zeros
__global__ __launch_bounds__(256) void k_steer_silence(double* __restrict__ out, int L, const int* __restrict__ beam_live) {
  if (beam_live[blockIdx.x]) return;                          // (uniform over the workgroup)
  double* y = out + size_t(blockIdx.x) * size_t(L);
  for (int i = threadIdx.x; i < L; i += 256) y[i] = 0.0;
}

#include "mvdr_kernels.h"

template <int ST>
void launch_steer_sum(dim3 grid, hipStream_t on, const cd* X, const int* flags, const double* delays, const double* weights, int M, int N,
                      int S, int s0, int ns, double val, cd* Y, int* beam_exp, int* beam_live) {
  k_steer_sum<ST><<<grid, dim3(kSteerBins), 0, on>>>(X, flags, delays, weights, M, N, S, s0, ns, val, Y, beam_exp, beam_live);
}

template <int ST>
void launch_separate(dim3 grid, hipStream_t on, const cd* X, const double* delays, const double* gains, int M, int N, int S, double val,
                     const double* diag, const int* beam_exp, const int* beam_live, cd* Z) {
  k_separate<ST><<<grid, dim3(kSteerBins), 0, on>>>(X, delays, gains, M, N, S, val, diag, beam_exp, beam_live, Z);
}

}  // namespace

int Engine::steer_check(int B, int M, int L, double fs, int S) {
  if (B < 1 || M < 1 || S < 1) return fail(PAL_ERR_INVALID, "need B >= 1, M >= 1, S >= 1 (got %d, %d, %d)", B, M, S);
  if (!(fs > 0) || !std::isfinite(fs)) return fail(PAL_ERR_INVALID, "fs must be positive and finite");
  if (L < 100) return fail(PAL_ERR_INVALID, "steering needs at least 100 samples (fade slice of signal_processing.py:75-78)");
  if (L > (1 << 19)) return fail(PAL_ERR_UNSUPPORTED, "frame length %d exceeds 2^19", L);
  if (int64_t(B) * M > INT32_MAX / 2 || int64_t(B) * S > INT32_MAX / 2) return fail(PAL_ERR_UNSUPPORTED, "too many rows");
  return PAL_OK;
}

int Engine::separate_check(int B, int M, int L, double fs, int S, double loading) {
  PAL_TRY(steer_check(B, M, L, fs, S));
  if (!std::isfinite(loading) || loading < 0) return fail(PAL_ERR_INVALID, "loading must be finite and >= 0");
  if (loading == 0 && S > 1) return fail(PAL_ERR_INVALID, "loading 0 with %d sources: bin 0 of the Gram matrix is singular", S);
  if (S > kSeparateMax) return fail(PAL_ERR_UNSUPPORTED, "%d sources per frame exceed %d (one solve cannot be split over passes)", S, kSeparateMax);
  return PAL_OK;
}

int Engine::steer_sum_dev(const double* d_frames, int B, int M, int L, double fs, const double* d_delays, const double* d_weights, int S,
                          double* d_out) {
  if (!d_frames || !d_delays || !d_weights || !d_out) return fail(PAL_ERR_INVALID, "NULL buffer");
  PAL_TRY(steer_check(B, M, L, fs, S));
  return beams_dev(d_frames, B, M, L, fs, d_delays, d_weights, S, d_out, false, 0.0);
}

int Engine::separate_dev(const double* d_frames, int B, int M, int L, double fs, const double* d_delays, const double* d_gains, int S,
                         double loading, double* d_out) {
  if (!d_frames || !d_delays || !d_gains || !d_out) return fail(PAL_ERR_INVALID, "NULL buffer");
  PAL_TRY(separate_check(B, M, L, fs, S, loading));
  return beams_dev(d_frames, B, M, L, fs, d_delays, d_gains, S, d_out, true, loading);
}

// what the two beamformers share: the table check, the slices of whole frames, the forward spectra, the beam spectra (k_steer_sum, or
// k_separate with `solve`), the packed inverse and the dead rows
int Engine::beams_dev(const double* d_frames, int B, int M, int L, double fs, const double* d_delays, const double* d_weights, int S,
                      double* d_out, bool solve, double loading) {
  Engine* e = this;
  Plan* pl = nullptr;
  PAL_TRY(get_plan(2 * L, L, L, &pl));
  if (pfa_forward_applies(*pl, L)) return fail(PAL_ERR_INTERNAL, "packed forward transform on a steering plan");
  int* status = nullptr;
  PAL_TRY(status_words(&status));
  const size_t ntab = size_t(B) * size_t(S) * size_t(M);
  k_steer_check<<<dim3(unsigned((ntab + 255) / 256)), dim3(256), 0, stream>>>(d_delays, d_weights, ntab, fs, double(L), status);
  PAL_TRY(check(hipGetLastError(), "k_steer_check"));
  // slices of whole frames: the spectra of one slice stay near 1 GiB (the bound of the SRP strips' slices), at most 32768 frames
  // (the grid's second dimension)
  const size_t H = size_t(pl->H);
  size_t per = (size_t(1) << 30) / (size_t(M) * H * sizeof(cd));
  if (beam_slice > 0) per = size_t(beam_slice);
  per = per < 1 ? 1 : (per > 32768 ? 32768 : per);
  const int F0 = int(per > size_t(B) ? size_t(B) : per);
  Carve cv;
  const size_t off_x = cv.take(size_t(F0) * M * H * sizeof(cd));
  const size_t off_y = cv.take(size_t(F0) * S * H * sizeof(cd));
  const size_t off_flags = cv.take(size_t(F0) * M * sizeof(int));
  const size_t off_exp = cv.take(size_t(F0) * S * sizeof(int));
  const size_t off_live = cv.take(size_t(F0) * S * sizeof(int));
  const size_t off_diag = solve ? cv.take(size_t(F0) * S * sizeof(double)) : 0;   // (last: the delay-and-sum layout is what it was)
  char* blk = nullptr;
  PAL_TRY(scratch(kWsBeam, cv.off, &blk));
  cd* X = reinterpret_cast<cd*>(blk + off_x);
  cd* Y = reinterpret_cast<cd*>(blk + off_y);
  int* flags = reinterpret_cast<int*>(blk + off_flags);
  int* beam_exp = reinterpret_cast<int*>(blk + off_exp);
  int* beam_live = reinterpret_cast<int*>(blk + off_live);
  double* diag = reinterpret_cast<double*>(blk + off_diag);
  const Conv& c = pl->inv;
  const int fl = int(0.01 * double(L));
  const double d = 1.0 / fs;
  const double val = 1.0 / (double(2 * L) * d);
  for (int f0 = 0; f0 < B; f0 += F0) {
    const int F = B - f0 < F0 ? B - f0 : F0;
    {
      ProfScope ps(e, "steer_forward_spectra");
      PAL_TRY(forward_spectra(*pl, d_frames + size_t(f0) * M * L, size_t(L), F * M, L, X, flags));
    }
    const double* dl = d_delays + size_t(f0) * S * M;
    const double* wt = d_weights + size_t(f0) * S * M;
    const dim3 grid(unsigned((H + kSteerBins - 1) / kSteerBins), unsigned(F));
    if (solve) {
      ProfScope ps(e, "k_separate");
      k_separate_frame<<<dim3(unsigned(F)), dim3(64), 0, stream>>>(flags, wt, M, S, loading, diag, beam_exp, beam_live);
      PAL_TRY(check(hipGetLastError(), "k_separate_frame"));
      if (S == 1) launch_separate<1>(grid, stream, X, dl, wt, M, L, S, val, diag, beam_exp, beam_live, Y);
      else if (S == 2) launch_separate<2>(grid, stream, X, dl, wt, M, L, S, val, diag, beam_exp, beam_live, Y);
      else if (S <= 4) launch_separate<4>(grid, stream, X, dl, wt, M, L, S, val, diag, beam_exp, beam_live, Y);
      else launch_separate<8>(grid, stream, X, dl, wt, M, L, S, val, diag, beam_exp, beam_live, Y);
    } else {
      ProfScope ps(e, "k_steer_sum");
      for (int s0 = 0; s0 < S; s0 += kSteerMaxTile) {
        const int ns = S - s0 < kSteerMaxTile ? S - s0 : kSteerMaxTile;
        if (ns == 1) launch_steer_sum<1>(grid, stream, X, flags, dl, wt, M, L, S, s0, ns, val, Y, beam_exp, beam_live);
        else if (ns == 2) launch_steer_sum<2>(grid, stream, X, flags, dl, wt, M, L, S, s0, ns, val, Y, beam_exp, beam_live);
        else if (ns <= 4) launch_steer_sum<4>(grid, stream, X, flags, dl, wt, M, L, S, s0, ns, val, Y, beam_exp, beam_live);
        else launch_steer_sum<8>(grid, stream, X, flags, dl, wt, M, L, S, s0, ns, val, Y, beam_exp, beam_live);
      }
    }
    PAL_TRY(check(hipGetLastError(), solve ? "k_separate" : "k_steer_sum"));
    const int rows = F * S;
    double* out = d_out + size_t(f0) * S * L;
    cd* W = nullptr;
    PAL_TRY(scratch(kWsWork, size_t(chunk) * c.M() * sizeof(cd), &W));
    {
      ProfScope ps(e, "steer_inverse");
      const int ntr = (rows + 1) / 2;
      for (int t0 = 0; t0 < ntr; t0 += chunk) {
        const int G = ntr - t0 < chunk ? ntr - t0 : chunk;
        const int r0 = 2 * t0;
        BeamLoader ld{Y, rows, L, r0, pl->w};
        SimStorer st{out, size_t(L), rows, L, L, fl, r0, fl > 1 ? 1.0 / double(fl - 1) : 0.0, fl > 1 ? -1.0 / double(fl - 1) : 0.0,
                     pl->w, beam_exp, 1};
        PAL_TRY(launch_cols_fwd(e, c, G, ld, W));
        PAL_TRY(launch_rows(e, c, G, W, true, 1.0));
        PAL_TRY(launch_cols_inv(e, c, G, W, st));
      }
      k_steer_silence<<<dim3(unsigned(rows)), dim3(256), 0, stream>>>(out, L, beam_live);
      PAL_TRY(check(hipGetLastError(), "k_steer_silence"));
    }
  }
  return PAL_OK;
}

int Engine::mvdr_check(int B, int M, int L, double fs, int G, int S, double loading) {
  PAL_TRY(steer_check(B, M, L, fs, S));
  if (G < 1 || B % G != 0) return fail(PAL_ERR_INVALID, "the %d frames do not split into %d groups", B, G);
  if (!std::isfinite(loading) || !(loading > 0)) return fail(PAL_ERR_INVALID, "loading must be finite and > 0");
  if (M > kMvdrMaxMics) return fail(PAL_ERR_UNSUPPORTED, "%d microphones exceed %d (one wavefront factors a bin)", M, kMvdrMaxMics);
  if (mvdr_unsupported(M, size_t(L) + 1))
    return fail(PAL_ERR_UNSUPPORTED, "the covariance triangle of %d microphones at %d samples exceeds %llu bytes", M, L,
                (unsigned long long)kMvdrTriangleBound);
  if ((S + 3) / 4 > 65535) return fail(PAL_ERR_UNSUPPORTED, "too many sources");
  return PAL_OK;
}

// MVDR beams (beamform.py, mvdr): per group of Q = B / G frames, sweep 1 adds every slice's spectra into the covariance triangle,
// k_mvdr_weights turns the triangle into W[s][m][H], sweep 2 applies W to every slice's spectra (kept where the group is one slice,
// formed again otherwise) and sends the rows through beams_dev's inverse.  Slices hold whole frames of one group.
int Engine::mvdr_dev(const double* d_frames, int B, int M, int L, double fs, const double* d_delays, const double* d_gains, int G, int S,
                     double loading, double* d_out, double* d_weights) {
  if (!d_frames || !d_delays || !d_gains || !d_out) return fail(PAL_ERR_INVALID, "NULL buffer");
  PAL_TRY(mvdr_check(B, M, L, fs, G, S, loading));
  Engine* e = this;
  Plan* pl = nullptr;
  PAL_TRY(get_plan(2 * L, L, L, &pl));
  if (pfa_forward_applies(*pl, L)) return fail(PAL_ERR_INTERNAL, "packed forward transform on a steering plan");
  int* status = nullptr;
  PAL_TRY(status_words(&status));
  const size_t ntab = size_t(G) * size_t(S) * size_t(M);
  k_steer_check<<<dim3(unsigned((ntab + 255) / 256)), dim3(256), 0, stream>>>(d_delays, d_gains, ntab, fs, double(L), status);
  PAL_TRY(check(hipGetLastError(), "k_steer_check"));
  const size_t H = size_t(pl->H);
  const int Q = B / G;
  const int F0 = mvdr_slice_frames(M, H, beam_slice, Q);
  const int nsl = mvdr_slice_count(Q, F0);
  const size_t wbytes = size_t(S) * M * H * sizeof(cd);
  Carve cv;
  const size_t off_x = cv.take(size_t(F0) * M * H * sizeof(cd));
  const size_t off_y = cv.take(size_t(F0) * S * H * sizeof(cd));
  const size_t off_flags = cv.take(size_t(F0) * M * sizeof(int));
  const size_t off_exp = cv.take(size_t(F0) * S * sizeof(int));
  const size_t off_live = cv.take(size_t(F0) * S * sizeof(int));
  const size_t off_r = cv.take(size_t(mvdr_triangle_bytes(M, H)));
  const size_t off_w = d_weights ? 0 : cv.take(wbytes);
  char* blk = nullptr;
  PAL_TRY(scratch(kWsBeam, cv.off, &blk));
  cd* X = reinterpret_cast<cd*>(blk + off_x);
  cd* Y = reinterpret_cast<cd*>(blk + off_y);
  int* flags = reinterpret_cast<int*>(blk + off_flags);
  int* row_exp = reinterpret_cast<int*>(blk + off_exp);
  int* beam_live = reinterpret_cast<int*>(blk + off_live);
  cd* R = reinterpret_cast<cd*>(blk + off_r);
  const Conv& c = pl->inv;
  const int fl = int(0.01 * double(L));
  const double val = 1.0 / (double(2 * L) * (1.0 / fs));
  const unsigned bin_tiles = unsigned((H + kMvdrBins - 1) / kMvdrBins);
  const int chunk_bins = int((H + 7) / 8);
  int ti, tj;
  mvdr_tile_shape(mvdr_tile, &ti, &tj);
  for (int g = 0; g < G; ++g) {
    const double* dl = d_delays + size_t(g) * S * M;
    const double* gn = d_gains + size_t(g) * S * M;
    cd* W = d_weights ? reinterpret_cast<cd*>(d_weights) + size_t(g) * S * M * H : reinterpret_cast<cd*>(blk + off_w);
    for (int sl = 0; sl < nsl; ++sl) {
      int f0, F;
      mvdr_slice_of(g, sl, Q, F0, &f0, &F);
      {
        ProfScope ps(e, "mvdr_forward_spectra_1");
        PAL_TRY(forward_spectra(*pl, d_frames + size_t(f0) * M * L, size_t(L), F * M, L, X, flags));
      }
      ProfScope ps(e, "k_mvdr_cov");
      const dim3 cov_grid(bin_tiles, unsigned(mvdr_tile_count(M, ti, tj)));
      if (ti == 4) k_mvdr_cov<4, 4><<<cov_grid, dim3(kMvdrBins), 0, stream>>>(X, M, int(H), F, sl == 0, R);
      else k_mvdr_cov<8, 4><<<cov_grid, dim3(kMvdrBins), 0, stream>>>(X, M, int(H), F, sl == 0, R);
      PAL_TRY(check(hipGetLastError(), "k_mvdr_cov"));
    }
    {
      ProfScope ps(e, "k_mvdr_weights");
      k_mvdr_weights<<<dim3(unsigned(8 * chunk_bins)), dim3(64), mvdr_weights_lds(M), stream>>>(R, dl, gn, M, L, S, val, loading, chunk_bins, W);
      PAL_TRY(check(hipGetLastError(), "k_mvdr_weights"));
    }
    for (int sl = 0; sl < nsl; ++sl) {
      int f0, F;
      mvdr_slice_of(g, sl, Q, F0, &f0, &F);
      if (nsl > 1) {                                          // a group of one slice still holds its spectra
        ProfScope ps(e, "mvdr_forward_spectra_2");
        PAL_TRY(forward_spectra(*pl, d_frames + size_t(f0) * M * L, size_t(L), F * M, L, X, flags));
      }
      const int rows = F * S;
      {
        ProfScope ps(e, "k_mvdr_apply");
        const unsigned row_blocks = unsigned((rows + 255) / 256);
        k_mvdr_rows<<<dim3(row_blocks), dim3(256), 0, stream>>>(flags, gn, M, S, rows, row_exp, beam_live);
        PAL_TRY(check(hipGetLastError(), "k_mvdr_rows"));
        if (S == 1)
          k_mvdr_apply<1, 8><<<dim3(bin_tiles, unsigned((F + 7) / 8), 1), dim3(kMvdrBins), 0, stream>>>(X, W, M, int(H), S, F, beam_live, Y, row_exp);
        else if (S == 2)
          k_mvdr_apply<2, 4><<<dim3(bin_tiles, unsigned((F + 3) / 4), 1), dim3(kMvdrBins), 0, stream>>>(X, W, M, int(H), S, F, beam_live, Y, row_exp);
        else
          k_mvdr_apply<4, 4><<<dim3(bin_tiles, unsigned((F + 3) / 4), unsigned((S + 3) / 4)), dim3(kMvdrBins), 0, stream>>>(X, W, M, int(H), S, F, beam_live, Y, row_exp);
        PAL_TRY(check(hipGetLastError(), "k_mvdr_apply"));
        k_mvdr_close<<<dim3(row_blocks), dim3(256), 0, stream>>>(rows, row_exp);
        PAL_TRY(check(hipGetLastError(), "k_mvdr_close"));
      }
      double* out = d_out + size_t(f0) * S * L;
      cd* work = nullptr;
      PAL_TRY(scratch(kWsWork, size_t(chunk) * c.M() * sizeof(cd), &work));
      ProfScope ps(e, "mvdr_inverse");
      const int ntr = (rows + 1) / 2;
      for (int t0 = 0; t0 < ntr; t0 += chunk) {
        const int n = ntr - t0 < chunk ? ntr - t0 : chunk;
        const int r0 = 2 * t0;
        MvdrLoader ld{Y, row_exp, rows, L, r0, pl->w};
        SimStorer st{out, size_t(L), rows, L, L, fl, r0, fl > 1 ? 1.0 / double(fl - 1) : 0.0, fl > 1 ? -1.0 / double(fl - 1) : 0.0,
                     pl->w, row_exp, 1};
        PAL_TRY(launch_cols_fwd(e, c, n, ld, work));
        PAL_TRY(launch_rows(e, c, n, work, true, 1.0));
        PAL_TRY(launch_cols_inv(e, c, n, work, st));
      }
      k_steer_silence<<<dim3(unsigned(rows)), dim3(256), 0, stream>>>(out, L, beam_live);
      PAL_TRY(check(hipGetLastError(), "k_steer_silence"));
    }
  }
  return PAL_OK;
}

}  // namespace pal

using namespace pal;

#define ENGINE(h)                                   \
  if (!(h)) return PAL_ERR_INVALID;                 \
  Engine* e = reinterpret_cast<Engine*>(h);         \
  if (hipSetDevice(e->device) != hipSuccess) return e->fail(PAL_ERR_HIP, "hipSetDevice(%d) failed", e->device)

#define UP(dst, src, bytes) PAL_TRY(e->check(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, e->stream), "upload"))
#define DOWN(dst, src, bytes) PAL_TRY(e->check(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->stream), "download"))

// the host forms check the tables as the device does: refused here before anything is uploaded
static int check_steer_tables(Engine* e, const double* delays, const double* weights, size_t ntab, double fs, int L) {
  for (size_t i = 0; i < ntab; ++i) {
    if (!std::isfinite(delays[i]) || !std::isfinite(weights[i])) return e->fail(PAL_ERR_INVALID, "a steering delay or weight is not finite");
    if (std::fabs(delays[i]) * fs > double(L)) return e->fail(PAL_ERR_INVALID, "a steering delay lies beyond the frame (|delay| fs > %d)", L);
  }
  return PAL_OK;
}

extern "C" {

int pal_steer_sum_dev(pal_handle h, const double* d_frames, int B, int M, int L, double fs, const double* d_delays,
                      const double* d_weights, int S, double* d_out) {
  ENGINE(h);
  return e->steer_sum_dev(d_frames, B, M, L, fs, d_delays, d_weights, S, d_out);
}

int pal_steer_sum(pal_handle h, const double* frames, int B, int M, int L, double fs, const double* delays, const double* weights, int S,
                  double* out) {
  ENGINE(h);
  if (!frames || !delays || !weights || !out) return e->fail(PAL_ERR_INVALID, "NULL buffer");
  PAL_TRY(e->steer_check(B, M, L, fs, S));
  const size_t nin = size_t(B) * M * L, ntab = size_t(B) * S * M, nout = size_t(B) * S * L;
  PAL_TRY(check_steer_tables(e, delays, weights, ntab, fs, L));
  double *dx = nullptr, *dt = nullptr, *dout = nullptr;
  PAL_TRY(e->scratch(kWsStageIn, nin * sizeof(double), &dx));
  PAL_TRY(e->scratch(kWsStageTable, 2 * ntab * sizeof(double), &dt));
  PAL_TRY(e->scratch(kWsStageOut, nout * sizeof(double), &dout));
  UP(dx, frames, nin * sizeof(double));
  UP(dt, delays, ntab * sizeof(double));
  UP(dt + ntab, weights, ntab * sizeof(double));
  PAL_TRY(e->check(hipStreamSynchronize(e->stream), "upload sync"));
  PAL_TRY(e->steer_sum_dev(dx, B, M, L, fs, dt, dt + ntab, S, dout));
  DOWN(out, dout, nout * sizeof(double));
  return pal_synchronize(h);
}

int pal_separate_dev(pal_handle h, const double* d_frames, int B, int M, int L, double fs, const double* d_delays, const double* d_gains,
                     int S, double loading, double* d_out) {
  ENGINE(h);
  return e->separate_dev(d_frames, B, M, L, fs, d_delays, d_gains, S, loading, d_out);
}

int pal_separate(pal_handle h, const double* frames, int B, int M, int L, double fs, const double* delays, const double* gains, int S,
                 double loading, double* out) {
  ENGINE(h);
  if (!frames || !delays || !gains || !out) return e->fail(PAL_ERR_INVALID, "NULL buffer");
  PAL_TRY(e->separate_check(B, M, L, fs, S, loading));
  PAL_TRY(check_steer_tables(e, delays, gains, size_t(B) * S * M, fs, L));
  const size_t nin = size_t(B) * M * L, ntab = size_t(B) * S * M, nout = size_t(B) * S * L;
  double *dx = nullptr, *dt = nullptr, *dout = nullptr;
  PAL_TRY(e->scratch(kWsStageIn, nin * sizeof(double), &dx));
  PAL_TRY(e->scratch(kWsStageTable, 2 * ntab * sizeof(double), &dt));
  PAL_TRY(e->scratch(kWsStageOut, nout * sizeof(double), &dout));
  UP(dx, frames, nin * sizeof(double));
  UP(dt, delays, ntab * sizeof(double));
  UP(dt + ntab, gains, ntab * sizeof(double));
  PAL_TRY(e->check(hipStreamSynchronize(e->stream), "upload sync"));
  PAL_TRY(e->separate_dev(dx, B, M, L, fs, dt, dt + ntab, S, loading, dout));
  DOWN(out, dout, nout * sizeof(double));
  return pal_synchronize(h);
}

int pal_mvdr_dev(pal_handle h, const double* d_frames, int B, int M, int L, double fs, const double* d_delays, const double* d_gains, int G,
                 int S, double loading, double* d_out, double* d_weights) {
  ENGINE(h);
  return e->mvdr_dev(d_frames, B, M, L, fs, d_delays, d_gains, G, S, loading, d_out, d_weights);
}

int pal_mvdr(pal_handle h, const double* frames, int B, int M, int L, double fs, const double* delays, const double* gains, int G, int S,
             double loading, double* out, double* weights) {
  ENGINE(h);
  if (!frames || !delays || !gains || !out) return e->fail(PAL_ERR_INVALID, "NULL buffer");
  PAL_TRY(e->mvdr_check(B, M, L, fs, G, S, loading));
  const size_t nin = size_t(B) * M * L, ntab = size_t(G) * S * M, nout = size_t(B) * S * L;
  const size_t nw = weights ? 2 * ntab * (size_t(L) + 1) : 0;
  PAL_TRY(check_steer_tables(e, delays, gains, ntab, fs, L));
  double *dx = nullptr, *dt = nullptr, *dout = nullptr;
  PAL_TRY(e->scratch(kWsStageIn, nin * sizeof(double), &dx));
  PAL_TRY(e->scratch(kWsStageTable, 2 * ntab * sizeof(double), &dt));
  PAL_TRY(e->scratch(kWsStageOut, (nout + nw) * sizeof(double), &dout));
  UP(dx, frames, nin * sizeof(double));
  UP(dt, delays, ntab * sizeof(double));
  UP(dt + ntab, gains, ntab * sizeof(double));
  PAL_TRY(e->check(hipStreamSynchronize(e->stream), "upload sync"));
  PAL_TRY(e->mvdr_dev(dx, B, M, L, fs, dt, dt + ntab, G, S, loading, dout, weights ? dout + nout : nullptr));
  DOWN(out, dout, nout * sizeof(double));
  if (weights) DOWN(weights, dout + nout, nw * sizeof(double));
  return pal_synchronize(h);
}

}  // extern "C"
