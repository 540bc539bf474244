// mvdr_kernels.h - the kernels of the MVDR beamformer (specification: pyaudiolocalization_amd/beamform.py, mvdr), included by
// beamform.hip inside pal's unnamed namespace.  Per group of Q frames and per bin k of the half spectrum (H = L + 1 bins):
//
//   k_mvdr_cov      R[tri(i,j)][k] += sum over the slice's frames of X[f,i,k] conj(X[f,j,k]), j <= i     (the packed lower triangle)
//   k_mvdr_weights  delta = loading tr(R) / M, the Cholesky factor of R + delta I, and per source s the steering vector a, u = L^-1 a,
//                   den = |u|^2, w = L^-H u / den  ->  W[s][m][k]
//   k_mvdr_rows     a slice's live marks (a frame with a live row, a source with gains) and its rows' exponents, not yet known
//   k_mvdr_apply    Y[f,s,k] = sum_m conj(W[s,m,k]) X[f,m,k], and each row's exponent from its own spectrum (atomicMax of ilogb)
//   k_mvdr_close    rows whose spectrum held nothing keep the exponent 0
//   MvdrLoader      BeamLoader with every row scaled by 2^-e of that row on the way into the inverse transform
//
// The products are written out as the specification writes them and the file is built with -ffp-contract=off.  The sums of
// k_mvdr_cov (frames ascending, continuing from the stored value), of the factor and of the forward substitution (k ascending) and of
// k_mvdr_apply (m ascending) run in the specification's order; the back substitution subtracts its terms k descending (the column
// form: z[k] is final before any row uses it), where the specification goes ascending.
// (beamform.hip includes <climits> and mvdr_geometry.h before it opens the namespace.)
#pragma once

constexpr int kMvdrNoExp = INT_MIN;       // a row's exponent before k_mvdr_apply has seen its spectrum
constexpr int kMvdrSolveTile = 4;         // sources whose substitutions k_mvdr_weights runs side by side

// One lane per bin, 256 consecutive bins per workgroup (blockIdx.x), one TI x TJ tile of microphone pairs per workgroup (blockIdx.y,
// mvdr_tile_of): every load is one coalesced 16-byte load, a frame costs TI + TJ of them for TI TJ updates.  Each (pair, bin) has one
// owner: no atomics.  `first`: the group's first slice starts from zero, the later ones from what is stored, so a sliced group
// gives the bytes of the unsliced one.  Pairs of a tile above the diagonal or beyond M are computed on clamped rows and dropped.
template <int TI, int TJ>
__global__ __launch_bounds__(256) void k_mvdr_cov(const cd* __restrict__ X, int M, int H, int F, int first, cd* __restrict__ R) {
  int bi, bj;
  mvdr_tile_of(int(blockIdx.y), M, TI, TJ, &bi, &bj);
  const int i0 = bi * TI, j0 = bj * TJ;
  const int k = blockIdx.x * kMvdrBins + threadIdx.x;
  const bool in_row = k < H;
  const size_t kk = size_t(in_row ? k : H - 1);             // lanes past the row compute the last bin again and store nothing
  double re[TI][TJ], im[TI][TJ];
#pragma unroll
  for (int a = 0; a < TI; ++a) {
#pragma unroll
    for (int c = 0; c < TJ; ++c) {
      re[a][c] = im[a][c] = 0.0;
      if (!first && mvdr_owned(i0 + a, j0 + c, M)) {           // (uniform)
        const cd v = R[size_t(mvdr_tri(i0 + a, j0 + c)) * size_t(H) + kk];
        re[a][c] = v.x;
        im[a][c] = v.y;
      }
    }
  }
  unsigned ri[TI], rj[TJ];                                    // M H < 2^31 elements (steer_check: L <= 2^19)
#pragma unroll
  for (int a = 0; a < TI; ++a) ri[a] = unsigned(i0 + a < M ? i0 + a : M - 1) * unsigned(H);
#pragma unroll
  for (int c = 0; c < TJ; ++c) rj[c] = unsigned(j0 + c < M ? j0 + c : M - 1) * unsigned(H);
  const cd* x = X + kk;
  for (int f = 0; f < F; ++f, x += size_t(M) * size_t(H)) {
    cd xi[TI], xj[TJ];
#pragma unroll
    for (int a = 0; a < TI; ++a) xi[a] = x[ri[a]];
#pragma unroll
    for (int c = 0; c < TJ; ++c) xj[c] = x[rj[c]];
#pragma unroll
    for (int a = 0; a < TI; ++a) {
#pragma unroll
      for (int c = 0; c < TJ; ++c) {
        re[a][c] = re[a][c] + (xi[a].x * xj[c].x + xi[a].y * xj[c].y);
        im[a][c] = im[a][c] + (xi[a].y * xj[c].x - xi[a].x * xj[c].y);
      }
    }
  }
  if (!in_row) return;
#pragma unroll
  for (int a = 0; a < TI; ++a) {
#pragma unroll
    for (int c = 0; c < TJ; ++c)
      if (mvdr_owned(i0 + a, j0 + c, M)) R[size_t(mvdr_tri(i0 + a, j0 + c)) * size_t(H) + kk] = mk(re[a][c], im[a][c]);
  }
}

// One wavefront per bin, the bin's triangle in LDS (mvdr_weights_lds(M) bytes), lane i owns row i of the factor.  Left-looking: for
// column j lane i >= j forms R[i,j] - sum_{k<j} L[i,k] conj(L[j,k]), k ascending (lane j's is the pivot s, its 1 / sqrt stays in lane
// j and is handed round by a shuffle; the diagonal of L is never stored).  The substitutions are column forms too: lane k finishes
// u[k] (z[k]), every lane below (above) subtracts its product with it; the steps of one source depend on each other through two
// shuffles, so four sources go side by side.  Consecutive bins go to workgroups that share an XCD's L2
// (bin = (block % 8) chunk + block / 8): a 128-byte line of R holds the entries of 8 consecutive bins.
__global__ __launch_bounds__(64) void k_mvdr_weights(const cd* __restrict__ R, const double* __restrict__ delays,
                                                     const double* __restrict__ gains, int M, int N, int S, double val, double loading,
                                                     int chunk, cd* __restrict__ W) {
  extern __shared__ __attribute__((aligned(16))) char mvdr_smem[];
  cd* Ls = reinterpret_cast<cd*>(mvdr_smem);
  const int H = N + 1, lane = threadIdx.x;
  const int k = int(blockIdx.x % 8) * chunk + int(blockIdx.x / 8);
  if (k >= H) return;                                         // (uniform: the last chunk may be short)
  const int T = mvdr_tri_count(M);
  for (int t = lane; t < T; t += 64) Ls[t] = R[size_t(t) * size_t(H) + size_t(k)];
  __syncthreads();
  double tr = 0.0;
  for (int i = 0; i < M; ++i) tr = tr + Ls[mvdr_tri(i, i)].x;
  const double delta = loading * (tr / double(M));
  const bool active = lane < M;
  const int i = active ? lane : M - 1;                        // idle lanes shadow the last row and store nothing
  double rinv = 0.0;                                          // 1 / L[i,i], known once column i is done
  for (int j = 0; j < M; ++j) {
    const int row = i >= j ? i : j;                           // lanes above the column shadow the pivot's row
    cd v = Ls[mvdr_tri(row, j)];
    if (row == j) {
      const double dg = v.x + delta;
      v = mk(dg == 0.0 ? 1.0 : dg, 0.0);                      // a silent bin
    }
#pragma unroll 4
    for (int q = 0; q < j; ++q) {
      const cd a = Ls[mvdr_tri(row, q)], c = Ls[mvdr_tri(j, q)];
      v.x = v.x - (a.x * c.x + a.y * c.y);
      v.y = v.y - (a.y * c.x - a.x * c.y);
    }
    const double r = 1.0 / __dsqrt_rn(__shfl(v.x, j, 64));
    if (i == j) rinv = r;
    if (active && i > j) Ls[mvdr_tri(i, j)] = mk(v.x * r, v.y * r);
    __syncthreads();                                          // column j is read by every later column
  }
  const double fk = k == N ? -double(N) * val : double(k) * val;   // fftfreq: bin N carries -fs/2
  const double ang = -6.283185307179586 * fk;
  for (int s0 = 0; s0 < S; s0 += kMvdrSolveTile) {            // kMvdrSolveTile sources share every load of L and overlap their shuffles
    size_t at[kMvdrSolveTile];
    cd v[kMvdrSolveTile], u[kMvdrSolveTile];
    double den[kMvdrSolveTile];
#pragma unroll
    for (int t = 0; t < kMvdrSolveTile; ++t) {
      at[t] = size_t(s0 + t < S ? s0 + t : S - 1) * size_t(M) + size_t(i);   // slots past S repeat the last source and store nothing
      double sn, cs;
      sincos(ang * delays[at[t]], &sn, &cs);
      const double g = gains[at[t]];
      v[t] = mk(g * cs, g * -sn);                             // a = gains conj(p)
      u[t] = mk(0, 0);
      den[t] = 0.0;
    }
    for (int q = 0; q < M; ++q) {                             // u = L^-1 a, and den = sum_i |u[i]|^2 as each u[i] becomes final
      const cd l = Ls[i > q ? mvdr_tri(i, q) : 0];            // L[i,q] below the diagonal (else: any entry, unused)
#pragma unroll
      for (int t = 0; t < kMvdrSolveTile; ++t) {
        const cd mine = mk(v[t].x * rinv, v[t].y * rinv);
        const cd uq = mk(__shfl(mine.x, q, 64), __shfl(mine.y, q, 64));
        den[t] = den[t] + (uq.x * uq.x + uq.y * uq.y);
        if (i == q) u[t] = mine;
        if (i > q) {
          v[t].x = v[t].x - (l.x * uq.x - l.y * uq.y);
          v[t].y = v[t].y - (l.x * uq.y + l.y * uq.x);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < kMvdrSolveTile; ++t) {
      den[t] = den[t] == 0.0 ? 1.0 : den[t];                  // a source without gains: w = 0
      v[t] = u[t];
    }
    for (int q = M - 1; q >= 0; --q) {                        // z = L^-H u, left in u
      const cd l = Ls[i < q ? mvdr_tri(q, i) : 0];            // L[q,i] above the diagonal (else: any entry, unused)
#pragma unroll
      for (int t = 0; t < kMvdrSolveTile; ++t) {
        const cd mine = mk(v[t].x * rinv, v[t].y * rinv);
        const cd zq = mk(__shfl(mine.x, q, 64), __shfl(mine.y, q, 64));
        if (i == q) u[t] = mine;
        if (i < q) {
          v[t].x = v[t].x - (l.x * zq.x + l.y * zq.y);
          v[t].y = v[t].y - (l.x * zq.y - l.y * zq.x);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < kMvdrSolveTile; ++t)
      if (active && s0 + t < S) W[at[t] * size_t(H) + size_t(k)] = mk(u[t].x / den[t], u[t].y / den[t]);
  }
}

// the rows of a slice before k_mvdr_apply: row (f, s) is live where frame f has a live microphone row and source s has a gain
__global__ __launch_bounds__(256) void k_mvdr_rows(const int* __restrict__ flags, const double* __restrict__ gains, int M, int S, int rows,
                                                   int* __restrict__ row_exp, int* __restrict__ beam_live) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= rows) return;
  const int f = row / S, s = row % S;
  bool heard = false, aimed = false;
  for (int m = 0; m < M; ++m) {
    heard = heard || flags[size_t(f) * size_t(M) + size_t(m)] != 0;
    aimed = aimed || gains[size_t(s) * size_t(M) + size_t(m)] != 0.0;
  }
  row_exp[row] = kMvdrNoExp;
  beam_live[row] = heard && aimed ? 1 : 0;
}

// Y[f,s,k] = sum_m conj(W[s,m,k]) X[f,m,k], m ascending.  One lane per bin, 256 bins per workgroup, a register tile of TS sources
// (blockIdx.z) x TF frames (blockIdx.y): a step over m is TS + TF coalesced 16-byte loads for TS TF products.  A row's exponent is
// taken from its own spectrum: a beam may lie 1e-10 below what the weights' bound allows (an interferer cancelled), so the largest
// part of the row, not a bound, decides what the row is scaled by beside its transform partner.  Dead rows are zero spectra.
template <int TS, int TF>
__global__ __launch_bounds__(256) void k_mvdr_apply(const cd* __restrict__ X, const cd* __restrict__ W, int M, int H, int S, int F,
                                                    const int* __restrict__ beam_live, cd* __restrict__ Y, int* __restrict__ row_exp) {
  const int k = blockIdx.x * kMvdrBins + threadIdx.x;
  const bool in_row = k < H;
  const size_t kk = size_t(in_row ? k : H - 1);
  const int f0 = blockIdx.y * TF, s0 = blockIdx.z * TS;
  const cd *x[TF], *w[TS];
#pragma unroll
  for (int p = 0; p < TF; ++p) x[p] = X + size_t(f0 + p < F ? f0 + p : F - 1) * size_t(M) * size_t(H) + kk;
#pragma unroll
  for (int q = 0; q < TS; ++q) w[q] = W + size_t(s0 + q < S ? s0 + q : S - 1) * size_t(M) * size_t(H) + kk;
  double re[TS][TF], im[TS][TF];
#pragma unroll
  for (int q = 0; q < TS; ++q) {
#pragma unroll
    for (int p = 0; p < TF; ++p) re[q][p] = im[q][p] = 0.0;
  }
  for (int m = 0; m < M; ++m) {
    cd xv[TF], wv[TS];
#pragma unroll
    for (int p = 0; p < TF; ++p) xv[p] = x[p][size_t(m) * size_t(H)];
#pragma unroll
    for (int q = 0; q < TS; ++q) wv[q] = w[q][size_t(m) * size_t(H)];
#pragma unroll
    for (int q = 0; q < TS; ++q) {
#pragma unroll
      for (int p = 0; p < TF; ++p) {
        re[q][p] = re[q][p] + (wv[q].x * xv[p].x + wv[q].y * xv[p].y);
        im[q][p] = im[q][p] + (wv[q].x * xv[p].y - wv[q].y * xv[p].x);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < TS; ++q) {
#pragma unroll
    for (int p = 0; p < TF; ++p) {
      if (s0 + q < S && f0 + p < F) {                         // (uniform)
        const int row = (f0 + p) * S + s0 + q;
        const bool live = beam_live[row] != 0;
        if (in_row) Y[size_t(row) * size_t(H) + kk] = live ? mk(re[q][p], im[q][p]) : mk(0, 0);
        double top = in_row && live ? fmax(fabs(re[q][p]), fabs(im[q][p])) : 0.0;
        for (int o = 32; o > 0; o >>= 1) top = fmax(top, __shfl_down(top, o, 64));
        if ((threadIdx.x & 63) == 0 && top > 0.0) atomicMax(row_exp + row, row_exponent(top));
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_mvdr_close(int rows, int* __restrict__ row_exp) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row < rows && row_exp[row] == kMvdrNoExp) row_exp[row] = 0;
}

// BeamLoader for rows stored at their own scale: row r enters the transform times 2^-ex[r] (SimStorer multiplies 2^ex[r] back), so
// a row never sees the amplitude of the row it shares a transform with
struct MvdrLoader {
  static constexpr const char* kName = "MvdrLoader";
  const cd* Y;            // beam spectra [rows][N + 1]
  const int* ex;          // [rows] exponent of each row (k_mvdr_apply, k_mvdr_close)
  int rows, N, row0;      // row0: first row of this launch group
  const cd* w;
  __device__ cd term(int r, unsigned kk, bool nyquist, bool mirror) const {
    r += row0;
    if (r >= rows) return mk(0, 0);
    const cd y = Y[size_t(r) * size_t(N + 1) + kk];
    cd z = mk(ldexp(y.x, -ex[r]), ldexp(y.y, -ex[r]));
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
