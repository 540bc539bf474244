// pal_api.hip - extern "C" surface of libpal_hip.so (include/pal_hip.h) and the engine's
// house-keeping: errors, scratch, HIP-event profiling, the RCCL gather.
#include <dlfcn.h>

#include <cmath>
#include <cstring>

#include "closure_tiles.h"
#include "engine.h"

namespace pal {

static std::string g_create_error;

int Engine::fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  err = buf;
  return code;
}

int Engine::check(hipError_t e, const char* what) {
  if (e == hipSuccess) return PAL_OK;
  const int code = e == hipErrorOutOfMemory ? PAL_ERR_NOMEM : PAL_ERR_HIP;
  return fail(code, "%s: %s", what, hipGetErrorString(e));
}

int Engine::scratch(Ws idx, size_t bytes, void** out) {
  if (ws_bytes[idx] < bytes) {
    if (ws[idx]) {                       // either stream may still be using the old block
      PAL_HIP(hipStreamSynchronize(stream));
      PAL_HIP(hipStreamSynchronize(stream2));
      PAL_HIP(hipStreamSynchronize(stream3));
      PAL_HIP(hipFree(ws[idx]));
      ws[idx] = nullptr;
      ws_bytes[idx] = 0;
    }
    PAL_HIP(hipMalloc(&ws[idx], bytes));
    PAL_HIP(hipMemsetAsync(ws[idx], 0, bytes, stream));
    PAL_HIP(hipStreamSynchronize(stream));   // the block may first be used on the other stream: zeroes must have landed
    ws_bytes[idx] = bytes;
  }
  *out = ws[idx];
  return PAL_OK;
}

// `lengths` is host memory: the copy has left it when this returns
int Engine::upload_lengths(const int32_t* lengths, int B, void* d_dst) {
  PAL_HIP(hipMemcpyAsync(d_dst, lengths, size_t(B) * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  return check(hipStreamSynchronize(stream), "lengths upload");
}

// ---- profiling: one event pair per launch, resolved after the stream drains ----
int Engine::prof_slot(const char* name) {
  for (size_t i = 0; i < slot_names.size(); ++i)
    if (slot_names[i] == name) return int(i);
  slot_names.emplace_back(name);
  slots.emplace_back();
  return int(slot_names.size() - 1);
}

static hipEvent_t take_event(Engine* e) {
  if (e->ev_used == e->ev_pool.size()) {
    hipEvent_t ev;
    if (hipEventCreate(&ev) != hipSuccess) return nullptr;
    e->ev_pool.push_back(ev);
  }
  return e->ev_pool[e->ev_used++];
}

void Engine::prof_begin(int, hipEvent_t* a, hipStream_t on) {
  if (pending.size() >= 16384) {
    hipStreamSynchronize(stream);
    hipStreamSynchronize(stream2);
    hipStreamSynchronize(stream3);
    prof_flush();
  }
  *a = take_event(this);
  if (*a) hipEventRecord(*a, on);
}

void Engine::prof_end(int slot, hipEvent_t a, hipStream_t on) {
  hipEvent_t b = take_event(this);
  if (!a || !b) return;
  hipEventRecord(b, on);
  pending.push_back({slot, a, b});
}

void Engine::prof_flush() {
  for (const Pending& p : pending) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
      slots[p.slot].ms += ms;
      slots[p.slot].launches += 1;
    }
  }
  pending.clear();
  ev_used = 0;
}

// ---- the status words (peak_types.h StatusWord): one read, then what was reported is cleared ----
static int check_status(Engine* e) {
  int* dev = static_cast<int*>(e->ws[kWsStatus]);
  if (!dev) return PAL_OK;
  int st[kStatusWords] = {};
  PAL_TRY(e->check(hipMemcpy(st, dev, sizeof st, hipMemcpyDeviceToHost), "status read"));
  if (getenv("PAL_DEBUG_FALLBACK")) {   // diagnostics: rows whose median needed the radix select since the last report
    if (st[kStRadixFallback]) {
      fprintf(stderr, "[pal] %d row(s) took the radix-select fallback\n", st[kStRadixFallback]);
      hipMemset(dev + kStRadixFallback, 0, sizeof(int));
    }
    if (st[kStExactMedian]) {
      fprintf(stderr, "[pal] %d row(s) needed the exact median (a threshold comparison inside the histogram interval)\n", st[kStExactMedian]);
      hipMemset(dev + kStExactMedian, 0, sizeof(int));
    }
    if (st[kStFlagged]) {
      const int* why = st + kStWhy;
      fprintf(stderr, "[pal] %d row(s) of the finishing column pass went through the stored-row path (no maximum / abandoned %d, tie %d, tie in window %d, "
                      "SNR window energy %d, histogram windows %d, threshold interval %d, window interval %d, window edge %d; waits given up %d)\n",
              st[kStFlagged], why[0], why[1], why[2], why[3], why[4], why[5], why[6], why[7], st[kStGaveUp]);
      hipMemset(dev + kStFlagged, 0, (1 + kStWhyCount) * sizeof(int));
      hipMemset(dev + kStGaveUp, 0, sizeof(int));
    }
  }
  if (st[kStInput]) {                        // input problems found by device-side checks
    hipMemset(dev + kStInput, 0, sizeof(int));
    if (st[kStInput] & kStInputBadRow) return e->fail(PAL_ERR_INVALID, "pair list references a row outside the frame batch");
    if (st[kStInput] & kStInputBadLag) return e->fail(PAL_ERR_INVALID, "a record of the TDOA table has k_sel outside 0..2 length - 2: the closure results of this call are not valid");
    if (st[kStInput] & kStInputBadCandidate)
      return e->fail(PAL_ERR_INVALID, "a candidate outside 0..2 length - 2, an absent candidate 0 or a gap in a pair's candidates: the consensus results of this call are not valid");
    if (st[kStInput] & kStInputBadSteer)
      return e->fail(PAL_ERR_INVALID, "a steering delay or weight that is not finite, or a delay beyond the frame (|delay| fs > length): the beams of this call are not valid");
    return e->fail(PAL_ERR_INVALID, "non-finite sample (NaN or infinity) in a frame: the pair packed with that microphone's "
                                    "pairs would be affected too, the table of this call is not valid");
  }
  if (st[kStOverflow]) {
    hipMemset(dev + kStOverflow, 0, sizeof(int));
    return e->fail(PAL_ERR_INTERNAL, "peak selection: suppression chain exceeded the on-chip memo/stack (rows fell back to argmax)");
  }
  return PAL_OK;
}

static int validate(Engine* e, const pal_phat_params* p) {
  if (!p) return e->fail(PAL_ERR_INVALID, "params is NULL");
  if (!(p->fs > 0)) return e->fail(PAL_ERR_INVALID, "fs must be positive");
  if (p->peak_distance < 1) return e->fail(PAL_ERR_INVALID, "`distance` must be greater or equal to 1");
  if (p->num_peaks < 1 || p->num_peaks > PAL_MAX_PEAKS)
    return e->fail(PAL_ERR_INVALID, "num_peaks %d outside 1..%d", p->num_peaks, PAL_MAX_PEAKS);
  if (p->threshold_method != 0 && p->threshold_method != 1) return e->fail(PAL_ERR_INVALID, "threshold_method must be 0 or 1");
  return PAL_OK;
}

// row-major i<j pairs of every trial, two pairs per complex transform
static void build_quads(int B, int M, std::vector<int4>& q) {
  const int64_t P = int64_t(M) * (M - 1) / 2, np = P * B;
  q.assign(size_t((np + 1) / 2), make_int4(0, 0, -1, -1));
  int64_t k = 0;
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < M; ++i)
      for (int j = i + 1; j < M; ++j, ++k) {
        int4& t = q[size_t(k / 2)];
        if (k & 1) { t.z = b * M + i; t.w = b * M + j; }
        else { t.x = b * M + i; t.y = b * M + j; }
      }
}

// The same pairs in blocks of `blk` x `blk` microphones (block rows I <= J; inside a block i ascending, j ascending): a launch group
// of 480 pairs then touches some 64 spectra instead of 480 (C4: 256 microphones - every pair of one row i brings its own spectrum j,
// 3 MB each).  perm[k] = row-major index of the pair processed k-th; the records are scattered back behind the call.
static void build_quads_blocked(int B, int M, int blk, std::vector<int4>& q, std::vector<int>& perm) {
  const int64_t P = int64_t(M) * (M - 1) / 2, np = P * B;
  q.assign(size_t((np + 1) / 2), make_int4(0, 0, -1, -1));
  perm.resize(size_t(np));
  int64_t k = 0;
  for (int b = 0; b < B; ++b)
    for (int I = 0; I < M; I += blk)
      for (int J = I; J < M; J += blk)
        for (int i = I; i < I + blk && i < M; ++i)
          for (int j = (J > i ? J : i + 1); j < J + blk && j < M; ++j, ++k) {
            int4& t = q[size_t(k / 2)];
            if (k & 1) { t.z = b * M + i; t.w = b * M + j; }
            else { t.x = b * M + i; t.y = b * M + j; }
            perm[size_t(k)] = int(int64_t(b) * P + pair_row(int64_t(i), int64_t(M)) + j);
          }
}

__global__ __launch_bounds__(256) void k_scatter_records(const pal_pair_record* __restrict__ src, const int* __restrict__ perm, int64_t n,
                                                         pal_pair_record* __restrict__ dst) {
  const int64_t k = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (k < n) dst[perm[k]] = src[k];
}

static int all_pairs_dev(Engine* e, const double* d_frames, int B, int M, int L, const pal_phat_params* prm,
                         pal_pair_record* d_table, double* d_corr, const CandOut* cands = nullptr) {
  PAL_TRY(validate(e, prm));
  if (B < 1 || M < 2 || L < 1) return e->fail(PAL_ERR_INVALID, "need B >= 1, M >= 2, L >= 1 (got %d, %d, %d)", B, M, L);
  if (int64_t(B) * M > INT32_MAX / 2) return e->fail(PAL_ERR_UNSUPPORTED, "too many rows");
  if (L > (1 << 20)) return e->fail(PAL_ERR_UNSUPPORTED, "frame length %d exceeds 2^20", L);
  Plan* pl = nullptr;
  PAL_TRY(e->get_plan(2 * L - 1, L, 2 * L - 1, &pl));
  const int rows = B * M;
  void* sp = nullptr;
  PAL_TRY(e->scratch(kWsSpectra, size_t(rows) * pl->spec_stride() * sizeof(cd) + size_t(rows) * sizeof(int), &sp));
  cd* spectra = static_cast<cd*>(sp);
  int* nonzero = reinterpret_cast<int*>(spectra + size_t(rows) * pl->spec_stride());   // per frame row: any non-zero sample
  PAL_TRY(e->forward_spectra(*pl, d_frames, size_t(L), rows, L, spectra, nonzero));
  // the pair table depends on (B, M) only: keep it on the device between calls of the same shape
  const size_t nquads = size_t((int64_t(B) * M * (M - 1) / 2 + 1) / 2);
  if (e->pair_block > 1 && M >= 96 && !d_corr && !cands && int64_t(B) * M * (M - 1) / 2 < INT32_MAX) {
    const int64_t np = int64_t(B) * M * (M - 1) / 2;
    if (e->blk_B != B || e->blk_M != M || !e->quads_blk) {
      std::vector<int4> quads;
      std::vector<int> perm;
      build_quads_blocked(B, M, e->pair_block, quads, perm);
      PAL_TRY(e->check(hipStreamSynchronize(e->stream), "stream sync"));
      if (e->quads_blk) { (void)hipFree(e->quads_blk); e->quads_blk = nullptr; }
      if (e->perm_blk) { (void)hipFree(e->perm_blk); e->perm_blk = nullptr; }
      PAL_TRY(e->check(hipMalloc(&e->quads_blk, nquads * sizeof(int4)), "quads alloc"));
      PAL_TRY(e->check(hipMalloc(&e->perm_blk, size_t(np) * sizeof(int)), "pair order alloc"));
      PAL_TRY(e->check(hipMemcpyAsync(e->quads_blk, quads.data(), nquads * sizeof(int4), hipMemcpyHostToDevice, e->stream), "quads"));
      PAL_TRY(e->check(hipMemcpyAsync(e->perm_blk, perm.data(), size_t(np) * sizeof(int), hipMemcpyHostToDevice, e->stream), "pair order"));
      PAL_TRY(e->check(hipStreamSynchronize(e->stream), "quads sync"));
      e->blk_B = B;
      e->blk_M = M;
    }
    void* tp = nullptr;
    PAL_TRY(e->scratch(kWsBlockTable, size_t(np) * sizeof(pal_pair_record), &tp));
    PAL_TRY(e->pair_correlations(*pl, spectra, rows, e->quads_blk, np, L, *prm, static_cast<pal_pair_record*>(tp), nullptr, nullptr, nonzero));
    k_scatter_records<<<dim3(unsigned((np + 255) / 256)), dim3(256), 0, e->stream>>>(static_cast<const pal_pair_record*>(tp), e->perm_blk, np, d_table);
    return e->check(hipGetLastError(), "k_scatter_records");
  }
  if (e->quad_B != B || e->quad_M != M || !e->quads) {
    std::vector<int4> quads;
    build_quads(B, M, quads);
    if (e->quads) { PAL_TRY(e->check(hipStreamSynchronize(e->stream), "stream sync")); (void)hipFree(e->quads); e->quads = nullptr; }
    PAL_TRY(e->check(hipMalloc(&e->quads, nquads * sizeof(int4)), "quads alloc"));
    PAL_TRY(e->check(hipMemcpyAsync(e->quads, quads.data(), nquads * sizeof(int4), hipMemcpyHostToDevice, e->stream), "quads"));
    PAL_TRY(e->check(hipStreamSynchronize(e->stream), "quads sync"));
    e->quad_B = B;
    e->quad_M = M;
  }
  void* qp = e->quads;
  const int64_t np = int64_t(B) * M * (M - 1) / 2;
  return e->pair_correlations(*pl, spectra, rows, static_cast<const int4*>(qp), np, L, *prm, d_table, nullptr, d_corr, nonzero, false, cands);
}

// Lag strips of every pair's row (srp.hip): the frames go through the pair pipeline in slices of whole frames whose rows
// [slice pairs][2L-1] sit in engine scratch - about 1 GiB where one frame's rows are less, otherwise one frame - and k_srp_strips cuts
// each slice's strips behind it on `stream` (the pipeline's side streams start behind `stream` and are joined into it, so a slice's rows
// are complete before they are read and read before the next slice overwrites them).  d_table (or nullptr): the one-peak table.
static int strips_dev(Engine* e, const double* d_frames, int B, int M, int L, const pal_phat_params* prm, int T, int W,
                      pal_pair_record* d_table, double* d_strips) {
  PAL_TRY(validate(e, prm));
  PAL_TRY(e->srp_strips_check(B, M, L, T, W));
  if (prm->num_peaks != 1) return e->fail(PAL_ERR_INVALID, "the strips call carries the one-peak table: num_peaks must be 1");
  const size_t P = size_t(M) * size_t(M - 1) / 2, n = size_t(2 * L - 1);
  const size_t frame_bytes = P * n * sizeof(double);
  const size_t fit = (size_t(1) << 30) / frame_bytes;
  const int per = int(fit < 1 ? 1 : (fit > size_t(B) ? size_t(B) : fit));
  Carve c;
  const size_t o_rows = c.take(size_t(per) * frame_bytes), o_tab = c.take(d_table ? 0 : size_t(per) * P * sizeof(pal_pair_record));
  char* base = nullptr;
  PAL_TRY(e->scratch(kWsSrp, c.off, &base));
  double* rows = reinterpret_cast<double*>(base + o_rows);
  for (int f0 = 0; f0 < B; f0 += per) {
    const int nb = B - f0 < per ? B - f0 : per;
    pal_pair_record* tab = d_table ? d_table + size_t(f0) * P : reinterpret_cast<pal_pair_record*>(base + o_tab);
    PAL_TRY(all_pairs_dev(e, d_frames + size_t(f0) * size_t(M) * size_t(L), nb, M, L, prm, tab, rows));
    PAL_TRY(e->srp_strips_rows(rows, int64_t(nb) * int64_t(P), L, T, W, d_strips + size_t(f0) * P * size_t(2 * T + 1)));
  }
  return PAL_OK;
}

// explicit pair list over R equal-length rows (host buffers): upload, then the device-resident form
static int pairs_host(Engine* e, const double* rows_in, int R, int L, const int32_t* pairs, int64_t P,
                      const pal_phat_params* prm, pal_pair_record* table) {
  PAL_TRY(validate(e, prm));
  if (!rows_in || !pairs || !table) return e->fail(PAL_ERR_INVALID, "NULL buffer");
  if (R < 1 || L < 1 || P < 1) return e->fail(PAL_ERR_INVALID, "need R >= 1, L >= 1, P >= 1");
  for (int64_t k = 0; k < 2 * P; ++k)
    if (pairs[k] < 0 || pairs[k] >= R) return e->fail(PAL_ERR_INVALID, "pair %lld references row outside 0..%d", (long long)(k / 2), R - 1);
  void *df = nullptr, *dt = nullptr, *dp = nullptr;
  PAL_TRY(e->scratch(kWsStageIn, size_t(R) * L * sizeof(double), &df));
  PAL_TRY(e->scratch(kWsStageTable, size_t(P) * sizeof(pal_pair_record), &dt));
  PAL_TRY(e->scratch(kWsStagePairs, size_t(2 * P) * sizeof(int32_t), &dp));
  PAL_TRY(e->check(hipMemcpyAsync(df, rows_in, size_t(R) * L * sizeof(double), hipMemcpyHostToDevice, e->stream), "rows upload"));
  PAL_TRY(e->check(hipMemcpyAsync(dp, pairs, size_t(2 * P) * sizeof(int32_t), hipMemcpyHostToDevice, e->stream), "pairs upload"));
  PAL_TRY(e->check(hipStreamSynchronize(e->stream), "upload sync"));
  PAL_TRY(e->pairs_dev(static_cast<const double*>(df), R, L, static_cast<const int32_t*>(dp), P, *prm, static_cast<pal_pair_record*>(dt)));
  return e->check(hipMemcpyAsync(table, dt, size_t(P) * sizeof(pal_pair_record), hipMemcpyDeviceToHost, e->stream), "table download");
}

}  // namespace pal

using namespace pal;

extern "C" {

int pal_abi_version(void) { return PAL_ABI_VERSION; }

int pal_create(int device, pal_handle* out) {
  if (!out) return PAL_ERR_INVALID;
  *out = nullptr;
  int count = 0;
  hipError_t rc = hipGetDeviceCount(&count);
  if (rc != hipSuccess || device < 0 || device >= count) {
    g_create_error = rc != hipSuccess ? std::string("hipGetDeviceCount: ") + hipGetErrorString(rc)
                                      : "device ordinal out of range (" + std::to_string(count) + " HIP devices visible)";
    return PAL_ERR_HIP;
  }
  Engine* e = new Engine();
  e->device = device;
  if ((rc = hipSetDevice(device)) != hipSuccess || (rc = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking)) != hipSuccess ||
      (rc = hipStreamCreateWithFlags(&e->stream2, hipStreamNonBlocking)) != hipSuccess ||
      (rc = hipStreamCreateWithFlags(&e->stream3, hipStreamNonBlocking)) != hipSuccess ||
      (rc = hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming)) != hipSuccess ||
      (rc = hipEventCreateWithFlags(&e->ev_join2, hipEventDisableTiming)) != hipSuccess ||
      (rc = hipEventCreateWithFlags(&e->ev_join3, hipEventDisableTiming)) != hipSuccess ||
      (rc = hipEventCreateWithFlags(&e->ev_fin, hipEventDisableTiming)) != hipSuccess) {
    g_create_error = std::string("device init: ") + hipGetErrorString(rc);
    delete e;
    return PAL_ERR_HIP;
  }
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) e->cu_count = cus;
  }
  const char* env = getenv("PAL_CHUNK");
  if (env && atoi(env) > 0) { e->chunk = atoi(env); e->chunk_auto = false; }
  env = getenv("PAL_OVERLAP");
  e->one_stream = env && atoi(env) == 0;
  env = getenv("PAL_RADIX3");
  if (env) e->plan_sw.allow_r3 = atoi(env) != 0;
  env = getenv("PAL_PFA");
  if (env) e->plan_sw.allow_pfa = atoi(env) != 0;
  env = getenv("PAL_RADER");
  if (env) e->plan_sw.allow_rader = atoi(env) != 0;
  env = getenv("PAL_PFA_BIG");
  if (env) e->plan_sw.allow_big = atoi(env) != 0;
  env = getenv("PAL_FOUR_REG");
  if (env) e->plan_sw.four_reg = atoi(env) != 0;
  env = getenv("PAL_XCD_ROWS");
  if (env) e->xcd_rows = atoi(env) != 0;
  env = getenv("PAL_ROWS_SHARED");
  if (env) e->rows_shared = atoi(env) != 0;
  env = getenv("PAL_PFA_FWD");
  if (env) e->pfa_forward = atoi(env) != 0;
  env = getenv("PAL_FUSED");
  if (env) e->fuse_peaks = atoi(env) != 0;
  env = getenv("PAL_R89");
  if (env) e->plan_sw.allow_r89 = atoi(env) != 0;
  env = getenv("PAL_FIN_SERIAL");
  if (env) e->fin_serial = atoi(env) != 0;
  env = getenv("PAL_FIN");
  if (env) e->fin_cols = atoi(env) != 0;
  env = getenv("PAL_ROWS_LEAN");
  if (env) e->rows_lean = atoi(env) != 0;
  env = getenv("PAL_PAIR_BLOCK");
  if (env) e->pair_block = atoi(env);
  env = getenv("PAL_ROWS_LEAN_MIN");
  if (env && atoll(env) >= 1) e->rows_lean_min = atoll(env);
  env = getenv("PAL_LEAN_STORE");
  if (env) e->lean_store = atoi(env) != 0;
  env = getenv("PAL_DEBUG_MEMO");
  if (env) e->debug_memo = atoi(env);
  env = getenv("PAL_DEBUG_FIN_WRAP");
  if (env && atoi(env) >= 2) e->fin_wrap = unsigned(atoi(env));
  env = getenv("PAL_FIN_STRIP");
  if (env) e->fin_strip_on = atoi(env) != 0;
  env = getenv("PAL_DEBUG_FIN_GIVEUP");
  if (env) e->fin_giveup = atoi(env) != 0 ? 1 : 0;
  env = getenv("PAL_MAX_PLANS");
  if (env && atoi(env) >= 2) e->max_plans = atoi(env);
  env = getenv("PAL_BEAM_SLICE");
  if (env && atoi(env) >= 1) e->beam_slice = atoi(env);
  env = getenv("PAL_MVDR_TILE");
  if (env) e->mvdr_tile = atoi(env);
  *out = reinterpret_cast<pal_handle>(e);
  return PAL_OK;
}

void pal_destroy(pal_handle h) {
  if (!h) return;
  Engine* e = reinterpret_cast<Engine*>(h);
  hipSetDevice(e->device);
  pal_comm_destroy(h);
  (void)e->clear_plans();                     // drains the three streams first
  for (cd* p : e->stage_tw) if (p) hipFree(p);
  for (cd* p : e->stage_twc) if (p) hipFree(p);
  for (void* p : e->ws) if (p) hipFree(p);
  if (e->quads) hipFree(e->quads);
  if (e->quads_blk) hipFree(e->quads_blk);
  if (e->perm_blk) hipFree(e->perm_blk);
  if (e->solve_idx) hipFree(e->solve_idx);
  for (hipEvent_t ev : e->ev_pool) hipEventDestroy(ev);
  hipStreamDestroy(e->stream2);
  hipStreamDestroy(e->stream3);
  hipEventDestroy(e->ev_fork);
  hipEventDestroy(e->ev_join2);
  hipEventDestroy(e->ev_join3);
  hipEventDestroy(e->ev_fin);
  hipStreamDestroy(e->stream);
  delete e;
}

const char* pal_last_error(pal_handle h) {
  if (!h) return g_create_error.c_str();
  return reinterpret_cast<Engine*>(h)->err.c_str();
}

#define ENGINE(h)                                   \
  if (!(h)) return PAL_ERR_INVALID;                 \
  Engine* e = reinterpret_cast<Engine*>(h);         \
  if (hipSetDevice(e->device) != hipSuccess) return e->fail(PAL_ERR_HIP, "hipSetDevice(%d) failed", e->device)

int pal_synchronize(pal_handle h) {
  ENGINE(h);
  PAL_TRY(e->check(hipStreamSynchronize(e->stream), "stream sync"));
  if (e->profiling) e->prof_flush();
  return check_status(e);
}

int pal_clear_plans(pal_handle h) {
  ENGINE(h);
  return e->clear_plans();
}

int pal_set_max_plans(pal_handle h, int max_plans) {
  ENGINE(h);
  if (max_plans < 2 || max_plans > 4096) return e->fail(PAL_ERR_INVALID, "max_plans %d outside 2..4096", max_plans);
  e->max_plans = max_plans;
  return PAL_OK;
}

int pal_plan_stats(pal_handle h, int64_t* built, int64_t* evicted) {
  ENGINE(h);
  if (built) *built = e->plans_built;
  if (evicted) *evicted = e->plans_evicted;
  return PAL_OK;
}

int pal_set_chunk(pal_handle h, int chunk) {
  ENGINE(h);
  if (chunk < 0 || chunk > 4096) return e->fail(PAL_ERR_INVALID, "chunk %d outside 0..4096", chunk);
  if (chunk > 0) { e->chunk = chunk; e->chunk_auto = false; }
  else { e->chunk = Engine::kDefaultChunk; e->chunk_auto = true; }   // 0: the default and the automatic pair group size again
  return PAL_OK;
}

int pal_device_alloc(pal_handle h, size_t bytes, void** dptr) {
  ENGINE(h);
  if (!dptr) return e->fail(PAL_ERR_INVALID, "dptr is NULL");
  return e->check(hipMalloc(dptr, bytes ? bytes : 1), "hipMalloc");
}

int pal_device_free(pal_handle h, void* dptr) {
  ENGINE(h);
  PAL_TRY(e->check(hipStreamSynchronize(e->stream), "stream sync"));
  PAL_TRY(e->check(hipStreamSynchronize(e->stream2), "stream sync"));
  PAL_TRY(e->check(hipStreamSynchronize(e->stream3), "stream sync"));
  return e->check(hipFree(dptr), "hipFree");
}

int pal_upload(pal_handle h, void* dptr, const void* host, size_t bytes) {
  ENGINE(h);
  PAL_TRY(e->check(hipMemcpyAsync(dptr, host, bytes, hipMemcpyHostToDevice, e->stream), "upload"));
  return e->check(hipStreamSynchronize(e->stream), "upload sync");
}

int pal_download(pal_handle h, void* host, const void* dptr, size_t bytes) {
  ENGINE(h);
  PAL_TRY(e->check(hipMemcpyAsync(host, dptr, bytes, hipMemcpyDeviceToHost, e->stream), "download"));
  return e->check(hipStreamSynchronize(e->stream), "download sync");
}

int pal_gcc_phat_all_pairs_dev(pal_handle h, const double* d_frames, int B, int M, int L, const pal_phat_params* prm,
                               pal_pair_record* d_table) {
  ENGINE(h);
  if (!d_frames || !d_table) return e->fail(PAL_ERR_INVALID, "NULL buffer");
  return all_pairs_dev(e, d_frames, B, M, L, prm, d_table, nullptr);
}

int pal_gcc_phat_all_pairs(pal_handle h, const double* frames, int B, int M, int L, const pal_phat_params* prm,
                           pal_pair_record* table, double* corr) {
  ENGINE(h);
  if (!frames || !table) return e->fail(PAL_ERR_INVALID, "NULL buffer");
  if (B < 1 || M < 2 || L < 1) return e->fail(PAL_ERR_INVALID, "need B >= 1, M >= 2, L >= 1 (got %d, %d, %d)", B, M, L);
  const size_t fbytes = size_t(B) * M * L * sizeof(double);
  const int64_t np = int64_t(B) * M * (M - 1) / 2;
  void *df = nullptr, *dt = nullptr, *dc = nullptr;
  PAL_TRY(e->scratch(kWsStageIn, fbytes, &df));
  PAL_TRY(e->scratch(kWsStageTable, size_t(np) * sizeof(pal_pair_record), &dt));
  if (corr) PAL_TRY(e->scratch(kWsStageOut, size_t(np) * size_t(2 * L - 1) * sizeof(double), &dc));
  PAL_TRY(e->check(hipMemcpyAsync(df, frames, fbytes, hipMemcpyHostToDevice, e->stream), "frames upload"));
  PAL_TRY(all_pairs_dev(e, static_cast<const double*>(df), B, M, L, prm, static_cast<pal_pair_record*>(dt),
                        static_cast<double*>(dc)));
  PAL_TRY(e->check(hipMemcpyAsync(table, dt, size_t(np) * sizeof(pal_pair_record), hipMemcpyDeviceToHost, e->stream), "table download"));
  if (corr) PAL_TRY(e->check(hipMemcpyAsync(corr, dc, size_t(np) * size_t(2 * L - 1) * sizeof(double), hipMemcpyDeviceToHost, e->stream), "corr download"));
  return pal_synchronize(h);
}

int pal_gcc_phat_pairs(pal_handle h, const double* rows, int R, int L, const int32_t* pairs, int64_t P,
                       const pal_phat_params* prm, pal_pair_record* table) {
  ENGINE(h);
  PAL_TRY(pairs_host(e, rows, R, L, pairs, P, prm, table));
  return pal_synchronize(h);
}

int pal_gcc_phat_pairs_dev(pal_handle h, const double* d_rows, int R, int L, const int32_t* d_pairs, int64_t P,
                           const pal_phat_params* prm, pal_pair_record* d_table) {
  ENGINE(h);
  PAL_TRY(validate(e, prm));
  if (!d_rows || !d_pairs || !d_table) return e->fail(PAL_ERR_INVALID, "NULL buffer");
  return e->pairs_dev(d_rows, R, L, d_pairs, P, *prm, d_table);
}

// ---- K candidate peaks per pair from the batched calls (K = prm->num_peaks in 1 .. PAL_MAX_CANDIDATES) ----
static int validate_peaks(Engine* e, const pal_phat_params* p) {
  PAL_TRY(validate(e, p));
  if (p->num_peaks > PAL_MAX_CANDIDATES) return e->fail(PAL_ERR_INVALID, "num_peaks %d outside 1..%d", p->num_peaks, PAL_MAX_CANDIDATES);
  return PAL_OK;
}

int pal_gcc_phat_all_pairs_peaks_dev(pal_handle h, const double* d_frames, int B, int M, int L, const pal_phat_params* prm,
                                     pal_pair_record* d_table, int32_t* d_cand_k, double* d_cand_h) {
  ENGINE(h);
  PAL_TRY(validate_peaks(e, prm));
  if (!d_frames || !d_table || !d_cand_k) return e->fail(PAL_ERR_INVALID, "NULL buffer");
  const CandOut cands{d_cand_k, d_cand_h};
  return all_pairs_dev(e, d_frames, B, M, L, prm, d_table, nullptr, &cands);
}

int pal_gcc_phat_all_pairs_peaks(pal_handle h, const double* frames, int B, int M, int L, const pal_phat_params* prm,
                                 pal_pair_record* table, int32_t* cand_k, double* cand_h) {
  ENGINE(h);
  PAL_TRY(validate_peaks(e, prm));
  if (!frames || !table || !cand_k) return e->fail(PAL_ERR_INVALID, "NULL buffer");
  if (B < 1 || M < 2 || L < 1) return e->fail(PAL_ERR_INVALID, "need B >= 1, M >= 2, L >= 1 (got %d, %d, %d)", B, M, L);
  const size_t fbytes = size_t(B) * M * L * sizeof(double);
  const size_t np = size_t(int64_t(B) * M * (M - 1) / 2), nc = np * size_t(prm->num_peaks);
  const size_t o_h = (nc * sizeof(int32_t) + 255) & ~size_t(255);
  void *df = nullptr, *dt = nullptr;
  char* dc = nullptr;
  PAL_TRY(e->scratch(kWsStageIn, fbytes, &df));
  PAL_TRY(e->scratch(kWsStageTable, np * sizeof(pal_pair_record), &dt));
  PAL_TRY(e->scratch(kWsStageOut, o_h + nc * sizeof(double), &dc));   // [cand_k | cand_h]
  PAL_TRY(e->check(hipMemcpyAsync(df, frames, fbytes, hipMemcpyHostToDevice, e->stream), "frames upload"));
  const CandOut cands{reinterpret_cast<int32_t*>(dc), cand_h ? reinterpret_cast<double*>(dc + o_h) : nullptr};
  PAL_TRY(all_pairs_dev(e, static_cast<const double*>(df), B, M, L, prm, static_cast<pal_pair_record*>(dt), nullptr, &cands));
  PAL_TRY(e->check(hipMemcpyAsync(table, dt, np * sizeof(pal_pair_record), hipMemcpyDeviceToHost, e->stream), "table download"));
  PAL_TRY(e->check(hipMemcpyAsync(cand_k, cands.k, nc * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream), "candidates download"));
  if (cand_h) PAL_TRY(e->check(hipMemcpyAsync(cand_h, cands.h, nc * sizeof(double), hipMemcpyDeviceToHost, e->stream), "heights download"));
  return pal_synchronize(h);
}

int pal_gcc_phat_pairs_peaks_dev(pal_handle h, const double* d_rows, int R, int L, const int32_t* d_pairs, int64_t P,
                                 const pal_phat_params* prm, pal_pair_record* d_table, int32_t* d_cand_k, double* d_cand_h) {
  ENGINE(h);
  PAL_TRY(validate_peaks(e, prm));
  if (!d_rows || !d_pairs || !d_table || !d_cand_k) return e->fail(PAL_ERR_INVALID, "NULL buffer");
  const CandOut cands{d_cand_k, d_cand_h};
  return e->pairs_dev(d_rows, R, L, d_pairs, P, *prm, d_table, &cands);
}

int pal_bootstrap_shuffle_dev(pal_handle h, const double* d_row, int L, int32_t i, int32_t j, int32_t mode, int32_t block_size,
                              uint64_t seed, int64_t s0, int32_t S, double* d_out) {
  ENGINE(h);
  if (!d_row || !d_out) return e->fail(PAL_ERR_INVALID, "NULL buffer");
  return e->bootstrap_shuffle_dev(d_row, L, i, j, mode, block_size, seed, s0, S, d_out);
}

int pal_bootstrap_peaks_dev(pal_handle h, const double* d_rows, int R, int L, const int32_t* d_pairs, int64_t P,
                            int32_t num_bootstrap, int32_t mode, int32_t block_size, uint64_t seed, double* d_peaks) {
  ENGINE(h);
  if (!d_rows || !d_pairs || !d_peaks) return e->fail(PAL_ERR_INVALID, "NULL buffer");
  return e->bootstrap_peaks_dev(d_rows, R, L, d_pairs, P, num_bootstrap, mode, block_size, seed, d_peaks);
}

int pal_bootstrap_peaks(pal_handle h, const double* rows, int R, int L, const int32_t* pairs, int64_t P, int32_t num_bootstrap,
                        int32_t mode, int32_t block_size, uint64_t seed, double* peaks) {
  ENGINE(h);
  if (!rows || !pairs || !peaks) return e->fail(PAL_ERR_INVALID, "NULL buffer");
  if (R < 1 || L < 1 || P < 1) return e->fail(PAL_ERR_INVALID, "need R >= 1, L >= 1, P >= 1");
  if (num_bootstrap < 1) return e->fail(PAL_ERR_INVALID, "num_bootstrap must be at least 1");
  if (P > (int64_t(1) << 40) / num_bootstrap) return e->fail(PAL_ERR_UNSUPPORTED, "too many pairs x shuffles");
  for (int64_t k = 0; k < 2 * P; ++k)
    if (pairs[k] < 0 || pairs[k] >= R) return e->fail(PAL_ERR_INVALID, "pair %lld references row outside 0..%d", (long long)(k / 2), R - 1);
  const size_t pbytes = size_t(P) * size_t(num_bootstrap) * sizeof(double);
  void *df = nullptr, *dp = nullptr, *dk = nullptr;
  PAL_TRY(e->scratch(kWsStageIn, size_t(R) * L * sizeof(double), &df));
  PAL_TRY(e->scratch(kWsStagePairs, size_t(2 * P) * sizeof(int32_t), &dp));
  PAL_TRY(e->scratch(kWsBootPeaks, pbytes, &dk));
  PAL_TRY(e->check(hipMemcpyAsync(df, rows, size_t(R) * L * sizeof(double), hipMemcpyHostToDevice, e->stream), "rows upload"));
  PAL_TRY(e->check(hipMemcpyAsync(dp, pairs, size_t(2 * P) * sizeof(int32_t), hipMemcpyHostToDevice, e->stream), "pairs upload"));
  PAL_TRY(e->bootstrap_peaks_dev(static_cast<const double*>(df), R, L, static_cast<const int32_t*>(dp), P, num_bootstrap, mode, block_size,
                                 seed, static_cast<double*>(dk)));
  PAL_TRY(e->check(hipMemcpyAsync(peaks, dk, pbytes, hipMemcpyDeviceToHost, e->stream), "peaks download"));
  return pal_synchronize(h);
}

int pal_solve_positions_dev(pal_handle h, const pal_pair_record* d_tables, int B, int M, const int32_t* lengths, const double* mics,
                            const double* calib, const double* weights, const double* extra_starts, const pal_solve_params* prm,
                            pal_position_record* out) {
  ENGINE(h);
  return e->solve_positions_dev(d_tables, B, M, lengths, mics, calib, weights, extra_starts, prm, out);
}

int pal_solve_positions(pal_handle h, const pal_pair_record* tables, int B, int M, const int32_t* lengths, const double* mics,
                        const double* calib, const double* weights, const double* extra_starts, const pal_solve_params* prm,
                        pal_position_record* out) {
  ENGINE(h);
  if (!tables) return e->fail(PAL_ERR_INVALID, "NULL buffer");
  if (B < 1) return e->fail(PAL_ERR_INVALID, "need B >= 1");
  if (M < 2) return e->fail(PAL_ERR_INVALID, "need at least 2 microphones (got %d)", M);
  const size_t bytes = size_t(B) * size_t(M) * size_t(M - 1) / 2 * sizeof(pal_pair_record);
  void* dt = nullptr;
  PAL_TRY(e->scratch(kWsStageTable, bytes, &dt));
  PAL_TRY(e->check(hipMemcpyAsync(dt, tables, bytes, hipMemcpyHostToDevice, e->stream), "tables upload"));
  return e->solve_positions_dev(static_cast<const pal_pair_record*>(dt), B, M, lengths, mics, calib, weights, extra_starts, prm, out);
}

int pal_solve_positions_loss_dev(pal_handle h, const pal_pair_record* d_tables, int B, int M, const int32_t* lengths, const double* mics,
                                 const double* calib, const double* weights, const double* extra_starts, const pal_solve_params* prm,
                                 pal_position_record* out, int32_t loss, double f_scale, double* pair_weights) {
  ENGINE(h);
  return e->solve_positions_loss_dev(d_tables, B, M, lengths, mics, calib, weights, extra_starts, prm, out, loss, f_scale, pair_weights);
}

int pal_solve_positions_loss(pal_handle h, const pal_pair_record* tables, int B, int M, const int32_t* lengths, const double* mics,
                             const double* calib, const double* weights, const double* extra_starts, const pal_solve_params* prm,
                             pal_position_record* out, int32_t loss, double f_scale, double* pair_weights) {
  ENGINE(h);
  if (!tables) return e->fail(PAL_ERR_INVALID, "NULL buffer");
  if (B < 1) return e->fail(PAL_ERR_INVALID, "need B >= 1");
  if (M < 2) return e->fail(PAL_ERR_INVALID, "need at least 2 microphones (got %d)", M);
  if (loss < PAL_SOLVE_LOSS_LINEAR || loss > PAL_SOLVE_LOSS_CAUCHY) return e->fail(PAL_ERR_INVALID, "unknown loss %d", loss);
  if (!(std::isfinite(f_scale) && f_scale > 0)) return e->fail(PAL_ERR_INVALID, "f_scale must be finite and positive");
  if (loss == PAL_SOLVE_LOSS_LINEAR) {
    const int rc = pal_solve_positions(h, tables, B, M, lengths, mics, calib, weights, extra_starts, prm, out);
    if (rc == PAL_OK && pair_weights) std::fill(pair_weights, pair_weights + size_t(B) * (size_t(M) * size_t(M - 1) / 2), 1.0);
    return rc;
  }
  const size_t bytes = size_t(B) * size_t(M) * size_t(M - 1) / 2 * sizeof(pal_pair_record);
  void* dt = nullptr;
  PAL_TRY(e->scratch(kWsStageTable, bytes, &dt));
  PAL_TRY(e->check(hipMemcpyAsync(dt, tables, bytes, hipMemcpyHostToDevice, e->stream), "tables upload"));
  return e->solve_positions_loss_dev(static_cast<const pal_pair_record*>(dt), B, M, lengths, mics, calib, weights, extra_starts, prm, out, loss,
                                     f_scale, pair_weights);
}

int pal_tdoa_closure_dev(pal_handle h, const pal_pair_record* d_tables, int B, int M, const int32_t* lengths, int32_t tol, int32_t min_votes,
                         int32_t weight_mode, int32_t* d_votes, int32_t* d_mic_closed, double* d_weights, pal_closure_frame* d_summary) {
  ENGINE(h);
  return e->tdoa_closure_dev(d_tables, B, M, lengths, tol, min_votes, weight_mode, d_votes, d_mic_closed, d_weights, d_summary);
}

int pal_tdoa_closure(pal_handle h, const pal_pair_record* tables, int B, int M, const int32_t* lengths, int32_t tol, int32_t min_votes,
                     int32_t weight_mode, int32_t* votes, int32_t* mic_closed, double* weights, pal_closure_frame* summary) {
  ENGINE(h);
  PAL_TRY(e->closure_check(B, M, lengths, tol, min_votes, weight_mode));
  if (!tables) return e->fail(PAL_ERR_INVALID, "NULL buffer");
  if (!votes && !mic_closed && !weights && !summary) return e->fail(PAL_ERR_INVALID, "no output requested");
  const size_t P = size_t(M) * size_t(M - 1) / 2, np = size_t(B) * P;
  for (size_t r = 0; r < np; ++r) {
    const int64_t k = tables[r].k_sel, len = lengths[r / P];
    if (k < 0 || k > 2 * len - 2)
      return e->fail(PAL_ERR_INVALID, "frame %d, pair %d: k_sel %d outside 0..%d", int(r / P), int(r % P), int(k), int(2 * len - 2));
  }
  // staged outputs in one block: [votes | mic_closed | weights | summary]
  Carve c;
  const size_t o_votes = c.take(votes ? np * sizeof(int32_t) : 0), o_mic = c.take(mic_closed ? size_t(B) * M * sizeof(int32_t) : 0);
  const size_t o_wt = c.take(weights ? np * sizeof(double) : 0), o_sum = c.take(summary ? size_t(B) * sizeof(pal_closure_frame) : 0);
  void* dt = nullptr;
  char* out = nullptr;
  PAL_TRY(e->scratch(kWsStageTable, np * sizeof(pal_pair_record), &dt));
  PAL_TRY(e->scratch(kWsStageOut, c.off, &out));
  PAL_TRY(e->check(hipMemcpyAsync(dt, tables, np * sizeof(pal_pair_record), hipMemcpyHostToDevice, e->stream), "tables upload"));
  int32_t* dv = votes ? reinterpret_cast<int32_t*>(out + o_votes) : nullptr;
  int32_t* dm = mic_closed ? reinterpret_cast<int32_t*>(out + o_mic) : nullptr;
  double* dw = weights ? reinterpret_cast<double*>(out + o_wt) : nullptr;
  pal_closure_frame* ds = summary ? reinterpret_cast<pal_closure_frame*>(out + o_sum) : nullptr;
  PAL_TRY(e->tdoa_closure_dev(static_cast<const pal_pair_record*>(dt), B, M, lengths, tol, min_votes, weight_mode, dv, dm, dw, ds));
  if (votes) PAL_TRY(e->check(hipMemcpyAsync(votes, dv, np * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream), "votes download"));
  if (mic_closed) PAL_TRY(e->check(hipMemcpyAsync(mic_closed, dm, size_t(B) * M * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream), "mic_closed download"));
  if (weights) PAL_TRY(e->check(hipMemcpyAsync(weights, dw, np * sizeof(double), hipMemcpyDeviceToHost, e->stream), "weights download"));
  if (summary) PAL_TRY(e->check(hipMemcpyAsync(summary, ds, size_t(B) * sizeof(pal_closure_frame), hipMemcpyDeviceToHost, e->stream), "summary download"));
  return pal_synchronize(h);
}

int pal_tdoa_consensus_dev(pal_handle h, const pal_pair_record* d_tables, const int32_t* d_cand_k, const double* d_cand_h, int B, int M,
                           int K, const int32_t* lengths, int32_t tol, int32_t rounds, int32_t* d_sel, pal_pair_record* d_table_out,
                           pal_consensus_frame* d_summary) {
  ENGINE(h);
  return e->tdoa_consensus_dev(d_tables, d_cand_k, d_cand_h, B, M, K, lengths, tol, rounds, d_sel, d_table_out, d_summary);
}

int pal_tdoa_consensus(pal_handle h, const pal_pair_record* tables, const int32_t* cand_k, const double* cand_h, int B, int M, int K,
                       const int32_t* lengths, int32_t tol, int32_t rounds, int32_t* sel, pal_pair_record* table_out,
                       pal_consensus_frame* summary) {
  ENGINE(h);
  PAL_TRY(e->consensus_check(B, M, K, lengths, tol, rounds));
  if (!cand_k) return e->fail(PAL_ERR_INVALID, "NULL buffer");
  if (!sel && !table_out && !summary) return e->fail(PAL_ERR_INVALID, "no output requested");
  if (table_out && !tables) return e->fail(PAL_ERR_INVALID, "table_out needs the input tables");
  const size_t P = size_t(M) * size_t(M - 1) / 2, np = size_t(B) * P;
  for (size_t r = 0; r < np; ++r) {
    const int64_t len = lengths[r / P];
    bool ended = false;
    for (int c = 0; c < K; ++c) {
      const int64_t k = cand_k[r * K + c];
      if (k == -1) {
        if (c == 0) return e->fail(PAL_ERR_INVALID, "frame %d, pair %d: candidate 0 is absent", int(r / P), int(r % P));
        ended = true;
      } else if (ended) {
        return e->fail(PAL_ERR_INVALID, "frame %d, pair %d: candidate %d follows an absent one", int(r / P), int(r % P), c);
      } else if (k < 0 || k > 2 * len - 2) {
        return e->fail(PAL_ERR_INVALID, "frame %d, pair %d: candidate %d is %d, outside 0..%d", int(r / P), int(r % P), c, int(k), int(2 * len - 2));
      }
    }
  }
  // staged inputs [cand_k | cand_h] and outputs [sel | table_out | summary], one block each
  const size_t nc = np * size_t(K);
  Carve ci, co;
  const size_t o_k = ci.take(nc * sizeof(int32_t)), o_h = ci.take(cand_h ? nc * sizeof(double) : 0);
  const size_t o_sel = co.take(sel ? np * sizeof(int32_t) : 0), o_tab = co.take(table_out ? np * sizeof(pal_pair_record) : 0);
  const size_t o_sum = co.take(summary ? size_t(B) * sizeof(pal_consensus_frame) : 0);
  void* dt = nullptr;
  char *in = nullptr, *out = nullptr;
  if (tables) {
    PAL_TRY(e->scratch(kWsStageTable, np * sizeof(pal_pair_record), &dt));
    PAL_TRY(e->check(hipMemcpyAsync(dt, tables, np * sizeof(pal_pair_record), hipMemcpyHostToDevice, e->stream), "tables upload"));
  }
  PAL_TRY(e->scratch(kWsStageIn, ci.off, &in));
  PAL_TRY(e->scratch(kWsStageOut, co.off, &out));
  PAL_TRY(e->check(hipMemcpyAsync(in + o_k, cand_k, nc * sizeof(int32_t), hipMemcpyHostToDevice, e->stream), "candidates upload"));
  if (cand_h) PAL_TRY(e->check(hipMemcpyAsync(in + o_h, cand_h, nc * sizeof(double), hipMemcpyHostToDevice, e->stream), "heights upload"));
  int32_t* ds = sel ? reinterpret_cast<int32_t*>(out + o_sel) : nullptr;
  pal_pair_record* dto = table_out ? reinterpret_cast<pal_pair_record*>(out + o_tab) : nullptr;
  pal_consensus_frame* dsum = summary ? reinterpret_cast<pal_consensus_frame*>(out + o_sum) : nullptr;
  PAL_TRY(e->tdoa_consensus_dev(static_cast<const pal_pair_record*>(dt), reinterpret_cast<const int32_t*>(in + o_k),
                                cand_h ? reinterpret_cast<const double*>(in + o_h) : nullptr, B, M, K, lengths, tol, rounds, ds, dto, dsum));
  if (sel) PAL_TRY(e->check(hipMemcpyAsync(sel, ds, np * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream), "sel download"));
  if (table_out) PAL_TRY(e->check(hipMemcpyAsync(table_out, dto, np * sizeof(pal_pair_record), hipMemcpyDeviceToHost, e->stream), "table download"));
  if (summary) PAL_TRY(e->check(hipMemcpyAsync(summary, dsum, size_t(B) * sizeof(pal_consensus_frame), hipMemcpyDeviceToHost, e->stream), "summary download"));
  return pal_synchronize(h);
}

// ---- steered-response power (srp.hip): lag strips of all pairs; the map over a box, its peaks and its zoom; the direction map ----
int pal_gcc_phat_all_pairs_strips_dev(pal_handle h, const double* d_frames, int B, int M, int L, const pal_phat_params* prm, int T, int W,
                                      pal_pair_record* d_table, double* d_strips) {
  ENGINE(h);
  if (!d_frames || !d_strips) return e->fail(PAL_ERR_INVALID, "NULL buffer");
  return strips_dev(e, d_frames, B, M, L, prm, T, W, d_table, d_strips);
}

int pal_gcc_phat_all_pairs_strips(pal_handle h, const double* frames, int B, int M, int L, const pal_phat_params* prm, int T, int W,
                                  pal_pair_record* table, double* strips) {
  ENGINE(h);
  if (!frames || !strips) return e->fail(PAL_ERR_INVALID, "NULL buffer");
  PAL_TRY(validate(e, prm));
  PAL_TRY(e->srp_strips_check(B, M, L, T, W));
  if (prm->num_peaks != 1) return e->fail(PAL_ERR_INVALID, "the strips call carries the one-peak table: num_peaks must be 1");
  const size_t fbytes = size_t(B) * M * L * sizeof(double);
  const size_t np = size_t(B) * (size_t(M) * size_t(M - 1) / 2), sbytes = np * size_t(2 * T + 1) * sizeof(double);
  void *df = nullptr, *dt = nullptr, *ds = nullptr;
  PAL_TRY(e->scratch(kWsStageIn, fbytes, &df));
  if (table) PAL_TRY(e->scratch(kWsStageTable, np * sizeof(pal_pair_record), &dt));
  PAL_TRY(e->scratch(kWsStageOut, sbytes, &ds));
  PAL_TRY(e->check(hipMemcpyAsync(df, frames, fbytes, hipMemcpyHostToDevice, e->stream), "frames upload"));
  PAL_TRY(strips_dev(e, static_cast<const double*>(df), B, M, L, prm, T, W, static_cast<pal_pair_record*>(dt), static_cast<double*>(ds)));
  if (table) PAL_TRY(e->check(hipMemcpyAsync(table, dt, np * sizeof(pal_pair_record), hipMemcpyDeviceToHost, e->stream), "table download"));
  PAL_TRY(e->check(hipMemcpyAsync(strips, ds, sbytes, hipMemcpyDeviceToHost, e->stream), "strips download"));
  return pal_synchronize(h);
}

// The staged host forms of the map, the peaks and the zoom, each written once for the box and the direction grid: behind the caller's
// check they take the grid's cell count G and `dev`, the engine's device call on the staged buffers.
extern "C++" {

// inputs [strips | pair_weights] and outputs [power | peaks | summary], one block each; dev(d_strips, d_weights, d_power, d_peaks, d_summary)
template <class DEV>
static int srp_map_staged(pal_handle h, Engine* e, const double* strips, int B, int M, int T, const double* pair_weights, int K, size_t G,
                          double* power, pal_srp_peak* peaks, pal_srp_frame* summary, DEV dev) {
  if (!strips) return e->fail(PAL_ERR_INVALID, "NULL buffer");
  const size_t np = size_t(B) * (size_t(M) * size_t(M - 1) / 2);
  Carve ci, co;
  const size_t sbytes = np * size_t(2 * T + 1) * sizeof(double);
  const size_t o_st = ci.take(sbytes), o_w = ci.take(pair_weights ? np * sizeof(double) : 0);
  const size_t o_pw = co.take(power ? size_t(B) * G * sizeof(double) : 0), o_pk = co.take(peaks ? size_t(B) * size_t(K) * sizeof(pal_srp_peak) : 0);
  const size_t o_sum = co.take(summary ? size_t(B) * sizeof(pal_srp_frame) : 0);
  char *in = nullptr, *out = nullptr;
  PAL_TRY(e->scratch(kWsStageIn, ci.off, &in));
  PAL_TRY(e->scratch(kWsStageOut, co.off, &out));
  PAL_TRY(e->check(hipMemcpyAsync(in + o_st, strips, sbytes, hipMemcpyHostToDevice, e->stream), "strips upload"));
  if (pair_weights) PAL_TRY(e->check(hipMemcpyAsync(in + o_w, pair_weights, np * sizeof(double), hipMemcpyHostToDevice, e->stream), "weights upload"));
  double* dpw = power ? reinterpret_cast<double*>(out + o_pw) : nullptr;
  pal_srp_peak* dpk = peaks ? reinterpret_cast<pal_srp_peak*>(out + o_pk) : nullptr;
  pal_srp_frame* dsum = summary ? reinterpret_cast<pal_srp_frame*>(out + o_sum) : nullptr;
  PAL_TRY(dev(reinterpret_cast<const double*>(in + o_st), pair_weights ? reinterpret_cast<const double*>(in + o_w) : nullptr, dpw, dpk, dsum));
  if (power) PAL_TRY(e->check(hipMemcpyAsync(power, dpw, size_t(B) * G * sizeof(double), hipMemcpyDeviceToHost, e->stream), "map download"));
  if (peaks) PAL_TRY(e->check(hipMemcpyAsync(peaks, dpk, size_t(B) * size_t(K) * sizeof(pal_srp_peak), hipMemcpyDeviceToHost, e->stream), "peaks download"));
  if (summary) PAL_TRY(e->check(hipMemcpyAsync(summary, dsum, size_t(B) * sizeof(pal_srp_frame), hipMemcpyDeviceToHost, e->stream), "summary download"));
  return pal_synchronize(h);
}

// the map in, [peaks | summary] out; dev(d_power, d_peaks, d_summary)
template <class DEV>
static int srp_peaks_staged(pal_handle h, Engine* e, const double* power, int B, int K, size_t G, pal_srp_peak* peaks, pal_srp_frame* summary,
                            DEV dev) {
  if (!power || !peaks) return e->fail(PAL_ERR_INVALID, "NULL buffer");
  Carve co;
  const size_t o_pk = co.take(size_t(B) * size_t(K) * sizeof(pal_srp_peak)), o_sum = co.take(summary ? size_t(B) * sizeof(pal_srp_frame) : 0);
  void* in = nullptr;
  char* out = nullptr;
  PAL_TRY(e->scratch(kWsStageIn, size_t(B) * G * sizeof(double), &in));
  PAL_TRY(e->scratch(kWsStageOut, co.off, &out));
  PAL_TRY(e->check(hipMemcpyAsync(in, power, size_t(B) * G * sizeof(double), hipMemcpyHostToDevice, e->stream), "map upload"));
  pal_srp_peak* dpk = reinterpret_cast<pal_srp_peak*>(out + o_pk);
  pal_srp_frame* dsum = summary ? reinterpret_cast<pal_srp_frame*>(out + o_sum) : nullptr;
  PAL_TRY(dev(static_cast<const double*>(in), dpk, dsum));
  PAL_TRY(e->check(hipMemcpyAsync(peaks, dpk, size_t(B) * size_t(K) * sizeof(pal_srp_peak), hipMemcpyDeviceToHost, e->stream), "peaks download"));
  if (summary) PAL_TRY(e->check(hipMemcpyAsync(summary, dsum, size_t(B) * sizeof(pal_srp_frame), hipMemcpyDeviceToHost, e->stream), "summary download"));
  return pal_synchronize(h);
}

// inputs [strips | pair_weights | seeds] and the output records, one block each; dev(d_strips, d_weights, d_seeds, d_out)
template <class DEV>
static int srp_zoom_staged(pal_handle h, Engine* e, const double* strips, int B, int M, int T, const double* pair_weights,
                           const pal_srp_peak* seeds, int K, pal_srp_zoom_record* out, DEV dev) {
  if (!strips || !seeds || !out) return e->fail(PAL_ERR_INVALID, "NULL buffer");
  const size_t np = size_t(B) * (size_t(M) * size_t(M - 1) / 2), nk = size_t(B) * size_t(K);
  Carve ci;
  const size_t sbytes = np * size_t(2 * T + 1) * sizeof(double);
  const size_t o_st = ci.take(sbytes), o_w = ci.take(pair_weights ? np * sizeof(double) : 0), o_sd = ci.take(nk * sizeof(pal_srp_peak));
  char *in = nullptr, *dout = nullptr;
  PAL_TRY(e->scratch(kWsStageIn, ci.off, &in));
  PAL_TRY(e->scratch(kWsStageOut, nk * sizeof(pal_srp_zoom_record), &dout));
  PAL_TRY(e->check(hipMemcpyAsync(in + o_st, strips, sbytes, hipMemcpyHostToDevice, e->stream), "strips upload"));
  if (pair_weights) PAL_TRY(e->check(hipMemcpyAsync(in + o_w, pair_weights, np * sizeof(double), hipMemcpyHostToDevice, e->stream), "weights upload"));
  PAL_TRY(e->check(hipMemcpyAsync(in + o_sd, seeds, nk * sizeof(pal_srp_peak), hipMemcpyHostToDevice, e->stream), "seeds upload"));
  PAL_TRY(dev(reinterpret_cast<const double*>(in + o_st), pair_weights ? reinterpret_cast<const double*>(in + o_w) : nullptr,
              reinterpret_cast<const pal_srp_peak*>(in + o_sd), reinterpret_cast<pal_srp_zoom_record*>(dout)));
  PAL_TRY(e->check(hipMemcpyAsync(out, dout, nk * sizeof(pal_srp_zoom_record), hipMemcpyDeviceToHost, e->stream), "zoom download"));
  return pal_synchronize(h);
}

}  // extern "C++"

int pal_srp_map_dev(pal_handle h, const double* d_strips, int B, int M, int T, const double* mics, double fs, double c,
                    const pal_srp_grid* grid, const double* d_pair_weights, int K, int R, double* d_power, pal_srp_peak* d_peaks,
                    pal_srp_frame* d_summary) {
  ENGINE(h);
  return e->srp_map_dev(d_strips, B, M, T, mics, fs, c, grid, d_pair_weights, K, R, d_power, d_peaks, d_summary);
}

int pal_srp_map(pal_handle h, const double* strips, int B, int M, int T, const double* mics, double fs, double c, const pal_srp_grid* grid,
                const double* pair_weights, int K, int R, double* power, pal_srp_peak* peaks, pal_srp_frame* summary) {
  ENGINE(h);
  PAL_TRY(e->srp_map_check(B, M, T, mics, fs, c, grid, K, R, power || peaks || summary, peaks != nullptr));
  const size_t G = size_t(grid->count[0]) * size_t(grid->count[1]) * size_t(grid->count[2]);
  return srp_map_staged(h, e, strips, B, M, T, pair_weights, K, G, power, peaks, summary,
                        [&](const double* ds, const double* dw, double* dpw, pal_srp_peak* dpk, pal_srp_frame* dsum) {
                          return e->srp_map_dev(ds, B, M, T, mics, fs, c, grid, dw, K, R, dpw, dpk, dsum);
                        });
}

int pal_srp_peaks_dev(pal_handle h, const double* d_power, int B, const pal_srp_grid* grid, int K, int R, pal_srp_peak* d_peaks,
                      pal_srp_frame* d_summary) {
  ENGINE(h);
  return e->srp_peaks_dev(d_power, B, grid, K, R, d_peaks, d_summary);
}

int pal_srp_peaks(pal_handle h, const double* power, int B, const pal_srp_grid* grid, int K, int R, pal_srp_peak* peaks,
                  pal_srp_frame* summary) {
  ENGINE(h);
  PAL_TRY(e->srp_peaks_check(B, grid, K, R));
  const size_t G = size_t(grid->count[0]) * size_t(grid->count[1]) * size_t(grid->count[2]);
  return srp_peaks_staged(h, e, power, B, K, G, peaks, summary, [&](const double* dp, pal_srp_peak* dpk, pal_srp_frame* dsum) {
    return e->srp_peaks_dev(dp, B, grid, K, R, dpk, dsum);
  });
}

int pal_srp_zoom_dev(pal_handle h, const double* d_strips, int B, int M, int T, const double* mics, double fs, double c,
                     const double* d_pair_weights, const pal_srp_peak* d_seeds, int K, const double* half0, int Z, int levels,
                     pal_srp_zoom_record* d_out) {
  ENGINE(h);
  return e->srp_zoom_dev(d_strips, B, M, T, mics, fs, c, d_pair_weights, d_seeds, K, half0, Z, levels, d_out);
}

int pal_srp_zoom(pal_handle h, const double* strips, int B, int M, int T, const double* mics, double fs, double c,
                 const double* pair_weights, const pal_srp_peak* seeds, int K, const double* half0, int Z, int levels,
                 pal_srp_zoom_record* out) {
  ENGINE(h);
  PAL_TRY(e->srp_zoom_check(B, M, T, mics, fs, c, K, half0, Z, levels));
  return srp_zoom_staged(h, e, strips, B, M, T, pair_weights, seeds, K, out,
                         [&](const double* ds, const double* dw, const pal_srp_peak* dsd, pal_srp_zoom_record* dout) {
                           return e->srp_zoom_dev(ds, B, M, T, mics, fs, c, dw, dsd, K, half0, Z, levels, dout);
                         });
}

// ---- the direction map (srp.hip): the same staged forms with G = n_az * n_el ----
int pal_srp_doa_dev(pal_handle h, const double* d_strips, int B, int M, int T, const double* mics, double fs, double c,
                    const pal_srp_doa_grid* grid, const double* az, const double* el, const double* d_pair_weights, int K, int R,
                    double* d_power, pal_srp_peak* d_peaks, pal_srp_frame* d_summary) {
  ENGINE(h);
  return e->srp_doa_dev(d_strips, B, M, T, mics, fs, c, grid, az, el, d_pair_weights, K, R, d_power, d_peaks, d_summary);
}

int pal_srp_doa(pal_handle h, const double* strips, int B, int M, int T, const double* mics, double fs, double c,
                const pal_srp_doa_grid* grid, const double* az, const double* el, const double* pair_weights, int K, int R, double* power,
                pal_srp_peak* peaks, pal_srp_frame* summary) {
  ENGINE(h);
  PAL_TRY(e->srp_doa_check(B, M, T, mics, fs, c, grid, az, el, K, R, power || peaks || summary, peaks != nullptr));
  return srp_map_staged(h, e, strips, B, M, T, pair_weights, K, size_t(grid->n_az) * size_t(grid->n_el), power, peaks, summary,
                        [&](const double* ds, const double* dw, double* dpw, pal_srp_peak* dpk, pal_srp_frame* dsum) {
                          return e->srp_doa_dev(ds, B, M, T, mics, fs, c, grid, az, el, dw, K, R, dpw, dpk, dsum);
                        });
}

int pal_srp_doa_peaks_dev(pal_handle h, const double* d_power, int B, const pal_srp_doa_grid* grid, const double* az, const double* el,
                          int K, int R, pal_srp_peak* d_peaks, pal_srp_frame* d_summary) {
  ENGINE(h);
  return e->srp_doa_peaks_dev(d_power, B, grid, az, el, K, R, d_peaks, d_summary);
}

int pal_srp_doa_peaks(pal_handle h, const double* power, int B, const pal_srp_doa_grid* grid, const double* az, const double* el, int K,
                      int R, pal_srp_peak* peaks, pal_srp_frame* summary) {
  ENGINE(h);
  PAL_TRY(e->srp_doa_peaks_check(B, grid, az, el, K, R));
  return srp_peaks_staged(h, e, power, B, K, size_t(grid->n_az) * size_t(grid->n_el), peaks, summary,
                          [&](const double* dp, pal_srp_peak* dpk, pal_srp_frame* dsum) {
                            return e->srp_doa_peaks_dev(dp, B, grid, az, el, K, R, dpk, dsum);
                          });
}

int pal_srp_doa_zoom_dev(pal_handle h, const double* d_strips, int B, int M, int T, const double* mics, double fs, double c,
                         const double* d_pair_weights, const pal_srp_peak* d_seeds, int K, double half0, int Z, int levels,
                         pal_srp_zoom_record* d_out) {
  ENGINE(h);
  return e->srp_doa_zoom_dev(d_strips, B, M, T, mics, fs, c, d_pair_weights, d_seeds, K, half0, Z, levels, d_out);
}

int pal_srp_doa_zoom(pal_handle h, const double* strips, int B, int M, int T, const double* mics, double fs, double c,
                     const double* pair_weights, const pal_srp_peak* seeds, int K, double half0, int Z, int levels,
                     pal_srp_zoom_record* out) {
  ENGINE(h);
  PAL_TRY(e->srp_doa_zoom_check(B, M, T, mics, fs, c, K, half0, Z, levels));
  return srp_zoom_staged(h, e, strips, B, M, T, pair_weights, seeds, K, out,
                         [&](const double* ds, const double* dw, const pal_srp_peak* dsd, pal_srp_zoom_record* dout) {
                           return e->srp_doa_zoom_dev(ds, B, M, T, mics, fs, c, dw, dsd, K, half0, Z, levels, dout);
                         });
}

static int single_pair(Engine* e, const double* sig1, int n1, const double* sig2, int n2, const pal_phat_params* prm,
                       int32_t* k_out, pal_pair_record* rec, double* corr) {
  if (!sig1 || !sig2) return e->fail(PAL_ERR_INVALID, "NULL signal");
  if (n1 < 1 || n2 < 1) return e->fail(PAL_ERR_INVALID, "empty signal");
  if (n1 > (1 << 20) || n2 > (1 << 20)) return e->fail(PAL_ERR_UNSUPPORTED, "signal longer than 2^20 samples");
  const int n = n1 + n2 - 1, lin = n1 > n2 ? n1 : n2;
  Plan* pl = nullptr;
  PAL_TRY(e->get_plan(n, lin, n, &pl));
  void *df = nullptr, *sp = nullptr, *dc = nullptr, *dt = nullptr, *qp = nullptr, *dk = nullptr;
  PAL_TRY(e->scratch(kWsStageIn, size_t(2) * lin * sizeof(double), &df));
  PAL_TRY(e->scratch(kWsSpectra, size_t(2) * pl->spec_stride() * sizeof(cd), &sp));
  PAL_TRY(e->scratch(kWsStageOut, size_t(n) * sizeof(double), &dc));
  PAL_TRY(e->scratch(kWsStageTable, sizeof(pal_pair_record) + PAL_MAX_PEAKS * sizeof(int32_t), &dt));
  PAL_TRY(e->scratch(kWsQuads, sizeof(int4), &qp));
  dk = static_cast<char*>(dt) + sizeof(pal_pair_record);
  double* d = static_cast<double*>(df);
  PAL_TRY(e->check(hipMemcpyAsync(d, sig1, size_t(n1) * sizeof(double), hipMemcpyHostToDevice, e->stream), "sig1 upload"));
  PAL_TRY(e->check(hipMemcpyAsync(d + lin, sig2, size_t(n2) * sizeof(double), hipMemcpyHostToDevice, e->stream), "sig2 upload"));
  const int4 quad = make_int4(0, 1, -1, -1);
  PAL_TRY(e->check(hipMemcpyAsync(qp, &quad, sizeof quad, hipMemcpyHostToDevice, e->stream), "quad upload"));
  PAL_TRY(e->check(hipStreamSynchronize(e->stream), "upload sync"));
  cd* S = static_cast<cd*>(sp);
  PAL_TRY(e->forward_spectra(*pl, d, size_t(lin), 1, n1, S));
  PAL_TRY(e->forward_spectra(*pl, d + lin, size_t(lin), 1, n2, S + pl->spec_stride()));
  pal_phat_params dummy{};
  PAL_TRY(e->pair_correlations(*pl, S, 2, static_cast<const int4*>(qp), 1, n2, prm ? *prm : dummy,
                               prm ? static_cast<pal_pair_record*>(dt) : nullptr,
                               prm ? static_cast<int32_t*>(dk) : nullptr, static_cast<double*>(dc)));
  if (corr) PAL_TRY(e->check(hipMemcpyAsync(corr, dc, size_t(n) * sizeof(double), hipMemcpyDeviceToHost, e->stream), "corr download"));
  if (prm && rec) PAL_TRY(e->check(hipMemcpyAsync(rec, dt, sizeof(pal_pair_record), hipMemcpyDeviceToHost, e->stream), "record download"));
  if (prm && k_out) PAL_TRY(e->check(hipMemcpyAsync(k_out, dk, size_t(prm->num_peaks) * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream), "k download"));
  return PAL_OK;
}

int pal_phat_correlation(pal_handle h, const double* sig1, int n1, const double* sig2, int n2, double* corr) {
  ENGINE(h);
  if (!corr) return e->fail(PAL_ERR_INVALID, "corr is NULL");
  PAL_TRY(single_pair(e, sig1, n1, sig2, n2, nullptr, nullptr, nullptr, corr));
  return pal_synchronize(h);
}

int pal_get_time_delays_phat(pal_handle h, const double* sig1, int n1, const double* sig2, int n2,
                             const pal_phat_params* prm, int32_t* k_out, pal_pair_record* rec, double* corr) {
  ENGINE(h);
  PAL_TRY(validate(e, prm));
  PAL_TRY(single_pair(e, sig1, n1, sig2, n2, prm, k_out, rec, corr));
  return pal_synchronize(h);
}

int pal_corr_metrics(pal_handle h, const double* corr, int n, pal_pair_record* rec) {
  ENGINE(h);
  if (!corr || !rec || n < 1) return e->fail(PAL_ERR_INVALID, "bad correlation row");
  void *dc = nullptr, *dt = nullptr;
  PAL_TRY(e->scratch(kWsStageOut, size_t(n) * sizeof(double), &dc));
  PAL_TRY(e->scratch(kWsStageTable, sizeof(pal_pair_record), &dt));
  PAL_TRY(e->check(hipMemcpyAsync(dc, corr, size_t(n) * sizeof(double), hipMemcpyHostToDevice, e->stream), "corr upload"));
  pal_phat_params p{};
  p.fs = 1; p.threshold_method = -1; p.peak_distance = 1; p.num_peaks = 1; p.max_expected_delay = NAN;
  PAL_TRY(e->peaks(static_cast<const double*>(dc), size_t(n), 1, n, 1, p, static_cast<pal_pair_record*>(dt), nullptr, 0));   // slot 0: on `stream`
  PAL_TRY(e->check(hipMemcpyAsync(rec, dt, sizeof(pal_pair_record), hipMemcpyDeviceToHost, e->stream), "record download"));
  return pal_synchronize(h);
}

int pal_select_peaks(pal_handle h, const double* corr, int R, int n, int n2, const pal_phat_params* prm,
                     pal_pair_record* table, int32_t* k_out) {
  ENGINE(h);
  PAL_TRY(validate(e, prm));
  if (!corr || !table) return e->fail(PAL_ERR_INVALID, "NULL buffer");
  if (R < 1 || n < 1 || n2 < 1 || n2 > n) return e->fail(PAL_ERR_INVALID, "need R >= 1, n >= 1, 1 <= n2 <= n (got %d, %d, %d)", R, n, n2);
  if (int64_t(R) * ((n + 2047) / 2048) > INT32_MAX) return e->fail(PAL_ERR_UNSUPPORTED, "too many rows");   // (one workgroup per tile at most)
  const size_t count = size_t(R) * size_t(n);
  for (size_t i = 0; i < count; ++i)                           // on the host, before any upload or launch
    if (!std::isfinite(corr[i]))
      return e->fail(PAL_ERR_INVALID, "non-finite sample (NaN or infinity) in correlation row %lld", (long long)(i / size_t(n)));
  const size_t tbytes = size_t(R) * sizeof(pal_pair_record);
  void *dc = nullptr, *dt = nullptr;
  PAL_TRY(e->scratch(kWsStageOut, count * sizeof(double), &dc));
  PAL_TRY(e->scratch(kWsStageTable, tbytes + size_t(R) * PAL_MAX_PEAKS * sizeof(int32_t), &dt));
  int32_t* dk = reinterpret_cast<int32_t*>(static_cast<char*>(dt) + tbytes);
  PAL_TRY(e->check(hipMemcpyAsync(dc, corr, count * sizeof(double), hipMemcpyHostToDevice, e->stream), "corr upload"));
  PAL_TRY(e->peaks(static_cast<const double*>(dc), size_t(n), R, n, n2, *prm, static_cast<pal_pair_record*>(dt), dk, 0));   // slot 0: on `stream`
  PAL_TRY(e->check(hipMemcpyAsync(table, dt, tbytes, hipMemcpyDeviceToHost, e->stream), "table download"));
  if (k_out)
    PAL_TRY(e->check(hipMemcpy2DAsync(k_out, size_t(prm->num_peaks) * sizeof(int32_t), dk, PAL_MAX_PEAKS * sizeof(int32_t),
                                      size_t(prm->num_peaks) * sizeof(int32_t), size_t(R), hipMemcpyDeviceToHost, e->stream), "k download"));
  return pal_synchronize(h);
}

int pal_plan_info(pal_handle h, int L, int32_t* n, int32_t* conv_len, int32_t* m1, int32_t* m2) {
  ENGINE(h);
  if (L < 1 || L > (1 << 20)) return e->fail(PAL_ERR_INVALID, "bad frame length");
  Plan* pl = nullptr;
  PAL_TRY(e->get_plan(2 * L - 1, L, 2 * L - 1, &pl));
  if (n) *n = pl->n;
  if (conv_len) *conv_len = int32_t(pl->inv.M());
  if (m1) *m1 = pl->inv.M1();
  if (m2) *m2 = pl->inv.M2();
  return PAL_OK;
}

int pal_pair_group_size(pal_handle h, int L, int32_t* transforms) {
  ENGINE(h);
  if (L < 1) return e->fail(PAL_ERR_INVALID, "frame length %d", L);
  if (transforms) *transforms = e->pair_group(2 * L - 1);
  return PAL_OK;
}

int pal_plan_factors(pal_handle h, int L, int32_t* n1, int32_t* n2, int32_t* tile_len) {
  ENGINE(h);
  if (L < 1 || L > (1 << 20)) return e->fail(PAL_ERR_INVALID, "bad frame length");
  Plan* pl = nullptr;
  PAL_TRY(e->get_plan(2 * L - 1, L, 2 * L - 1, &pl));
  if (n1) *n1 = pl->pfa.n1;
  if (n2) *n2 = pl->pfa.n2;
  if (tile_len) *tile_len = pl->pfa.on() ? (pl->pfa.rader ? pl->pfa.n2 - 1 : 1 << pl->pfa.lm) : 0;
  return PAL_OK;
}

// ---- profiling -----------------------------------------------------------------------------
int pal_profile_begin(pal_handle h) {
  ENGINE(h);
  PAL_TRY(e->check(hipStreamSynchronize(e->stream), "stream sync"));
  e->pending.clear();
  e->ev_used = 0;
  for (auto& s : e->slots) s = ProfileSlot();
  e->profiling = true;
  return PAL_OK;
}

int pal_profile_sampling(pal_handle h, int every) {
  ENGINE(h);
  if (every < 1) return e->fail(PAL_ERR_INVALID, "sampling period must be >= 1");
  e->prof_every = every;
  e->prof_tick = 0;
  return PAL_OK;
}

int pal_profile_end(pal_handle h) {
  ENGINE(h);
  PAL_TRY(e->check(hipStreamSynchronize(e->stream), "stream sync"));
  e->prof_flush();
  e->profiling = false;
  return PAL_OK;
}

int pal_profile_get(pal_handle h, const char* name, double* total_ms, int64_t* launches) {
  ENGINE(h);
  if (!name) return e->fail(PAL_ERR_INVALID, "name is NULL");
  for (size_t i = 0; i < e->slot_names.size(); ++i)
    if (e->slot_names[i] == name) {
      if (total_ms) *total_ms = e->slots[i].ms;
      if (launches) *launches = e->slots[i].launches;
      return PAL_OK;
    }
  if (total_ms) *total_ms = 0;
  if (launches) *launches = 0;
  return PAL_OK;
}

int pal_profile_entry(pal_handle h, int index, char* name, int cap, double* total_ms, int64_t* launches) {
  ENGINE(h);
  if (index < 0 || size_t(index) >= e->slot_names.size()) return PAL_ERR_INVALID;
  if (name && cap > 0) snprintf(name, size_t(cap), "%s", e->slot_names[size_t(index)].c_str());
  if (total_ms) *total_ms = e->slots[size_t(index)].ms;
  if (launches) *launches = e->slots[size_t(index)].launches;
  return PAL_OK;
}

// ---- RCCL gather (librccl is opened on first use so that the library loads on hosts without it) ----
namespace {
struct NcclId { char bytes[128]; };               // ncclUniqueId is an opaque 128-byte struct passed by value
struct Rccl {
  void* lib = nullptr;
  int (*GetUniqueId)(NcclId*) = nullptr;
  int (*CommInitRank)(void**, int, NcclId, int) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};
Rccl g_rccl;
bool rccl_open() {
  if (g_rccl.lib) return true;
  void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
  if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
  if (!lib) return false;
  g_rccl.GetUniqueId = reinterpret_cast<decltype(g_rccl.GetUniqueId)>(dlsym(lib, "ncclGetUniqueId"));
  g_rccl.CommInitRank = reinterpret_cast<decltype(g_rccl.CommInitRank)>(dlsym(lib, "ncclCommInitRank"));
  g_rccl.AllGather = reinterpret_cast<decltype(g_rccl.AllGather)>(dlsym(lib, "ncclAllGather"));
  g_rccl.CommDestroy = reinterpret_cast<decltype(g_rccl.CommDestroy)>(dlsym(lib, "ncclCommDestroy"));
  g_rccl.GetErrorString = reinterpret_cast<decltype(g_rccl.GetErrorString)>(dlsym(lib, "ncclGetErrorString"));
  if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllGather || !g_rccl.CommDestroy) return false;
  g_rccl.lib = lib;
  return true;
}
}  // namespace

int pal_comm_unique_id(void* id128) {
  if (!id128) return PAL_ERR_INVALID;
  if (!rccl_open()) return PAL_ERR_COMM;
  return g_rccl.GetUniqueId(static_cast<NcclId*>(id128)) == 0 ? PAL_OK : PAL_ERR_COMM;
}

int pal_comm_init(pal_handle h, int nranks, int rank, const void* id128) {
  ENGINE(h);
  if (!id128 || nranks < 1 || rank < 0 || rank >= nranks) return e->fail(PAL_ERR_INVALID, "bad communicator geometry");
  if (!rccl_open()) return e->fail(PAL_ERR_COMM, "librccl not loadable: %s", dlerror());
  if (e->comm) return e->fail(PAL_ERR_INVALID, "communicator already initialised");
  NcclId id;
  memcpy(&id, id128, sizeof id);
  const int rc = g_rccl.CommInitRank(&e->comm, nranks, id, rank);
  if (rc != 0) return e->fail(PAL_ERR_COMM, "ncclCommInitRank: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "error");
  return PAL_OK;
}

int pal_comm_all_gather(pal_handle h, const void* d_send, void* d_recv, size_t bytes_per_rank) {
  ENGINE(h);
  if (!e->comm) return e->fail(PAL_ERR_COMM, "communicator not initialised");
  const int rc = g_rccl.AllGather(d_send, d_recv, bytes_per_rank, /* ncclInt8 */ 0, e->comm, e->stream);
  if (rc != 0) return e->fail(PAL_ERR_COMM, "ncclAllGather: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "error");
  return PAL_OK;
}

int pal_comm_destroy(pal_handle h) {
  ENGINE(h);
  if (e->comm && g_rccl.CommDestroy) {
    hipStreamSynchronize(e->stream);
    g_rccl.CommDestroy(e->comm);
  }
  e->comm = nullptr;
  return PAL_OK;
}

}  // extern "C"
