// acf_neumf.hip — MI355X (gfx950) C-ABI for NeuMF and adversarial NeuMF
// training (include/acf_neumf.h; SURVEY.md §8(f)3, BASELINE configs[3]).
//
// Reference graph: NeuMF.py:10-52 (Keras), trained by MF.py:30-33 (fit: mean
// binary cross-entropy + Adam) and scored by MF.py:38-40.
//
// One translation unit; this file is its host half and defines no kernel.  The
// kernels are three headers, included below in the order their code has in the
// code object:
//   acf_neumf_step.h  the parameter layout, NArgs and one training step (Keras
//                     train_on_batch): k_nmf_inst, k_nmf_step, k_nmf_wsum,
//                     k_nmf_rows and their MFMA tile helpers
//   acf_neumf_rank.h  all-items ranking: k_nmf_rank, k_nmf_rank_pos (§4e)
//   acf_neumf_lazy.h  the dense Keras Adam (k_nmf_adam) and acf_neumf_train's
//                     lazy one: k_nmf_adam_next, k_nmf_adam_catchup (§9)
// Here: the library's error string, the context and its setters, the failsafe
// (error word, snapshot / restore, with_failsafe), the launch helpers and the
// entry points -- grad, adam, train, predict, rank_all and its workspace.
//
// The library's other unit, acf_keras_mf.hip (Keras BPR, FastAdversarialMF),
// takes two things from here: the one thread-local error string behind
// acf_set_error, and acf_dense_adam (acf_neumf_adam.h), the k_nmf_adam launch.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>

#include "acf_apr.h"
#include "acf_neumf.h"
#include "acf_host.h"         // HIP_TRY, ACF_CHECK, range_err
#include "acf_neumf_adam.h"   // acf_dense_adam
#include "acf_topk_select.h"  // topk_key, topk_prune, k_topk_merge (k_nmf_rank)

// libacf_neumf.so's one error string (acf_neumf_last_error), for acf_keras_mf.hip too
static thread_local std::string g_neumf_error;

int acf_set_error(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_neumf_error = buf;
  return code;
}

#include "acf_neumf_step.h"
#include "acf_neumf_rank.h"
#include "acf_neumf_lazy.h"

struct acf_neumf_ctx {
  int64_t U1 = 0, I1 = 0;
  int32_t d = 0, maxB = 0;
  Layout L;
  float *contrib = nullptr, *delta = nullptr;
  float *h0 = nullptr, *a1 = nullptr, *dz1 = nullptr, *dz2 = nullptr;  // weight-gradient operands
  float* wpart = nullptr;  // [2 passes][slots][weight-gradient outputs]
  int32_t nslot = 0;       // workgroups (slots) of a training pass at max_batch
  int32_t *owner = nullptr, *err = nullptr;
  int32_t* rcnt = nullptr;  // rows in line: arrivals per row [2][U1 + I1] (clean, adversarial)
  unsigned long long* rdone = nullptr;  // [U1 + I1] k_nmf_step's published rows
  int32_t gen = 0;                      // k_nmf_step launches so far
  int32_t rows_in_line = 1;  // B <= FR_MAXB: rows in line (acf_neumf_set_rows_in_line: 0 = k_nmf_rows)
  // acf_neumf_train's lazy Adam: each row's last iteration, the side stream and its events
  int32_t *last_u = nullptr, *last_i = nullptr, *pend_u = nullptr, *pend_i = nullptr;
  hipStream_t side = nullptr;
  hipEvent_t ev_next = nullptr, ev_rest = nullptr;
  int32_t lazy_s = LAZY_S;           // catch-up period (< LAZY_W)
  int64_t catchup_wg = CATCHUP_WG;   // workgroups of a catch-up slice
  // rows-in-line failure safety (acf_neumf_set_spin_limit / _set_failsafe): a give-up
  // (err bit 512) is replayed from a snapshot of the call's inputs on the row-sum path
  int32_t spin = ACF_SPIN_LIMIT;
  int32_t failsafe = 1;
  int64_t recoveries = 0;     // calls replayed
  bool unchecked_fr = false;  // an unchecked rows-in-line grad has not been verified yet
  float* snap = nullptr;      // [P | G | m | v] of the call being verified (allocated at first use)
  size_t snap_n = 0;          // floats in snap
  std::vector<void*> allocs;
};

extern "C" const char* acf_neumf_last_error(void) { return g_neumf_error.c_str(); }

#ifndef ACF_BUILD_HASH
#define ACF_BUILD_HASH "unhashed"
#endif
extern "C" const char* acf_neumf_build_hash(void) { return "ACF_BUILD_HASH=" ACF_BUILD_HASH; }

static int check_dims(int64_t U1, int64_t I1, int32_t d) {
  ACF_CHECK(U1 > 0 && I1 > 0 && U1 < (1ll << 31) && I1 < (1ll << 31), ACF_E_INVALID,
            "table rows must be in [1, 2^31): got %lld, %lld", (long long)U1, (long long)I1);
  ACF_CHECK(d >= 4 && d <= 64 * MAX_Q && d % 4 == 0, ACF_E_INVALID,
            "dim must be a multiple of 4 in [4, %d], got %d", 64 * MAX_Q, d);
  return ACF_OK;
}

extern "C" int64_t acf_neumf_param_count(int64_t U1, int64_t I1, int32_t d) {
  if (check_dims(U1, I1, d) != ACF_OK) return -1;
  return make_layout(U1, I1, d).total;
}

extern "C" int acf_neumf_param_offsets(int64_t U1, int64_t I1, int32_t d, int64_t* off) {
  ACF_RET(check_dims(U1, I1, d));
  ACF_CHECK(off != nullptr, ACF_E_INVALID, "offsets pointer is NULL");
  const Layout L = make_layout(U1, I1, d);
  for (int k = 0; k < S_COUNT; ++k) off[k] = L.off[k];
  return ACF_OK;
}

extern "C" int acf_neumf_set_rows_in_line(acf_neumf_ctx* c, int32_t on) {
  ACF_CHECK(c != nullptr, ACF_E_INVALID, "ctx is NULL");
  c->rows_in_line = on ? 1 : 0;
  return ACF_OK;
}

extern "C" int acf_neumf_set_spin_limit(acf_neumf_ctx* c, int32_t polls) {
  ACF_CHECK(c != nullptr, ACF_E_INVALID, "ctx is NULL");
  ACF_CHECK(polls >= 0, ACF_E_INVALID, "spin limit must be >= 0, got %d", polls);
  c->spin = polls;
  return ACF_OK;
}

extern "C" int acf_neumf_set_failsafe(acf_neumf_ctx* c, int32_t on) {
  ACF_CHECK(c != nullptr, ACF_E_INVALID, "ctx is NULL");
  c->failsafe = on ? 1 : 0;
  return ACF_OK;
}

extern "C" int acf_neumf_recoveries(acf_neumf_ctx* c, int64_t* out) {
  ACF_CHECK(c != nullptr && out != nullptr, ACF_E_INVALID, "NULL argument");
  *out = c->recoveries;
  return ACF_OK;
}

extern "C" int acf_neumf_destroy(acf_neumf_ctx* c) {
  if (!c) return ACF_OK;
  if (c->side) (void)hipStreamSynchronize(c->side);
  for (void* p : c->allocs) (void)hipFree(p);
  if (c->snap) (void)hipFree(c->snap);
  if (c->ev_next) (void)hipEventDestroy(c->ev_next);
  if (c->ev_rest) (void)hipEventDestroy(c->ev_rest);
  if (c->side) (void)hipStreamDestroy(c->side);
  delete c;
  return ACF_OK;
}

static int set_inst_smem_limit();

extern "C" int acf_neumf_create(acf_neumf_ctx** out, int64_t U1, int64_t I1, int32_t d,
                                int32_t maxB) {
  ACF_CHECK(out != nullptr, ACF_E_INVALID, "out is NULL");
  *out = nullptr;
  ACF_RET(check_dims(U1, I1, d));
  ACF_CHECK(maxB > 0 && maxB <= (1 << 24), ACF_E_INVALID, "max_batch must be in (0, 2^24], got %d", maxB);
  acf_neumf_ctx* c = new acf_neumf_ctx();
  c->U1 = U1; c->I1 = I1; c->d = d; c->maxB = maxB;
  c->L = make_layout(U1, I1, d);
  const size_t B = (size_t)maxB, dd = (size_t)d;
  int r = ACF_OK;  // the first failure; the allocations after it are skipped
  auto A = [&](auto** p, size_t n) {
    if (r != ACF_OK) return;
    void* q = nullptr;
    if (hipMalloc(&q, n * sizeof(**p) + 16) != hipSuccess) {
      (void)hipGetLastError();
      r = acf_set_error(ACF_E_NOMEM, "hipMalloc of %zu bytes failed", n * sizeof(**p));
      return;
    }
    c->allocs.push_back(q);
    *p = static_cast<std::remove_reference_t<decltype(*p)>>(q);
  };
  A(&c->contrib, B * 4 * dd); A(&c->delta, B * 4 * dd); A(&c->owner, 2 * B); A(&c->err, 4);
  A(&c->rcnt, 2 * (size_t)(U1 + I1)); A(&c->rdone, (size_t)(U1 + I1));
  // two sets (clean / adversarial pass): the clean pass's gradient workgroups read theirs
  // while the adversarial k_nmf_inst writes its own
  A(&c->h0, 2 * B * 2 * dd); A(&c->a1, 2 * B * 2 * dd); A(&c->dz1, 2 * B * 2 * dd); A(&c->dz2, 2 * B * dd);
  A(&c->last_u, (size_t)U1); A(&c->last_i, (size_t)I1); A(&c->pend_u, (size_t)U1); A(&c->pend_i, (size_t)I1);
  // (the catch-up stream at the least stream priority measured the same:
  // profiles/r05/neumf_side_priority_ab.txt)
  if (r == ACF_OK && (hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) != hipSuccess ||
                      hipEventCreateWithFlags(&c->ev_next, hipEventDisableTiming) != hipSuccess ||
                      hipEventCreateWithFlags(&c->ev_rest, hipEventDisableTiming) != hipSuccess))
    r = acf_set_error(ACF_E_HIP, "lazy-Adam setup failed");
  c->nslot = (int32_t)std::min<int64_t>(((int64_t)maxB + MR - 1) / MR, NSLOT);
  A(&c->wpart, 2 * (size_t)c->nslot * (size_t)wout(d).n);
  if (r == ACF_OK && (hipMemset(c->err, 0, 16) != hipSuccess || hipMemset(c->rcnt, 0, 2 * (size_t)(U1 + I1) * sizeof(int32_t)) != hipSuccess ||
                      hipMemset(c->rdone, 0, (size_t)(U1 + I1) * sizeof(unsigned long long)) != hipSuccess ||
                      hipDeviceSynchronize() != hipSuccess))
    r = acf_set_error(ACF_E_HIP, "hipMemset failed");
  if (r == ACF_OK) r = set_inst_smem_limit();
  if (r != ACF_OK) { acf_neumf_destroy(c); return r; }
  *out = c;
  return ACF_OK;
}

static NArgs make_args(acf_neumf_ctx* c, const float* P, float* G, const int32_t* u, const int32_t* i,
                       const float* y, int32_t B, float scale) {
  NArgs a;
  a.P = P; a.G = G;
  for (int k = 0; k < S_COUNT; ++k) a.off[k] = c->L.off[k];
  a.u = u; a.i = i; a.y = y;
  a.U1 = c->U1; a.I1 = c->I1; a.B = B; a.d = c->d;
  a.scale_over_B = (float)((double)scale / (double)B);
  a.contrib = c->contrib; a.wpart = c->wpart;
  a.h0 = c->h0; a.a1 = c->a1; a.dz1 = c->dz1; a.dz2 = c->dz2;
  a.delta = c->delta; a.owner = c->owner; a.pred = nullptr; a.err = c->err;
  a.rcnt = c->rcnt; a.with_delta = 0; a.eps = 0.f; a.rdone = c->rdone; a.gen = 0; a.spin = c->spin;
  return a;
}

// fr_b: the batch of a rows-in-line launch (its row waves stage its indices), 0 otherwise
static size_t inst_smem(int d, int fr_b = 0) {
  return (size_t)std::max<int64_t>(inst_floats(d), 2 * (int64_t)fr_b) * sizeof(float);
}

// allow the large dynamic LDS of k_nmf_inst (gfx950: 160 KB per CU)
static int set_inst_smem_limit() {
  static int done = 0;
  if (done) return ACF_OK;
  const int bytes = 150 * 1024;
  const void* fns[] = {reinterpret_cast<const void*>(&k_nmf_inst<0, 0>),
                       reinterpret_cast<const void*>(&k_nmf_inst<1, 0>),
                       reinterpret_cast<const void*>(&k_nmf_inst<2, 0>),
                       reinterpret_cast<const void*>(&k_nmf_inst<0, DFAST>),
                       reinterpret_cast<const void*>(&k_nmf_inst<1, DFAST>),
                       reinterpret_cast<const void*>(&k_nmf_inst<2, DFAST>),
                       reinterpret_cast<const void*>(&k_nmf_inst<0, 0, true>),
                       reinterpret_cast<const void*>(&k_nmf_inst<1, 0, true>),
                       reinterpret_cast<const void*>(&k_nmf_inst<0, DFAST, true>),
                       reinterpret_cast<const void*>(&k_nmf_inst<1, DFAST, true>),
                       reinterpret_cast<const void*>(&k_nmf_step<0>),
                       reinterpret_cast<const void*>(&k_nmf_rank<0>),
                       reinterpret_cast<const void*>(&k_nmf_rank<DFAST>),
                       reinterpret_cast<const void*>(&k_nmf_step<DFAST>)};
  for (const void* f : fns) HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  // k_nmf_rows: 16 KB of indices + the gradient workgroups' operands (d = 128: 58 KB)
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_nmf_rows),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)wgrad_smem(128)));
  done = 1;
  return ACF_OK;
}

static int fetch_err(acf_neumf_ctx* c, hipStream_t s, int32_t* herr) {
  *herr = 0;
  HIP_TRY(hipMemcpyAsync(herr, c->err, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return ACF_OK;
}

static int check_err(int32_t herr) {
  ACF_CHECK(!(herr & 256), ACF_E_HIP, "lazy Adam: a row fell behind the learning-rate window (internal)");
  ACF_CHECK(!(herr & 512), ACF_E_HIP, "rows in line: a row wave timed out waiting for its arrivals "
            "(failsafe off: the call's results are undefined)");
  return range_err(herr);
}

static int read_err(acf_neumf_ctx* c, hipStream_t s) {
  int32_t herr = 0;
  ACF_RET(fetch_err(c, s, &herr));
  return check_err(herr);
}

// After a give-up: late arrivals may have landed after their owner re-armed its
// counter, so every arrival counter is zeroed (the stream is idle: fetch_err
// synchronised it) before anything else runs on this context.  rdone needs no
// reset: its entries carry the launch generation.
static int reset_row_counters(acf_neumf_ctx* c, hipStream_t s) {
  HIP_TRY(hipMemsetAsync(c->rcnt, 0, 2 * (size_t)(c->U1 + c->I1) * sizeof(int32_t), s));
  HIP_TRY(hipMemsetAsync(c->err, 0, sizeof(int32_t), s));
  HIP_TRY(hipStreamSynchronize(s));
  return ACF_OK;
}

// An unchecked acf_neumf_grad on the rows-in-line path is verified by the next
// call that reads the error word (grad with check, train, predict) before that
// call clears it: a give-up there cannot be replayed any more (the caller may have
// consumed the gradient), so it is reported, never dropped.
static int settle_unchecked(acf_neumf_ctx* c, hipStream_t s) {
  if (!c->unchecked_fr) return ACF_OK;
  int32_t herr = 0;
  ACF_RET(fetch_err(c, s, &herr));
  c->unchecked_fr = false;
  if (herr & 512) {
    ACF_RET(reset_row_counters(c, s));
    return acf_set_error(ACF_E_HIP, "rows in line: an earlier unchecked acf_neumf_grad call timed out waiting for "
                     "its arrivals; the gradient it added is undefined");
  }
  return ACF_OK;
}

// the failsafe's snapshot of the buffers a call writes (nbuf of P, G, m, v: each
// L.total floats), taken on the call's stream before its first launch
static int take_snapshot(acf_neumf_ctx* c, hipStream_t s, float* const* bufs, int nbuf) {
  const size_t n = (size_t)c->L.total;
  if (c->snap_n < 4 * n) {
    if (c->snap) HIP_TRY(hipFree(c->snap));
    c->snap = nullptr;
    c->snap_n = 0;
    if (hipMalloc(&c->snap, 4 * n * sizeof(float)) != hipSuccess) {
      (void)hipGetLastError();
      c->snap = nullptr;
      return acf_set_error(ACF_E_NOMEM, "failsafe snapshot: hipMalloc of %zu bytes failed", 4 * n * sizeof(float));
    }
    c->snap_n = 4 * n;
  }
  for (int k = 0; k < nbuf; ++k)
    HIP_TRY(hipMemcpyAsync(c->snap + k * n, bufs[k], n * sizeof(float), hipMemcpyDeviceToDevice, s));
  return ACF_OK;
}

static int restore_snapshot(acf_neumf_ctx* c, hipStream_t s, float* const* bufs, int nbuf) {
  const size_t n = (size_t)c->L.total;
  for (int k = 0; k < nbuf; ++k)
    HIP_TRY(hipMemcpyAsync(bufs[k], c->snap + k * n, n * sizeof(float), hipMemcpyDeviceToDevice, s));
  return ACF_OK;
}

// The failsafe frame of a checked call (acf_neumf_grad, acf_neumf_train): run() is
// the call's launches on s, and it is verified once, at its end (it synchronises
// there anyway).  fr: the call can run a batch in line; with the failsafe on, the
// nbuf buffers it writes are copied first.  A give-up (err bit 512) zeroes the
// arrival counters; with a snapshot the buffers are restored and the whole call
// is replayed on the row-sum path, which gives the same bits
// (test_neumf_give_up_replays_exactly).  replay_needs_fr: grad acts on the bit
// only when fr, train on the bit alone (whatever gave up, no stale counter
// outlives the call).
template <class Run>
static int with_failsafe(acf_neumf_ctx* c, hipStream_t s, bool fr, bool replay_needs_fr, float* const* bufs,
                         int nbuf, Run run) {
  const bool snap = fr && c->failsafe;
  if (snap) ACF_RET(take_snapshot(c, s, bufs, nbuf));
  ACF_RET(run());
  int32_t herr = 0;
  ACF_RET(fetch_err(c, s, &herr));
  if ((herr & 512) && (fr || !replay_needs_fr)) {
    ACF_RET(reset_row_counters(c, s));
    if (!snap) return check_err(herr);  // (snap implies fr)
    ACF_RET(restore_snapshot(c, s, bufs, nbuf));
    c->rows_in_line = 0;
    const int r = run();
    c->rows_in_line = 1;
    ACF_RET(r);
    ++c->recoveries;
    ACF_RET(fetch_err(c, s, &herr));
  }
  return check_err(herr);
}

// grid = inst workgroups + (optional) the previous pass's weight-gradient workgroups (args wg)
template <int MODE, bool FR = false>
static void launch_inst(const NArgs& a, unsigned inst_blocks, hipStream_t s, const NArgs* wg = nullptr,
                        unsigned wg_blocks = 0) {
  const NArgs& w = wg ? *wg : a;
  // extra workgroups: the previous pass's weight-gradient workgroups (wg), or FR's row waves
  const unsigned grid = inst_blocks + ((wg || FR) ? wg_blocks : 0u);
  const size_t sm = inst_smem(a.d, FR ? a.B : 0);
  if (a.d == DFAST)
    k_nmf_inst<MODE, DFAST, FR><<<grid, 256, sm, s>>>(a, w, inst_blocks);
  else
    k_nmf_inst<MODE, 0, FR><<<grid, 256, sm, s>>>(a, w, inst_blocks);
}

// clean pass: k_nmf_inst<0> -> k_nmf_rows (owners, rows, delta; + the pass's
// weight-gradient tiles); adversarial pass: k_nmf_inst<1> -> k_nmf_rows; then
// k_nmf_wsum sums the passes' slots into G, unless the caller leaves that to
// k_nmf_adam (acf_neumf_train).  B <= FR_MAXB: one k_nmf_inst<.., true> per pass
// (rows and weight-gradient tiles in line).
static int launch_grad(acf_neumf_ctx* c, const float* P, float* G, const int32_t* u, const int32_t* i,
                       const float* y, int32_t B, const acf_neumf_hparams* hp, float* loss_out,
                       hipStream_t s, bool wsum = true) {
  const unsigned gi = (unsigned)std::min<int64_t>(((int64_t)B + MR - 1) / MR, NSLOT);
  const unsigned gr = (unsigned)((2 * (int64_t)B + 3) / 4);
  const unsigned gw = gi * (unsigned)((wtiles(c->d) + WG_TILES - 1) / WG_TILES);  // gradient workgroups
  const size_t sw = wgrad_smem(c->d);
  const WOut o = wout(c->d);
  const int npass = hp->adver ? 2 : 1;
  NArgs a = make_args(c, P, G, u, i, y, B, 1.0f);
  // both passes in one launch: faster than one launch per pass
  // (profiles/r05/neumf_rows_in_line_ab.txt; DESIGN.md §9, knob table)
  if (B <= FR_MAXB && c->rows_in_line && hp->adver) {
    a.with_delta = 1;
    a.eps = hp->eps;
    a.gen = ++c->gen;
    NArgs b = make_args(c, P, G, u, i, y, B, hp->reg_adv);
    b.wpart = c->wpart + (int64_t)gi * o.n;
    b.rcnt = c->rcnt + (c->U1 + c->I1);
    b.gen = a.gen;
    const size_t sm = inst_smem(c->d, B);
    if (c->d == DFAST) k_nmf_step<DFAST><<<2 * (gi + gr), 256, sm, s>>>(a, b, gi, gr);
    else k_nmf_step<0><<<2 * (gi + gr), 256, sm, s>>>(a, b, gi, gr);
    HIP_TRY(hipGetLastError());
  } else if (B <= FR_MAXB && c->rows_in_line) {
    a.with_delta = hp->adver ? 1 : 0;
    a.eps = hp->eps;
    // a row wave per (instance, side): fewer measured slower
    // (profiles/r05/neumf_rows_in_line_ab.txt; DESIGN.md §9, knob table)
    launch_inst<0, true>(a, gi, s, nullptr, gr);
    HIP_TRY(hipGetLastError());
    if (hp->adver) {
      NArgs b = make_args(c, P, G, u, i, y, B, hp->reg_adv);
      b.wpart = c->wpart + (int64_t)gi * o.n;
      launch_inst<1, true>(b, gi, s, nullptr, gr);
      HIP_TRY(hipGetLastError());
    }
  } else {
    launch_inst<0>(a, gi, s);
    // APR-style: the clean pass's gradient workgroups ride in the adversarial
    // k_nmf_inst (32 workgroups at B = 512: the other CUs are idle); BPR-style
    // (no adversary) in its k_nmf_rows
    k_nmf_rows<<<gr + (hp->adver ? 0u : gw), 256, sw, s>>>(a, c->owner, c->delta, hp->adver ? 1 : 0, hp->eps, gr,
                                                          (int)gi);
    HIP_TRY(hipGetLastError());
    if (hp->adver) {
      NArgs b = make_args(c, P, G, u, i, y, B, hp->reg_adv);
      b.wpart = c->wpart + (int64_t)gi * o.n;
      const int64_t ab = (int64_t)c->maxB;  // the second activation buffer
      b.h0 += ab * 2 * c->d; b.a1 += ab * 2 * c->d; b.dz1 += ab * 2 * c->d; b.dz2 += ab * c->d;
      launch_inst<1>(b, gi, s, &a, gw);
      k_nmf_rows<<<gr + gw, 256, sw, s>>>(b, c->owner, c->delta, 0, 0.f, gr, (int)gi);
      HIP_TRY(hipGetLastError());
    }
  }
  if (wsum) {
    k_nmf_wsum<<<(unsigned)((o.n + 255) / 256), 256, 0, s>>>(a, (int)gi, npass, c->wpart, loss_out);
    HIP_TRY(hipGetLastError());
  }
  return ACF_OK;
}

extern "C" int acf_neumf_grad(acf_neumf_ctx* c, const float* P, float* G, const int32_t* u,
                              const int32_t* i, const float* y, int32_t B, const acf_neumf_hparams* hp,
                              float* loss_out, int32_t check, void* stream_) {
  ACF_CHECK(c && P && G && u && i && y && hp, ACF_E_INVALID, "NULL argument");
  ACF_CHECK(B > 0 && B <= c->maxB, ACF_E_INVALID, "batch %d outside (0, %d]", B, c->maxB);
  hipStream_t s = static_cast<hipStream_t>(stream_);
  const bool fr = B <= FR_MAXB && c->rows_in_line;
  if (!check) {  // verified by the next checking call (settle_unchecked)
    ACF_RET(launch_grad(c, P, G, u, i, y, B, hp, loss_out, s));
    if (fr) c->unchecked_fr = true;
    return ACF_OK;
  }
  ACF_RET(settle_unchecked(c, s));
  HIP_TRY(hipMemsetAsync(c->err, 0, sizeof(int32_t), s));
  float* bufs[1] = {G};  // the exact replay: G as the call found it
  return with_failsafe(c, s, fr, true, bufs, 1, [&] { return launch_grad(c, P, G, u, i, y, B, hp, loss_out, s); });
}

// lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t), evaluated in float32 as Keras does
static float adam_lr_t(const acf_neumf_hparams* hp, int64_t t) {
  const float tt = (float)t;
  return hp->lr * (sqrtf(1.0f - powf(hp->beta2, tt)) / (1.0f - powf(hp->beta1, tt)));
}

// the dense k_nmf_adam launch of this library (acf_neumf_adam.h): NeuMF's, Keras BPR's, FastAdversarialMF's
int acf_dense_adam(float* P, float* G, float* m, float* v, int64_t n4, int64_t t, const acf_neumf_hparams* hp,
                   hipStream_t s) {
  const float lr_t = adam_lr_t(hp, t);
  const unsigned grid = (unsigned)std::min<int64_t>((n4 + 255) / 256, 256 * 32);
  k_nmf_adam<<<grid, 256, 0, s>>>(reinterpret_cast<float4*>(P), reinterpret_cast<float4*>(G),
                                  reinterpret_cast<float4*>(m), reinterpret_cast<float4*>(v), n4,
                                  hp->beta1, hp->beta2, lr_t, hp->adam_eps);
  HIP_TRY(hipGetLastError());
  return ACF_OK;
}

static int launch_adam(acf_neumf_ctx* c, float* P, float* G, float* m, float* v, int64_t t,
                       const acf_neumf_hparams* hp, hipStream_t s) {
  return acf_dense_adam(P, G, m, v, c->L.total / 4, t, hp, s);
}

extern "C" int acf_neumf_adam(acf_neumf_ctx* c, float* P, float* G, float* m, float* v, int64_t t,
                              const acf_neumf_hparams* hp, void* stream_) {
  ACF_CHECK(c && P && G && m && v && hp, ACF_E_INVALID, "NULL argument");
  ACF_CHECK(t >= 1, ACF_E_INVALID, "Adam iteration must be >= 1, got %lld", (long long)t);
  return launch_adam(c, P, G, m, v, t, hp, static_cast<hipStream_t>(stream_));
}

static int train_launches(acf_neumf_ctx* c, float* P, float* G, float* m, float* v, const int32_t* u,
                          const int32_t* i, const float* y, int64_t n, int32_t batch, int64_t t_first,
                          const acf_neumf_hparams* hp, float* losses, hipStream_t s) {
  HIP_TRY(hipMemsetAsync(c->err, 0, sizeof(int32_t), s));
  float4 *P4 = reinterpret_cast<float4*>(P), *G4 = reinterpret_cast<float4*>(G);
  float4 *m4 = reinterpret_cast<float4*>(m), *v4 = reinterpret_cast<float4*>(v);
  const int64_t n4 = c->L.total / 4, emb4 = c->L.off[S_W1] / 4;
  const int64_t nsteps = (n + batch - 1) / batch;
  ACF_CHECK(t_first + nsteps < INT32_MAX, ACF_E_INVALID, "Adam iteration overflows int32");
  AdamLazy z;
  z.U1 = c->U1; z.I1 = c->I1; z.d4 = c->d / 4;
  z.last_u = c->last_u; z.last_i = c->last_i; z.pend_u = c->pend_u; z.pend_i = c->pend_i; z.err = c->err;
  // every row has taken iteration t_first - 1, and G holds its gradient of
  // iteration t_first (what the caller accumulated, plus step 0's)
  k_nmf_fill_i32<<<(unsigned)((c->U1 + 255) / 256), 256, 0, s>>>(c->last_u, c->U1, (int32_t)(t_first - 1));
  k_nmf_fill_i32<<<(unsigned)((c->I1 + 255) / 256), 256, 0, s>>>(c->last_i, c->I1, (int32_t)(t_first - 1));
  k_nmf_fill_i32<<<(unsigned)((c->U1 + 255) / 256), 256, 0, s>>>(c->pend_u, c->U1, (int32_t)t_first);
  k_nmf_fill_i32<<<(unsigned)((c->I1 + 255) / 256), 256, 0, s>>>(c->pend_i, c->I1, (int32_t)t_first);
  HIP_TRY(hipGetLastError());
  const int64_t nrows = c->U1 + c->I1;
  // k_nmf_adam_next's tail: 32 / gp float4s per wave, gp = the slot groups of a full
  // batch rounded up to a power of two (a smaller last batch packs more per wave)
  const int ng_max = (int)((std::min<int64_t>((batch + MR - 1) / MR, NSLOT) + SB - 1) / SB);
  int gp2 = 1;
  while (gp2 < ng_max) gp2 <<= 1;
  const int64_t tail_waves = (n4 - emb4 + 32 / gp2 - 1) / (32 / gp2);
  const unsigned tail_blocks = (unsigned)std::min<int64_t>((tail_waves + 3) / 4, 2048);
  const int lpr = 2 * z.d4 <= 32 ? 32 : 64;
  auto rows_grid = [&](int64_t rows, int64_t cap) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((rows * lpr + 255) / 256, cap));
  };
  const int64_t slice = (nrows + c->lazy_s - 1) / c->lazy_s;
  bool side_pending = false;
  AdamK ak{};
  int64_t k = 0;
  for (int64_t o = 0; o < n; o += batch, ++k) {
    const int32_t B = (int32_t)std::min<int64_t>(batch, n - o);
    int r = launch_grad(c, P, G, u + o, i + o, y + o, B, hp, nullptr, s, false);
    if (r != ACF_OK) {
      if (side_pending) (void)hipStreamWaitEvent(s, c->ev_rest, 0);
      return r;
    }
    // Adam iteration t of step k: batch k+1's rows (up to t) and the parameter tail
    // now, with the weight-gradient slot sums (acf_neumf_grad's wsum arithmetic);
    // every other row's iterations later (k_nmf_adam_catchup)
    AdamSlots ws;
    ws.part = c->wpart;
    ws.nslot = (int)std::min<int64_t>(((int64_t)B + MR - 1) / MR, NSLOT);
    ws.npass = hp->adver ? 2 : 1;
    ws.base4 = emb4;
    ws.nout = wout(c->d).n;
    ws.loss_out = losses ? losses + 2 * k : nullptr;
    ws.B = (float)B;
    const int64_t t = t_first + k;
    ak = AdamK{hp->beta1, hp->beta2, adam_lr_t(hp, t), hp->adam_eps};
    z.t = (int32_t)t;
    for (int x = 0; x < LAZY_W; ++x) {
      const int64_t tau = t - (LAZY_W - 1) + x;
      z.lr[x] = tau >= 1 ? adam_lr_t(hp, tau) : 0.f;
    }
    const int64_t on = o + batch;
    const int32_t Bn = on < n ? (int32_t)std::min<int64_t>(batch, n - on) : 0;
    const unsigned row_blocks = (unsigned)((2 * (int64_t)Bn * 64 + 255) / 256);
    if (side_pending) HIP_TRY(hipStreamWaitEvent(s, c->ev_rest, 0));  // the catch-up of step k-1
    k_nmf_adam_next<<<row_blocks + tail_blocks, 256, 0, s>>>(P4, G4, m4, v4, n4, emb4, ak, ws, z, u + on, i + on,
                                                            Bn, row_blocks);
    HIP_TRY(hipGetLastError());
    side_pending = false;
    if (Bn > 0) {  // slice k % LAZY_S of the rows, beside step k+1
      const int64_t lo = (k % c->lazy_s) * slice, hi = std::min<int64_t>(lo + slice, nrows);
      if (lo < hi) {
        HIP_TRY(hipEventRecord(c->ev_next, s));
        HIP_TRY(hipStreamWaitEvent(c->side, c->ev_next, 0));
        k_nmf_adam_catchup<<<rows_grid(hi - lo, c->catchup_wg), 256, 0, c->side>>>(P4, G4, m4, v4, ak, z, lo, hi);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(c->ev_rest, c->side));
        side_pending = true;
      }
    }
  }
  if (side_pending) HIP_TRY(hipStreamWaitEvent(s, c->ev_rest, 0));
  if (k > 0) {  // every row to the last iteration
    k_nmf_adam_catchup<<<rows_grid(nrows, 256 * 16), 256, 0, s>>>(P4, G4, m4, v4, ak, z, 0, nrows);
    HIP_TRY(hipGetLastError());
  }
  return ACF_OK;
}

// One failsafe frame round the whole call (with_failsafe): with the rows-in-line
// step and the failsafe on, P, G, m, v are copied first (4 x the parameter bytes,
// D2D: ~40 us for the yelp shape against a ~150 ms epoch).
extern "C" int acf_neumf_train(acf_neumf_ctx* c, float* P, float* G, float* m, float* v,
                               const int32_t* u, const int32_t* i, const float* y, int64_t n,
                               int32_t batch, int64_t t_first, const acf_neumf_hparams* hp,
                               float* losses, void* stream_) {
  ACF_CHECK(c && P && G && m && v && u && i && y && hp, ACF_E_INVALID, "NULL argument");
  ACF_CHECK(batch > 0 && batch <= c->maxB, ACF_E_INVALID, "batch %d outside (0, %d]", batch, c->maxB);
  ACF_CHECK(n >= 0 && t_first >= 1, ACF_E_INVALID, "bad instance count or Adam iteration");
  hipStream_t s = static_cast<hipStream_t>(stream_);
  ACF_RET(settle_unchecked(c, s));
  // any batch of the call in line: the full batches, or a shorter last one
  const int64_t tail = n % batch;
  const bool fr = n > 0 && c->rows_in_line && (batch <= FR_MAXB || (tail != 0 && tail <= FR_MAXB));
  float* bufs[4] = {P, G, m, v};
  return with_failsafe(c, s, fr, false, bufs, 4, [&] {
    return train_launches(c, P, G, m, v, u, i, y, n, batch, t_first, hp, losses, s);
  });
}

#ifdef NMF_DIAG
extern "C" int acf_neumf_diag_stamps(uint64_t* out) {
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_nmf_stamps), 16 * sizeof(uint64_t)));
  HIP_TRY(hipMemcpyFromSymbol(out + 16, HIP_SYMBOL(g_nmf_rstamps), 8 * sizeof(uint64_t)));
  HIP_TRY(hipMemcpyFromSymbol(out + 24, HIP_SYMBOL(g_nmf_wstamps), 8 * sizeof(uint64_t)));
  return ACF_OK;
}
#endif

extern "C" int acf_neumf_predict(acf_neumf_ctx* c, const float* P, const int32_t* u, const int32_t* i,
                                 int64_t n, float* out, void* stream_) {
  ACF_CHECK(c && P && u && i && out, ACF_E_INVALID, "NULL argument");
  ACF_CHECK(n >= 0, ACF_E_INVALID, "negative count");
  hipStream_t s = static_cast<hipStream_t>(stream_);
  ACF_RET(settle_unchecked(c, s));
  HIP_TRY(hipMemsetAsync(c->err, 0, sizeof(int32_t), s));
  const int64_t chunk = 1 << 28;
  for (int64_t o = 0; o < n; o += chunk) {
    const int32_t m = (int32_t)std::min(chunk, n - o);
    NArgs a = make_args(c, P, nullptr, u + o, i + o, nullptr, m, 1.0f);
    a.pred = out + o;
    launch_inst<2>(a, (unsigned)std::min<int64_t>(((int64_t)m + MR - 1) / MR, 512), s);
    HIP_TRY(hipGetLastError());
  }
  return read_err(c, s);
}

// ---- all-items ranking: strips, workspace, the call -------------------------
// Strips of equal length (a multiple of MR) in [RK_STRIP_MIN, RK_STRIP_MAX]: as few
// as the bitmap allows when the users alone fill the device, more (down to
// RK_STRIP_MIN candidates each) when they do not.
static void rank_strips(int32_t n_users, int32_t nc, int* S, int* strip_len) {
  const int64_t lo = ((int64_t)nc + RK_STRIP_MAX - 1) / RK_STRIP_MAX;
  const int64_t hi = std::max<int64_t>(lo, ((int64_t)nc + RK_STRIP_MIN - 1) / RK_STRIP_MIN);
  const int64_t want = ((int64_t)RK_TARGET_WG + std::max(n_users, 1) - 1) / std::max(n_users, 1);
  const int64_t s = std::min(std::max(want, lo), hi);
  int64_t len = ((int64_t)nc + s - 1) / s;
  len = (len + MR - 1) / MR * MR;
  *strip_len = (int)len;
  *S = (int)(((int64_t)nc + len - 1) / len);
}

struct RankWs {
  size_t keys, cnt, tscore, total;  // byte offsets
};

static size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

static RankWs rank_ws(int32_t n_users, int32_t nc, int32_t k) {
  int S, len;
  rank_strips(n_users, nc, &S, &len);
  RankWs w;
  w.keys = 0;
  w.cnt = up16((size_t)n_users * S * k * sizeof(uint64_t));
  w.tscore = w.cnt + up16((size_t)n_users * S * sizeof(int32_t));
  w.total = w.tscore + up16((size_t)n_users * sizeof(float)) + 16;
  return w;
}

static int rank_check_shape(int32_t n_users, int32_t nc, int32_t k) {
  ACF_CHECK(n_users >= 0, ACF_E_INVALID, "n_users must be >= 0, got %d", n_users);
  ACF_CHECK(nc >= 1, ACF_E_INVALID, "num_candidates must be >= 1, got %d", nc);
  ACF_CHECK(k >= 0 && k <= TOPK_MAX_K, ACF_E_INVALID, "k must be in [0, %d], got %d", TOPK_MAX_K, k);
  return ACF_OK;
}

extern "C" int acf_neumf_rank_all_workspace(int32_t n_users, int32_t nc, int32_t k, size_t* bytes) {
  ACF_CHECK(bytes != nullptr, ACF_E_INVALID, "bytes pointer is NULL");
  ACF_RET(rank_check_shape(n_users, nc, k));
  *bytes = rank_ws(n_users, nc, k).total;
  return ACF_OK;
}

extern "C" int acf_neumf_rank_all(acf_neumf_ctx* c, const float* P, const int32_t* users, int32_t n_users,
                                  int32_t nc, const int64_t* excl_off, const int32_t* excl_items,
                                  const int32_t* test_items, int32_t* positions, int32_t k,
                                  int32_t* out_items, float* out_scores, void* ws, size_t ws_bytes,
                                  void* stream_) {
  ACF_CHECK(c && P, ACF_E_INVALID, "NULL argument");
  ACF_RET(rank_check_shape(n_users, nc, k));
  ACF_CHECK(nc <= c->I1, ACF_E_INVALID, "num_candidates %d exceeds num_item_rows %lld", nc, (long long)c->I1);
  ACF_CHECK((test_items == nullptr) == (positions == nullptr), ACF_E_INVALID,
            "test_items and positions must both be set or both be NULL");
  ACF_CHECK(k > 0 || positions, ACF_E_INVALID, "nothing to compute: k == 0 and no positions");
  ACF_CHECK(k == 0 ? (!out_items && !out_scores) : (out_items && out_scores), ACF_E_INVALID,
            "out_items / out_scores must both be set for k > 0 and both be NULL for k == 0");
  ACF_CHECK(excl_off == nullptr || excl_items != nullptr, ACF_E_INVALID, "excl_off without excl_items");
  ACF_CHECK(n_users == 0 || users, ACF_E_INVALID, "users is NULL");
  const RankWs w = rank_ws(n_users, nc, k);
  ACF_CHECK(ws != nullptr && ws_bytes >= w.total, ACF_E_INVALID,
            "workspace of %zu bytes, acf_neumf_rank_all_workspace asks for %zu", ws_bytes, w.total);
  ACF_CHECK(rank_smem(c->d) <= 150 * 1024, ACF_E_INVALID, "dim %d is not served by the ranking kernel", c->d);
  hipStream_t s = static_cast<hipStream_t>(stream_);
  ACF_RET(settle_unchecked(c, s));
  if (n_users == 0) return ACF_OK;
  HIP_TRY(hipMemsetAsync(c->err, 0, sizeof(int32_t), s));
  char* base = static_cast<char*>(ws);
  float* tscore = reinterpret_cast<float*>(base + w.tscore);
  if (positions) {  // the test items' scores: predict's own kernel
    NArgs pa = make_args(c, P, nullptr, users, test_items, nullptr, n_users, 1.0f);
    pa.pred = tscore;
    launch_inst<2>(pa, (unsigned)std::min<int64_t>(((int64_t)n_users + MR - 1) / MR, 512), s);
    HIP_TRY(hipGetLastError());
  }
  RankArgs a;
  a.P = P;
  for (int q = 0; q < S_COUNT; ++q) a.off[q] = c->L.off[q];
  a.U1 = c->U1; a.d = c->d;
  a.users = users; a.n_users = n_users; a.nc = nc;
  a.excl_off = excl_off; a.excl = excl_items;
  a.tscore = positions ? tscore : nullptr;
  a.K = k;
  rank_strips(n_users, nc, &a.S, &a.strip_len);
  a.keys = reinterpret_cast<uint64_t*>(base + w.keys);
  a.cnt = reinterpret_cast<int32_t*>(base + w.cnt);
  a.err = c->err;
  const unsigned grid = (unsigned)std::min<int64_t>((int64_t)n_users * a.S, RK_TARGET_WG);
  const size_t sm = (size_t)rank_smem(c->d);
  if (c->d == DFAST) k_nmf_rank<DFAST><<<grid, 256, sm, s>>>(a);
  else k_nmf_rank<0><<<grid, 256, sm, s>>>(a);
  HIP_TRY(hipGetLastError());
  if (k > 0) {
    k_topk_merge<<<(unsigned)n_users, 256, 0, s>>>(a.keys, a.S, k, out_items, out_scores);
    HIP_TRY(hipGetLastError());
  }
  if (positions) {
    k_nmf_rank_pos<<<(unsigned)((n_users + 255) / 256), 256, 0, s>>>(a.cnt, a.S, n_users, positions);
    HIP_TRY(hipGetLastError());
  }
  return read_err(c, s);
}
