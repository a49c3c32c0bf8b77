// acf_rank.hip — the ranking family of libacf_apr.so: read-only kernels over the trained
// tables (the headers included below) and their C-ABI entry points; nothing here touches a
// training context (acf_apr.hip).  Every entry point follows one frame: argument checks,
// workspace size and alignment, zero the error word, launch, sum the strips, read the error
// word back when `check` is set; its repeated pieces are the first section's functions.
// Build: one hipcc line with acf_apr.hip, acf_plan.hip and acf_ops.hip, same flags.

#include <hip/hip_runtime.h>
#include <rocprim/block/block_radix_sort.hpp>
#include <rocprim/block/block_scan.hpp>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "acf_apr.h"
#include "acf_host.h"
#include "acf_rows.h"

#include "acf_sweep.h"  // seq_dot and the score sweep the ranking kernels share: DESIGN.md §4
#include "acf_eval.h"  // all-items evaluation (k_eval_*): DESIGN.md §4
#include "acf_topk.h"  // top-K recommendation lists (k_topk_*): DESIGN.md §4b
#include "acf_neighbors.h"  // nearest-neighbour lists (k_nbr_*): DESIGN.md §4h
#include "acf_adv.h"   // whole-stream adversarial direction (k_adv_*): DESIGN.md §4c
#include "acf_eval_multi.h"  // multi-item evaluation and rank metrics (k_evx_*): DESIGN.md §4f
#include "acf_lists.h"  // list-level robustness: list overlap and item exposure (k_lst_*): DESIGN.md §4l
#include "acf_diverse.h"  // intra-list similarity and MMR re-ranking (k_div_*): DESIGN.md §4n
#include "acf_eval_worst.h"  // the certified margin sweep (k_cert_sweep), worst-case positions: DESIGN.md §4g
#include "acf_eval_radius.h"  // certified radius, the K weakest candidates (its selecting sink): DESIGN.md §4j

// ---- the host frame's shared pieces --------------------------------------------
static int check_kernel(int32_t kernel) {
  ACF_CHECK(kernel >= 0 && kernel <= 2, ACF_E_INVALID, "kernel must be 0 (auto), 1 (MFMA) or 2 (VALU), got %d",
            kernel);
  return ACF_OK;
}

static int check_excl_pair(const int64_t* excl_off, const int32_t* excl) {
  ACF_CHECK((excl_off == nullptr) == (excl == nullptr), ACF_E_INVALID, "excl_off and excl_items go together");
  return ACF_OK;
}

// The workspace precondition: aligned to `align` bytes, at least `need` bytes.  (NULL is
// refused with the entry point's other pointers, as before: callers see the order of checks.)
static int check_workspace(const void* workspace, size_t bytes, size_t need, int align) {
  ACF_CHECK(reinterpret_cast<uintptr_t>(workspace) % align == 0, ACF_E_INVALID, "workspace must be %d-byte aligned",
            align);
  ACF_CHECK(bytes >= need, ACF_E_INVALID, "workspace too small: %zu < %zu bytes", bytes, need);
  return ACF_OK;
}

// The kernels' error word on the host (one sync); the caller words what its bits mean.
static int read_error_word(const int32_t* err, hipStream_t s, int32_t* word) {
  int32_t herr = 0;
  HIP_TRY(hipMemcpyAsync(&herr, err, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *word = herr;
  return ACF_OK;
}

// ... for the evaluation sweeps: bit 0 a user, bit 1 a test item outside its table
static int check_eval_range(const int32_t* err, hipStream_t s) {
  int32_t herr = 0;
  ACF_RET(read_error_word(err, s, &herr));
  ACF_CHECK(herr == 0, ACF_E_RANGE, "index out of range (%s%s)", (herr & 1) ? "user >= num_user_rows " : "",
            (herr & 2) ? "test item >= num_item_rows" : "");
  return ACF_OK;
}

// S > 1 strips write their counts to `part`, summed into `out` afterwards; one strip writes `out`.
static int32_t* strip_target(int32_t* part, int S, int32_t* out) { return S > 1 ? part : out; }

static int sum_strips(const int32_t* part, int S, int64_t n_out, int32_t* out, hipStream_t s) {
  if (S > 1) {
    k_evx_sum<<<grid_for(n_out), 256, 0, s>>>(part, S, n_out, out);
    HIP_TRY(hipGetLastError());
  }
  return ACF_OK;
}

// Dynamic LDS of the VALU top-K sweeps (k_topk_valu, k_nbr_valu): 32 KB of keys + 8 rows, at d = 1024 above the
// 64 KB default: they opt in to the largest (per call: the attribute belongs to the current device's copy).
constexpr size_t tkv_lds(int d) { return (size_t)TKV_UB * (TKV_CAP * sizeof(uint64_t) + d * sizeof(float)); }
constexpr int TKV_LDS_MAX = (int)tkv_lds(1024);

// ---- all-items evaluation (acf_eval.h) ------------------------------------------
// kernel: 0 auto, 1 the fused MFMA sweep, 2 the VALU sweep k_eval_all (A/B and
// tests); positions are identical.  auto is the MFMA sweep.
static int eval_positions_all(const float* P, const float* Q, int64_t U1, int64_t I1, int32_t d,
                              const int32_t* users, const int32_t* tests, int32_t n_users, int32_t num_cand,
                              const int64_t* excl_off, const int32_t* excl, int32_t* positions, int32_t kernel,
                              void* stream_) {
  ACF_RET(check_dim(d));
  ACF_CHECK(P && Q && users && tests && excl_off && positions, ACF_E_INVALID, "NULL argument");
  ACF_CHECK(num_cand >= 0 && num_cand <= I1, ACF_E_INVALID, "num_candidates %d > item rows", num_cand);
  ACF_RET(check_kernel(kernel));
  if (n_users <= 0) return ACF_OK;
  hipStream_t s = static_cast<hipStream_t>(stream_);
  if (kernel == 2) {
    const size_t lds = (size_t)EVAL_UB * d * sizeof(float);
    k_eval_all<<<(n_users + EVAL_UB - 1) / EVAL_UB, 256, lds, s>>>(P, Q, d, users, tests, n_users, num_cand, excl_off,
                                                                    excl, positions);
    HIP_TRY(hipGetLastError());
    return ACF_OK;
  }
  float* tscore = nullptr;
  HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&tscore), (size_t)n_users * sizeof(float), s));
  k_eval_tscore<<<grid_for(n_users), 256, 0, s>>>(P, Q, d, users, tests, n_users, tscore, positions);
  if (num_cand > 0) {
    float eb, floor_e;
    mfma_err_band(d, &eb, &floor_e);
    const dim3 grid((unsigned)((num_cand + EVM_C - 1) / EVM_C), (unsigned)((n_users + EVM_U - 1) / EVM_U));
    k_eval_fused<<<grid, 256, 0, s>>>(P, Q, d, users, tscore, n_users, num_cand, excl_off, excl, eb, floor_e,
                                      positions);
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipFreeAsync(tscore, s));
  return ACF_OK;
}

extern "C" int acf_eval_positions_all(const float* P, const float* Q, int64_t U1, int64_t I1, int32_t d,
                                      const int32_t* users, const int32_t* tests, int32_t n_users, int32_t num_cand,
                                      const int64_t* excl_off, const int32_t* excl, int32_t* positions,
                                      void* stream_) {
  return eval_positions_all(P, Q, U1, I1, d, users, tests, n_users, num_cand, excl_off, excl, positions, 0, stream_);
}

extern "C" int acf_eval_positions_all_kernel(const float* P, const float* Q, int64_t U1, int64_t I1, int32_t d,
                                             const int32_t* users, const int32_t* tests, int32_t n_users,
                                             int32_t num_cand, const int64_t* excl_off, const int32_t* excl,
                                             int32_t* positions, int32_t kernel, void* stream_) {
  return eval_positions_all(P, Q, U1, I1, d, users, tests, n_users, num_cand, excl_off, excl, positions, kernel,
                            stream_);
}

extern "C" int acf_eval_positions_list(const float* P, const float* Q, int64_t U1, int64_t I1, int32_t d,
                                       const int32_t* users, const int32_t* tests, int32_t n_users,
                                       const int64_t* cand_off, const int32_t* cand, int32_t* positions,
                                       void* stream_) {
  ACF_RET(check_dim(d));
  ACF_CHECK(P && Q && users && tests && cand_off && positions, ACF_E_INVALID, "NULL argument");
  if (n_users <= 0) return ACF_OK;
  hipStream_t s = static_cast<hipStream_t>(stream_);
  k_eval_list<<<n_users, 256, d * sizeof(float), s>>>(P, Q, d, users, tests, cand_off, cand, positions);
  HIP_TRY(hipGetLastError());
  return ACF_OK;
}

// ---- top-K recommendation lists (acf_topk.h) --------------------------------------
// kernel: 0 auto, 1 the MFMA sweep k_topk_mfma, 2 the VALU sweep k_topk_valu;
// identical outputs.  Measured at K = 100, d = 64 the VALU sweep is
// 5-6x faster than the MFMA sweep at ml-1m (22M pairs) and pinterest-20 (547M pairs)
// alike, so no measured size crosses over: auto is the VALU sweep.
static int topk_kernel(int32_t kernel) { return kernel == 0 ? 2 : kernel; }

static int topk_check(int32_t n_users, int32_t num_cand, int32_t k, int32_t kernel) {
  ACF_CHECK(k >= 1 && k <= TOPK_MAX_K, ACF_E_INVALID, "k must be in [1, %d], got %d", TOPK_MAX_K, k);
  ACF_RET(check_kernel(kernel));
  ACF_CHECK(n_users >= 0 && num_cand >= 0, ACF_E_INVALID, "negative size");
  return ACF_OK;
}

extern "C" int acf_recommend_topk_workspace(int32_t n_users, int32_t num_cand, int32_t k, int32_t kernel,
                                            size_t* bytes) {
  ACF_CHECK(bytes, ACF_E_INVALID, "NULL argument");
  ACF_RET(topk_check(n_users, num_cand, k, kernel));
  int wper = 0, S = 0;
  topk_strips(n_users, num_cand, k, topk_kernel(kernel), &wper, &S);
  *bytes = (size_t)std::max(n_users, 1) * S * k * sizeof(uint64_t);
  return ACF_OK;
}

// the MFMA sweep's dynamic LDS (up to 96 KB of keys) is above the 64 KB default too (see tkv_lds)
static int topk_lds_optin(int kernel) {
  if (kernel == 1)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_topk_mfma),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(EVM_U * TKM_CAP_MAX * sizeof(uint64_t))));
  else
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_topk_valu),
                                hipFuncAttributeMaxDynamicSharedMemorySize, TKV_LDS_MAX));
  return ACF_OK;
}

extern "C" int acf_recommend_topk(const float* P, const float* Q, int64_t U1, int64_t I1, int32_t d,
                                  const int32_t* users, int32_t n_users, int32_t num_cand,
                                  const int64_t* excl_off, const int32_t* excl, int32_t k, int32_t* out_items,
                                  float* out_scores, void* workspace, size_t workspace_bytes, int32_t kernel,
                                  void* stream_) {
  ACF_RET(check_dim(d));
  ACF_RET(topk_check(n_users, num_cand, k, kernel));
  ACF_CHECK(P && Q && users && excl_off && excl && out_items && out_scores && workspace, ACF_E_INVALID,
            "NULL argument");
  ACF_CHECK(num_cand <= I1, ACF_E_INVALID, "num_candidates %d > item rows", num_cand);
  kernel = topk_kernel(kernel);
  int wper = 0, S = 0;
  topk_strips(n_users, num_cand, k, kernel, &wper, &S);
  ACF_RET(check_workspace(workspace, workspace_bytes, (size_t)std::max(n_users, 1) * S * k * sizeof(uint64_t), 8));
  if (n_users == 0) return ACF_OK;
  ACF_RET(topk_lds_optin(kernel));
  hipStream_t s = static_cast<hipStream_t>(stream_);
  uint64_t* ws = static_cast<uint64_t*>(workspace);
  if (kernel == 2) {
    const dim3 grid((unsigned)((n_users + TKV_UB - 1) / TKV_UB), (unsigned)S);
    k_topk_valu<<<grid, 256, tkv_lds(d), s>>>(P, Q, d, users, n_users, num_cand, excl_off, excl, k, wper, S, ws);
  } else {
    float eb, floor_e;
    mfma_err_band(d, &eb, &floor_e);
    const int cap = topk_mfma_cap(k);
    const dim3 grid((unsigned)((n_users + EVM_U - 1) / EVM_U), (unsigned)S);
    k_topk_mfma<<<grid, 256, (size_t)EVM_U * cap * sizeof(uint64_t), s>>>(P, Q, d, users, n_users, num_cand,
                                                                         excl_off, excl, eb, floor_e, k, cap, wper,
                                                                         S, ws);
  }
  HIP_TRY(hipGetLastError());
  k_topk_merge<<<(unsigned)n_users, 256, 0, s>>>(ws, S, k, out_items, out_scores);
  HIP_TRY(hipGetLastError());
  return ACF_OK;
}

// ---- nearest-neighbour lists (acf_neighbors.h) ---------------------------------
static int nbr_check(int32_t n_q, int32_t num_cand, int32_t k) {
  ACF_CHECK(k >= 1 && k <= TOPK_MAX_K, ACF_E_INVALID, "k must be in [1, %d], got %d", TOPK_MAX_K, k);
  ACF_CHECK(n_q >= 0 && num_cand >= 0, ACF_E_INVALID, "negative size");
  return ACF_OK;
}

extern "C" int acf_neighbors_topk_workspace(int32_t n_q, int32_t num_cand, int32_t k, size_t* bytes) {
  ACF_CHECK(bytes, ACF_E_INVALID, "NULL argument");
  ACF_RET(nbr_check(n_q, num_cand, k));
  *bytes = nbr_workspace(n_q, num_cand, k, true);
  return ACF_OK;
}

template <int METRIC>
static int launch_nbr(const float* T, const float* X, int d, int64_t XR, const int32_t* queries, int n_q,
                      int num_cand, int exclude_self, const int64_t* excl_off, const int32_t* excl,
                      const float* cnorm, int K, int wper, int S, uint64_t* lists, int32_t* err, hipStream_t s) {
  HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_nbr_valu<METRIC>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, TKV_LDS_MAX));
  const dim3 grid((unsigned)((n_q + TKV_UB - 1) / TKV_UB), (unsigned)S);
  k_nbr_valu<METRIC><<<grid, 256, tkv_lds(d), s>>>(T, X, d, XR, queries, n_q, num_cand, exclude_self, excl_off, excl,
                                                   cnorm, K, wper, S, lists, err);
  HIP_TRY(hipGetLastError());
  return ACF_OK;
}

extern "C" int acf_neighbors_topk(const float* T, int64_t TR, int32_t d, const float* X, int64_t XR,
                                  const int32_t* queries, int32_t n_q, int32_t num_cand, int32_t metric,
                                  int32_t exclude_self, const int64_t* excl_off, const int32_t* excl, int32_t k,
                                  int32_t* out_items, float* out_scores, void* workspace, size_t workspace_bytes,
                                  int32_t check, void* stream_) {
  ACF_RET(check_dim(d));
  ACF_RET(nbr_check(n_q, num_cand, k));
  ACF_CHECK(metric >= NBR_DOT && metric <= NBR_EUC, ACF_E_INVALID,
            "metric must be 0 (dot), 1 (cosine) or 2 (Euclidean), got %d", metric);
  ACF_CHECK(TR > 0 && XR > 0, ACF_E_INVALID, "empty table");
  ACF_CHECK(num_cand <= TR, ACF_E_INVALID, "num_candidates %d > table rows", num_cand);
  ACF_CHECK(T && X && queries && out_items && out_scores && workspace, ACF_E_INVALID, "NULL argument");
  ACF_RET(check_excl_pair(excl_off, excl));
  int wper = 0, S = 0;
  const size_t lists_bytes = nbr_lists_bytes(n_q, num_cand, k, &wper, &S);
  ACF_RET(check_workspace(workspace, workspace_bytes, nbr_workspace(n_q, num_cand, k, metric == NBR_COS), 8));
  if (n_q == 0) return ACF_OK;
  hipStream_t s = static_cast<hipStream_t>(stream_);
  int32_t* err = static_cast<int32_t*>(workspace);
  uint64_t* lists = reinterpret_cast<uint64_t*>(static_cast<char*>(workspace) + NBR_WS_HEAD);
  float* cnorm = reinterpret_cast<float*>(static_cast<char*>(workspace) + NBR_WS_HEAD + lists_bytes);
  HIP_TRY(hipMemsetAsync(err, 0, sizeof(int32_t), s));
  if (metric == NBR_COS && num_cand > 0) {
    k_nbr_norms<<<grid_for(num_cand), 256, 0, s>>>(T, d, num_cand, cnorm);
    HIP_TRY(hipGetLastError());
  }
  const auto launch = metric == NBR_DOT ? &launch_nbr<NBR_DOT> : metric == NBR_COS ? &launch_nbr<NBR_COS>
                                                                                   : &launch_nbr<NBR_EUC>;
  ACF_RET(launch(T, X, d, XR, queries, n_q, num_cand, exclude_self != 0, excl_off, excl, cnorm, k, wper, S, lists,
                 err, s));
  k_topk_merge<<<(unsigned)n_q, 256, 0, s>>>(lists, S, k, out_items, out_scores);
  HIP_TRY(hipGetLastError());
  if (check) {
    int32_t herr = 0;
    ACF_RET(read_error_word(err, s, &herr));
    ACF_CHECK(herr == 0, ACF_E_RANGE, "index out of range (query >= num_query_rows)");
  }
  return ACF_OK;
}

// ---- multi-item evaluation (acf_eval_multi.h) ---------------------------------
static int evx_check(int32_t n_users, int64_t n_tests, int32_t num_cand) {
  ACF_CHECK(n_users >= 0 && n_tests >= 0, ACF_E_INVALID, "negative count");
  ACF_CHECK(n_tests < ((int64_t)1 << 31), ACF_E_INVALID, "more than 2^31 - 1 test items");
  ACF_CHECK(num_cand >= 1, ACF_E_INVALID, "num_candidates must be >= 1, got %d", num_cand);
  return ACF_OK;
}

extern "C" int acf_eval_positions_multi_workspace(int32_t n_users, int64_t n_tests, int32_t num_cand,
                                                  size_t* bytes) {
  ACF_CHECK(bytes, ACF_E_INVALID, "NULL argument");
  ACF_RET(evx_check(n_users, n_tests, num_cand));
  *bytes = evx_workspace(n_users, n_tests, num_cand);
  return ACF_OK;
}

extern "C" int acf_eval_positions_multi(const float* P, const float* Q, int64_t U1, int64_t I1, int32_t d,
                                        const int32_t* users, const int64_t* test_off, const int32_t* test_items,
                                        int32_t n_users, int64_t n_tests, int32_t num_cand, const int64_t* excl_off,
                                        const int32_t* excl, int32_t* positions, void* workspace,
                                        size_t workspace_bytes, int32_t check, void* stream_) {
  ACF_RET(check_dim(d));
  ACF_RET(evx_check(n_users, n_tests, num_cand));
  ACF_CHECK(U1 > 0 && I1 > 0, ACF_E_INVALID, "empty table");
  ACF_CHECK(num_cand <= I1, ACF_E_INVALID, "num_candidates %d > item rows", num_cand);
  ACF_CHECK(P && Q && users && test_off && test_items && positions && workspace, ACF_E_INVALID, "NULL argument");
  ACF_RET(check_excl_pair(excl_off, excl));
  ACF_RET(check_workspace(workspace, workspace_bytes, evx_workspace(n_users, n_tests, num_cand), 4));
  if (n_users == 0 || n_tests == 0) return ACF_OK;
  int wper = 0, S = 0;
  evx_strips(n_users, n_tests, num_cand, &wper, &S);
  hipStream_t s = static_cast<hipStream_t>(stream_);
  int32_t* err = static_cast<int32_t*>(workspace);
  int32_t* part = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + EVX_WS_HEAD);
  HIP_TRY(hipMemsetAsync(err, 0, sizeof(int32_t), s));
  const dim3 grid((unsigned)((n_users + EVX_UB - 1) / EVX_UB), (unsigned)S);
  k_evx_sweep<<<grid, 256, (size_t)EVX_UB * d * sizeof(float), s>>>(P, Q, d, U1, I1, users, test_off, test_items,
                                                                     n_users, n_tests, num_cand, excl_off, excl, wper,
                                                                     strip_target(part, S, positions), err);
  HIP_TRY(hipGetLastError());
  ACF_RET(sum_strips(part, S, n_tests, positions, s));
  if (check) ACF_RET(check_eval_range(err, s));
  return ACF_OK;
}

extern "C" int acf_eval_rank_metrics(const int32_t* positions, const int64_t* test_off, int32_t n_users,
                                     const int32_t* n_neg, const int32_t* cutoffs, int32_t n_cutoffs,
                                     double* per_user, double* per_user_free, double* mean_cut, double* mean_free,
                                     int64_t* n_scored, void* stream_) {
  ACF_CHECK(n_users >= 0, ACF_E_INVALID, "negative count");
  ACF_CHECK(n_cutoffs >= 0 && n_cutoffs <= EVX_MAX_CUT, ACF_E_INVALID, "n_cutoffs %d outside [0, %d]", n_cutoffs,
            EVX_MAX_CUT);
  ACF_CHECK(cutoffs || n_cutoffs == 0, ACF_E_INVALID, "NULL argument");
  EvxCuts cuts{};
  cuts.n = n_cutoffs;
  for (int c = 0; c < n_cutoffs; ++c) {
    ACF_CHECK(cutoffs[c] >= 1 && cutoffs[c] <= EVX_MAX_K, ACF_E_INVALID, "cutoff %d outside [1, %d]", cutoffs[c],
              EVX_MAX_K);
    cuts.k[c] = cutoffs[c];
  }
  ACF_CHECK(test_off && mean_free && n_scored && (mean_cut || n_cutoffs == 0), ACF_E_INVALID, "NULL argument");
  ACF_CHECK(n_users == 0 || (positions && n_neg && per_user_free && (per_user || n_cutoffs == 0)), ACF_E_INVALID,
            "NULL argument");
  hipStream_t s = static_cast<hipStream_t>(stream_);
  if (n_users > 0) {
    k_evx_metrics<<<(unsigned)n_users, 256, 0, s>>>(positions, test_off, n_neg, cuts, per_user, per_user_free);
    HIP_TRY(hipGetLastError());
  }
  const int ncol = n_cutoffs * EVX_NM;
  k_evx_means<<<(unsigned)(ncol + 2), 256, 0, s>>>(per_user, per_user_free, test_off, n_users, ncol, mean_cut,
                                                   mean_free, n_scored);
  HIP_TRY(hipGetLastError());
  return ACF_OK;
}

// ---- list-level robustness: list overlap, item exposure (acf_lists.h) ------------
static int lst_cuts(int32_t k, const int32_t* cutoffs, int32_t n_cutoffs, LstCuts* cuts) {
  ACF_CHECK(k >= 1 && k <= LST_MAX_K, ACF_E_INVALID, "k must be in [1, %d], got %d", LST_MAX_K, k);
  ACF_CHECK(n_cutoffs >= 1 && n_cutoffs <= LST_MAX_CUT, ACF_E_INVALID, "n_cutoffs %d outside [1, %d]", n_cutoffs,
            LST_MAX_CUT);
  ACF_CHECK(cutoffs, ACF_E_INVALID, "NULL argument");
  *cuts = LstCuts{};
  cuts->n = n_cutoffs;
  for (int c = 0; c < n_cutoffs; ++c) {
    ACF_CHECK(cutoffs[c] >= 1 && cutoffs[c] <= k, ACF_E_INVALID, "cutoff %d outside [1, k = %d]", cutoffs[c], k);
    cuts->k[c] = cutoffs[c];
  }
  return ACF_OK;
}

extern "C" int acf_list_compare(const int32_t* A, const int32_t* B, int32_t n, int32_t k, const int32_t* cutoffs,
                                int32_t n_cutoffs, double p, double* per_user, double* mean, int64_t* n_scored,
                                void* stream_) {
  ACF_CHECK(n >= 0, ACF_E_INVALID, "negative count");
  LstCuts cuts;
  ACF_RET(lst_cuts(k, cutoffs, n_cutoffs, &cuts));
  ACF_CHECK(p > 0.0 && p < 1.0, ACF_E_INVALID, "p must lie in (0, 1), got %g", p);
  ACF_CHECK(mean && n_scored && (n == 0 || (A && B && per_user)), ACF_E_INVALID, "NULL argument");
  hipStream_t s = static_cast<hipStream_t>(stream_);
  uint8_t* scored = nullptr;  // which rows count: the means' only scratch
  HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&scored), (size_t)std::max(n, 1), s));
  if (n > 0) k_lst_compare<<<grid_for(n, LST_WAVES), 64 * LST_WAVES, 0, s>>>(A, B, n, k, cuts, p, per_user, scored);
  k_lst_means<<<(unsigned)(n_cutoffs * LST_NM), 256, 0, s>>>(per_user, scored, n, n_cutoffs * LST_NM, mean, n_scored);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipFreeAsync(scored, s));
  return ACF_OK;
}

extern "C" int acf_list_exposure(const int32_t* lists, int32_t n, int32_t k, int32_t num_items,
                                 const int32_t* cutoffs, int32_t n_cutoffs, int32_t* counts, void* stream_) {
  ACF_CHECK(n >= 0, ACF_E_INVALID, "negative count");
  ACF_CHECK(num_items >= 1, ACF_E_INVALID, "num_items must be >= 1, got %d", num_items);
  LstCuts cuts;
  ACF_RET(lst_cuts(k, cutoffs, n_cutoffs, &cuts));
  ACF_CHECK((int64_t)n * k < ((int64_t)1 << 31), ACF_E_INVALID, "n * k must stay below 2^31");
  ACF_CHECK(counts && (n == 0 || lists), ACF_E_INVALID, "NULL argument");
  hipStream_t s = static_cast<hipStream_t>(stream_);
  HIP_TRY(hipMemsetAsync(counts, 0, (size_t)n_cutoffs * num_items * sizeof(int32_t), s));
  if (n == 0) return ACF_OK;
  k_lst_exposure<<<grid_for(n, LSX_ROWS), 256, 0, s>>>(lists, n, k, num_items, cuts, counts);
  HIP_TRY(hipGetLastError());
  return ACF_OK;
}

static int lsm_check(int32_t num_items, int32_t n_cutoffs) {
  ACF_CHECK(num_items >= 1, ACF_E_INVALID, "num_items must be >= 1, got %d", num_items);
  ACF_CHECK(n_cutoffs >= 1 && n_cutoffs <= LST_MAX_CUT, ACF_E_INVALID, "n_cutoffs %d outside [1, %d]", n_cutoffs,
            LST_MAX_CUT);
  return ACF_OK;
}

extern "C" int acf_exposure_metrics_workspace(int32_t num_items, int32_t n_cutoffs, size_t* bytes) {
  ACF_CHECK(bytes, ACF_E_INVALID, "NULL argument");
  ACF_RET(lsm_check(num_items, n_cutoffs));
  *bytes = lsm_layout(num_items, n_cutoffs).total;
  return ACF_OK;
}

extern "C" int acf_exposure_metrics(const int32_t* counts, int32_t num_items, int32_t n_cutoffs, const int32_t* pop,
                                    const uint8_t* tail, double* out, void* workspace, size_t workspace_bytes,
                                    void* stream_) {
  ACF_RET(lsm_check(num_items, n_cutoffs));
  ACF_CHECK(counts && out && workspace, ACF_E_INVALID, "NULL argument");
  const int64_t N = num_items;
  const LsmLayout L = lsm_layout(N, n_cutoffs);
  ACF_RET(check_workspace(workspace, workspace_bytes, L.total, 8));
  hipStream_t s = static_cast<hipStream_t>(stream_);
  char* ws = static_cast<char*>(workspace);
  uint32_t* sorted = reinterpret_cast<uint32_t*>(ws + L.sorted);
  long long* part = reinterpret_cast<long long*>(ws + L.part);
  double* epart = reinterpret_cast<double*>(ws + L.epart);
  // counts are >= 0, so they sort as unsigned.  rocPRIM sizes its temporary storage by the device's
  // architecture, which a host-only workspace query cannot ask for: it comes from the stream's allocator.
  const uint32_t* keys = reinterpret_cast<const uint32_t*>(counts);
  size_t tb = 0;
  HIP_TRY(rocprim::radix_sort_keys(nullptr, tb, keys, sorted, (size_t)N, 0, 32, s));
  void* tmp = nullptr;
  HIP_TRY(hipMallocAsync(&tmp, std::max<size_t>(tb, 1), s));
  for (int c = 0; c < n_cutoffs; ++c)
    HIP_TRY(rocprim::radix_sort_keys(tmp, tb, keys + c * N, sorted + c * N, (size_t)N, 0, 32, s));
  HIP_TRY(hipFreeAsync(tmp, s));
  const int B = lsm_blocks(N);
  const dim3 grid((unsigned)B, (unsigned)n_cutoffs);
  k_lst_expo_ints<<<grid, 256, 0, s>>>(counts, sorted, N, pop, tail, part);
  k_lst_expo_entropy<<<grid, 256, 0, s>>>(counts, N, part, epart);
  k_lst_expo_final<<<(unsigned)n_cutoffs, 256, 0, s>>>(part, epart, B, N, out);
  HIP_TRY(hipGetLastError());
  return ACF_OK;
}

// ---- diversity: intra-list similarity, MMR re-ranking (acf_diverse.h) ----------------
static int div_check(int64_t TR, int32_t d, int32_t n, int32_t metric) {
  ACF_RET(check_dim(d));
  ACF_CHECK(n >= 0, ACF_E_INVALID, "negative count");
  ACF_CHECK(TR > 0, ACF_E_INVALID, "empty table");
  ACF_CHECK(metric >= NBR_DOT && metric <= NBR_EUC, ACF_E_INVALID,
            "metric must be 0 (dot), 1 (cosine) or 2 (Euclidean), got %d", metric);
  return ACF_OK;
}

// the instance of a kernel family KFN<METRIC, EPL, LDS> for a row of `len` positions
#define DIV_PICK(KFN, metric, len, lds)                                                           \
  ((metric) == NBR_DOT   ? DIV_PICK2(KFN, NBR_DOT, len, lds)                                      \
   : (metric) == NBR_COS ? DIV_PICK2(KFN, NBR_COS, len, lds)                                      \
                         : DIV_PICK2(KFN, NBR_EUC, len, lds))
#define DIV_PICK2(KFN, M, len, lds)                                                               \
  ((len) > 64 ? ((lds) ? &KFN<M, 2, true> : &KFN<M, 2, false>) : ((lds) ? &KFN<M, 1, true> : &KFN<M, 1, false>))

// the error word of a call, from the stream's allocator; with `check`, read back once after the launches
static int div_finish(int32_t* err, int32_t check, hipStream_t s) {
  int32_t herr = 0;
  if (check) ACF_RET(read_error_word(err, s, &herr));
  HIP_TRY(hipFreeAsync(err, s));
  ACF_CHECK(herr == 0, ACF_E_RANGE, "index out of range (id >= num_rows)");
  return ACF_OK;
}

extern "C" int acf_list_similarity(const float* T, int64_t TR, int32_t d, const int32_t* lists, int32_t n, int32_t k,
                                   const int32_t* cutoffs, int32_t n_cutoffs, int32_t metric, double* ils,
                                   double* means, int32_t check, void* stream_) {
  ACF_RET(div_check(TR, d, n, metric));
  LstCuts cuts;
  ACF_RET(lst_cuts(k, cutoffs, n_cutoffs, &cuts));
  ACF_CHECK(T && lists && ils && means, ACF_E_INVALID, "NULL argument");
  if (n == 0) return ACF_OK;
  int kmax = 0;
  for (int c = 0; c < n_cutoffs; ++c) kmax = std::max(kmax, cuts.k[c]);
  const size_t rows_bytes = div_rows_bytes(kmax, d);
  const bool lds = rows_bytes <= DIV_ROWS_LDS;
  hipStream_t s = static_cast<hipStream_t>(stream_);
  // [ error word, padded to 16 bytes | flag [n][n_cutoffs]: which rows count in which mean ]
  char* tmp = nullptr;
  HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&tmp), 16 + (size_t)n * n_cutoffs, s));
  int32_t* err = reinterpret_cast<int32_t*>(tmp);
  uint8_t* flag = reinterpret_cast<uint8_t*>(tmp + 16);
  HIP_TRY(hipMemsetAsync(err, 0, sizeof(int32_t), s));
  const auto kfn = DIV_PICK(k_div_ils, metric, kmax, lds);
  kfn<<<(unsigned)n, 64, lds ? rows_bytes : 0, s>>>(T, TR, d, lists, k, cuts, ils, flag, err);
  HIP_TRY(hipGetLastError());
  k_div_means<<<(unsigned)n_cutoffs, 256, 0, s>>>(ils, flag, n, n_cutoffs, means);
  HIP_TRY(hipGetLastError());
  return div_finish(err, check, s);
}

extern "C" int acf_rerank_mmr(const float* T, int64_t TR, int32_t d, const int32_t* cand, const float* rel, int32_t n,
                              int32_t m, int32_t k_out, float lam, int32_t metric, int32_t* items, float* rel_out,
                              float* obj, int32_t check, void* stream_) {
  ACF_RET(div_check(TR, d, n, metric));
  ACF_CHECK(m >= 1 && m <= DIV_MAX_M, ACF_E_INVALID, "m must be in [1, %d], got %d", DIV_MAX_M, m);
  ACF_CHECK(k_out >= 1 && k_out <= m, ACF_E_INVALID, "k_out must be in [1, m = %d], got %d", m, k_out);
  ACF_CHECK(lam >= 0.f && lam <= 1.f, ACF_E_INVALID, "lam must lie in [0, 1], got %g", (double)lam);
  ACF_CHECK(T && cand && rel && items && rel_out && obj, ACF_E_INVALID, "NULL argument");
  if (n == 0) return ACF_OK;
  const float oml = 1.0f - lam;
  const size_t rows_bytes = div_rows_bytes(m, d);
  const bool lds = rows_bytes <= DIV_ROWS_LDS;
  hipStream_t s = static_cast<hipStream_t>(stream_);
  int32_t* err = nullptr;
  HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&err), 16, s));
  HIP_TRY(hipMemsetAsync(err, 0, sizeof(int32_t), s));
  const auto kfn = DIV_PICK(k_div_mmr, metric, m, lds);
  kfn<<<(unsigned)n, 64, lds ? rows_bytes : 0, s>>>(T, TR, d, cand, rel, m, k_out, lam, oml, items, rel_out, obj, err);
  HIP_TRY(hipGetLastError());
  return div_finish(err, check, s);
}

// ---- the certified evaluations' host frame (k_cert_sweep: acf_eval_worst.h, acf_eval_radius.h) ----
static int cert_check(int32_t n_users, int32_t num_cand) {
  ACF_CHECK(n_users >= 0, ACF_E_INVALID, "negative count");
  ACF_CHECK(num_cand >= 1, ACF_E_INVALID, "num_candidates must be >= 1, got %d", num_cand);
  return ACF_OK;
}

// The entries of a call, as both entry points take them.
struct CertCall {
  const float *P, *Q;
  int64_t U1, I1;
  int32_t d;
  const int32_t *users, *tests;
  int32_t n_users, num_cand;
  const int64_t* excl_off;
  const int32_t* excl;
  int32_t side;
  void* workspace;
  size_t workspace_bytes;
  int32_t check;
  void* stream;
};

// Dynamic LDS: the sink's keys, then the rows.  A sink with keys passes the 64 KB default (side user at d = 512: 64 KB
// + the static part), so each of its instances opts in to its largest, as topk_lds_optin does; UB = 8 serves d <= 512,
// UB = 4 d <= 1024.
template <int UB, bool USER, template <int> class SINK>
static int launch_cert(const CertCall& c, int wper, int S, const typename SINK<UB>::Args& a, int32_t* err,
                       hipStream_t s) {
  constexpr size_t keys = SINK<UB>::KEYS * sizeof(uint64_t), row = (USER ? 2 : 1) * UB * sizeof(float);
  if (keys > 0)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_cert_sweep<UB, USER, SINK<UB>>),
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(keys + row * (UB == EVW_UB ? EVW_D_SPLIT : 1024))));
  const dim3 grid((unsigned)((c.n_users + UB - 1) / UB), (unsigned)S);
  k_cert_sweep<UB, USER, SINK<UB>><<<grid, 256, keys + row * c.d, s>>>(c.P, c.Q, c.d, c.U1, c.I1, c.users, c.tests,
                                                                       c.n_users, c.num_cand, c.excl_off, c.excl, wper,
                                                                       a, err);
  HIP_TRY(hipGetLastError());
  return ACF_OK;
}

// What both entry points do around their sweep.  The caller has checked the arguments of its own (cert_check among
// them: `need` is computed from them) and says whether its outputs are there; own(launch, err, s) cuts its strips,
// lays out its workspace behind the error word, calls launch(c, wper, S, its sink's arguments, err, s) and queues its
// tail.
template <template <int> class SINK, class OWN>
static int cert_run(const CertCall& c, bool outputs, size_t need, int align, OWN own) {
  ACF_RET(check_dim(c.d));
  ACF_CHECK(c.side == 0 || c.side == 1, ACF_E_INVALID, "side must be 0 (user) or 1 (item), got %d", c.side);
  ACF_CHECK(c.U1 > 0 && c.I1 > 0, ACF_E_INVALID, "empty table");
  ACF_CHECK(c.num_cand <= c.I1, ACF_E_INVALID, "num_candidates %d > item rows", c.num_cand);
  ACF_CHECK(c.P && c.Q && c.users && c.tests && outputs && c.workspace, ACF_E_INVALID, "NULL argument");
  ACF_RET(check_excl_pair(c.excl_off, c.excl));
  ACF_RET(check_workspace(c.workspace, c.workspace_bytes, need, align));
  if (c.n_users == 0) return ACF_OK;
  hipStream_t s = static_cast<hipStream_t>(c.stream);
  int32_t* err = static_cast<int32_t*>(c.workspace);
  HIP_TRY(hipMemsetAsync(err, 0, sizeof(int32_t), s));
  const bool wide = c.d <= EVW_D_SPLIT;  // 8 entries per workgroup, 4 above: the rows stay within 32 KB of LDS
  const auto launch = c.side == 0 ? (wide ? &launch_cert<EVW_UB, true, SINK> : &launch_cert<EVW_UB / 2, true, SINK>)
                                  : (wide ? &launch_cert<EVW_UB, false, SINK> : &launch_cert<EVW_UB / 2, false, SINK>);
  ACF_RET(own(launch, err, s));
  if (c.check) ACF_RET(check_eval_range(err, s));
  return ACF_OK;
}

// ---- certified worst-case positions: the counting sink (acf_eval_worst.h) ---------
static int evw_check(int32_t n_users, int32_t num_cand, int32_t n_eps) {
  ACF_RET(cert_check(n_users, num_cand));
  ACF_CHECK(n_eps >= 1 && n_eps <= EVW_MAX_EPS, ACF_E_INVALID, "n_eps %d outside [1, %d]", n_eps, EVW_MAX_EPS);
  return ACF_OK;
}

extern "C" int acf_eval_positions_worst_workspace(int32_t n_users, int32_t num_cand, int32_t n_eps, size_t* bytes) {
  ACF_CHECK(bytes, ACF_E_INVALID, "NULL argument");
  ACF_RET(evw_check(n_users, num_cand, n_eps));
  *bytes = evw_workspace(n_users, num_cand, n_eps);
  return ACF_OK;
}

extern "C" int acf_eval_positions_worst(const float* P, const float* Q, int64_t U1, int64_t I1, int32_t d,
                                        const int32_t* users, const int32_t* test_items, int32_t n_users,
                                        int32_t num_cand, const int64_t* excl_off, const int32_t* excl,
                                        const float* eps, int32_t n_eps, int32_t side, int32_t* worst,
                                        void* workspace, size_t workspace_bytes, int32_t check, void* stream_) {
  ACF_RET(evw_check(n_users, num_cand, n_eps));
  ACF_CHECK(eps, ACF_E_INVALID, "NULL argument");
  EvwEps ev{};
  ev.n = n_eps;
  for (int e = 0; e < EVW_MAX_EPS; ++e) {
    const float v = eps[std::min(e, n_eps - 1)];  // the unused slots repeat the last one
    ACF_CHECK(std::isfinite(v) && v >= 0.f, ACF_E_INVALID, "eps must be finite and >= 0, got %g", (double)v);
    ev.e[e] = v;
  }
  const CertCall c{P,        Q,    U1,   I1,        d,               users, test_items, n_users,
                   num_cand, excl_off, excl, side, workspace, workspace_bytes, check, stream_};
  return cert_run<CertCount>(c, worst != nullptr, evw_workspace(n_users, num_cand, n_eps), 4,
                             [&](auto launch, int32_t* err, hipStream_t s) -> int {
    int wper = 0, S = 0;
    evw_strips(n_users, num_cand, n_eps, &wper, &S);
    int32_t* part = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + EVW_WS_HEAD);
    ACF_RET(launch(c, wper, S, CertCountArgs{ev, strip_target(part, S, worst)}, err, s));
    return sum_strips(part, S, (int64_t)n_eps * n_users, worst, s);
  });
}

// ---- certified radius: the selecting sink (acf_eval_radius.h) ---------------------
static int evr_check(int32_t n_users, int32_t num_cand, int32_t k) {
  ACF_RET(cert_check(n_users, num_cand));
  ACF_CHECK(k >= 1 && k <= TOPK_MAX_K, ACF_E_INVALID, "k must be in [1, %d], got %d", TOPK_MAX_K, k);
  return ACF_OK;
}

extern "C" int acf_eval_radius_workspace(int32_t n_users, int32_t num_cand, int32_t k, size_t* bytes) {
  ACF_CHECK(bytes, ACF_E_INVALID, "NULL argument");
  ACF_RET(evr_check(n_users, num_cand, k));
  *bytes = evr_workspace(n_users, num_cand, k);
  return ACF_OK;
}

extern "C" int acf_eval_radius(const float* P, const float* Q, int64_t U1, int64_t I1, int32_t d,
                               const int32_t* users, const int32_t* test_items, int32_t n_users, int32_t num_cand,
                               const int64_t* excl_off, const int32_t* excl, int32_t k, int32_t side, float* eps_out,
                               int32_t* items_out, void* workspace, size_t workspace_bytes, int32_t check,
                               void* stream_) {
  ACF_RET(evr_check(n_users, num_cand, k));
  const CertCall c{P,        Q,    U1,   I1,        d,               users, test_items, n_users,
                   num_cand, excl_off, excl, side, workspace, workspace_bytes, check, stream_};
  return cert_run<CertSelect>(c, eps_out && items_out, evr_workspace(n_users, num_cand, k), 8,
                              [&](auto launch, int32_t* err, hipStream_t s) -> int {
    int wper = 0, S = 0;
    evr_strips(n_users, num_cand, k, &wper, &S);
    uint64_t* lists = reinterpret_cast<uint64_t*>(static_cast<char*>(workspace) + EVR_WS_HEAD);
    ACF_RET(launch(c, wper, S, CertSelectArgs{k, S, lists}, err, s));
    k_topk_merge<<<(unsigned)n_users, 256, 0, s>>>(lists, S, k, items_out, eps_out);  // scores: -eps
    HIP_TRY(hipGetLastError());
    k_evr_negate<<<grid_for((int64_t)n_users * k), 256, 0, s>>>(eps_out, (int64_t)n_users * k);
    HIP_TRY(hipGetLastError());
    return ACF_OK;
  });
}

// ---- whole-stream adversarial direction (acf_adv.h) -------------------------
static int adv_check(int64_t n, int64_t U1, int64_t I1, int32_t d) {
  ACF_RET(check_dim(d));
  ACF_CHECK(U1 > 0 && I1 > 0, ACF_E_INVALID, "empty table");
  ACF_CHECK(U1 + I1 < ((int64_t)1 << 31), ACF_E_INVALID, "more than 2^31 - 1 table rows");
  ACF_CHECK(n >= 0 && n < ((int64_t)1 << 29), ACF_E_INVALID, "n must lie in [0, 2^29), got %lld", (long long)n);
  return ACF_OK;
}

extern "C" int acf_adv_direction_workspace(int64_t n, int64_t U1, int64_t I1, int32_t d, size_t* bytes) {
  ACF_CHECK(bytes, ACF_E_INVALID, "NULL argument");
  ACF_RET(adv_check(n, U1, I1, d));
  *bytes = adv_layout(n, U1, I1, d).total;
  return ACF_OK;
}

template <int LPR, int NV>
static void launch_adv_random(uint64_t seed, uint32_t call, int32_t t, int d, int64_t U1, int64_t R, float* nP,
                              float* nQ, hipStream_t s) {
  k_adv_random<LPR, NV><<<grid_for(R * LPR), 256, 0, s>>>(seed, call, t, d, U1, R, nP, nQ);
}

template <int LPR, int NV>
static void launch_adv_sum(const float* P, const float* Q, int d, int64_t U1, int64_t R, const int32_t* off,
                           const int2* rec, float* part, float* nP, float* nQ, int64_t units, hipStream_t s) {
  k_adv_chunks<LPR, NV><<<grid_for(units * LPR), 256, 0, s>>>(P, Q, d, U1, R, off, rec, part, nP, nQ, units);
  k_adv_combine<LPR, NV><<<grid_for(R * LPR), 256, 0, s>>>(d, U1, R, off, part, nP, nQ);
}

// The plan's part (stages 1 keys, 2, k_adv_offsets) in a workspace laid out by adv_layout:
// zeroes *err, range-checks when `check` is set, leaves the offsets in `off` and the sorted
// term values in *sorted: `vals_dst` when given (the last pass writes there), else the
// workspace's pair *end, whose other pair is then free.  n > 0.
static int adv_plan_run(const int32_t* user, const int32_t* ipos, const int32_t* ineg, int64_t n, int64_t U1,
                        int64_t I1, const AdvLayout& L, char* ws, uint32_t* vals_dst, int32_t* off, int32_t* err,
                        int32_t check, hipStream_t s, const uint32_t** sorted, int* end) {
  uint32_t* kb[2] = {reinterpret_cast<uint32_t*>(ws + L.k0), reinterpret_cast<uint32_t*>(ws + L.k1)};
  uint32_t* vb[2] = {reinterpret_cast<uint32_t*>(ws + L.v0), reinterpret_cast<uint32_t*>(ws + L.v1)};
  uint32_t* counts = reinterpret_cast<uint32_t*>(ws + L.counts);
  uint32_t* tsum = reinterpret_cast<uint32_t*>(ws + L.tsum);
  HIP_TRY(hipMemsetAsync(err, 0, sizeof(int32_t), s));
  k_adv_keys<<<grid_for(n), 256, 0, s>>>(user, ipos, ineg, n, U1, I1, kb[0], vb[0], err);
  HIP_TRY(hipGetLastError());
  if (check) {  // before anything is built on the indices
    int32_t herr = 0;
    ACF_RET(read_error_word(err, s, &herr));
    ACF_CHECK(herr == 0, ACF_E_RANGE, "triplet index out of range (%s%s)",
              (herr & 1) ? "user >= num_user_rows " : "", (herr & 2) ? "item >= num_item_rows" : "");
  }
  int cur = 0;
  const uint32_t* out = vb[0];
  for (int p = 0; p < L.passes; ++p, cur ^= 1) {
    uint32_t* vout = (vals_dst && p == L.passes - 1) ? vals_dst : vb[cur ^ 1];
    k_adv_hist<<<(unsigned)L.ntiles, ADV_SORT_BS, 0, s>>>(kb[cur], L.N, 8 * p, L.ntiles, counts);
    k_adv_scan1<<<(unsigned)L.T, 256, 0, s>>>(counts, L.M, tsum);
    k_adv_scan2<<<1, 1024, 0, s>>>(tsum, L.T);
    k_adv_scan3<<<(unsigned)L.T, 256, 0, s>>>(counts, L.M, tsum);
    k_adv_reorder<<<(unsigned)L.ntiles, ADV_SORT_BS, 0, s>>>(kb[cur], vb[cur], kb[cur ^ 1], vout, L.N, 8 * p, L.ntiles,
                                                            counts);
    HIP_TRY(hipGetLastError());
    out = vout;
  }
  k_adv_offsets<<<grid_for(U1 + I1 + 1), 256, 0, s>>>(kb[cur], L.N, U1 + I1, off);
  HIP_TRY(hipGetLastError());
  *sorted = out;
  *end = cur;
  return ACF_OK;
}

// The tables' part: coefficients at (P, Q) (with lpart: the stream's loss to *loss), the
// records from the sorted values, chunk sums, combine.  coef [n], rec [4n], part as adv_layout.
static int adv_planned_run(const float* P, const float* Q, int64_t U1, int64_t I1, int32_t d, const int32_t* user,
                           const int32_t* ipos, const int32_t* ineg, int64_t n, float lo, float hi,
                           const uint32_t* vals, const int32_t* off, float* coef, int2* rec, float* part,
                           double* lpart, double* loss, float* nP, float* nQ, hipStream_t s) {
  const int64_t N = 4 * n, R = U1 + I1;
  k_adv_coef<<<grid_for(n), 256, 0, s>>>(P, Q, d, user, ipos, ineg, n, U1, I1, lo, hi, coef, lpart);
  if (lpart) k_adv_loss_sum<<<1, 256, 0, s>>>(lpart, (int64_t)grid_for(n), loss);
  HIP_TRY(hipGetLastError());
  if (!nP) return ACF_OK;  // the loss alone
  k_adv_records<<<grid_for(N), 256, 0, s>>>(vals, N, n, user, ipos, ineg, U1, I1, coef, rec);
  HIP_TRY(hipGetLastError());
  const int64_t units = N / ADV_CHUNK + R + 1;
  ACF_RET(DISPATCH_GEOM(d, launch_adv_sum, P, Q, d, U1, R, off, rec, part, nP, nQ, units, s));
  HIP_TRY(hipGetLastError());
  return ACF_OK;
}

extern "C" int acf_adv_direction(const float* P, const float* Q, int64_t U1, int64_t I1, int32_t d,
                                 const int32_t* user, const int32_t* ipos, const int32_t* ineg, int64_t n,
                                 float clip_lo, float clip_hi, int32_t adv_mode, uint64_t seed, uint32_t call,
                                 int32_t t, float* nP, float* nQ, void* workspace, size_t workspace_bytes,
                                 int32_t check, void* stream_) {
  ACF_RET(adv_check(n, U1, I1, d));
  ACF_CHECK(adv_mode == 0 || adv_mode == 1, ACF_E_INVALID, "adv_mode must be 0 (grad) or 1 (random), got %d",
            adv_mode);
  ACF_CHECK(P && Q && nP && nQ, ACF_E_INVALID, "NULL argument");
  hipStream_t s = static_cast<hipStream_t>(stream_);
  const int64_t R = U1 + I1;
  if (adv_mode == 1) {  // the triplets are not read
    ACF_RET(DISPATCH_GEOM(d, launch_adv_random, seed, call, t, d, U1, R, nP, nQ, s));
    HIP_TRY(hipGetLastError());
    return ACF_OK;
  }
  if (n == 0) {
    HIP_TRY(hipMemsetAsync(nP, 0, (size_t)U1 * d * sizeof(float), s));
    HIP_TRY(hipMemsetAsync(nQ, 0, (size_t)I1 * d * sizeof(float), s));
    return ACF_OK;
  }
  ACF_CHECK(user && ipos && ineg && workspace, ACF_E_INVALID, "NULL argument");
  const AdvLayout L = adv_layout(n, U1, I1, d);
  ACF_RET(check_workspace(workspace, workspace_bytes, L.total, 16));
  char* ws = static_cast<char*>(workspace);
  const uint32_t* vals = nullptr;
  int end = 0;
  int32_t* off = reinterpret_cast<int32_t*>(ws + L.off);
  ACF_RET(adv_plan_run(user, ipos, ineg, n, U1, I1, L, ws, nullptr, off, reinterpret_cast<int32_t*>(ws + L.err), check,
                       s, &vals, &end));
  int2* rec = reinterpret_cast<int2*>(ws + (end ? L.k0 : L.k1));  // the free (keys, values) pair: N * 8 bytes
  return adv_planned_run(P, Q, U1, I1, d, user, ipos, ineg, n, clip_lo, clip_hi, vals, off,
                         reinterpret_cast<float*>(ws + L.coef), rec, reinterpret_cast<float*>(ws + L.part), nullptr,
                         nullptr, nP, nQ, s);
}

// ---- a plan that outlives the call, the planned direction, the iterated attack: DESIGN.md §4k ----
extern "C" int acf_adv_plan_workspace(int64_t n, int64_t U1, int64_t I1, size_t* plan_bytes, size_t* bytes) {
  ACF_CHECK(plan_bytes && bytes, ACF_E_INVALID, "NULL argument");
  ACF_RET(adv_check(n, U1, I1, 4));
  *plan_bytes = adv_plan_layout(n, U1, I1).total;
  *bytes = n ? adv_layout(n, U1, I1, 4).part : 0;  // the sort's buffers: everything below the chunk sums
  return ACF_OK;
}

static int adv_plan_pointers(void* plan, size_t plan_bytes, int64_t n, int64_t U1, int64_t I1, uint32_t** vals,
                             int32_t** off, int32_t** err) {
  const AdvPlanLayout PL = adv_plan_layout(n, U1, I1);
  ACF_CHECK(plan, ACF_E_INVALID, "NULL argument");
  ACF_CHECK(reinterpret_cast<uintptr_t>(plan) % 16 == 0, ACF_E_INVALID, "plan must be 16-byte aligned");
  ACF_CHECK(plan_bytes >= PL.total, ACF_E_INVALID, "plan too small: %zu < %zu bytes", plan_bytes, PL.total);
  char* pb = static_cast<char*>(plan);
  *vals = reinterpret_cast<uint32_t*>(pb + PL.vals);
  *off = reinterpret_cast<int32_t*>(pb + PL.off);
  *err = reinterpret_cast<int32_t*>(pb + PL.err);
  return ACF_OK;
}

extern "C" int acf_adv_plan(const int32_t* user, const int32_t* ipos, const int32_t* ineg, int64_t n, int64_t U1,
                            int64_t I1, void* plan, size_t plan_bytes, void* workspace, size_t workspace_bytes,
                            int32_t check, void* stream_) {
  ACF_RET(adv_check(n, U1, I1, 4));
  uint32_t* vals;
  int32_t *off, *err;
  ACF_RET(adv_plan_pointers(plan, plan_bytes, n, U1, I1, &vals, &off, &err));
  hipStream_t s = static_cast<hipStream_t>(stream_);
  if (n == 0) {  // no terms: every row starts and ends at 0
    HIP_TRY(hipMemsetAsync(off, 0, (size_t)(U1 + I1 + 1) * sizeof(int32_t), s));
    HIP_TRY(hipMemsetAsync(err, 0, sizeof(int32_t), s));
    return ACF_OK;
  }
  ACF_CHECK(user && ipos && ineg && workspace, ACF_E_INVALID, "NULL argument");
  const AdvLayout L = adv_layout(n, U1, I1, 4);
  ACF_RET(check_workspace(workspace, workspace_bytes, L.part, 16));
  const uint32_t* sorted = nullptr;
  int end = 0;
  return adv_plan_run(user, ipos, ineg, n, U1, I1, L, static_cast<char*>(workspace), vals, off, err, check, s, &sorted,
                      &end);
}

// The planned direction in a workspace of acf_adv_direction_workspace(n, ...) bytes: the
// coefficients, the records where the sort's first pair lay, the loss partials in its second.
static int adv_planned_in(const float* P, const float* Q, int64_t U1, int64_t I1, int32_t d, const int32_t* user,
                          const int32_t* ipos, const int32_t* ineg, int64_t n, float lo, float hi, const uint32_t* vals,
                          const int32_t* off, char* ws, double* loss, float* nP, float* nQ, hipStream_t s) {
  const AdvLayout L = adv_layout(n, U1, I1, d);
  return adv_planned_run(P, Q, U1, I1, d, user, ipos, ineg, n, lo, hi, vals, off,
                         reinterpret_cast<float*>(ws + L.coef), reinterpret_cast<int2*>(ws + L.k0),
                         reinterpret_cast<float*>(ws + L.part), loss ? reinterpret_cast<double*>(ws + L.k1) : nullptr,
                         loss, nP, nQ, s);
}

extern "C" int acf_adv_direction_planned(const float* P, const float* Q, int64_t U1, int64_t I1, int32_t d,
                                         const int32_t* user, const int32_t* ipos, const int32_t* ineg, int64_t n,
                                         float clip_lo, float clip_hi, const void* plan, size_t plan_bytes, float* nP,
                                         float* nQ, double* loss_out, void* workspace, size_t workspace_bytes,
                                         void* stream_) {
  ACF_RET(adv_check(n, U1, I1, d));
  ACF_CHECK(P && Q && nP && nQ, ACF_E_INVALID, "NULL argument");
  uint32_t* vals;
  int32_t *off, *err;
  ACF_RET(adv_plan_pointers(const_cast<void*>(plan), plan_bytes, n, U1, I1, &vals, &off, &err));
  hipStream_t s = static_cast<hipStream_t>(stream_);
  if (n == 0) {
    HIP_TRY(hipMemsetAsync(nP, 0, (size_t)U1 * d * sizeof(float), s));
    HIP_TRY(hipMemsetAsync(nQ, 0, (size_t)I1 * d * sizeof(float), s));
    if (loss_out) HIP_TRY(hipMemsetAsync(loss_out, 0, sizeof(double), s));
    return ACF_OK;
  }
  ACF_CHECK(user && ipos && ineg && workspace, ACF_E_INVALID, "NULL argument");
  ACF_RET(check_workspace(workspace, workspace_bytes, adv_layout(n, U1, I1, d).total, 16));
  return adv_planned_in(P, Q, U1, I1, d, user, ipos, ineg, n, clip_lo, clip_hi, vals, off,
                        static_cast<char*>(workspace), loss_out, nP, nQ, s);
}

template <int LPR, int NV>
static void launch_adv_pgd_step(const float* W, const float* delta, const float* n, int64_t rows, int d, float alpha,
                                float eps, float* delta_out, float* sum_out, hipStream_t s) {
  k_adv_pgd_step<LPR, NV><<<grid_for(rows * LPR), 256, 0, s>>>(W, delta, n, rows, d, alpha, eps, delta_out, sum_out);
}

// acf_adv_pgd's workspace: the perturbed tables, the direction tables, a plan of its own, the
// planned direction's workspace.
struct PgdLayout {
  size_t sumP, sumQ, nP, nQ, plan, dir, total;
};

static PgdLayout pgd_layout(int64_t n, int64_t U1, int64_t I1, int32_t d) {
  PgdLayout L;
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t a = at;
    at += adv_up(bytes);
    return a;
  };
  const size_t tp = (size_t)U1 * d * sizeof(float), tq = (size_t)I1 * d * sizeof(float);
  L.sumP = take(tp);
  L.sumQ = take(tq);
  L.nP = take(tp);
  L.nQ = take(tq);
  L.plan = take(adv_plan_layout(n, U1, I1).total);
  L.dir = take(n ? adv_layout(n, U1, I1, d).total : 0);
  L.total = at;
  return L;
}

extern "C" int acf_adv_pgd_workspace(int64_t n, int64_t U1, int64_t I1, int32_t d, size_t* bytes) {
  ACF_CHECK(bytes, ACF_E_INVALID, "NULL argument");
  ACF_RET(adv_check(n, U1, I1, d));
  *bytes = pgd_layout(n, U1, I1, d).total;
  return ACF_OK;
}

extern "C" int acf_adv_pgd(const float* P, const float* Q, int64_t U1, int64_t I1, int32_t d, const int32_t* user,
                           const int32_t* ipos, const int32_t* ineg, int64_t n, float clip_lo, float clip_hi,
                           const void* plan, size_t plan_bytes, float eps, float alpha, int32_t iters, int32_t side,
                           const float* dP0, const float* dQ0, float* dP, float* dQ, double* loss, void* workspace,
                           size_t workspace_bytes, int32_t check, void* stream_) {
  ACF_RET(adv_check(n, U1, I1, d));
  ACF_CHECK(iters >= 1 && iters <= ACF_ADV_PGD_MAX_ITERS, ACF_E_INVALID, "iters must lie in [1, %d], got %d",
            ACF_ADV_PGD_MAX_ITERS, iters);
  ACF_CHECK(std::isfinite(eps) && eps >= 0.f, ACF_E_INVALID, "eps must be finite and >= 0");
  ACF_CHECK(std::isfinite(alpha) && alpha >= 0.f, ACF_E_INVALID, "alpha must be finite and >= 0");
  ACF_CHECK(side >= ACF_ADV_SIDE_BOTH && side <= ACF_ADV_SIDE_ITEM, ACF_E_INVALID,
            "side must be 0 (both), 1 (user) or 2 (item), got %d", side);
  ACF_CHECK(P && Q && dP && dQ && loss && workspace, ACF_E_INVALID, "NULL argument");
  ACF_CHECK(n == 0 || (user && ipos && ineg), ACF_E_INVALID, "NULL argument");
  const PgdLayout L = pgd_layout(n, U1, I1, d);
  ACF_RET(check_workspace(workspace, workspace_bytes, L.total, 16));
  char* ws = static_cast<char*>(workspace);
  uint32_t* vals;
  int32_t *off, *err;
  if (plan) ACF_RET(adv_plan_pointers(const_cast<void*>(plan), plan_bytes, n, U1, I1, &vals, &off, &err));
  else ACF_RET(adv_plan_pointers(ws + L.plan, adv_plan_layout(n, U1, I1).total, n, U1, I1, &vals, &off, &err));
  hipStream_t s = static_cast<hipStream_t>(stream_);
  float* sumP = reinterpret_cast<float*>(ws + L.sumP);
  float* sumQ = reinterpret_cast<float*>(ws + L.sumQ);
  float* nP = reinterpret_cast<float*>(ws + L.nP);
  float* nQ = reinterpret_cast<float*>(ws + L.nQ);
  char* dir = ws + L.dir;
  if (n > 0 && !plan) {  // plan once; the direction's workspace is free until the first iteration
    const uint32_t* sorted = nullptr;
    int end = 0;
    ACF_RET(adv_plan_run(user, ipos, ineg, n, U1, I1, adv_layout(n, U1, I1, d), dir, vals, off, err, check, s, &sorted,
                         &end));
  } else if (n > 0 && check) {  // the word the plan's own call left
    int32_t herr = 0;
    ACF_RET(read_error_word(err, s, &herr));
    ACF_CHECK(herr == 0, ACF_E_RANGE, "triplet index out of range (%s%s)",
              (herr & 1) ? "user >= num_user_rows " : "", (herr & 2) ? "item >= num_item_rows" : "");
  }
  // iterate 0: the start as given (not projected: a chained call continues bit for bit), W + start
  struct Side {
    const float* W;
    const float* d0;
    float *dl, *sum, *dirn;
    int64_t rows;
    bool moves;
  } sides[2] = {{P, dP0, dP, sumP, nP, U1, side != ACF_ADV_SIDE_ITEM}, {Q, dQ0, dQ, sumQ, nQ, I1, side != ACF_ADV_SIDE_USER}};
  for (const Side& t : sides) {
    const size_t bytes = (size_t)t.rows * d * sizeof(float);
    if (!t.d0) {
      HIP_TRY(hipMemsetAsync(t.dl, 0, bytes, s));
      HIP_TRY(hipMemcpyAsync(t.sum, t.W, bytes, hipMemcpyDeviceToDevice, s));
    } else {
      if (t.d0 != t.dl) HIP_TRY(hipMemcpyAsync(t.dl, t.d0, bytes, hipMemcpyDeviceToDevice, s));
      k_adv_apply<<<grid_for(t.rows * (int64_t)d), 256, 0, s>>>(t.W, t.d0, t.rows * (int64_t)d, 1.0f, nullptr, t.sum);
      HIP_TRY(hipGetLastError());
    }
  }
  if (n == 0) {  // no gradient: the projection of the start, once; no loss
    for (const Side& t : sides)
      if (t.moves) ACF_RET(DISPATCH_GEOM(d, launch_adv_pgd_step, t.W, t.dl, nullptr, t.rows, d, 0.f, eps, t.dl, t.sum, s));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(loss, 0, (size_t)(iters + 1) * sizeof(double), s));
    return ACF_OK;
  }
  for (int k = 0; k <= iters; ++k) {
    const bool last = k == iters;  // one more coefficient pass: the loss at the final iterate
    ACF_RET(adv_planned_in(sumP, sumQ, U1, I1, d, user, ipos, ineg, n, clip_lo, clip_hi, vals, off, dir, loss + k,
                           last ? nullptr : nP, last ? nullptr : nQ, s));
    if (last) break;
    for (const Side& t : sides)
      if (t.moves) ACF_RET(DISPATCH_GEOM(d, launch_adv_pgd_step, t.W, t.dl, t.dirn, t.rows, d, alpha, eps, t.dl, t.sum, s));
    HIP_TRY(hipGetLastError());
  }
  return ACF_OK;
}

extern "C" int acf_adv_apply(const float* W, const float* N, int64_t rows, int32_t d, float eps, float* delta_out,
                             float* sum_out, void* stream_) {
  ACF_CHECK(rows >= 0 && d > 0, ACF_E_INVALID, "negative size");
  ACF_CHECK(N && (W || !sum_out), ACF_E_INVALID, "NULL argument");
  const int64_t count = rows * (int64_t)d;
  if (count == 0 || (!delta_out && !sum_out)) return ACF_OK;
  k_adv_apply<<<grid_for(count), 256, 0, static_cast<hipStream_t>(stream_)>>>(W, N, count, eps, delta_out, sum_out);
  HIP_TRY(hipGetLastError());
  return ACF_OK;
}
