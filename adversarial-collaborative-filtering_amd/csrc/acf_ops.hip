// acf_ops.hip — the APR step decomposed into the TF ops it replaces, one kernel
// each, for callers that compose the step themselves (PyTorch custom ops
// acf::gather_bpr_fwd_bwd / row_segment_sum / l2norm_perturb /
// sparse_adagrad_apply, adversarial-collaborative-filtering_amd/csrc/acf_torch.cpp)
// and for op-level tests.  The fused streamed step (acf_apr.hip) is the
// training path; these are the same arithmetic with TF's data flow:
//
//   gather_bpr_fwd_bwd   the inference gathers + BPR loss + the gradient of the
//                        gathered rows as IndexedSlices values      APR.py:121-150
//   row_segment_sum      IndexedSlices -> unique rows, duplicates summed in
//                        index order (unsorted_segment_sum)          APR.py:183-187,195
//   l2norm_perturb       delta = eps * l2_normalize(g, 1)            APR.py:186-191
//   sparse_adagrad_apply acc += g^2; w -= lr * g * rsqrt(acc)        APR.py:193-195
//
// One lane-group of LPR lanes per row (float4 per lane), as in the step kernels.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>

#include "acf_apr.h"
#include "acf_host.h"  // HIP_TRY, ACF_CHECK, ACF_RET, grid_for, geometry, check_dim
#include "acf_rows.h"

static inline unsigned ops_grid(int64_t items, int lpr) {
  return (unsigned)((items * lpr + 255) / 256);
}

// lane-group geometry: item index and lane inside the group
template <int LPR>
__device__ __forceinline__ int64_t ops_item(int& l) {
  const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  l = (int)(threadIdx.x & (LPR - 1));
  return gid / LPR;
}

template <int LPR, int NV>
__global__ void __launch_bounds__(256) k_gather_bpr(const float* __restrict__ P, const float* __restrict__ Q,
                                                    int d, const int32_t* __restrict__ u,
                                                    const int32_t* __restrict__ ip, const int32_t* __restrict__ in,
                                                    int64_t n, float lo, float hi, float* __restrict__ loss,
                                                    float* __restrict__ xout, int32_t* __restrict__ p_idx,
                                                    float* __restrict__ p_val, int32_t* __restrict__ q_idx,
                                                    float* __restrict__ q_val) {
  int l;
  const int64_t b = ops_item<LPR>(l);
  if (b >= n) return;
  const RowV<NV> p = load_row<LPR, NV>(P, u[b], d, l);
  const RowV<NV> qi = load_row<LPR, NV>(Q, ip[b], d, l);
  const RowV<NV> qj = load_row<LPR, NV>(Q, in[b], d, l);
  const float x = dot_row<LPR, NV>(p, qi) - dot_row<LPR, NV>(p, qj);
  float g, ls;
  bpr_term(x, lo, hi, g, ls);
  if (l == 0) {
    loss[b] = ls;
    xout[b] = x;
    p_idx[b] = u[b]; p_idx[n + b] = u[b];    // pos-branch lookup, then neg-branch lookup
    q_idx[b] = ip[b]; q_idx[n + b] = in[b];
  }
  // IndexedSlices values: d(loss)/d(gathered row) = upstream * partner (rounded products)
  store_row<LPR, NV>(p_val, b, d, l, scale_row(qi, g));
  store_row<LPR, NV>(p_val, n + b, d, l, scale_row(qj, -g));
  store_row<LPR, NV>(q_val, b, d, l, scale_row(p, g));
  store_row<LPR, NV>(q_val, n + b, d, l, scale_row(p, -g));
}

__global__ void k_iota(int64_t m, int32_t* __restrict__ out) {
  const int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (x < m) out[x] = (int32_t)x;
}

// sorted (index, position) pairs -> head flags
__global__ void k_seg_heads(const uint32_t* __restrict__ key, int64_t m, int32_t* __restrict__ flag) {
  const int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (x < m) flag[x] = (x == 0 || key[x] != key[x - 1]) ? 1 : 0;
}

// after an inclusive scan of the heads: unique index and segment start
__global__ void k_seg_compact(const uint32_t* __restrict__ key, const int32_t* __restrict__ inc, int64_t m,
                              int32_t* __restrict__ uniq, int32_t* __restrict__ start, int64_t* __restrict__ k_out) {
  const int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (x >= m) return;
  const int32_t s = inc[x] - 1;
  if (x == 0 || key[x] != key[x - 1]) {
    uniq[s] = (int32_t)key[x];
    start[s] = (int32_t)x;
  }
  if (x == m - 1) *k_out = s + 1;
}

// segment sums in input order (a sequential sum per unique row: TF's
// unsorted_segment_sum order); count from the segment bounds
template <int LPR, int NV>
__global__ void __launch_bounds__(256) k_seg_sum(const float* __restrict__ vals, int d,
                                                 const int32_t* __restrict__ pos, const int32_t* __restrict__ start,
                                                 int32_t* __restrict__ count, const int64_t* __restrict__ k_ptr,
                                                 int64_t m, float* __restrict__ out) {
  int l;
  const int64_t s = ops_item<LPR>(l);
  const int64_t k = *k_ptr;
  if (s >= k) return;
  const int32_t a = start[s], e = s + 1 < k ? start[s + 1] : (int32_t)m;
  RowV<NV> acc = zero_row<NV>();
  for (int32_t x = a; x < e; ++x) acc = add_row(acc, load_row<LPR, NV>(vals, pos[x], d, l));
  store_row<LPR, NV>(out, s, d, l, acc);
  if (l == 0) count[s] = e - a;
}

template <int LPR, int NV>
__global__ void __launch_bounds__(256) k_l2norm_perturb(const float* __restrict__ g, int64_t k, int d, float eps,
                                                        float* __restrict__ out) {
  int l;
  const int64_t r = ops_item<LPR>(l);
  if (r >= k) return;
  store_row<LPR, NV>(out, r, d, l, l2_delta<LPR, NV>(load_row<LPR, NV>(g, r, d, l), eps));
}

template <int LPR, int NV>
__global__ void __launch_bounds__(256) k_sparse_adagrad(float* __restrict__ W, float* __restrict__ acc,
                                                        const int32_t* __restrict__ idx, const float* __restrict__ g,
                                                        int64_t k, int d, float lr) {
  int l;
  const int64_t r = ops_item<LPR>(l);
  if (r >= k) return;
  const int64_t row = idx[r];
  RowV<NV> w = load_row<LPR, NV>(W, row, d, l), c = load_row<LPR, NV>(acc, row, d, l);
  adagrad_apply(w, c, load_row<LPR, NV>(g, r, d, l), lr);
  store_row<LPR, NV>(acc, row, d, l, c);
  store_row<LPR, NV>(W, row, d, l, w);
}

// lanes per row and float4 per lane for dim d (as the step kernels)
#define OPS_GEOM(d, BODY)                                                             \
  do {                                                                                \
    int lpr_, nv_;                                                                    \
    geometry((d), &lpr_, &nv_);                                                       \
    switch (lpr_ * 100 + nv_) {                                                       \
      case 101: { constexpr int LPR = 1, NV = 1; BODY; } break;                       \
      case 201: { constexpr int LPR = 2, NV = 1; BODY; } break;                       \
      case 401: { constexpr int LPR = 4, NV = 1; BODY; } break;                       \
      case 801: { constexpr int LPR = 8, NV = 1; BODY; } break;                       \
      case 1601: { constexpr int LPR = 16, NV = 1; BODY; } break;                     \
      case 3201: { constexpr int LPR = 32, NV = 1; BODY; } break;                     \
      case 6401: { constexpr int LPR = 64, NV = 1; BODY; } break;                     \
      case 6402: { constexpr int LPR = 64, NV = 2; BODY; } break;                     \
      case 6403: { constexpr int LPR = 64, NV = 3; BODY; } break;                     \
      case 6404: { constexpr int LPR = 64, NV = 4; BODY; } break;                     \
      default: return acf_set_error(ACF_E_INVALID, "unsupported dim %d", (int)(d));   \
    }                                                                                 \
  } while (0)

extern "C" int acf_gather_bpr_fwd_bwd(const float* P, const float* Q, int64_t U1, int64_t I1, int32_t d,
                                      const int32_t* u, const int32_t* ip, const int32_t* in, int64_t n,
                                      float clip_lo, float clip_hi, float* loss, float* x, int32_t* p_idx,
                                      float* p_val, int32_t* q_idx, float* q_val, void* stream) {
  ACF_RET(check_dim(d));
  if (!P || !Q || !u || !ip || !in || !loss || !x || !p_idx || !p_val || !q_idx || !q_val || n < 0 || U1 <= 0 ||
      I1 <= 0)
    return acf_set_error(ACF_E_INVALID, "gather_bpr_fwd_bwd: NULL argument or bad size");
  if (n == 0) return ACF_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  OPS_GEOM(d, (k_gather_bpr<LPR, NV><<<ops_grid(n, LPR), 256, 0, s>>>(P, Q, d, u, ip, in, n, clip_lo, clip_hi,
                                                                         loss, x, p_idx, p_val, q_idx, q_val)));
  HIP_TRY(hipGetLastError());
  return ACF_OK;
}

// workspace: sorted keys, positions in / out, head flags, their scan, rocPRIM temp
static size_t seg_temp_bytes(int64_t m) {
  size_t a = 0, b = 0;
  (void)rocprim::radix_sort_pairs(nullptr, a, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int32_t*)nullptr,
                                  (int32_t*)nullptr, (size_t)m, 0, 32);
  (void)rocprim::inclusive_scan(nullptr, b, (int32_t*)nullptr, (int32_t*)nullptr, (size_t)m,
                                rocprim::plus<int32_t>());
  return std::max(a, b);
}

static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

extern "C" int acf_row_segment_sum_workspace(int64_t m, size_t* bytes) {
  if (!bytes || m < 0) return acf_set_error(ACF_E_INVALID, "row_segment_sum_workspace: bad argument");
  *bytes = 5 * align256((size_t)m * 4 + 4) + align256(seg_temp_bytes(m));
  return ACF_OK;
}

extern "C" int acf_row_segment_sum(const int32_t* idx, const float* vals, int64_t m, int32_t d,
                                   int64_t num_rows, void* workspace, size_t ws_bytes, int32_t* out_uniq,
                                   float* out_sum, int32_t* out_count, int64_t* out_k, void* stream) {
  ACF_RET(check_dim(d));
  size_t need = 0;
  acf_row_segment_sum_workspace(m, &need);
  if (!idx || !vals || !out_uniq || !out_sum || !out_count || !out_k || (m > 0 && (!workspace || ws_bytes < need)))
    return acf_set_error(ACF_E_INVALID, "row_segment_sum: NULL argument or workspace < %zu bytes", need);
  if (num_rows <= 0 || num_rows > (1ll << 31))
    return acf_set_error(ACF_E_INVALID, "row_segment_sum: num_rows outside (0, 2^31]");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (m == 0) {
    HIP_TRY(hipMemsetAsync(out_k, 0, sizeof(int64_t), s));
    return ACF_OK;
  }
  char* w = static_cast<char*>(workspace);
  const size_t a = align256((size_t)m * 4 + 4);
  uint32_t* kout = reinterpret_cast<uint32_t*>(w);
  int32_t* pin = reinterpret_cast<int32_t*>(w + a);
  int32_t* pout = reinterpret_cast<int32_t*>(w + 2 * a);
  int32_t* flag = reinterpret_cast<int32_t*>(w + 3 * a);
  int32_t* inc = reinterpret_cast<int32_t*>(w + 4 * a);
  void* tmp = w + 5 * a;
  size_t tb = ws_bytes - 5 * a;
  int32_t* start = pin;  // free once sorted
  const unsigned g = (unsigned)((m + 255) / 256);
  k_iota<<<g, 256, 0, s>>>(m, pin);
  int bits = 1;
  while (bits < 32 && (1ll << bits) < num_rows) ++bits;
  // indices in [0, num_rows) sort as unsigned on their low `bits`; stable: the
  // positions of one index stay in input order
  HIP_TRY(rocprim::radix_sort_pairs(tmp, tb, reinterpret_cast<const uint32_t*>(idx), kout, pin, pout, (size_t)m,
                                    0, bits, s));
  k_seg_heads<<<g, 256, 0, s>>>(kout, m, flag);
  tb = ws_bytes - 5 * a;
  HIP_TRY(rocprim::inclusive_scan(tmp, tb, flag, inc, (size_t)m, rocprim::plus<int32_t>(), s));
  k_seg_compact<<<g, 256, 0, s>>>(kout, inc, m, out_uniq, start, out_k);
  OPS_GEOM(d, (k_seg_sum<LPR, NV><<<ops_grid(m, LPR), 256, 0, s>>>(vals, d, pout, start, out_count, out_k, m,
                                                                      out_sum)));
  HIP_TRY(hipGetLastError());
  return ACF_OK;
}

extern "C" int acf_l2norm_perturb(const float* g, int64_t k, int32_t d, float eps, float* out, void* stream) {
  ACF_RET(check_dim(d));
  if (!g || !out || k < 0) return acf_set_error(ACF_E_INVALID, "l2norm_perturb: bad argument");
  if (k == 0) return ACF_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  OPS_GEOM(d, (k_l2norm_perturb<LPR, NV><<<ops_grid(k, LPR), 256, 0, s>>>(g, k, d, eps, out)));
  HIP_TRY(hipGetLastError());
  return ACF_OK;
}

extern "C" int acf_sparse_adagrad_apply(float* W, float* acc, int64_t rows, int32_t d, const int32_t* idx,
                                        const float* g, int64_t k, float lr, void* stream) {
  ACF_RET(check_dim(d));
  if (!W || !acc || !idx || !g || k < 0 || rows <= 0)
    return acf_set_error(ACF_E_INVALID, "sparse_adagrad_apply: bad argument");
  if (k == 0) return ACF_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  OPS_GEOM(d, (k_sparse_adagrad<LPR, NV><<<ops_grid(k, LPR), 256, 0, s>>>(W, acc, idx, g, k, d, lr)));
  HIP_TRY(hipGetLastError());
  return ACF_OK;
}

#include "acf_fold.h"
#include "acf_fold_items.h"
