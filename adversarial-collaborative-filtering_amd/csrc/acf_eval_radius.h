// Certified radius: the smallest eps at which each candidate breaks the
// certificate, and per entry the K smallest of them (k_evr_*): included by
// acf_rank.hip after acf_eval_worst.h (its frame constants; acf_sweep.h's pieces)
// and acf_topk.h (acf_topk_select.h: the key, topk_prune, the partial lists and
// k_topk_merge); one translation unit.  DESIGN.md §4j.
#pragma once

// ---------------------------------------------------------------------------
// eval_radius: entries, candidates C_r, exclusions, the test item t and the fp32
// values m_c, D_c, Np are k_evw_sweep's (acf_eval_worst.h), bit for bit: the same
// statements under the same flags.  With
//   pred_c(e) = m_c <= e * D_c              (side user)
//   pred_c(e) = m_c <= (2 e) * Np           (side item)
// as k_evw_sweep evaluates them, eps_c = the smallest finite fp32 e >= 0 with
// pred_c(e), +inf when there is none (m_c > 0 with base 0; a NaN).  Both products
// are rounded once and do not decrease in e, so pred_c is monotone over [0,
// FLT_MAX] and the minimum exists; m_c <= 0 gives 0 (finite base).  Per entry
// the kernel keeps the K smallest (eps_c, c), ties to the lower id: eps[r][k - 1]
// is the budget below which worst < k and from which worst >= k, i.e. the
// certified radius at k, for every k <= K.
//
// evr_min_eps: e = m / base is within a few ulps of the minimum (division is
// correctly rounded; fl(fl(m / D) D) is off by about 2^-23 m), so up to
// EVR_STEPS single steps over neighbouring floats end at pred(e) && (e == 0 ||
// !pred(prev(e))).  Whatever is left (denormal products, an overflowing or
// underflowing quotient) is finished by bisection on the bit pattern over
// (0, FLT_MAX]: non-negative floats order like their bits, at most 31 steps.
//
// The sweep is k_evw_sweep's frame (rows in LDS, the 2,048-candidate exclusion
// bitmap with t's own bit set, 256 candidates a step, tiles of 8 entries up to d
// = 512 and 4 above, strips of 256-candidate windows) with k_topk_valu's
// selection: per entry TKV_CAP keys topk_key(-eps_c, c) (larger = smaller eps;
// -0.0 maps to the key of +0.0, -inf is an entry like any other), a count and the
// threshold thr = the exact K-th best key so far.  A candidate is admitted in
// two steps: pred_c at e = the threshold's eps (one multiply; true iff eps_c <=
// that eps, so a superset of the keys > thr; no threshold yet, or an infinite
// one: everything passes), and only the survivors compute eps_c and append iff
// their exact key > thr.  Every step appends at most 256 keys per entry and
// topk_prune runs after it, as in k_topk_valu.  The strips' partial lists go
// through k_topk_merge, whose scores are -eps; k_evr_negate turns them over.
// Integer LDS atomics only, nothing accumulated in floating point across
// threads, every loop bounded by its inputs: equal inputs give equal bits.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   k_evr_sweep<8, true>   133 VGPRs, 106 SGPRs, no scratch, 2,608 B of static LDS
//   k_evr_sweep<8, false>   91 VGPRs, 106 SGPRs, no scratch, 2,608 B
//   k_evr_sweep<4, true>    82 VGPRs, 100 SGPRs, no scratch, 1,440 B
//   k_evr_sweep<4, false>   67 VGPRs,  98 SGPRs, no scratch, 1,440 B
// Dynamic LDS (evr_lds): UB * TKV_CAP keys (32 KB at UB = 8, 16 KB at 4) + the
// rows (side user: 2 UB d floats, at most 32 KB; side item: half).  Side user at
// d = 512 takes 64 KB + the static part = 68,144 B, above the 64 KB default, so
// the launcher opts every instance in to its largest (launch_evr); two such
// workgroups still share a CU's 160 KB.
// ---------------------------------------------------------------------------
constexpr int EVR_STEPS = 4;  // single-float steps before the bisection

template <bool USER>
__device__ __forceinline__ bool evr_pred(float m, float e, float base) {
  return USER ? m <= e * base : m <= (2.f * e) * base;
}

// The smallest finite e >= 0 with evr_pred(m, e, base), +inf when there is none.
template <bool USER>
__device__ __forceinline__ float evr_min_eps(float m, float base) {
  constexpr float FMAX = 3.402823466e+38f;
  if (evr_pred<USER>(m, 0.f, base)) return 0.f;  // m <= 0 (finite base)
  if (!evr_pred<USER>(m, FMAX, base)) return INFINITY;  // m > 0 with base 0, or a NaN
  float e = USER ? m / base : (m / base) * 0.5f;
  if (!(e <= FMAX)) e = FMAX;  // an overflowing quotient
  if (!(e > 0.f)) e = __uint_as_float(1u);  // an underflowing one: the smallest denormal
  for (int it = 0; it < EVR_STEPS; ++it) {  // pred(0) is false: e stays > 0
    if (evr_pred<USER>(m, e, base)) {
      const float lo = __uint_as_float(__float_as_uint(e) - 1u);
      if (!evr_pred<USER>(m, lo, base)) return e;
      e = lo;
    } else {
      e = __uint_as_float(__float_as_uint(e) + 1u);  // e < FMAX: pred(FMAX) holds
    }
  }
  uint32_t lo = 0u, hi = __float_as_uint(FMAX);  // !pred(lo), pred(hi)
  while (hi - lo > 1u) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (evr_pred<USER>(m, __uint_as_float(mid), base)) hi = mid; else lo = mid;
  }
  return __uint_as_float(hi);
}

template <int UB, bool USER>
__global__ void __launch_bounds__(256) k_evr_sweep(const float* __restrict__ P, const float* __restrict__ Q, int d,
                                                   int64_t U1, int64_t I1, const int32_t* __restrict__ users,
                                                   const int32_t* __restrict__ test_items, int n_users, int num_cand,
                                                   const int64_t* __restrict__ excl_off,
                                                   const int32_t* __restrict__ excl, int K, int wper, int S,
                                                   uint64_t* __restrict__ ws, int32_t* __restrict__ err) {
  // [UB][TKV_CAP] keys, [UB][d] user rows, (USER) [UB][d] test-item rows
  extern __shared__ __attribute__((aligned(16))) uint64_t evr_smem[];
  uint64_t* const buf = evr_smem;
  float* const rows = reinterpret_cast<float*>(evr_smem + UB * TKV_CAP);
  float* const trows = rows + UB * d;
  __shared__ float s_test[UB];    // seq_dot(p, Q[t])
  __shared__ float s_np[UB];      // side item: Np
  __shared__ float s_thrf[UB];    // -(the threshold's eps); -inf: none yet, or an infinite one
  __shared__ int s_cnt[UB];
  __shared__ uint64_t s_thr[UB];
  __shared__ int32_t s_tid[UB];   // the test items, range-checked
  __shared__ uint32_t s_ex[UB][EVW_BM / 32];
  __shared__ int64_t s_eoff[UB + 1];
  const int tid = threadIdx.x, strip = blockIdx.y;
  const int u0 = blockIdx.x * UB;
  const int nu = min(UB, n_users - u0);
  const int64_t c_begin = (int64_t)strip * wper * EVW_WIN;
  const int64_t c_end = min((int64_t)num_cand, c_begin + (int64_t)wper * EVW_WIN);
  sweep_load_rows<UB, true>(rows, P, d, users, u0, nu, U1, err);  // reported when the caller checks
  if (tid < UB) {
    int64_t t = tid < nu ? test_items[u0 + tid] : 0;
    if (t < 0 || t >= I1) {
      t = 0;
      atomicOr(err, 2);
    }
    s_tid[tid] = (int32_t)t;
    s_cnt[tid] = 0;
    s_thr[tid] = 0;
    s_thrf[tid] = -INFINITY;
  }
  if (tid <= UB) s_eoff[tid] = excl_off ? excl_off[u0 + min(tid, nu)] : 0;  // past the tile: empty lists
  __syncthreads();
  if (USER) {
    sweep_load_rows<UB, false>(trows, Q, d, s_tid, 0, nu, 0, nullptr);
    __syncthreads();
  }
  if (tid < UB) {
    const float* p = rows + tid * d;
    s_test[tid] = seq_dot(p, Q + (int64_t)s_tid[tid] * d, d);
    float n2 = 0.f;
    if (!USER)
      for (int k = 0; k < d; ++k) n2 = n2 + p[k] * p[k];
    s_np[tid] = sqrtf(n2);
  }
  for (int64_t cc = c_begin; cc < c_end; cc += EVW_BM) {
    const int64_t ce = min(c_end, cc + EVW_BM);
    __syncthreads();  // the previous bitmap's reads (first pass: s_test, s_np)
    sweep_excl_strided<UB, EVW_BM>(s_ex, s_eoff, nu, excl, cc, ce - cc);  // no lists: s_eoff is all 0
    if (tid < nu) {  // the test item never counts
      const int64_t w = (int64_t)s_tid[tid] - cc;
      if (w >= 0 && w < ce - cc) atomicOr(&s_ex[tid][w >> 5], 1u << (w & 31));
    }
    __syncthreads();
    for (int64_t cb = cc; cb < ce; cb += 256) {
      const int64_t c = cb + tid;
      if (c < ce) {
        const float* q = Q + c * d;
        float acc[UB], d2[UB];
#pragma unroll
        for (int uu = 0; uu < UB; ++uu) acc[uu] = d2[uu] = 0.f;
        for (int k = 0; k < d; k += 4) {  // acc[uu] = seq_dot(row uu, q): the loop stays here (acf_sweep.h)
          const float4 qv = *reinterpret_cast<const float4*>(q + k);
#pragma unroll
          for (int uu = 0; uu < UB; ++uu) {
            acc[uu] = seq_step(acc[uu], *reinterpret_cast<const float4*>(rows + uu * d + k), qv);
            if (USER) {
              const float4 tv = *reinterpret_cast<const float4*>(trows + uu * d + k);
              const float dx = tv.x - qv.x, dy = tv.y - qv.y, dz = tv.z - qv.z, dw = tv.w - qv.w;
              d2[uu] = d2[uu] + dx * dx;
              d2[uu] = d2[uu] + dy * dy;
              d2[uu] = d2[uu] + dz * dz;
              d2[uu] = d2[uu] + dw * dw;
            }
          }
        }
        const int w = (int)(c - cc);
#pragma unroll
        for (int uu = 0; uu < UB; ++uu) {
          if (uu >= nu || ((s_ex[uu][w >> 5] >> (w & 31)) & 1u)) continue;
          const float m = s_test[uu] - acc[uu];
          const float base = USER ? sqrtf(d2[uu]) : s_np[uu];
          const float tf = s_thrf[uu];
          if (tf != -INFINITY && !evr_pred<USER>(m, 0.f - tf, base)) continue;  // eps_c > the threshold's eps
          const uint64_t key = topk_key(0.f - evr_min_eps<USER>(m, base), (int32_t)c);
          if (key > s_thr[uu]) {
            const int pos = atomicAdd(&s_cnt[uu], 1);
            if (pos < TKV_CAP) buf[uu * TKV_CAP + pos] = key;
          }
        }
      }
      __syncthreads();
      topk_prune<UB, TKV_CAP / 64>(buf, s_cnt, s_thr, s_thrf, TKV_CAP, K, TKV_CAP - 256);
    }
  }
  __syncthreads();
  topk_prune<UB, TKV_CAP / 64>(buf, s_cnt, s_thr, s_thrf, TKV_CAP, K, -1);
  for (int uu = 0; uu < nu; ++uu)
    topk_store_partial(ws, buf + uu * TKV_CAP, s_cnt[uu], K, u0 + uu, strip, S, tid, 256);
}

// k_topk_merge's scores are -eps_c (-inf past the entry's candidates): eps = 0 - score
__global__ void __launch_bounds__(256) k_evr_negate(float* __restrict__ eps, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) eps[i] = 0.f - eps[i];
}

// ---- host: strips, workspace, LDS (no device is touched) -----------------------
// k_evw_sweep's windows; a strip's partial lists are n_users * K keys.  The cut does
// not know d, so it counts tiles of EVW_UB entries whatever the kernel's tile.
constexpr size_t EVR_WS_HEAD = 16;  // the range-error flag, padded to the keys' alignment

static void evr_strips(int32_t n_users, int32_t num_cand, int32_t k, int* wper, int* S) {
  sweep_strips(num_cand, EVW_WIN, n_users, EVW_UB, 2048, std::max<int64_t>(1, n_users) * k * 8, wper, S);
}

static size_t evr_workspace(int32_t n_users, int32_t num_cand, int32_t k) {
  int wper = 0, S = 0;
  evr_strips(n_users, num_cand, k, &wper, &S);
  return EVR_WS_HEAD + (size_t)std::max(n_users, 1) * (size_t)S * (size_t)k * sizeof(uint64_t);
}

constexpr size_t evr_lds(int ub, bool user, int d) {
  return (size_t)ub * (TKV_CAP * sizeof(uint64_t) + (size_t)(user ? 2 : 1) * d * sizeof(float));
}
