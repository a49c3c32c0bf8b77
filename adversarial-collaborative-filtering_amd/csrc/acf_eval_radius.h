// Certified radius: the smallest eps at which each candidate breaks the
// certificate, and per entry the K smallest of them (CertSelect, the selecting
// sink of k_cert_sweep): included by acf_rank.hip after acf_eval_worst.h (the
// frame, cert_pred, its constants) and acf_topk.h (acf_topk_select.h: the key,
// topk_prune, the partial lists and k_topk_merge); one translation unit.
// DESIGN.md §4j.
#pragma once

// ---------------------------------------------------------------------------
// eval_radius: the pairs, m_c and base are the frame's (acf_eval_worst.h), so
// they are the counting sink's by construction.  eps_c = the smallest finite
// fp32 e >= 0 with cert_pred(m_c, e, base), +inf when there is none (m_c > 0
// with base 0; a NaN).  The predicate's product is rounded once and does not
// decrease in e, so it is monotone over [0, FLT_MAX] and the minimum exists;
// m_c <= 0 gives 0 (finite base).  Per entry the sink keeps the K smallest
// (eps_c, c), ties to the lower id: eps[r][k - 1] is the budget below which
// worst < k and from which worst >= k, i.e. the certified radius at k, for
// every k <= K.
//
// evr_min_eps: e = m / base is within a few ulps of the minimum (division is
// correctly rounded; fl(fl(m / D) D) is off by about 2^-23 m), so up to
// EVR_STEPS single steps over neighbouring floats end at pred(e) && (e == 0 ||
// !pred(prev(e))).  Whatever is left (denormal products, an overflowing or
// underflowing quotient) is finished by bisection on the bit pattern over
// (0, FLT_MAX]: non-negative floats order like their bits, at most 31 steps.
//
// The selection is k_topk_valu's: per entry TKV_CAP keys topk_key(-eps_c, c)
// (larger = smaller eps; -0.0 maps to the key of +0.0, -inf is an entry like any
// other), a count and the threshold thr = the exact K-th best key so far.  A
// pair is admitted in two steps: cert_pred at e = the threshold's eps (one
// multiply; true iff eps_c <= that eps, so a superset of the keys > thr; no
// threshold yet, or an infinite one: everything passes), and only the survivors
// compute eps_c and append iff their exact key > thr.  Every step appends at
// most 256 keys per entry and topk_prune runs after it, as in k_topk_valu.  The
// strips' partial lists go through k_topk_merge, whose scores are -eps;
// k_evr_negate turns them over.  Every loop is bounded by its inputs.
//
// Resources of k_cert_sweep<UB, USER, CertSelect<UB>> (hipcc -O3 --offload-arch=gfx950
// -Rpass-analysis=kernel-resource-usage; in brackets the separate kernel this
// sink had before the frame; profiles/cert_frame_resources.txt has both sinks):
//   <8, true>   143 VGPRs [133], 106 SGPRs [106], 3 waves/SIMD [3], no scratch, 2,576 B of static LDS [2,608]
//   <8, false>   91 VGPRs  [91], 106 SGPRs [106], 5 waves/SIMD [5], no scratch, 2,608 B [2,608]
//   <4, true>    83 VGPRs  [82], 106 SGPRs [100], 5 waves/SIMD [5], no scratch, 1,424 B [1,440]
//   <4, false>   67 VGPRs  [67], 106 SGPRs  [98], 7 waves/SIMD [7], no scratch, 1,440 B [1,440]
// Dynamic LDS: KEYS = UB * TKV_CAP keys (32 KB at UB = 8, 16 KB at 4) + the
// rows (side user: 2 UB d floats, at most 32 KB; side item: half).  Side user at
// d = 512 takes 64 KB + the static part, above the 64 KB default, so the
// launcher opts every instance in to its largest (launch_cert); two such
// workgroups still share a CU's 160 KB.
// ---------------------------------------------------------------------------
constexpr int EVR_STEPS = 4;  // single-float steps before the bisection

// The smallest finite e >= 0 with cert_pred(m, e, base), +inf when there is none.
template <bool USER>
__device__ __forceinline__ float evr_min_eps(float m, float base) {
  constexpr float FMAX = 3.402823466e+38f;
  if (cert_pred<USER>(m, 0.f, base)) return 0.f;  // m <= 0 (finite base)
  if (!cert_pred<USER>(m, FMAX, base)) return INFINITY;  // m > 0 with base 0, or a NaN
  float e = USER ? m / base : (m / base) * 0.5f;
  if (!(e <= FMAX)) e = FMAX;  // an overflowing quotient
  if (!(e > 0.f)) e = __uint_as_float(1u);  // an underflowing one: the smallest denormal
  for (int it = 0; it < EVR_STEPS; ++it) {  // pred(0) is false: e stays > 0
    if (cert_pred<USER>(m, e, base)) {
      const float lo = __uint_as_float(__float_as_uint(e) - 1u);
      if (!cert_pred<USER>(m, lo, base)) return e;
      e = lo;
    } else {
      e = __uint_as_float(__float_as_uint(e) + 1u);  // e < FMAX: pred(FMAX) holds
    }
  }
  uint32_t lo = 0u, hi = __float_as_uint(FMAX);  // !pred(lo), pred(hi)
  while (hi - lo > 1u) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (cert_pred<USER>(m, __uint_as_float(mid), base)) hi = mid; else lo = mid;
  }
  return __uint_as_float(hi);
}

struct CertSelectArgs {
  int K, S;
  uint64_t* ws;
};

template <int UB>
struct CertSelect {
  static constexpr int KEYS = UB * TKV_CAP;
  using Args = CertSelectArgs;
  struct Lds {
    float thrf[UB];  // -(the threshold's eps); -inf: none yet, or an infinite one
    int cnt[UB];
    uint64_t thr[UB];
  };
  const Args& a;
  Lds& l;
  uint64_t* const buf;  // [UB][TKV_CAP] keys

  __device__ __forceinline__ CertSelect(const Args& a_, Lds& l_, uint64_t* keys) : a(a_), l(l_), buf(keys) {}
  __device__ __forceinline__ void init(int uu) {
    l.cnt[uu] = 0;
    l.thr[uu] = 0;
    l.thrf[uu] = -INFINITY;
  }
  template <bool USER>
  __device__ __forceinline__ void pair(int uu, bool in, float m, float base, int32_t c) {
    if (!in) return;
    const float tf = l.thrf[uu];
    if (tf != -INFINITY && !cert_pred<USER>(m, 0.f - tf, base)) return;  // eps_c > the threshold's eps
    const uint64_t key = topk_key(0.f - evr_min_eps<USER>(m, base), c);
    if (key > l.thr[uu]) {
      const int pos = atomicAdd(&l.cnt[uu], 1);
      if (pos < TKV_CAP) buf[uu * TKV_CAP + pos] = key;
    }
  }
  __device__ __forceinline__ void step() {
    __syncthreads();
    topk_prune<UB, TKV_CAP / 64>(buf, l.cnt, l.thr, l.thrf, TKV_CAP, a.K, TKV_CAP - 256);
  }
  __device__ __forceinline__ void finish(int u0, int nu, int, int strip) {
    topk_prune<UB, TKV_CAP / 64>(buf, l.cnt, l.thr, l.thrf, TKV_CAP, a.K, -1);
    for (int uu = 0; uu < nu; ++uu)
      topk_store_partial(a.ws, buf + uu * TKV_CAP, l.cnt[uu], a.K, u0 + uu, strip, a.S, threadIdx.x, 256);
  }
};

// k_topk_merge's scores are -eps_c (-inf past the entry's candidates): eps = 0 - score
__global__ void __launch_bounds__(256) k_evr_negate(float* __restrict__ eps, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) eps[i] = 0.f - eps[i];
}

// ---- host: strips and workspace (no device is touched) -------------------------
// The frame's windows; a strip's partial lists are n_users * K keys.  The cut does
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
