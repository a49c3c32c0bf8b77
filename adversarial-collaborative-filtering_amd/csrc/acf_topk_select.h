// Exact bounded-buffer top-K selection shared by libacf_apr.so (acf_topk.h) and
// libacf_neumf.so (acf_neumf.hip): the 64-bit key, the rank-sort prune, the
// strips' partial lists and the merge kernel.  acf_topk.h states the scheme.
#pragma once

constexpr int TOPK_MAX_K = 128;
constexpr int TKV_CAP = 512;     // keys per user of the VALU sweep and of the merge

__device__ __forceinline__ uint64_t topk_key(float s, int32_t id) {
  uint32_t b = __float_as_uint(s);
  if (s == 0.f) b = 0u;
  b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((uint64_t)b << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)id);
}

__device__ __forceinline__ float topk_key_score(uint64_t key) {
  if (key == 0) return -INFINITY;
  const uint32_t h = (uint32_t)(key >> 32);
  return __uint_as_float((h & 0x80000000u) ? (h ^ 0x80000000u) : ~h);
}

__device__ __forceinline__ int32_t topk_key_item(uint64_t key) {
  return key == 0 ? -1 : (int32_t)(0xFFFFFFFFu - (uint32_t)key);
}

// All 256 threads of the workgroup, after a barrier that made the appends
// visible.  Users [0, NU) own buf[u * cap .. + cap), cnt[u], thr[u]; a user whose
// count exceeds `limit` is rank-sorted (its keys descending in buf[u * cap ..
// + min(count, K))), cut to K, and thr[u] / thrf[u] (the threshold's score, -inf
// for none; thrf may be NULL) are refreshed.  Wave w serves users w, w + 4, ...;
// TPL * 64 >= cap.  Ends with a barrier.
template <int NU, int TPL>
__device__ __forceinline__ void topk_prune(uint64_t* __restrict__ buf, int* __restrict__ cnt,
                                           uint64_t* __restrict__ thr, float* __restrict__ thrf, int cap, int K,
                                           int limit) {
  const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63;
  if (!__syncthreads_or(tid < NU && cnt[tid] > limit)) return;
  for (int ub = 0; ub < NU; ub += 4) {
    const int u = ub + wave;
    const int n = u < NU ? min(cnt[u], cap) : 0;
    const bool need = u < NU && n > limit;
    uint64_t* b = buf + (size_t)(u < NU ? u : 0) * cap;
    uint64_t my[TPL];
    int rk[TPL];
    if (need) {
#pragma unroll
      for (int t = 0; t < TPL; ++t) {
        const int idx = l + 64 * t;
        my[t] = idx < n ? b[idx] : 0;
        rk[t] = 0;
      }
      for (int i = 0; i < n; ++i) {
        const uint64_t o = b[i];
#pragma unroll
        for (int t = 0; t < TPL; ++t) rk[t] += o > my[t] ? 1 : 0;
      }
    }
    __syncthreads();  // every key is in a register before a slot is overwritten
    if (need) {
#pragma unroll
      for (int t = 0; t < TPL; ++t)
        if (l + 64 * t < n && rk[t] < K) b[rk[t]] = my[t];
      if (l == 0) cnt[u] = min(n, K);
    }
    __syncthreads();
    if (need && l == 0) {
      const uint64_t th = n >= K ? b[K - 1] : 0;
      thr[u] = th;
      if (thrf) thrf[u] = topk_key_score(th);
    }
  }
  __syncthreads();
}

// the strip's partial list of user row k: K keys, descending, 0-padded
__device__ __forceinline__ void topk_store_partial(uint64_t* __restrict__ ws, const uint64_t* __restrict__ b,
                                                   int n, int K, int64_t k, int strip, int S, int lane, int nl) {
  uint64_t* o = ws + ((size_t)k * S + strip) * K;
  for (int i = lane; i < K; i += nl) o[i] = i < n ? b[i] : 0;
}

// ---- merge: the final K of user k from its S partial lists -------------------
// One workgroup per user streams the S * K keys (0 = padding) through the same
// buffer-and-threshold selection and decodes the K best into items / scores
// (-1 / -inf past the user's candidates).
__global__ void __launch_bounds__(256) k_topk_merge(const uint64_t* __restrict__ ws, int S, int K,
                                                    int32_t* __restrict__ items, float* __restrict__ scores) {
  __shared__ uint64_t buf[TKV_CAP];
  __shared__ int s_cnt[1];
  __shared__ uint64_t s_thr[1];
  const int tid = threadIdx.x;
  const int64_t k = blockIdx.x;
  const uint64_t* in = ws + (size_t)k * S * K;
  const int64_t total = (int64_t)S * K;
  if (tid == 0) {
    s_cnt[0] = 0;
    s_thr[0] = 0;
  }
  __syncthreads();
  for (int64_t base = 0; base < total; base += 256) {
    const uint64_t key = base + tid < total ? in[base + tid] : 0;
    if (key > s_thr[0]) {
      const int pos = atomicAdd(&s_cnt[0], 1);
      if (pos < TKV_CAP) buf[pos] = key;
    }
    __syncthreads();
    topk_prune<1, TKV_CAP / 64>(buf, s_cnt, s_thr, nullptr, TKV_CAP, K, TKV_CAP - 256);
  }
  topk_prune<1, TKV_CAP / 64>(buf, s_cnt, s_thr, nullptr, TKV_CAP, K, -1);
  if (tid < K) {
    const uint64_t key = tid < s_cnt[0] ? buf[tid] : 0;
    items[k * K + tid] = topk_key_item(key);
    scores[k * K + tid] = topk_key_score(key);
  }
}
