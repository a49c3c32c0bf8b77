// Nearest-neighbour lists of libacf_apr.so (k_nbr_*): included by acf_rank.hip
// after acf_topk.h (acf_sweep.h's pieces, the key, topk_prune, k_topk_merge, the
// strip cut); one translation unit.  DESIGN.md §4h.
#pragma once

// ---------------------------------------------------------------------------
// neighbors_topk: per query row a = X[queries[r]] the K best candidates b = T[c]
// of [0, num_cand) minus the SET of its exclusion entries (and minus c ==
// queries[r] when exclude_self), ordered by (score descending, id ascending).
// The score is a compile-time policy over the same sweep as k_topk_valu:
//   NBR_DOT  s = seq_dot(a, b)
//   NBR_COS  den = sqrtf(seq_dot(a, a)) * sqrtf(seq_dot(b, b));
//            den > 0 ? (s / den) + 0.0f : +0.0f
//   NBR_EUC  0.0f - D2, D2 = k_cert_sweep's chain: the sum over k ascending from
//            +0.0 of round((a[k] - b[k])^2)
// every operation fp32 and rounded on its own (-ffp-contract=off), the square
// roots and the division correctly rounded.
//
// No score is -0.0, which topk_key relies on (it maps a zero score to the key
// of +0.0, so a -0.0 would come back as +0.0 bits): seq_dot never yields it
// (acf_sweep.h); a quotient that underflows on the negative side is -0.0 and
// the "+ 0.0f" turns it into +0.0 (x + 0.0f is x for every other x); D2 is a
// sum of squares from +0.0, so it is >= +0.0 and 0.0f - D2 is +0.0 exactly when
// D2 is +0.0 (identical rows) and negative otherwise.
//
// The candidates' norms sqrtf(seq_dot(b, b)) are computed once per call by
// k_nbr_norms into the workspace (one float per candidate: no normalised copy
// of T exists) and read back one coalesced float per lane and step; the query
// norms come from the rows the workgroup staged.  Self-exclusion sets the
// query's own bit in the exclusion bitmap of the chunk that holds it, a compare
// of the staged id against the chunk's range: no list is built for it.
// Selection, partial lists and merge are acf_topk.h's, so the result is exact
// and deterministic whatever the order of the appends.
//
// No MFMA variant: DESIGN §4b measured that selection, not scoring, is what a
// top-K sweep costs here; the MFMA filter lost to the VALU sweep by 5x.
// ---------------------------------------------------------------------------
constexpr int NBR_DOT = 0, NBR_COS = 1, NBR_EUC = 2;
constexpr size_t NBR_WS_HEAD = 16;  // the range-error flag, padded: the partial lists stay 8-byte aligned

// norms[c] = sqrtf(seq_dot(T[c], T[c])), one row per lane (the chain is
// sequential: more lanes per row could only share its loads)
__global__ void __launch_bounds__(256) k_nbr_norms(const float* __restrict__ T, int d, int64_t n,
                                                   float* __restrict__ norms) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  const float* b = T + c * d;
  float s = 0.f;
  for (int k = 0; k < d; k += 4) {
    const float4 v = *reinterpret_cast<const float4*>(b + k);
    s = seq_step(s, v, v);
  }
  norms[c] = sqrtf(s);
}

// one term of the chain of row uu against candidate values qv (acc from +0.0)
template <int METRIC>
__device__ __forceinline__ float nbr_step(float acc, const float4 pv, const float4 qv) {
  if (METRIC != NBR_EUC) return seq_step(acc, pv, qv);
  const float dx = pv.x - qv.x, dy = pv.y - qv.y, dz = pv.z - qv.z, dw = pv.w - qv.w;
  acc = acc + dx * dx;
  acc = acc + dy * dy;
  acc = acc + dz * dz;
  acc = acc + dw * dw;
  return acc;
}

// the score of a finished chain: na / nb are the rows' norms (NBR_COS only)
template <int METRIC>
__device__ __forceinline__ float nbr_score(float acc, float na, float nb) {
  if (METRIC == NBR_DOT) return acc;
  if (METRIC == NBR_EUC) return 0.0f - acc;
  const float den = na * nb;
  return den > 0.f ? (acc / den) + 0.0f : 0.0f;
}

// k_topk_valu's sweep (TKV_UB query rows in LDS, 256 candidates a step, the
// exclusion bitmap per TKV_CHUNK candidates, topk_prune with cap TKV_CAP and
// burst 256) with the score as the policy METRIC.  A query outside [0, XR) is
// read as row 0 (its id, for exclude_self, is then 0 as well) and bit 1 is ORed
// into *err.  excl_off == NULL: no lists.
template <int METRIC>
__global__ void __launch_bounds__(256) k_nbr_valu(const float* __restrict__ T, const float* __restrict__ X, int d,
                                                  int64_t XR, const int32_t* __restrict__ queries, int n_q,
                                                  int num_cand, int exclude_self,
                                                  const int64_t* __restrict__ excl_off,
                                                  const int32_t* __restrict__ excl,
                                                  const float* __restrict__ cnorm, int K, int wper, int S,
                                                  uint64_t* __restrict__ ws, int32_t* __restrict__ err) {
  extern __shared__ uint64_t tk_smem[];  // [TKV_UB][TKV_CAP] keys, then [TKV_UB][d] rows
  uint64_t* buf = tk_smem;
  float* rows = reinterpret_cast<float*>(tk_smem + TKV_UB * TKV_CAP);
  __shared__ int s_cnt[TKV_UB];
  __shared__ uint64_t s_thr[TKV_UB];
  __shared__ uint32_t s_ex[TKV_UB][TKV_CHUNK / 32];
  __shared__ int64_t s_off[TKV_UB + 1];
  __shared__ int32_t s_qid[TKV_UB];  // the staged query ids, range-checked
  __shared__ float s_qn[TKV_UB];     // NBR_COS: the query rows' norms
  const int tid = threadIdx.x, strip = blockIdx.y;
  const int u0 = blockIdx.x * TKV_UB;
  const int nu = min(TKV_UB, n_q - u0);
  const int64_t c_begin = (int64_t)strip * wper * EVM_C;
  const int64_t c_end = min((int64_t)num_cand, c_begin + (int64_t)wper * EVM_C);
  sweep_load_rows<TKV_UB, true>(rows, X, d, queries, u0, nu, XR, err);  // reported when the caller checks
  if (tid < TKV_UB) {
    s_cnt[tid] = 0;
    s_thr[tid] = 0;
    int64_t q = tid < nu ? queries[u0 + tid] : 0;
    if (q < 0 || q >= XR) q = 0;
    s_qid[tid] = (int32_t)q;
  }
  if (tid <= TKV_UB) s_off[tid] = excl_off ? excl_off[u0 + min(tid, nu)] : 0;  // past the tile: empty lists
  if (METRIC == NBR_COS) {
    __syncthreads();  // the rows
    if (tid < TKV_UB) {
      const float* a = rows + tid * d;
      float n2 = 0.f;
      for (int k = 0; k < d; ++k) n2 = n2 + a[k] * a[k];
      s_qn[tid] = sqrtf(n2);
    }
  }
  for (int64_t cc = c_begin; cc < c_end; cc += TKV_CHUNK) {
    const int64_t ce = min(c_end, cc + TKV_CHUNK);
    __syncthreads();  // the previous chunk's bitmap reads (first pass: the rows, s_qid, s_qn)
    sweep_excl_strided<TKV_UB, TKV_CHUNK>(s_ex, s_off, nu, excl, cc, ce - cc);  // no lists: s_off is all 0
    if (exclude_self && tid < nu) {  // the query itself is no candidate
      const int64_t w = (int64_t)s_qid[tid] - cc;
      if (w >= 0 && w < ce - cc) atomicOr(&s_ex[tid][w >> 5], 1u << (w & 31));
    }
    __syncthreads();
    for (int64_t base = cc; base < ce; base += 256) {
      const int64_t c = base + tid;
      if (c < ce) {
        const float* q = T + c * d;
        float acc[TKV_UB];
#pragma unroll
        for (int uu = 0; uu < TKV_UB; ++uu) acc[uu] = 0.f;
        for (int k = 0; k < d; k += 4) {  // the loop stays here (acf_sweep.h)
          const float4 qv = *reinterpret_cast<const float4*>(q + k);
#pragma unroll
          for (int uu = 0; uu < TKV_UB; ++uu)
            acc[uu] = nbr_step<METRIC>(acc[uu], *reinterpret_cast<const float4*>(rows + uu * d + k), qv);
        }
        const float nb = METRIC == NBR_COS ? cnorm[c] : 0.f;
        const int w = (int)(c - cc);
#pragma unroll
        for (int uu = 0; uu < TKV_UB; ++uu) {
          if (uu >= nu || ((s_ex[uu][w >> 5] >> (w & 31)) & 1u)) continue;
          const float sc = nbr_score<METRIC>(acc[uu], METRIC == NBR_COS ? s_qn[uu] : 0.f, nb);
          const uint64_t key = topk_key(sc, (int32_t)c);
          if (key > s_thr[uu]) {
            const int pos = atomicAdd(&s_cnt[uu], 1);
            if (pos < TKV_CAP) buf[uu * TKV_CAP + pos] = key;
          }
        }
      }
      __syncthreads();
      topk_prune<TKV_UB, TKV_CAP / 64>(buf, s_cnt, s_thr, nullptr, TKV_CAP, K, TKV_CAP - 256);
    }
  }
  __syncthreads();
  topk_prune<TKV_UB, TKV_CAP / 64>(buf, s_cnt, s_thr, nullptr, TKV_CAP, K, -1);
  for (int uu = 0; uu < nu; ++uu)
    topk_store_partial(ws, buf + uu * TKV_CAP, s_cnt[uu], K, u0 + uu, strip, S, tid, 256);
}

// ---- host: workspace layout (no device is touched) ----------------------------
// [ NBR_WS_HEAD | n_queries * S * k keys (topk_strips' VALU cut) | num_cand floats ]
// the norms are used by NBR_COS only; the query reports the layout whole, and a
// call with another metric needs the part before them.
static size_t nbr_lists_bytes(int32_t n_q, int32_t num_cand, int32_t k, int* wper, int* S) {
  topk_strips(n_q, num_cand, k, 2, wper, S);
  return (size_t)std::max(n_q, 1) * (size_t)*S * (size_t)k * sizeof(uint64_t);
}

static size_t nbr_workspace(int32_t n_q, int32_t num_cand, int32_t k, bool norms) {
  int wper = 0, S = 0;
  return NBR_WS_HEAD + nbr_lists_bytes(n_q, num_cand, k, &wper, &S) + (norms ? (size_t)num_cand * sizeof(float) : 0);
}
