// Top-K recommendation kernels of libacf_apr.so (k_topk_*): included by
// acf_rank.hip after acf_sweep.h and acf_eval.h (seq_dot, the shared sweep pieces,
// the EVM_* tiling); one translation unit.
#pragma once

// ---------------------------------------------------------------------------
// recommend_topk: per user the K best candidates of [0, num_cand) minus the SET
// of its exclusion entries, ordered by (seq_dot score descending, item id
// ascending).  No U x I score array exists: the candidate range is cut into
// strips of 128-candidate windows, a workgroup sweeps one strip for a tile of
// users and keeps, per user, a bounded LDS buffer of admitted entries, and a
// merge kernel selects the final K from the strips' partial lists.
//
// An entry is one 64-bit key, larger = better:
//   high word: the score's bits mapped so that unsigned order = float order
//   low word:  0xFFFFFFFF - item id   (ties go to the ascending id)
// Ids are unique within a user, so keys are unique and the order is total (a
// NaN is just some key: the order with NaNs is unspecified, but every loop
// terminates and every index stays in bounds).  Key 0 is never an entry (the low
// word of an entry is >= 2^31) and stands for "none": padding, and "no
// threshold yet".  seq_dot never yields -0.0 (the chain starts at +0.0 and a
// round-to-nearest sum is -0.0 only from two negative zeros), so mapping a zero
// score to the key of +0.0 loses no bits and makes -0.0 == +0.0 hold anyway.
//
// Selection (both sweeps and the merge): a user's buffer holds `cap` keys, a
// count and a threshold thr = the exact K-th best key seen so far (0 until K
// entries were seen).  A candidate is appended iff its exact key > thr; every
// step appends at most `burst` keys per user, and topk_prune runs after each
// step for the users whose count exceeds cap - burst: an exact rank sort keeps
// the K best in order and raises thr.  Whatever the arrival order of the
// appends, the kept set is the exact top-K of what was seen, so the output is
// deterministic; nothing is accumulated in floating point.
// ---------------------------------------------------------------------------
// the key, topk_prune, the partial lists and k_topk_merge; TOPK_MAX_K, TKV_CAP (the
// VALU sweep appends one candidate per thread and step: burst 256)
#include "acf_topk_select.h"

constexpr int TKV_UB = 8;        // VALU sweep: users per workgroup
constexpr int TKV_CHUNK = 2048;  // ... candidates per exclusion bitmap
constexpr int TKM_SW = 4;        // MFMA sweep: windows per exclusion bitmap
constexpr int TKM_BURST = 64;    // ... keys per user and half epilogue (4 waves x 16 lanes)
constexpr int TKM_CAP_MAX = TOPK_MAX_K + TKM_BURST;  // 192

// ---- VALU sweep: the straightforward restatement ---------------------------
// A workgroup holds TKV_UB users' rows in LDS and sweeps its strip
// [strip * wper * 128, ...) 256 candidates a step, every thread one candidate
// against the 8 rows (seq_step); the exclusion lists are applied as a bitmap per
// TKV_CHUNK candidates (sweep_excl_strided).
__global__ void __launch_bounds__(256) k_topk_valu(const float* __restrict__ P, const float* __restrict__ Q, int d,
                                                   const int32_t* __restrict__ users, int n_users, int num_cand,
                                                   const int64_t* __restrict__ excl_off,
                                                   const int32_t* __restrict__ excl, int K, int wper, int S,
                                                   uint64_t* __restrict__ ws) {
  extern __shared__ uint64_t tk_smem[];  // [TKV_UB][TKV_CAP] keys, then [TKV_UB][d] rows
  uint64_t* buf = tk_smem;
  float* rows = reinterpret_cast<float*>(tk_smem + TKV_UB * TKV_CAP);
  __shared__ int s_cnt[TKV_UB];
  __shared__ uint64_t s_thr[TKV_UB];
  __shared__ uint32_t s_ex[TKV_UB][TKV_CHUNK / 32];
  __shared__ int64_t s_off[TKV_UB + 1];
  const int tid = threadIdx.x, strip = blockIdx.y;
  const int u0 = blockIdx.x * TKV_UB;
  const int nu = min(TKV_UB, n_users - u0);
  const int64_t c_begin = (int64_t)strip * wper * EVM_C;
  const int64_t c_end = min((int64_t)num_cand, c_begin + (int64_t)wper * EVM_C);
  sweep_load_rows<TKV_UB, false>(rows, P, d, users, u0, nu, 0, nullptr);
  if (tid < TKV_UB) {
    s_cnt[tid] = 0;
    s_thr[tid] = 0;
  }
  if (tid <= nu) s_off[tid] = excl_off[u0 + tid];
  for (int64_t cc = c_begin; cc < c_end; cc += TKV_CHUNK) {
    const int64_t ce = min(c_end, cc + TKV_CHUNK);
    __syncthreads();  // the previous chunk's bitmap reads (first pass: the rows)
    sweep_excl_strided<TKV_UB, TKV_CHUNK>(s_ex, s_off, nu, excl, cc, ce - cc);
    __syncthreads();
    for (int64_t base = cc; base < ce; base += 256) {
      const int64_t c = base + tid;
      if (c < ce) {
        const float* q = Q + c * d;
        float acc[TKV_UB];
#pragma unroll
        for (int uu = 0; uu < TKV_UB; ++uu) acc[uu] = 0.f;
        for (int k = 0; k < d; k += 4) {  // acc[uu] = seq_dot(row uu, q): the loop stays here (acf_sweep.h)
          const float4 qv = *reinterpret_cast<const float4*>(q + k);
#pragma unroll
          for (int uu = 0; uu < TKV_UB; ++uu)
            acc[uu] = seq_step(acc[uu], *reinterpret_cast<const float4*>(rows + uu * d + k), qv);
        }
        const int w = (int)(c - cc);
#pragma unroll
        for (int uu = 0; uu < TKV_UB; ++uu) {
          if (uu >= nu || ((s_ex[uu][w >> 5] >> (w & 31)) & 1u)) continue;
          const uint64_t key = topk_key(acc[uu], (int32_t)c);
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

// ---- MFMA sweep: MFMA as the filter, seq_dot as the judge -------------------
// k_eval_fused's tiling (64 users x 128 candidates a window, 4 waves of 4 x 2
// v_mfma_f32_16x16x4_f32 tiles, K staged through LDS in chunks of 32), walked
// over the strip's windows.  s_mfma and the seq_dot score s are both within
// E = eb |p| |q| + floor_e of the real dot product's neighbourhood that
// k_eval_fused's comment derives, so |s_mfma - s| <= E.  A candidate can enter
// the strip's top-K only if its key > thr, hence s >= score(thr), hence
// s_mfma + E >= score(thr): candidates failing that test are dropped unseen, the
// others are rescored with seq_dot and appended iff their exact key > thr.  Only
// exact scores are ever stored or compared, so the result has k_topk_valu's bits.
// With every score tied the filter passes every candidate, and the exact key
// test then rejects all but the lowest ids: the worst case costs rescoring, not
// buffer space.  Buffer: cap = min(2K + 64, 192) keys per user (<= 96 KB of LDS).
__global__ void __launch_bounds__(256) k_topk_mfma(const float* __restrict__ P, const float* __restrict__ Q, int d,
                                                   const int32_t* __restrict__ users, int n_users, int num_cand,
                                                   const int64_t* __restrict__ excl_off,
                                                   const int32_t* __restrict__ excl, float eb, float floor_e, int K,
                                                   int cap, int wper, int S, uint64_t* __restrict__ ws) {
  extern __shared__ uint64_t tk_smem[];  // [EVM_U][cap] keys
  uint64_t* buf = tk_smem;
  __shared__ float sP[EVM_U][EVM_KC + 1];
  __shared__ float sQ[EVM_C][EVM_KC + 1];
  __shared__ int s_cnt[EVM_U];
  __shared__ uint64_t s_thr[EVM_U];
  __shared__ float s_thrf[EVM_U], s_pn[EVM_U], s_qn[EVM_C];
  __shared__ int32_t s_row[EVM_U];
  __shared__ uint32_t s_ex[EVM_U][TKM_SW * EVM_C / 32];
  __shared__ int64_t s_off[EVM_U + 1];
  const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63;
  const int strip = blockIdx.y;
  const int u0 = blockIdx.x * EVM_U;
  const int nu = min(EVM_U, n_users - u0);
  const int64_t c_begin = (int64_t)strip * wper * EVM_C;
  const int64_t c_end = min((int64_t)num_cand, c_begin + (int64_t)wper * EVM_C);
  if (tid < EVM_U) {
    const int32_t row = tid < nu ? users[u0 + tid] : -1;
    s_row[tid] = row;
    s_cnt[tid] = 0;
    s_thr[tid] = 0;
    s_thrf[tid] = -INFINITY;
    double ss = 0.0;  // the user's squared norm, once per strip
    if (row >= 0)
      for (int k = 0; k < d; ++k) ss += (double)P[(int64_t)row * d + k] * (double)P[(int64_t)row * d + k];
    s_pn[tid] = (float)(sqrt(ss) * (1.0 + 1e-6));  // rounded up
  }
  if (tid <= nu) s_off[tid] = excl_off[u0 + tid];
  for (int64_t cs = c_begin; cs < c_end; cs += TKM_SW * EVM_C) {
    __syncthreads();  // the previous bitmap's reads (first pass: s_off)
    for (int x = tid; x < EVM_U * (TKM_SW * EVM_C / 32); x += 256) (&s_ex[0][0])[x] = 0u;
    __syncthreads();
    // exclusion bitmap of [cs, cs + 512): as k_eval_fused, the tile's lists are
    // one contiguous span of excl; each entry's user by a binary search of s_off
    {
      const int64_t a0 = s_off[0], a1 = s_off[nu];
      for (int64_t x0 = a0 + tid; x0 < a1; x0 += 4 * 256) {
        int32_t v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = x0 + q * 256 < a1 ? excl[x0 + q * 256] : -1;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int64_t x = x0 + q * 256;
          const int64_t it = (int64_t)v[q] - cs;
          if (x >= a1 || it < 0 || it >= TKM_SW * EVM_C) continue;
          int lo = 0, hi = nu;  // the user: last ur with s_off[ur] <= x
          while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (s_off[mid] <= x) lo = mid; else hi = mid;
          }
          atomicOr(&s_ex[lo][it >> 5], 1u << (it & 31));
        }
      }
    }
    for (int wi = 0; wi < TKM_SW; ++wi) {
      const int64_t c0 = cs + (int64_t)wi * EVM_C;
      if (c0 >= c_end) break;
      double ss = 0.0;  // 64 <= tid < 192: candidate tid - 64's squared norm
      f32x4 acc[4][2];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[r][c] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int k0 = 0; k0 < d; k0 += EVM_KC) {
        __syncthreads();  // the previous chunk's reads (and the bitmap's writes)
        constexpr int C4 = EVM_KC / 4;
#pragma unroll
        for (int j = 0; j < EVM_U * C4 / 256; ++j) {
          const int idx = tid + 256 * j, row = idx / C4, c4 = idx - row * C4, k = k0 + 4 * c4;
          const int32_t pr = s_row[row];
          const float4 v = (pr >= 0 && k < d) ? *reinterpret_cast<const float4*>(P + (int64_t)pr * d + k)
                                              : make_float4(0.f, 0.f, 0.f, 0.f);
          sP[row][4 * c4] = v.x; sP[row][4 * c4 + 1] = v.y; sP[row][4 * c4 + 2] = v.z; sP[row][4 * c4 + 3] = v.w;
        }
#pragma unroll
        for (int j = 0; j < EVM_C * C4 / 256; ++j) {
          const int idx = tid + 256 * j, row = idx / C4, c4 = idx - row * C4, k = k0 + 4 * c4;
          const int64_t cand = c0 + row;
          const float4 v = (cand < c_end && k < d) ? *reinterpret_cast<const float4*>(Q + cand * d + k)
                                                   : make_float4(0.f, 0.f, 0.f, 0.f);
          sQ[row][4 * c4] = v.x; sQ[row][4 * c4 + 1] = v.y; sQ[row][4 * c4 + 2] = v.z; sQ[row][4 * c4 + 3] = v.w;
        }
        __syncthreads();
        const int kend = min(EVM_KC, d - k0);
        if (tid >= EVM_U && tid < EVM_U + EVM_C)
          for (int k = 0; k < kend; ++k) ss += (double)sQ[tid - EVM_U][k] * (double)sQ[tid - EVM_U][k];
        for (int kk = 0; kk < kend; kk += 4) {
          float a[4], b[2];
#pragma unroll
          for (int r = 0; r < 4; ++r) a[r] = sP[16 * r + (l & 15)][kk + (l >> 4)];
#pragma unroll
          for (int c = 0; c < 2; ++c) b[c] = sQ[wave * 32 + 16 * c + (l & 15)][kk + (l >> 4)];
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 2; ++c)
              acc[r][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], b[c], acc[r][c], 0, 0, 0);
        }
      }
      if (tid >= EVM_U && tid < EVM_U + EVM_C) s_qn[tid - EVM_U] = (float)(sqrt(ss) * (1.0 + 1e-6));
      __syncthreads();
      // epilogue: lane l holds users 16r + 4(l >> 4) + reg, candidate 16c + (l & 15);
      // one c at a time, so a user gets at most 4 waves x 16 lanes = TKM_BURST keys
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int cl = wave * 32 + 16 * c + (l & 15);
        const int64_t cand = c0 + cl;
        const int w = wi * EVM_C + cl;
        if (cand < c_end) {
          const float qn = s_qn[cl];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
              const int ur = 16 * r + 4 * (l >> 4) + reg;
              if (ur >= nu || ((s_ex[ur][w >> 5] >> (w & 31)) & 1u)) continue;
              const float e = eb * s_pn[ur] * qn + floor_e;
              if (!(acc[r][c][reg] + e >= s_thrf[ur])) continue;
              const float s = seq_dot(P + (int64_t)s_row[ur] * d, Q + cand * d, d);
              const uint64_t key = topk_key(s, (int32_t)cand);
              if (key > s_thr[ur]) {
                const int pos = atomicAdd(&s_cnt[ur], 1);
                if (pos < cap) buf[(size_t)ur * cap + pos] = key;
              }
            }
          }
        }
        __syncthreads();
        topk_prune<EVM_U, TKM_CAP_MAX / 64>(buf, s_cnt, s_thr, s_thrf, cap, K, cap - TKM_BURST);
      }
    }
  }
  __syncthreads();
  topk_prune<EVM_U, TKM_CAP_MAX / 64>(buf, s_cnt, s_thr, s_thrf, cap, K, -1);
  for (int uu = wave; uu < nu; uu += 4)
    topk_store_partial(ws, buf + (size_t)uu * cap, s_cnt[uu], K, u0 + uu, strip, S, l, 64);
}


// ---- host: strips and workspace ----------------------------------------------
// kernel 1 (MFMA) / 2 (VALU) -> windows per strip and the number of strips S
// (sweep_strips; 64 users x 5M items: 1 user tile x 512 strips); a strip's
// partial lists are n_users * K keys.
static void topk_strips(int32_t n_users, int32_t num_cand, int32_t k, int kernel, int* wper, int* S) {
  sweep_strips(num_cand, EVM_C, n_users, kernel == 1 ? EVM_U : TKV_UB, kernel == 1 ? 512 : 2048,
               std::max<int64_t>(1, n_users) * k * 8, wper, S);
}

static int topk_mfma_cap(int k) { return std::min(2 * k + TKM_BURST, TKM_CAP_MAX); }
