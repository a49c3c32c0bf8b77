// Certified worst-case positions under an eps attack (k_evw_*): included by
// acf_rank.hip after acf_eval_multi.h (acf_sweep.h's pieces, k_evx_sum); one
// translation unit.  DESIGN.md §4g.
#pragma once

// ---------------------------------------------------------------------------
// eval_positions_worst: entry r has the user row p = P[users[r]], the test item
// t = test_items[r] and the candidates C_r = [0, num_cand) minus the SET of its
// exclusion entries.  With m_c = seq_dot(p, Q[t]) - seq_dot(p, Q[c]),
//   worst[e][r] = #{ c in C_r, c != t : m_c <= thr_e(c) }
//   side user:  thr_e(c) = eps_e * D_c,  D_c = sqrtf(D2), D2 = the sum over k
//               ascending from +0.0 of round((Q[t][k] - Q[c][k])^2)
//   side item:  thr_e    = (2 eps_e) * Np, Np = sqrtf(the same chain over p[k]^2)
// all of it fp32, every operation rounded on its own (-ffp-contract=off), the
// square roots correctly rounded.  No single perturbation within the budget
// (|delta|_2 <= eps on the user row; on every item row) can put more than
// worst[e][r] candidates at or above t.  At eps = 0 the predicate is
// seq_dot(p, Q[c]) >= seq_dot(p, Q[t]) exactly (x - y <= 0 iff x <= y: fp32
// subtraction keeps denormals), so the row equals k_eval_all's positions.
//
// A VALU sweep like k_evx_sweep: a workgroup of 256 holds UB entries' user rows
// in LDS (side user: their test items' rows as well), one candidate per lane and
// step, its score out of seq_step; every eps of the call is compared against the
// same m and D, so the candidates are swept once whatever their number.  The
// test item is kept out by setting its bit in the exclusion bitmap.  A wave counts
// a predicate with one ballot, so the counts are wave-uniform ints, added per
// workgroup by one lane of each wave with integer LDS atomics; a strip of
// the candidate range (grid.y) writes its counts to out + strip * n_eps *
// n_users (the caller's workspace, or worst itself when there is one strip) and
// k_evx_sum adds the strips in strip order.  No float is accumulated across
// threads: equal inputs give equal bits.
//
// LDS: UB = 8 entries per workgroup up to d = 512, 4 above, so the rows take at
// most 2 * 8 * 512 * 4 = 2 * 4 * 1024 * 4 = 32 KB (side item: half of that),
// the bitmap 2 KB and the rest under 1 KB: within the 64 KB default.
// ---------------------------------------------------------------------------
constexpr int EVW_MAX_EPS = 8;
constexpr int EVW_WIN = 256;   // candidates per window; strips are whole windows
constexpr int EVW_BM = 2048;   // candidates per exclusion bitmap
constexpr int EVW_UB = 8;      // entries per workgroup (4 above d = 512); the strip cut counts tiles of 8
constexpr int EVW_D_SPLIT = 512;
constexpr int EVW_WAVE = 64;   // lanes per wave (gfx950): a wave counts with one ballot

struct EvwEps {
  int32_t n;
  float e[EVW_MAX_EPS];
};

template <int UB, bool USER>
__global__ void __launch_bounds__(256) k_evw_sweep(const float* __restrict__ P, const float* __restrict__ Q, int d,
                                                   int64_t U1, int64_t I1, const int32_t* __restrict__ users,
                                                   const int32_t* __restrict__ test_items, int n_users, int num_cand,
                                                   const int64_t* __restrict__ excl_off,
                                                   const int32_t* __restrict__ excl, EvwEps eps, int wper,
                                                   int32_t* __restrict__ out, int32_t* __restrict__ err) {
  extern __shared__ float evw_rows[];  // [UB][d] user rows, then (USER) [UB][d] test-item rows
  __shared__ float s_test[UB];                 // seq_dot(p, Q[t])
  __shared__ float s_thr[EVW_MAX_EPS][UB];     // side item: (2 eps) * Np
  __shared__ int s_cnt[EVW_MAX_EPS][UB];
  __shared__ int32_t s_tid[UB];                // the test items, range-checked
  __shared__ uint32_t s_ex[UB][EVW_BM / 32];
  __shared__ int64_t s_eoff[UB + 1];
  float* const trows = evw_rows + UB * d;
  const int tid = threadIdx.x, strip = blockIdx.y;
  const int u0 = blockIdx.x * UB;
  const int nu = min(UB, n_users - u0);
  const int64_t c_begin = (int64_t)strip * wper * EVW_WIN;
  const int64_t c_end = min((int64_t)num_cand, c_begin + (int64_t)wper * EVW_WIN);
  int32_t* const dst = out + (int64_t)strip * eps.n * n_users;
  sweep_load_rows<UB, true>(evw_rows, P, d, users, u0, nu, U1, err);  // reported when the caller checks
  if (tid < UB) {
    int64_t t = tid < nu ? test_items[u0 + tid] : 0;
    if (t < 0 || t >= I1) {
      t = 0;
      atomicOr(err, 2);
    }
    s_tid[tid] = (int32_t)t;
  }
  if (tid <= UB) s_eoff[tid] = excl_off ? excl_off[u0 + min(tid, nu)] : 0;  // past the tile: empty lists
  __syncthreads();
  if (USER) {
    sweep_load_rows<UB, false>(trows, Q, d, s_tid, 0, nu, 0, nullptr);
    __syncthreads();
  }
  if (tid < UB) {
    const float* p = evw_rows + tid * d;
    s_test[tid] = seq_dot(p, Q + (int64_t)s_tid[tid] * d, d);
    if (!USER) {
      float n2 = 0.f;
      for (int k = 0; k < d; ++k) n2 = n2 + p[k] * p[k];
      const float np = sqrtf(n2);
#pragma unroll
      for (int e = 0; e < EVW_MAX_EPS; ++e) s_thr[e][tid] = (2.f * eps.e[e]) * np;
    }
#pragma unroll
    for (int e = 0; e < EVW_MAX_EPS; ++e) s_cnt[e][tid] = 0;
  }
  int cnt[EVW_MAX_EPS][UB];
#pragma unroll
  for (int e = 0; e < EVW_MAX_EPS; ++e)
#pragma unroll
    for (int uu = 0; uu < UB; ++uu) cnt[e][uu] = 0;
  for (int64_t cc = c_begin; cc < c_end; cc += EVW_BM) {
    const int64_t ce = min(c_end, cc + EVW_BM);
    __syncthreads();  // the previous bitmap's reads (first pass: s_test, s_thr, s_cnt)
    sweep_excl_strided<UB, EVW_BM>(s_ex, s_eoff, nu, excl, cc, ce - cc);  // no lists: s_eoff is all 0
    if (tid < nu) {  // the test item never counts
      const int64_t w = (int64_t)s_tid[tid] - cc;
      if (w >= 0 && w < ce - cc) atomicOr(&s_ex[tid][w >> 5], 1u << (w & 31));
    }
    __syncthreads();
    for (int64_t cb = cc; cb < ce; cb += 256) {
      const bool live = cb + tid < ce;  // a lane past the end rescans the last candidate and counts nothing
      const int64_t c = live ? cb + tid : ce - 1;
      const float* q = Q + c * d;
      float acc[UB], d2[UB];
#pragma unroll
      for (int uu = 0; uu < UB; ++uu) acc[uu] = d2[uu] = 0.f;
      for (int k = 0; k < d; k += 4) {  // acc[uu] = seq_dot(row uu, q): the loop stays here (acf_sweep.h)
        const float4 qv = *reinterpret_cast<const float4*>(q + k);
#pragma unroll
        for (int uu = 0; uu < UB; ++uu) {
          acc[uu] = seq_step(acc[uu], *reinterpret_cast<const float4*>(evw_rows + uu * d + k), qv);
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
        const bool in = live && !((s_ex[uu][w >> 5] >> (w & 31)) & 1u);
        const float m = s_test[uu] - acc[uu];
        const float dist = USER ? sqrtf(d2[uu]) : 0.f;
#pragma unroll
        for (int e = 0; e < EVW_MAX_EPS; ++e) {
          if (e < eps.n) {
            const float thr = USER ? eps.e[e] * dist : s_thr[e][uu];
            cnt[e][uu] += __popcll(__ballot(in && m <= thr));  // the wave's count: the same in all its lanes
          }
        }
      }
    }
  }
  __syncthreads();  // s_cnt's zeros when no window ran
#pragma unroll
  for (int e = 0; e < EVW_MAX_EPS; ++e) {
    if (e < eps.n) {
#pragma unroll
      for (int uu = 0; uu < UB; ++uu)
        if (tid % EVW_WAVE == 0) atomicAdd(&s_cnt[e][uu], cnt[e][uu]);
    }
  }
  __syncthreads();
  if (tid < nu) {
    for (int e = 0; e < eps.n; ++e) dst[(int64_t)e * n_users + u0 + tid] = s_cnt[e][tid];
  }
}

// ---- host: strips and workspace (no device is touched) ------------------------
// As evx_strips, with n_eps counts per entry and strip.  The cut does not know d,
// so it counts tiles of EVW_UB entries whatever the kernel's tile.
constexpr size_t EVW_WS_HEAD = 16;  // the range-error flag, padded

static void evw_strips(int32_t n_users, int32_t num_cand, int32_t n_eps, int* wper, int* S) {
  sweep_strips(num_cand, EVW_WIN, n_users, EVW_UB, 2048, std::max<int64_t>(1, (int64_t)n_users * n_eps) * 4, wper, S);
}

static size_t evw_workspace(int32_t n_users, int32_t num_cand, int32_t n_eps) {
  int wper = 0, S = 0;
  evw_strips(n_users, num_cand, n_eps, &wper, &S);
  return EVW_WS_HEAD + (S > 1 ? (size_t)S * (size_t)n_users * (size_t)n_eps * sizeof(int32_t) : 0);
}
