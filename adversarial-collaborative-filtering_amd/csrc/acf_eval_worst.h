// The margin sweep of the certified evaluations (k_cert_sweep) and its counting
// sink, certified worst-case positions under an eps attack (CertCount): included
// by acf_rank.hip after acf_eval_multi.h (acf_sweep.h's pieces, k_evx_sum); one
// translation unit.  The selecting sink is acf_eval_radius.h.  DESIGN.md §4g.
#pragma once

// ---------------------------------------------------------------------------
// The frame.  Entry r has the user row p = P[users[r]], the test item t =
// test_items[r] and the candidates C_r = [0, num_cand) minus the SET of its
// exclusion entries, minus t.  For every pair (r, c in C_r) the sweep hands its
// sink
//   m_c  = seq_dot(p, Q[t]) - seq_dot(p, Q[c])
//   base = D_c = sqrtf(D2), D2 = the sum over k ascending from +0.0 of
//          round((Q[t][k] - Q[c][k])^2)                          (side user)
//   base = Np = sqrtf(the same chain over p[k]^2)                (side item)
// all of it fp32, every operation rounded on its own (-ffp-contract=off), the
// square roots correctly rounded, and the one predicate both sinks decide by:
//   cert_pred(m, e, base) = m <= e * base (user), m <= (2 e) * base (item).
// No single perturbation within the budget e (|delta|_2 <= e on the user row; on
// every item row) can put c at or above t unless cert_pred holds.
//
// A VALU sweep like k_evx_sweep: a workgroup of 256 holds UB entries' user rows
// in LDS (side user: their test items' rows as well), one candidate per lane and
// step of 256, its score out of seq_step.  The exclusion bitmap covers 2,048
// candidates; t is kept out by setting its own bit.  A strip of the candidate
// range (grid.y) is a whole number of 256-candidate windows.  Every lane stays
// in the loop to the end of a window, so that a sink may ballot: a lane past the
// end rescans the last candidate and hands its sink in = false, as do excluded
// pairs and the tile's entries past n_users (zero rows).
//
// A sink owns its kernel arguments (Args), its static LDS (Lds), KEYS 64-bit
// slots of dynamic LDS in front of the rows, and four hooks: init (thread uu <
// UB, before the first barrier), pair, step (all threads, after each 256
// candidates; it brings the barriers it needs) and finish (all threads, after a
// barrier).  Integer LDS atomics only, no float accumulated across threads:
// equal inputs give equal bits.
//
// LDS: UB = 8 entries per workgroup up to d = 512, 4 above, so the rows take at
// most 2 * 8 * 512 * 4 = 2 * 4 * 1024 * 4 = 32 KB (side item: half of that),
// the bitmap 2 KB and the rest under 1 KB.
// ---------------------------------------------------------------------------
constexpr int EVW_MAX_EPS = 8;
constexpr int EVW_WIN = 256;   // candidates per window; strips are whole windows
constexpr int EVW_BM = 2048;   // candidates per exclusion bitmap
constexpr int EVW_UB = 8;      // entries per workgroup (4 above d = 512); the strip cuts count tiles of 8
constexpr int EVW_D_SPLIT = 512;
constexpr int EVW_WAVE = 64;   // lanes per wave (gfx950): a wave counts with one ballot

template <bool USER>
__device__ __forceinline__ bool cert_pred(float m, float e, float base) {
  return USER ? m <= e * base : m <= (2.f * e) * base;
}

template <int UB, bool USER, class SINK>
__global__ void __launch_bounds__(256) k_cert_sweep(const float* __restrict__ P, const float* __restrict__ Q, int d,
                                                    int64_t U1, int64_t I1, const int32_t* __restrict__ users,
                                                    const int32_t* __restrict__ test_items, int n_users,
                                                    int num_cand, const int64_t* __restrict__ excl_off,
                                                    const int32_t* __restrict__ excl, int wper,
                                                    typename SINK::Args args, int32_t* __restrict__ err) {
  // the sink's keys, [UB][d] user rows, (USER) [UB][d] test-item rows
  extern __shared__ __attribute__((aligned(16))) uint64_t cert_smem[];
  float* const rows = reinterpret_cast<float*>(cert_smem + SINK::KEYS);
  float* const trows = rows + UB * d;
  __shared__ float s_test[UB];   // seq_dot(p, Q[t])
  __shared__ float s_np[UB];     // side item: Np
  __shared__ int32_t s_tid[UB];  // the test items, range-checked
  __shared__ uint32_t s_ex[UB][EVW_BM / 32];
  __shared__ int64_t s_eoff[UB + 1];
  __shared__ typename SINK::Lds s_sink;
  const int tid = threadIdx.x, strip = blockIdx.y;
  const int u0 = blockIdx.x * UB;
  const int nu = min(UB, n_users - u0);
  const int64_t c_begin = (int64_t)strip * wper * EVW_WIN;
  const int64_t c_end = min((int64_t)num_cand, c_begin + (int64_t)wper * EVW_WIN);
  SINK sink(args, s_sink, cert_smem);
  sweep_load_rows<UB, true>(rows, P, d, users, u0, nu, U1, err);  // reported when the caller checks
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
    const float* p = rows + tid * d;
    s_test[tid] = seq_dot(p, Q + (int64_t)s_tid[tid] * d, d);
    if (!USER) {
      float n2 = 0.f;
      for (int k = 0; k < d; ++k) n2 = n2 + p[k] * p[k];
      s_np[tid] = sqrtf(n2);
    }
    sink.init(tid);
  }
  for (int64_t cc = c_begin; cc < c_end; cc += EVW_BM) {
    const int64_t ce = min(c_end, cc + EVW_BM);
    __syncthreads();  // the previous bitmap's reads (first pass: s_test, s_np, the sink's init)
    sweep_excl_strided<UB, EVW_BM>(s_ex, s_eoff, nu, excl, cc, ce - cc);  // no lists: s_eoff is all 0
    if (tid < nu) {  // the test item never counts
      const int64_t w = (int64_t)s_tid[tid] - cc;
      if (w >= 0 && w < ce - cc) atomicOr(&s_ex[tid][w >> 5], 1u << (w & 31));
    }
    __syncthreads();
    for (int64_t cb = cc; cb < ce; cb += 256) {
      const bool live = cb + tid < ce;  // a lane past the end rescans the last candidate: in = false
      const int64_t c = live ? cb + tid : ce - 1;
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
        const bool in = live && uu < nu && !((s_ex[uu][w >> 5] >> (w & 31)) & 1u);
        sink.template pair<USER>(uu, in, s_test[uu] - acc[uu], USER ? sqrtf(d2[uu]) : s_np[uu], (int32_t)c);
      }
      sink.step();
    }
  }
  __syncthreads();  // the sink's init when no window ran
  sink.finish(u0, nu, n_users, strip);
}

// ---------------------------------------------------------------------------
// The counting sink, eval_positions_worst:
//   worst[e][r] = #{ c in C_r : cert_pred(m_c, eps_e, base) }
// so no single perturbation within eps_e can put more than worst[e][r]
// candidates at or above t.  At eps = 0 the predicate is seq_dot(p, Q[c]) >=
// seq_dot(p, Q[t]) exactly (x - y <= 0 iff x <= y: fp32 subtraction keeps
// denormals), so the row equals k_eval_all's positions.  Every eps of the call
// is compared against the same m and base, so the candidates are swept once
// whatever their number.  A wave counts a predicate with one ballot, so the
// counts are wave-uniform ints, added per workgroup by one lane of each wave; a
// strip writes its counts to out + strip * n_eps * n_users (the caller's
// workspace, or worst itself when there is one strip) and k_evx_sum adds the
// strips in strip order.
// ---------------------------------------------------------------------------
struct EvwEps {
  int32_t n;
  float e[EVW_MAX_EPS];
};

struct CertCountArgs {
  EvwEps eps;
  int32_t* out;
};

template <int UB>
struct CertCount {
  static constexpr int KEYS = 0;
  using Args = CertCountArgs;
  struct Lds {
    int cnt[EVW_MAX_EPS][UB];
  };
  const Args& a;
  Lds& l;
  int cnt[EVW_MAX_EPS][UB];  // this wave's counts: the same in all its lanes

  __device__ __forceinline__ CertCount(const Args& a_, Lds& l_, uint64_t*) : a(a_), l(l_) {
#pragma unroll
    for (int e = 0; e < EVW_MAX_EPS; ++e)
#pragma unroll
      for (int uu = 0; uu < UB; ++uu) cnt[e][uu] = 0;
  }
  __device__ __forceinline__ void init(int uu) {
#pragma unroll
    for (int e = 0; e < EVW_MAX_EPS; ++e) l.cnt[e][uu] = 0;
  }
  template <bool USER>
  __device__ __forceinline__ void pair(int uu, bool in, float m, float base, int32_t) {
#pragma unroll
    for (int e = 0; e < EVW_MAX_EPS; ++e)
      if (e < a.eps.n) cnt[e][uu] += __popcll(__ballot(in && cert_pred<USER>(m, a.eps.e[e], base)));
  }
  __device__ __forceinline__ void step() {}
  __device__ __forceinline__ void finish(int u0, int nu, int n_users, int strip) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int e = 0; e < EVW_MAX_EPS; ++e) {
      if (e < a.eps.n) {
#pragma unroll
        for (int uu = 0; uu < UB; ++uu)
          if (tid % EVW_WAVE == 0) atomicAdd(&l.cnt[e][uu], cnt[e][uu]);
      }
    }
    __syncthreads();
    int32_t* const dst = a.out + (int64_t)strip * a.eps.n * n_users;
    if (tid < nu) {
      for (int e = 0; e < a.eps.n; ++e) dst[(int64_t)e * n_users + u0 + tid] = l.cnt[e][tid];
    }
  }
};

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
