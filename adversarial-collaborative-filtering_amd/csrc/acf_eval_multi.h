// Multi-item all-items evaluation kernels of libacf_apr.so (k_evx_*): included by
// acf_rank.hip after acf_sweep.h (seq_dot, the shared sweep pieces); one
// translation unit.  DESIGN.md §4f.
#pragma once

// ---------------------------------------------------------------------------
// eval_positions_multi: entry r (row users[r] of P) has the test list
// test_items[test_off[r] .. test_off[r+1]); for each of its items t
//   positions[x] = #{ c in C_r, c != t : seq_dot(p, Q[c]) >= seq_dot(p, Q[t]) },
// C_r = [0, num_cand) minus the SET of r's exclusion entries.  One sweep of the
// candidates serves a whole chunk of EVX_CH test items: the chunk's test scores
// are sorted ascending in LDS, every candidate score s is placed by a binary
// search at b = (number of test scores <= s) - 1 (skipped after one compare
// when it is below the lowest) and counted in an integer LDS histogram, and the
// suffix sums of the histogram are the counts: slot k's test item is reached by
// every candidate placed at b >= k.  The comparisons are float <= / >= on
// seq_dot scores, so ties are decided on equal bits exactly as in k_eval_all.
// The test item itself is a candidate like any other during the sweep; where it
// was counted (in range and not excluded) 1 is taken off its own count.
//
// The candidate range is cut into strips of whole EVX_WIN-candidate windows
// (grid.y); a strip writes its partial counts to out + strip * n_tests (the
// caller's workspace, or positions itself when there is one strip) and
// k_evx_sum adds the strips.  Only integer LDS atomics; no float is ever
// accumulated across threads, so the result has the same bits every run.
// ---------------------------------------------------------------------------
constexpr int EVX_UB = 8;      // entries per workgroup (as k_eval_all)
constexpr int EVX_CH = 256;    // test items per chunk (= the workgroup size)
constexpr int EVX_WIN = 256;   // candidates per window; strips are whole windows
constexpr int EVX_BM = 2048;   // candidates per exclusion bitmap

__global__ void __launch_bounds__(256) k_evx_sweep(const float* __restrict__ P, const float* __restrict__ Q, int d,
                                                   int64_t U1, int64_t I1, const int32_t* __restrict__ users,
                                                   const int64_t* __restrict__ test_off,
                                                   const int32_t* __restrict__ test_items, int n_users,
                                                   int64_t n_tests, int num_cand,
                                                   const int64_t* __restrict__ excl_off,
                                                   const int32_t* __restrict__ excl, int wper,
                                                   int32_t* __restrict__ out, int32_t* __restrict__ err) {
  extern __shared__ float evx_rows[];      // [EVX_UB][d]
  __shared__ float s_ts[EVX_UB][EVX_CH];   // the chunk's test scores, ascending
  __shared__ int s_hist[EVX_UB][EVX_CH];   // first the unsorted scores' bits, then the histogram
  __shared__ uint16_t s_ord[EVX_UB][EVX_CH];  // sorted slot -> index within the chunk
  __shared__ uint8_t s_self[EVX_UB][EVX_CH];  // by index within the chunk: the item was counted itself
  __shared__ uint32_t s_ex[EVX_UB][EVX_BM / 32];
  __shared__ int64_t s_toff[EVX_UB + 1], s_eoff[EVX_UB + 1];
  const int tid = threadIdx.x, strip = blockIdx.y;
  const int u0 = blockIdx.x * EVX_UB;
  const int nu = min(EVX_UB, n_users - u0);
  const int64_t c_begin = (int64_t)strip * wper * EVX_WIN;
  const int64_t c_end = min((int64_t)num_cand, c_begin + (int64_t)wper * EVX_WIN);
  int32_t* const dst = out + (int64_t)strip * n_tests;
  sweep_load_rows<EVX_UB, true>(evx_rows, P, d, users, u0, nu, U1, err);  // reported when the caller checks
  if (tid <= EVX_UB) {
    const int r = min(tid, nu);  // entries past the tile repeat its end: empty lists
    s_toff[tid] = min(max(test_off[u0 + r], (int64_t)0), n_tests);
    s_eoff[tid] = excl_off ? excl_off[u0 + r] : 0;
  }
  __syncthreads();
  int64_t maxm = 0;
#pragma unroll
  for (int uu = 0; uu < EVX_UB; ++uu) maxm = max(maxm, s_toff[uu + 1] - s_toff[uu]);
  for (int64_t base = 0; base < maxm; base += EVX_CH) {
    int mc[EVX_UB];  // the entries' chunk lengths
#pragma unroll
    for (int uu = 0; uu < EVX_UB; ++uu)
      mc[uu] = (int)min((int64_t)EVX_CH, max((int64_t)0, s_toff[uu + 1] - s_toff[uu] - base));
    __syncthreads();  // the previous chunk's reads
    // test scores (thread j: item j of every entry's chunk), unsorted, as bits
#pragma unroll
    for (int uu = 0; uu < EVX_UB; ++uu) {
      s_self[uu][tid] = 0;
      if (tid < mc[uu]) {
        int64_t t = test_items[s_toff[uu] + base + tid];
        if (t < 0 || t >= I1) {
          t = 0;
          atomicOr(err, 2);
        }
        s_hist[uu][tid] = __float_as_int(seq_dot(evx_rows + uu * d, Q + t * d, d));
      }
    }
    __syncthreads();
    // rank sort: ascending by score, equal scores by index
    float mine[EVX_UB];
    int rank[EVX_UB];
#pragma unroll
    for (int uu = 0; uu < EVX_UB; ++uu) {
      rank[uu] = 0;
      if (tid < mc[uu]) {
        const float v = __int_as_float(s_hist[uu][tid]);
        mine[uu] = v;
        int rk = 0;
        for (int i = 0; i < mc[uu]; ++i) {
          const float o = __int_as_float(s_hist[uu][i]);
          rk += (o < v || (o == v && i < tid)) ? 1 : 0;
        }
        rank[uu] = rk;
      }
    }
    __syncthreads();
#pragma unroll
    for (int uu = 0; uu < EVX_UB; ++uu) {
      s_hist[uu][tid] = 0;
      if (tid < mc[uu]) {
        s_ts[uu][rank[uu]] = mine[uu];
        s_ord[uu][rank[uu]] = (uint16_t)tid;
      }
    }
    // the sweep of this strip
    for (int64_t cc = c_begin; cc < c_end; cc += EVX_BM) {
      const int64_t ce = min(c_end, cc + EVX_BM);
      __syncthreads();  // the previous bitmap's reads (first pass: the sorted scores' writes)
      sweep_excl_strided<EVX_UB, EVX_BM>(s_ex, s_eoff, nu, excl, cc, ce - cc);  // no lists: s_eoff is all 0
      __syncthreads();
      // a test item inside this bitmap that is not excluded counts itself below
#pragma unroll
      for (int uu = 0; uu < EVX_UB; ++uu) {
        if (tid < mc[uu]) {
          int64_t t = test_items[s_toff[uu] + base + tid];
          if (t < 0 || t >= I1) t = 0;
          const int64_t w = t - cc;
          if (w >= 0 && w < ce - cc && !((s_ex[uu][w >> 5] >> (w & 31)) & 1u)) s_self[uu][tid] = 1;
        }
      }
      for (int64_t cb = cc; cb < ce; cb += 256) {
        const int64_t c = cb + tid;
        if (c >= ce) continue;
        const float* q = Q + c * d;
        float acc[EVX_UB];
#pragma unroll
        for (int uu = 0; uu < EVX_UB; ++uu) acc[uu] = 0.f;
        for (int k = 0; k < d; k += 4) {  // acc[uu] = seq_dot(row uu, q): the loop stays here (acf_sweep.h)
          const float4 qv = *reinterpret_cast<const float4*>(q + k);
#pragma unroll
          for (int uu = 0; uu < EVX_UB; ++uu)
            acc[uu] = seq_step(acc[uu], *reinterpret_cast<const float4*>(evx_rows + uu * d + k), qv);
        }
        const int w = (int)(c - cc);
#pragma unroll
        for (int uu = 0; uu < EVX_UB; ++uu) {
          if (mc[uu] == 0 || ((s_ex[uu][w >> 5] >> (w & 31)) & 1u)) continue;
          const float s = acc[uu];
          if (!(s >= s_ts[uu][0])) continue;  // below every test score of the chunk
          int lo = 0, hi = mc[uu];            // the last slot whose score is <= s
          while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (s_ts[uu][mid] <= s) lo = mid; else hi = mid;
          }
          atomicAdd(&s_hist[uu][lo], 1);
        }
      }
    }
    // suffix sums of the histograms (slot tid of every entry), then the counts
    for (int off = 1; off < EVX_CH; off <<= 1) {
      __syncthreads();
      int v[EVX_UB];
#pragma unroll
      for (int uu = 0; uu < EVX_UB; ++uu) v[uu] = tid + off < EVX_CH ? s_hist[uu][tid + off] : 0;
      __syncthreads();
#pragma unroll
      for (int uu = 0; uu < EVX_UB; ++uu) s_hist[uu][tid] += v[uu];
    }
    __syncthreads();
#pragma unroll
    for (int uu = 0; uu < EVX_UB; ++uu) {
      if (tid < mc[uu]) {
        const int j = s_ord[uu][tid];
        dst[s_toff[uu] + base + j] = s_hist[uu][tid] - (int)s_self[uu][j];
      }
    }
  }
}

// positions[x] = the sum of the strips' partial counts, in strip order
__global__ void __launch_bounds__(256) k_evx_sum(const int32_t* __restrict__ part, int S, int64_t n_tests,
                                                 int32_t* __restrict__ positions) {
  const int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (x >= n_tests) return;
  int32_t s = 0;
  for (int k = 0; k < S; ++k) s += part[(int64_t)k * n_tests + x];
  positions[x] = s;
}

// ---- host: strips and workspace (no device is touched) ------------------------
// Windows per strip and the number of strips S: enough strips that the grid
// fills the device when there are few entries (3 entries x 70,000 candidates:
// 1 tile x 274 strips), no more than there are windows, and few enough that the
// partial counts (S * n_tests int32) stay under 48 MiB.
constexpr size_t EVX_WS_HEAD = 16;  // the range-error flag, padded

static void evx_strips(int32_t n_users, int64_t n_tests, int32_t num_cand, int* wper, int* S) {
  sweep_strips(num_cand, EVX_WIN, n_users, EVX_UB, 2048, std::max<int64_t>(1, n_tests) * 4, wper, S);
}

static size_t evx_workspace(int32_t n_users, int64_t n_tests, int32_t num_cand) {
  int wper = 0, S = 0;
  evx_strips(n_users, n_tests, num_cand, &wper, &S);
  return EVX_WS_HEAD + (S > 1 ? (size_t)S * (size_t)n_tests * sizeof(int32_t) : 0);
}

// ---------------------------------------------------------------------------
// rank_metrics: ranking metrics of the integer positions, in fp64.  A workgroup
// per user: item x's j is the number of the user's entries with a smaller
// position, or an equal position and a smaller index (an O(m^2) count, any m);
// every thread adds its items' terms in index order and the 256 partial sums
// are added by a fixed tree, so equal inputs give equal bits.  k_evx_means sums
// one output column per workgroup over the users in the same way.
// Per user and cutoff: hit, recall, precision, ndcg, map; per user: mrr, auc.
// ---------------------------------------------------------------------------
constexpr int EVX_MAX_CUT = 8, EVX_MAX_K = 1024, EVX_NM = 5;
struct EvxCuts {
  int32_t n;
  int32_t k[EVX_MAX_CUT];
};

// the sum of v over the workgroup, in every thread (a fixed tree over s_red[256])
__device__ __forceinline__ double evx_block_sum(double v, double* s_red) {
  const int tid = threadIdx.x;
  __syncthreads();  // the previous sum's reads
  s_red[tid] = v;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) s_red[tid] += s_red[tid + off];
    __syncthreads();
  }
  return s_red[0];
}

__global__ void __launch_bounds__(256) k_evx_metrics(const int32_t* __restrict__ positions,
                                                     const int64_t* __restrict__ test_off,
                                                     const int32_t* __restrict__ n_neg, EvxCuts cuts,
                                                     double* __restrict__ per_user,
                                                     double* __restrict__ per_user_free) {
  __shared__ double s_red[256];
  __shared__ double s_disc[EVX_MAX_K];  // 1 / log2(i + 2), i < min(m, Kmax)
  __shared__ int s_min[256];
  const int tid = threadIdx.x;
  const int64_t u = blockIdx.x;
  const int64_t a0 = test_off[u], m = test_off[u + 1] - a0;
  double* const pu = per_user + u * cuts.n * EVX_NM;
  if (m <= 0) {
    for (int x = tid; x < cuts.n * EVX_NM; x += 256) pu[x] = 0.0;
    if (tid < 2) per_user_free[u * 2 + tid] = 0.0;
    return;
  }
  const int32_t* pos = positions + a0;
  int kmax = 0;
  for (int c = 0; c < cuts.n; ++c) kmax = max(kmax, cuts.k[c]);
  const int nd = (int)min((int64_t)kmax, m);
  for (int i = tid; i < nd; i += 256) s_disc[i] = 1.0 / log2((double)i + 2.0);
  double cnt[EVX_MAX_CUT], dcg[EVX_MAX_CUT], ap[EVX_MAX_CUT], auc = 0.0;
#pragma unroll
  for (int c = 0; c < EVX_MAX_CUT; ++c) cnt[c] = dcg[c] = ap[c] = 0.0;
  int rmin = INT_MAX;
  const double nn = (double)n_neg[u];
  for (int64_t x = tid; x < m; x += 256) {
    const int32_t r = pos[x];
    int64_t j = 0;
    for (int64_t y = 0; y < m; ++y) {
      const int32_t o = pos[y];
      j += (o < r || (o == r && y < x)) ? 1 : 0;
    }
    rmin = min(rmin, r);
    auc += 1.0 - ((double)r - (double)j) / nn;
    const double disc = 1.0 / log2((double)r + 2.0), prec = ((double)j + 1.0) / ((double)r + 1.0);
#pragma unroll
    for (int c = 0; c < EVX_MAX_CUT; ++c) {
      if (c < cuts.n && r < cuts.k[c]) {
        cnt[c] += 1.0;
        dcg[c] += disc;
        ap[c] += prec;
      }
    }
  }
  s_min[tid] = rmin;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) s_min[tid] = min(s_min[tid], s_min[tid + off]);
    __syncthreads();
  }
  const int r0 = s_min[0];
  const double auc_s = evx_block_sum(auc, s_red);
  if (tid == 0) {
    per_user_free[u * 2] = 1.0 / ((double)r0 + 1.0);
    per_user_free[u * 2 + 1] = auc_s / (double)m;
  }
  for (int c = 0; c < cuts.n; ++c) {
    const double cnt_s = evx_block_sum(cnt[c], s_red);
    const double dcg_s = evx_block_sum(dcg[c], s_red);
    const double ap_s = evx_block_sum(ap[c], s_red);
    if (tid == 0) {
      const int K = cuts.k[c], top = (int)min((int64_t)K, m);
      double idcg = 0.0;
      for (int i = 0; i < top; ++i) idcg += s_disc[i];
      pu[c * EVX_NM + 0] = r0 < K ? 1.0 : 0.0;
      pu[c * EVX_NM + 1] = cnt_s / (double)m;
      pu[c * EVX_NM + 2] = cnt_s / (double)K;
      pu[c * EVX_NM + 3] = dcg_s / idcg;
      pu[c * EVX_NM + 4] = ap_s / (double)top;
    }
  }
}

// workgroup q: the mean of column q of [per_user | per_user_free] over the users
// with a non-empty list; workgroup 0 also writes their number
__global__ void __launch_bounds__(256) k_evx_means(const double* __restrict__ per_user,
                                                   const double* __restrict__ per_user_free,
                                                   const int64_t* __restrict__ test_off, int n_users, int ncol,
                                                   double* __restrict__ mean_cut, double* __restrict__ mean_free,
                                                   int64_t* __restrict__ n_scored) {
  __shared__ double s_red[256];
  __shared__ long long s_n[256];
  const int tid = threadIdx.x, q = blockIdx.x;
  const bool cut = q < ncol;
  const double* src = cut ? per_user + q : per_user_free + (q - ncol);
  const int stride = cut ? ncol : 2;
  double v = 0.0;
  long long n = 0;
  for (int64_t u = tid; u < n_users; u += 256) {
    if (test_off[u + 1] - test_off[u] <= 0) continue;
    v += src[u * stride];
    ++n;
  }
  s_n[tid] = n;
  const double sum = evx_block_sum(v, s_red);  // its barriers cover s_n
  if (tid == 0) {
    long long total = 0;
    for (int i = 0; i < 256; ++i) total += s_n[i];
    const double mean = total > 0 ? sum / (double)total : 0.0;
    if (cut) mean_cut[q] = mean; else mean_free[q - ncol] = mean;
    if (q == 0) *n_scored = total;
  }
}
