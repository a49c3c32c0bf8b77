// List-level robustness kernels of libacf_apr.so (k_lst_*): how far two sets of
// top-K lists differ, and what a set of lists does to the items.  Included by
// acf_rank.hip after acf_eval_multi.h (evx_block_sum); one translation unit.
// DESIGN.md §4l.
#pragma once

#include <rocprim/device/device_radix_sort.hpp>

// A list array is int32 [n][k], row-major, 1 <= k <= LST_MAX_K, in the form
// acf_recommend_topk writes: a negative entry is "none" wherever it stands.
constexpr int LST_MAX_K = 128;   // = TOPK_MAX_K
constexpr int LST_MAX_CUT = 8;
constexpr int LST_WAVES = 4;     // rows per k_lst_compare workgroup, one wave each
constexpr int LST_NM = 3;        // overlap, jaccard, rbo
struct LstCuts {
  int32_t n;
  int32_t k[LST_MAX_CUT];
};

// ---------------------------------------------------------------------------
// list_compare: one wave per row, both rows in LDS.  Every valid A[i] looks for
// its place j in B (B is read as a broadcast); a match is counted in an integer
// LDS histogram at max(i, j), the depth from which the id is in both prefixes, so
// X_d = the number of ids in both A[0..d) and B[0..d) is the histogram's prefix
// sum: integers throughout.  Lane c then walks d = 1..D_c for cutoff c, adding
// (X_d / d) p^d in fp64, d ascending, p^d by repeated multiplication: one thread,
// one order, the same bits every run.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(64 * LST_WAVES) k_lst_compare(const int32_t* __restrict__ A,
                                                                const int32_t* __restrict__ B, int n, int k,
                                                                LstCuts cuts, double p, double* __restrict__ per_user,
                                                                uint8_t* __restrict__ scored) {
  __shared__ int32_t s_a[LST_WAVES][LST_MAX_K], s_b[LST_WAVES][LST_MAX_K], s_h[LST_WAVES][LST_MAX_K];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t r = blockIdx.x * (int64_t)LST_WAVES + w;
  const bool live = r < n;  // a wave past the end keeps the barriers company
  int la = 0, lb = 0;
  for (int x = lane; x < LST_MAX_K; x += 64) {
    int32_t a = -1, b = -1;
    if (live && x < k) {
      a = A[r * k + x];
      b = B[r * k + x];
    }
    s_a[w][x] = a;
    s_b[w][x] = b;
    s_h[w][x] = 0;
    la += __popcll(__ballot(a >= 0));
    lb += __popcll(__ballot(b >= 0));
  }
  __syncthreads();
  for (int i = lane; i < k; i += 64) {
    const int32_t a = s_a[w][i];
    if (a < 0) continue;
    for (int j = 0; j < k; ++j) {
      if (s_b[w][j] == a) {
        atomicAdd(&s_h[w][max(i, j)], 1);
        break;
      }
    }
  }
  __syncthreads();
  if (!live) return;
  const int longest = max(la, lb);
  if (lane == 0) scored[r] = longest > 0;
#pragma unroll
  for (int c = 0; c < LST_MAX_CUT; ++c) {
    if (lane != c || c >= cuts.n) continue;
    double* const o = per_user + (r * cuts.n + c) * LST_NM;
    const int D = min(cuts.k[c], longest);
    if (D == 0) {
      o[0] = o[1] = o[2] = 0.0;
      continue;
    }
    int X = 0;
    double pw = 1.0, sum = 0.0;
    for (int d = 1; d <= D; ++d) {
      X += s_h[w][d - 1];
      pw *= p;
      sum += ((double)X / (double)d) * pw;
    }
    o[0] = (double)X;
    o[1] = (double)X / (double)(min(la, D) + min(lb, D) - X);
    o[2] = ((double)X / (double)D) * pw + ((1.0 - p) / p) * sum;
  }
}

// workgroup q: the mean of column q of per_user [n][ncol] over the scored rows, by evx_block_sum's fixed
// tree (k_evx_means' pattern; an unscored row holds zeros and adds nothing); the first column of a cutoff
// also writes the cutoff's number of scored rows
__global__ void __launch_bounds__(256) k_lst_means(const double* __restrict__ per_user,
                                                   const uint8_t* __restrict__ scored, int n, int ncol,
                                                   double* __restrict__ mean, int64_t* __restrict__ n_scored) {
  __shared__ double s_red[256];
  __shared__ long long s_n[256];
  const int tid = threadIdx.x, q = blockIdx.x;
  double v = 0.0;
  long long cnt = 0;
  for (int64_t r = tid; r < n; r += 256) {
    if (!scored[r]) continue;
    v += per_user[r * ncol + q];
    ++cnt;
  }
  s_n[tid] = cnt;
  const double sum = evx_block_sum(v, s_red);  // its barriers cover s_n
  if (tid == 0) {
    long long total = 0;
    for (int i = 0; i < 256; ++i) total += s_n[i];
    mean[q] = total > 0 ? sum / (double)total : 0.0;
    if (q % LST_NM == 0) n_scored[q / LST_NM] = total;
  }
}

// ---------------------------------------------------------------------------
// list_exposure: counts[c][i] = #{(r, x) : x < K_c, lists[r][x] = i}.  A
// workgroup takes LSX_ROWS rows into LDS (coalesced; the rows padded by one word,
// so a column is read without bank conflicts) and each of its waves a position x,
// lane = row: the lanes of a wave that hold the same id are found by ballot and
// one of them adds their number.  When every user is recommended the same few
// items a counter therefore takes n / 64 integer atomics, not n; integer adds
// commute, so the counts are exact in any order.
// ---------------------------------------------------------------------------
constexpr int LSX_ROWS = 64;

__global__ void __launch_bounds__(256) k_lst_exposure(const int32_t* __restrict__ lists, int n, int k, int num_items,
                                                      LstCuts cuts, int32_t* __restrict__ counts) {
  __shared__ int32_t s_t[LSX_ROWS][LST_MAX_K + 1];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t r0 = blockIdx.x * (int64_t)LSX_ROWS;
  const int rows = (int)min((int64_t)LSX_ROWS, n - r0);
  const int32_t* src = lists + r0 * k;
  for (int e = tid; e < rows * k; e += 256) s_t[e / k][e % k] = src[e];
  __syncthreads();
  int kmax = 0;
#pragma unroll
  for (int c = 0; c < LST_MAX_CUT; ++c) kmax = max(kmax, c < cuts.n ? cuts.k[c] : 0);
  for (int x = w; x < min(k, kmax); x += 4) {
    const int32_t id = lane < rows ? s_t[lane][x] : -1;
    const bool valid = id >= 0 && id < num_items;
    unsigned long long todo = __ballot(valid);
    while (todo) {  // wave-uniform: every pass retires all lanes of one id
      const int lead = __ffsll(todo) - 1;
      const int32_t lid = __shfl(id, lead);
      const unsigned long long same = __ballot(valid && id == lid);
      if (lane == lead) {
        const int cnt = __popcll(same);
#pragma unroll
        for (int c = 0; c < LST_MAX_CUT; ++c)
          if (c < cuts.n && x < cuts.k[c]) atomicAdd(&counts[(int64_t)c * num_items + lid], cnt);
      }
      todo &= ~same;
    }
  }
}

// ---------------------------------------------------------------------------
// exposure_metrics: per cutoff, of the counts c_i and the same counts sorted
// ascending (rocPRIM's device radix sort): T, #{c_i > 0}, G = sum_j (2j - N - 1)
// c_(j), sum c_i pop_i and sum_{tail} c_i as int64 (integer sums: exact whatever
// the order), then the entropy terms in fp64 given T.  The item range is cut into
// B = lsm_blocks(N) slices, a function of N alone; a slice is summed by its
// workgroup (thread-strided, then a fixed tree) and the slices by one workgroup in
// slice order, so the fp64 sum has one order on every device.
// ---------------------------------------------------------------------------
constexpr int LSM_INTS = 5;  // T, covered, G, arp numerator, tail numerator
constexpr int LSM_NM = 6;    // total, coverage, gini, entropy, arp, aplt

static int lsm_blocks(int64_t N) { return (int)std::min<int64_t>(256, (N + 255) / 256); }

// the sum of v over the workgroup in thread 0 (a fixed tree over s_red[256])
__device__ __forceinline__ long long lsm_block_sum(long long v, long long* s_red) {
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

// grid (B, n_cutoffs): part[c][b][LSM_INTS]
__global__ void __launch_bounds__(256) k_lst_expo_ints(const int32_t* __restrict__ counts,
                                                       const uint32_t* __restrict__ sorted, int64_t N,
                                                       const int32_t* __restrict__ pop,
                                                       const uint8_t* __restrict__ tail,
                                                       long long* __restrict__ part) {
  __shared__ long long s_red[256];
  const int tid = threadIdx.x, b = blockIdx.x, c = blockIdx.y;
  const int32_t* cc = counts + c * N;
  const uint32_t* sc = sorted + c * N;
  long long v[LSM_INTS] = {0, 0, 0, 0, 0};
  for (int64_t i = b * 256 + tid; i < N; i += (int64_t)gridDim.x * 256) {
    const long long ci = cc[i];
    v[0] += ci;
    v[1] += ci > 0;
    v[2] += (2 * (i + 1) - N - 1) * (long long)sc[i];
    if (pop) v[3] += ci * pop[i];
    if (tail && tail[i]) v[4] += ci;
  }
  long long* const o = part + ((int64_t)c * gridDim.x + b) * LSM_INTS;
  for (int m = 0; m < LSM_INTS; ++m) {
    const long long s = lsm_block_sum(v[m], s_red);
    if (tid == 0) o[m] = s;
  }
}

// grid (B, n_cutoffs): epart[c][b] = the slice's sum of (c_i / T) log2(c_i / T) over c_i > 0
__global__ void __launch_bounds__(256) k_lst_expo_entropy(const int32_t* __restrict__ counts, int64_t N,
                                                          const long long* __restrict__ part,
                                                          double* __restrict__ epart) {
  __shared__ double s_red[256];
  const int tid = threadIdx.x, b = blockIdx.x, c = blockIdx.y;
  long long T = 0;
  for (int x = 0; x < (int)gridDim.x; ++x) T += part[((int64_t)c * gridDim.x + x) * LSM_INTS];
  const int32_t* cc = counts + c * N;
  double v = 0.0;
  for (int64_t i = b * 256 + tid; i < N; i += (int64_t)gridDim.x * 256) {
    const int32_t ci = cc[i];
    if (ci <= 0) continue;
    const double f = (double)ci / (double)T;
    v += f * log2(f);
  }
  const double s = evx_block_sum(v, s_red);
  if (tid == 0) epart[(int64_t)c * gridDim.x + b] = s;
}

// workgroup c: the slices in order, then out[c][LSM_NM]
__global__ void __launch_bounds__(256) k_lst_expo_final(const long long* __restrict__ part,
                                                        const double* __restrict__ epart, int B, int64_t N,
                                                        double* __restrict__ out) {
  if (threadIdx.x != 0) return;  // at most 256 slices: one thread, one order
  const int c = blockIdx.x;
  long long v[LSM_INTS] = {0, 0, 0, 0, 0};
  double e = 0.0;
  for (int b = 0; b < B; ++b) {
    for (int m = 0; m < LSM_INTS; ++m) v[m] += part[((int64_t)c * B + b) * LSM_INTS + m];
    e += epart[(int64_t)c * B + b];
  }
  double* const o = out + c * LSM_NM;
  const long long T = v[0];
  if (T <= 0) {
    for (int m = 0; m < LSM_NM; ++m) o[m] = 0.0;
    return;
  }
  o[0] = (double)T;
  o[1] = (double)v[1] / (double)N;
  o[2] = (double)v[2] / (double)(N * T);
  o[3] = 0.0 - e;
  o[4] = (double)v[3] / (double)T;
  o[5] = (double)v[4] / (double)T;
}

// ---- host: the workspace of exposure_metrics (no device is touched) ----------
// the sorted counts of every cutoff, the integer partial sums, the entropy partial sums
struct LsmLayout {
  size_t sorted, part, epart, total;
};

static LsmLayout lsm_layout(int64_t N, int n_cut) {
  const auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t B = (size_t)lsm_blocks(N);
  LsmLayout L;
  L.sorted = 0;
  L.part = up((size_t)n_cut * (size_t)N * sizeof(uint32_t));
  L.epart = L.part + up((size_t)n_cut * B * LSM_INTS * sizeof(long long));
  L.total = L.epart + up((size_t)n_cut * B * sizeof(double));
  return L;
}
