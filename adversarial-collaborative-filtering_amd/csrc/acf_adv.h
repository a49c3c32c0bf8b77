// Whole-stream adversarial direction kernels of libacf_apr.so (k_adv_*): included
// by acf_rank.hip after acf_topk.h (seq_dot; bpr_term, random_delta and the row
// helpers); one translation unit.  DESIGN.md §4c.
//
// acf_adv_direction, grad mode: the clean-loss gradient of ALL n triplets as one
// batch (utils.py:145-154), summed per table row and l2-normalised.  Every
// triplet contributes four terms, numbered e in [0, 4n) in the concat order of
// the reference's IndexedSlices (pos branch, then neg branch):
//   e in [0, n)    row user[e]       of P:  +g_e * Q[ipos[e]]
//   e in [n, 2n)   row user[e-n]     of P:  -g   * Q[ineg[e-n]]
//   e in [2n, 3n)  row ipos[e-2n]    of Q:  +g   * P[user[e-2n]]
//   e in [3n, 4n)  row ineg[e-3n]    of Q:  -g   * P[user[e-3n]]
// A row's terms are summed in ascending e: the sum never depends on scheduling.
//   1. k_adv_keys: the term keys (user row r -> r, item row r -> U1 + r) and
//      values e; k_adv_coef: g per triplet (seq_dot scores, the step's bpr_term);
//   2. a stable LSD radix sort of (key, e) on 8-bit digits (k_adv_hist, the
//      three k_adv_scan* passes, k_adv_reorder), so the terms of a row lie
//      together in ascending e;
//   3. k_adv_offsets: first term of every row; k_adv_records: (partner row,
//      signed g) per sorted term;
//   4. k_adv_chunks: one lane-group per ADV_CHUNK consecutive terms of a row,
//      summed in order; a row of one chunk is normalised and written at once,
//      a longer row's chunk sums go to the workspace;
//   5. k_adv_combine: one lane-group per long row adds its chunk sums in chunk
//      order, normalises and writes.
// No float atomics anywhere (the histogram's integer LDS atomics give counts).
// Stages 1 (keys), 2 and k_adv_offsets read the triplets alone: acf_adv_plan keeps
// their result (sorted e, offsets, error word), acf_adv_direction_planned runs the
// rest on it, acf_adv_pgd iterates that with k_adv_pgd_step.  DESIGN.md §4k.
#pragma once

#include <rocprim/block/block_reduce.hpp>

constexpr int ADV_CHUNK = 256;  // terms per chunk sum: part of the bit contract, not a knob
constexpr int ADV_SORT_BS = 256;
constexpr int ADV_SORT_IPT = 8;
constexpr int ADV_TILE = ADV_SORT_BS * ADV_SORT_IPT;  // terms per sort workgroup
constexpr int ADV_SCAN_IPT = 4;
constexpr int ADV_SCAN_TILE = 256 * ADV_SCAN_IPT;  // counters per k_adv_scan1/3 workgroup

__device__ __forceinline__ int32_t adv_clamp(int32_t x, int64_t rows) { return (x < 0 || x >= rows) ? 0 : x; }

// ---- 1. term keys (the plan's part), per-triplet coefficient -------------------
// Reads the triplets only: whatever the tables hold, the keys, the sort and the
// offsets are the same, so a plan (acf_adv_plan) serves every table pair.
__global__ void __launch_bounds__(256) k_adv_keys(const int32_t* __restrict__ user, const int32_t* __restrict__ ipos,
                                                  const int32_t* __restrict__ ineg, int64_t n, int64_t U1, int64_t I1,
                                                  uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                  int32_t* __restrict__ err) {
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (t >= n) return;
  int32_t u = user[t], i = ipos[t], j = ineg[t];
  if (u < 0 || u >= U1) { atomicOr(err, 1); u = 0; }
  if (i < 0 || i >= I1) { atomicOr(err, 2); i = 0; }
  if (j < 0 || j >= I1) { atomicOr(err, 2); j = 0; }
  keys[t] = (uint32_t)u;
  keys[n + t] = (uint32_t)u;
  keys[2 * n + t] = (uint32_t)(U1 + i);
  keys[3 * n + t] = (uint32_t)(U1 + j);
  vals[t] = (uint32_t)t;
  vals[n + t] = (uint32_t)(n + t);
  vals[2 * n + t] = (uint32_t)(2 * n + t);
  vals[3 * n + t] = (uint32_t)(3 * n + t);
}

// g per triplet (seq_dot scores, the step's bpr_term; an index outside its table
// is read as row 0).  With lpart, also the workgroup's loss: every thread's term as
// a double (0 past n), added by a fixed tree over the 256 threads, to lpart[block].
__global__ void __launch_bounds__(256) k_adv_coef(const float* __restrict__ P, const float* __restrict__ Q, int d,
                                                  const int32_t* __restrict__ user, const int32_t* __restrict__ ipos,
                                                  const int32_t* __restrict__ ineg, int64_t n, int64_t U1, int64_t I1,
                                                  float lo, float hi, float* __restrict__ coef,
                                                  double* __restrict__ lpart) {
  __shared__ double sm[256];
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  double mine = 0.0;
  if (t < n) {
    const int32_t u = adv_clamp(user[t], U1), i = adv_clamp(ipos[t], I1), j = adv_clamp(ineg[t], I1);
    const float* p = P + (int64_t)u * d;
    const float x = seq_dot(p, Q + (int64_t)i * d, d) - seq_dot(p, Q + (int64_t)j * d, d);
    float g, loss;
    bpr_term(x, lo, hi, g, loss);
    coef[t] = g;
    mine = (double)loss;
  }
  if (!lpart) return;  // uniform: the whole grid or none of it
  sm[threadIdx.x] = mine;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sm[threadIdx.x] += sm[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) lpart[blockIdx.x] = sm[0];
}

// out[0] = the sum of lpart[0, nb): thread x adds lpart[x], lpart[x + 256], ... in
// that order, then the same tree.  One workgroup: a fixed order whatever the device.
__global__ void __launch_bounds__(256) k_adv_loss_sum(const double* __restrict__ lpart, int64_t nb,
                                                      double* __restrict__ out) {
  __shared__ double sm[256];
  double s = 0.0;
  for (int64_t x = threadIdx.x; x < nb; x += 256) s += lpart[x];
  sm[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sm[threadIdx.x] += sm[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = sm[0];
}

// ---- 2. stable radix sort pass on bits [shift, shift + 8) -------------------
// counts[digit * ntiles + tile]: digit-major, so that an exclusive scan of the
// whole array gives every (digit, tile) run its first output position.
__global__ void __launch_bounds__(ADV_SORT_BS) k_adv_hist(const uint32_t* __restrict__ keys, int64_t N, int shift,
                                                          int64_t ntiles, uint32_t* __restrict__ counts) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int64_t base = blockIdx.x * (int64_t)ADV_TILE;
#pragma unroll
  for (int k = 0; k < ADV_SORT_IPT; ++k) {
    const int64_t x = base + threadIdx.x + k * ADV_SORT_BS;
    if (x < N) atomicAdd(&h[(keys[x] >> shift) & 255u], 1u);
  }
  __syncthreads();
  counts[threadIdx.x * ntiles + blockIdx.x] = h[threadIdx.x];
}

// exclusive scan of c[0, M) in place: tile sums, a one-workgroup scan of the tile
// sums, then the scan inside every tile
__global__ void __launch_bounds__(256) k_adv_scan1(const uint32_t* __restrict__ c, int64_t M,
                                                   uint32_t* __restrict__ tsum) {
  using Reduce = rocprim::block_reduce<uint32_t, 256>;
  __shared__ typename Reduce::storage_type st;
  const int64_t base = blockIdx.x * (int64_t)ADV_SCAN_TILE + threadIdx.x * ADV_SCAN_IPT;
  uint32_t s = 0;
#pragma unroll
  for (int k = 0; k < ADV_SCAN_IPT; ++k) s += (base + k < M) ? c[base + k] : 0u;
  uint32_t total;
  Reduce().reduce(s, total, st);
  if (threadIdx.x == 0) tsum[blockIdx.x] = total;
}

__global__ void __launch_bounds__(1024) k_adv_scan2(uint32_t* __restrict__ tsum, int64_t T) {
  using Scan = rocprim::block_scan<uint32_t, 1024>;
  __shared__ typename Scan::storage_type st;
  const int64_t per = (T + 1023) / 1024;
  const int64_t b = threadIdx.x * per, e = b + per < T ? b + per : T;
  uint32_t s = 0;
  for (int64_t x = b; x < e; ++x) s += tsum[x];
  uint32_t run;
  Scan().exclusive_scan(s, run, 0u, st);
  for (int64_t x = b; x < e; ++x) {
    const uint32_t v = tsum[x];
    tsum[x] = run;
    run += v;
  }
}

__global__ void __launch_bounds__(256) k_adv_scan3(uint32_t* __restrict__ c, int64_t M,
                                                   const uint32_t* __restrict__ tsum) {
  using Scan = rocprim::block_scan<uint32_t, 256>;
  __shared__ typename Scan::storage_type st;
  const int64_t base = blockIdx.x * (int64_t)ADV_SCAN_TILE + threadIdx.x * ADV_SCAN_IPT;
  uint32_t v[ADV_SCAN_IPT], s = 0;
#pragma unroll
  for (int k = 0; k < ADV_SCAN_IPT; ++k) {
    v[k] = (base + k < M) ? c[base + k] : 0u;
    s += v[k];
  }
  uint32_t run;
  Scan().exclusive_scan(s, run, 0u, st);
  run += tsum[blockIdx.x];
#pragma unroll
  for (int k = 0; k < ADV_SCAN_IPT; ++k) {
    if (base + k < M) c[base + k] = run;
    run += v[k];
  }
}

// One tile: a stable workgroup sort on the digit, then every term goes to its
// (digit, tile) run at its rank inside the tile's digit run.
__global__ void __launch_bounds__(ADV_SORT_BS) k_adv_reorder(const uint32_t* __restrict__ kin,
                                                             const uint32_t* __restrict__ vin,
                                                             uint32_t* __restrict__ kout,
                                                             uint32_t* __restrict__ vout, int64_t N, int shift,
                                                             int64_t ntiles, const uint32_t* __restrict__ first) {
  using Sort = rocprim::block_radix_sort<uint32_t, ADV_SORT_BS, ADV_SORT_IPT, uint32_t>;
  __shared__ union {
    typename Sort::storage_type sort;
    uint32_t key[ADV_TILE];
  } sm;
  __shared__ int32_t dstart[256];
  const int tid = threadIdx.x;
  const int64_t base = blockIdx.x * (int64_t)ADV_TILE;
  uint32_t keys[ADV_SORT_IPT], vals[ADV_SORT_IPT];
#pragma unroll
  for (int k = 0; k < ADV_SORT_IPT; ++k) {
    const int64_t x = base + tid * ADV_SORT_IPT + k;  // blocked: the tile's order is the input order
    // padding: digit 255 and behind every term of the tile, so it stays behind them (stable)
    keys[k] = x < N ? kin[x] : ~0u;
    vals[k] = x < N ? vin[x] : ~0u;
  }
  Sort().sort(keys, vals, sm.sort, (unsigned)shift, (unsigned)shift + 8u);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < ADV_SORT_IPT; ++k) sm.key[tid * ADV_SORT_IPT + k] = keys[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < ADV_SORT_IPT; ++k) {
    const int q = tid * ADV_SORT_IPT + k;
    const uint32_t dg = (keys[k] >> shift) & 255u;
    if (q == 0 || ((sm.key[q - 1] >> shift) & 255u) != dg) dstart[dg] = q;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < ADV_SORT_IPT; ++k) {
    if (vals[k] == ~0u) continue;  // padding
    const int q = tid * ADV_SORT_IPT + k;
    const uint32_t dg = (keys[k] >> shift) & 255u;
    const int64_t dst = (int64_t)first[dg * ntiles + blockIdx.x] + (q - dstart[dg]);
    if (dst < N) {  // always true for a consistent histogram; never write outside the buffers
      kout[dst] = keys[k];
      vout[dst] = vals[k];
    }
  }
}

// ---- 3. row offsets and term records ---------------------------------------
// off[r] = first sorted term with key >= r, r in [0, R]
__global__ void __launch_bounds__(256) k_adv_offsets(const uint32_t* __restrict__ keys, int64_t N, int64_t R,
                                                     int32_t* __restrict__ off) {
  const int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (r > R) return;
  int64_t lo = 0, hi = N;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)keys[mid] < r) lo = mid + 1;
    else hi = mid;
  }
  off[r] = (int32_t)lo;
}

// rec[x] = (partner row, bits of the signed coefficient) of sorted term x
__global__ void __launch_bounds__(256) k_adv_records(const uint32_t* __restrict__ vals, int64_t N, int64_t n,
                                                     const int32_t* __restrict__ user,
                                                     const int32_t* __restrict__ ipos,
                                                     const int32_t* __restrict__ ineg, int64_t U1, int64_t I1,
                                                     const float* __restrict__ coef, int2* __restrict__ rec) {
  const int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (x >= N) return;
  int64_t e = vals[x];
  if (e >= N) e = 0;
  const int q = (int)(e / n);
  const int64_t t = e - q * n;
  const int32_t partner = q == 0 ? adv_clamp(ipos[t], I1) : q == 1 ? adv_clamp(ineg[t], I1) : adv_clamp(user[t], U1);
  const float g = coef[t];
  rec[x] = make_int2(partner, __float_as_int((q & 1) ? -g : g));
}

// ---- 4./5. chunk sums, normalisation ----------------------------------------
// tf.nn.l2_normalize(g, 1): g * rsqrt(max(sum g^2, 1e-12)), as the step's make_delta
template <int LPR, int NV>
__device__ __forceinline__ RowV<NV> adv_normalize(const RowV<NV>& G) {
  const float ss = dot_row<LPR, NV>(G, G);
  return scale_row(G, __builtin_amdgcn_rsqf(fmaxf(ss, 1e-12f)));
}

__device__ __forceinline__ int64_t adv_chunks_of(int32_t cnt) { return ((int64_t)cnt + ADV_CHUNK - 1) / ADV_CHUNK; }

// Unit w (a lane-group) -> (row r, chunk c): row r owns the units
// [off[r] / ADV_CHUNK + r, off[r + 1] / ADV_CHUNK + r + 1), at least one and at
// least its chunk count, so no scan of chunk counts is needed; spare units idle.
// Chunk sums of long rows go to part[2 * (first term / ADV_CHUNK) + (c > 0)]: a slot
// no other chunk of a long row maps to.
template <int LPR, int NV>
__global__ void __launch_bounds__(256) k_adv_chunks(const float* __restrict__ P, const float* __restrict__ Q, int d,
                                                    int64_t U1, int64_t R, const int32_t* __restrict__ off,
                                                    const int2* __restrict__ rec, float* __restrict__ part,
                                                    float* __restrict__ nP, float* __restrict__ nQ, int64_t units) {
  const int64_t w = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / LPR;
  const int l = threadIdx.x & (LPR - 1);
  if (w >= units) return;
  int64_t lo = 0, hi = R - 1;
  while (lo < hi) {  // the last row whose first unit is <= w
    const int64_t mid = (lo + hi + 1) >> 1;
    if ((int64_t)(off[mid] / ADV_CHUNK) + mid <= w) lo = mid;
    else hi = mid - 1;
  }
  const int64_t r = lo;
  const int32_t o = off[r], cnt = off[r + 1] - o;
  const int64_t nch = adv_chunks_of(cnt);
  const int64_t c = w - ((int64_t)(o / ADV_CHUNK) + r);
  if (c >= (nch > 0 ? nch : 1)) return;
  float* out = r < U1 ? nP : nQ;
  const int64_t orow = r < U1 ? r : r - U1;
  if (nch == 0) {  // a row no triplet touches: exact zeros
    store_row<LPR, NV>(out, orow, d, l, zero_row<NV>());
    return;
  }
  const float* tab = r < U1 ? Q : P;
  const int64_t b = (int64_t)o + c * ADV_CHUNK;
  const int64_t e = b + ADV_CHUNK < (int64_t)o + cnt ? b + ADV_CHUNK : (int64_t)o + cnt;
  RowV<NV> acc = zero_row<NV>();
  for (int64_t x = b; x < e; ++x) {
    const int2 rc = rec[x];
    const RowV<NV> v = load_row<LPR, NV>(tab, rc.x, d, l);
    axpy_row(acc, __int_as_float(rc.y), v);
  }
  if (nch == 1) store_row<LPR, NV>(out, orow, d, l, adv_normalize<LPR, NV>(acc));
  else store_row<LPR, NV>(part, 2 * (b / ADV_CHUNK) + (c > 0 ? 1 : 0), d, l, acc);
}

template <int LPR, int NV>
__global__ void __launch_bounds__(256) k_adv_combine(int d, int64_t U1, int64_t R, const int32_t* __restrict__ off,
                                                     const float* __restrict__ part, float* __restrict__ nP,
                                                     float* __restrict__ nQ) {
  const int64_t r = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / LPR;
  const int l = threadIdx.x & (LPR - 1);
  if (r >= R) return;
  const int32_t o = off[r], cnt = off[r + 1] - o;
  const int64_t nch = adv_chunks_of(cnt);
  if (nch < 2) return;
  RowV<NV> acc = load_row<LPR, NV>(part, 2 * (int64_t)(o / ADV_CHUNK), d, l);
  for (int64_t c = 1; c < nch; ++c)  // chunk order
    acc = add_row(acc, load_row<LPR, NV>(part, 2 * (((int64_t)o + c * ADV_CHUNK) / ADV_CHUNK) + 1, d, l));
  store_row<LPR, NV>(r < U1 ? nP : nQ, r < U1 ? r : r - U1, d, l, adv_normalize<LPR, NV>(acc));
}

// random mode: the step's draw for (seed, call, t, table, row) at eps = 1 (x * 1.0f is x)
template <int LPR, int NV>
__global__ void __launch_bounds__(256) k_adv_random(uint64_t seed, uint32_t call, int32_t t, int d, int64_t U1,
                                                    int64_t R, float* __restrict__ nP, float* __restrict__ nQ) {
  const int64_t r = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / LPR;
  const int l = threadIdx.x & (LPR - 1);
  if (r >= R) return;
  const int is_item = r >= U1 ? 1 : 0;
  const int64_t row = is_item ? r - U1 : r;
  store_row<LPR, NV>(is_item ? nQ : nP, row, d, l,
                     random_delta<LPR, NV>(seed, call, t, d, 1.0f, is_item, (int32_t)row, l));
}

// ---- acf_adv_apply: delta = N * eps, sum = W + delta (two rounded operations) -
__global__ void __launch_bounds__(256) k_adv_apply(const float* __restrict__ W, const float* __restrict__ N,
                                                   int64_t count, float eps, float* __restrict__ delta,
                                                   float* __restrict__ sum) {
  const int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (x >= count) return;
  const float dl = N[x] * eps;
  if (delta) delta[x] = dl;
  if (sum) sum[x] = W[x] + dl;
}

// ---- acf_adv_pgd: one projected step on every row of one table ------------------
// v = delta + alpha * n (the product rounded, then the sum), s = sqrt(dot_row(v, v))
// in fp32 (per-lane partial sums of rounded squares, then group_sum's order),
// delta' = v when s <= eps (s = 0 included: eps >= 0), else v * (eps / s): one
// division per row, one product per element; sum = W + delta'.  delta NULL: zeros;
// n NULL: no step, the projection alone.  delta_out may be delta (a lane reads its
// own elements before it writes them).
template <int LPR, int NV>
__global__ void __launch_bounds__(256) k_adv_pgd_step(const float* __restrict__ W, const float* delta, const float* n,
                                                      int64_t rows, int d, float alpha, float eps, float* delta_out,
                                                      float* __restrict__ sum_out) {
  const int64_t r = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / LPR;
  const int l = threadIdx.x & (LPR - 1);
  if (r >= rows) return;
  RowV<NV> v = delta ? load_row<LPR, NV>(delta, r, d, l) : zero_row<NV>();
  if (n) v = add_row(v, scale_row(load_row<LPR, NV>(n, r, d, l), alpha));
  const float s = sqrtf(dot_row<LPR, NV>(v, v));
  if (!(s <= eps)) v = scale_row(v, eps / s);
  store_row<LPR, NV>(delta_out, r, d, l, v);
  store_row<LPR, NV>(sum_out, r, d, l, add_row(load_row<LPR, NV>(W, r, d, l), v));
}

// ---- host: workspace layout --------------------------------------------------
struct AdvLayout {
  size_t coef, k0, v0, k1, v1, counts, tsum, off, part, err, total;
  int64_t N, ntiles, M, T, R;
  int passes;
};

static inline size_t adv_up(size_t x) { return (x + 255) & ~(size_t)255; }

// n triplets -> N = 4n terms; R = U1 + I1 row keys
static AdvLayout adv_layout(int64_t n, int64_t U1, int64_t I1, int32_t d) {
  AdvLayout L;
  L.N = 4 * n;
  L.R = U1 + I1;
  L.ntiles = (L.N + ADV_TILE - 1) / ADV_TILE;
  L.M = 256 * L.ntiles;
  L.T = (L.M + ADV_SCAN_TILE - 1) / ADV_SCAN_TILE;
  int bits = 1;
  while (bits < 32 && ((int64_t)1 << bits) < L.R) ++bits;
  L.passes = (bits + 7) / 8;
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t a = at;
    at += adv_up(bytes);
    return a;
  };
  L.coef = take((size_t)n * sizeof(float));
  L.k0 = take((size_t)L.N * 4);  // (k0, v0) and (k1, v1) are adjacent: the pair the sort
  L.v0 = take((size_t)L.N * 4);  // does not end in becomes the N 8-byte term records
  L.k1 = take((size_t)L.N * 4);
  L.v1 = take((size_t)L.N * 4);
  L.counts = take((size_t)L.M * 4);
  L.tsum = take((size_t)L.T * 4);
  L.off = take((size_t)(L.R + 1) * 4);
  L.part = take((size_t)2 * (L.N / ADV_CHUNK + 1) * d * sizeof(float));
  L.err = take(sizeof(int32_t));
  L.total = at;
  return L;
}

// A plan (acf_adv_plan): what stages 1 (keys), 2 and k_adv_offsets leave, in one
// caller-owned buffer: the sorted term values, the row offsets, the error word.
struct AdvPlanLayout {
  size_t vals, off, err, total;
};

static AdvPlanLayout adv_plan_layout(int64_t n, int64_t U1, int64_t I1) {
  AdvPlanLayout L;
  L.vals = 0;
  L.off = adv_up((size_t)4 * n * 4);
  L.err = L.off + adv_up((size_t)(U1 + I1 + 1) * 4);
  L.total = L.err + adv_up(sizeof(int32_t));
  return L;
}
