// Diversity kernels of libacf_apr.so (k_div_*): the intra-list similarity of a set
// of lists, and the greedy MMR re-ranking of candidate pools.  Included by
// acf_rank.hip after acf_neighbors.h (nbr_step, nbr_score: the similarities are
// section 4h's, from the same device functions), acf_eval_multi.h (evx_block_sum)
// and acf_lists.h (LstCuts); one translation unit.  DESIGN.md §4n.
#pragma once

// ---------------------------------------------------------------------------
// Both kernels give one row (a list, a pool) to one wave, a workgroup of 64:
// nothing crosses a wave, so there is no barrier between steps and no
// communication between workgroups.  Position x of the row belongs to lane
// x & 63, slot x >> 6 (EPL = 1 slot for rows of up to 64 positions, 2 up to 128);
// what a position carries (id, relevance, penalty, norm, running sum) lives in
// its lane's registers.  The rows of T that the positions name are staged in LDS
// once, with a stride of d + DIV_PAD words: the stride keeps a row float4-aligned
// and sends the b128 reads of 16 consecutive lanes to 64 different banks.  One
// "round" is then: the row of one position s is read as a broadcast, every lane
// runs the chain of each of its positions against it (nbr_step, k ascending from
// +0.0: two independent chains per lane at EPL = 2) and finishes it with
// nbr_score.  ILS runs a round per position a and adds into the sums of the
// positions b > a; MMR runs a round per pick.
//
// LDS: m (d + 4) 4 bytes per row of m positions: 34,816 B at m = 128, d = 64.
// Up to DIV_ROWS_LDS bytes the rows are staged (the static part, under 2 KB,
// keeps the workgroup inside the 64 KB that need no opt-in); above it (m = 128:
// d > 116; d = 1024: m > 14) the same chains read the rows from global memory
// through the caches (LDS = false).  The arithmetic is the same, so are the bits.
// ---------------------------------------------------------------------------
constexpr int DIV_MAX_M = LST_MAX_K;  // 128: a pool is as long as a list
constexpr int DIV_PAD = 4;
constexpr size_t DIV_ROWS_LDS = 60 * 1024;
constexpr int DIV_NONE = 0x7fffffff;  // "no position" in the argmax

static size_t div_rows_bytes(int m, int d) { return (size_t)m * (d + DIV_PAD) * sizeof(float); }

// The ids of a row of `len` positions (the first `use` of them take part) into the lanes: id[e] as given (-1
// past `use`), tr[e] the row of T to read (0 for none and for an id >= rows, which sets *err), row[e] where
// that row is read from, staged into `srows` [use][d + DIV_PAD] when LDS.  s_tr [DIV_MAX_M] is the staging's copy of tr.
template <int EPL, bool LDS>
__device__ __forceinline__ void div_load_rows(const float* __restrict__ T, int64_t rows, int d,
                                              const int32_t* __restrict__ ids, int len, int use, float* srows,
                                              int32_t* s_tr, int32_t (&id)[EPL], int32_t (&tr)[EPL],
                                              const float* (&row)[EPL], int32_t* __restrict__ err) {
  const int lane = threadIdx.x, stride = d + DIV_PAD;
  bool bad = false;
  for (int x = lane; x < len; x += 64) bad |= (int64_t)ids[x] >= rows;  // the whole row is checked
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const int x = lane + 64 * e;
    id[e] = x < use ? ids[x] : -1;
    tr[e] = (id[e] < 0 || (int64_t)id[e] >= rows) ? 0 : id[e];
    s_tr[x] = tr[e];
    row[e] = LDS ? srows + (x < use ? x : 0) * stride : T + (int64_t)tr[e] * d;  // past `use`: any staged row
  }
  if (__any(bad) && lane == 0) atomicOr(err, 1);
  if (LDS) {
    __syncthreads();  // s_tr
    const int d4 = d >> 2;
    for (int idx = lane; idx < use * d4; idx += 64) {
      const int x = idx / d4, q = idx - x * d4;
      *reinterpret_cast<float4*>(srows + x * stride + 4 * q) =
          *reinterpret_cast<const float4*>(T + (int64_t)s_tr[x] * d + 4 * q);
    }
    __syncthreads();  // the rows
  }
}

// One round: acc[e] = the finished chain of row[e] against `sel`, slots below e0 left alone.
template <int METRIC, int EPL>
__device__ __forceinline__ void div_round(const float* (&row)[EPL], const float* sel, int d, int e0,
                                          float (&acc)[EPL]) {
#pragma unroll
  for (int e = 0; e < EPL; ++e) acc[e] = 0.f;
  if (EPL == 2 && e0 == 1) {  // wave-uniform: the first slot has nothing left to score
    for (int k = 0; k < d; k += 4)
      acc[EPL - 1] = nbr_step<METRIC>(acc[EPL - 1], *reinterpret_cast<const float4*>(row[EPL - 1] + k),
                                      *reinterpret_cast<const float4*>(sel + k));
    return;
  }
  for (int k = 0; k < d; k += 4) {
    const float4 sv = *reinterpret_cast<const float4*>(sel + k);
#pragma unroll
    for (int e = 0; e < EPL; ++e) acc[e] = nbr_step<METRIC>(acc[e], *reinterpret_cast<const float4*>(row[e] + k), sv);
  }
}

// the value of slot x >> 6 in lane x & 63, for a wave-uniform position x
template <int EPL, class V>
__device__ __forceinline__ V div_at(const V (&v)[EPL], int x) {
  return __shfl(EPL == 2 && x >= 64 ? v[EPL - 1] : v[0], x & 63);
}

// ---------------------------------------------------------------------------
// list_similarity.  Position b's sum c_b = sum over the valid a < b of
// (double)sim(T[id_a], T[id_b]), a ascending: lane-private, so one order.  Lane c
// then walks b = 0 .. K_c - 1 for cutoff c, adding the c_b of the valid b into
// S and counting them in L: ils = S / (L (L - 1) / 2), one fp64 division; L < 2
// writes 0.0 and leaves the row out of that cutoff's mean (flag).
// ---------------------------------------------------------------------------
template <int METRIC, int EPL, bool LDS>
__global__ void __launch_bounds__(64) k_div_ils(const float* __restrict__ T, int64_t rows, int d,
                                                const int32_t* __restrict__ lists, int k, LstCuts cuts,
                                                double* __restrict__ ils, uint8_t* __restrict__ flag,
                                                int32_t* __restrict__ err) {
  extern __shared__ float4 div_smem[];
  __shared__ int32_t s_tr[DIV_MAX_M];
  __shared__ double s_c[DIV_MAX_M];
  __shared__ uint8_t s_v[DIV_MAX_M];
  const int lane = threadIdx.x;
  const int64_t r = blockIdx.x;
  int kmax = 0;
#pragma unroll
  for (int c = 0; c < LST_MAX_CUT; ++c) kmax = max(kmax, c < cuts.n ? cuts.k[c] : 0);
  int32_t id[EPL], tr[EPL];
  const float* row[EPL];
  div_load_rows<EPL, LDS>(T, rows, d, lists + r * k, k, kmax, reinterpret_cast<float*>(div_smem), s_tr, id, tr, row,
                          err);
  float nrm[EPL];
  double c[EPL];
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    nrm[e] = METRIC == NBR_COS ? sqrtf(seq_dot(row[e], row[e], d)) : 0.f;
    c[e] = 0.0;
  }
  for (int a = 0; a + 1 < kmax; ++a) {
    if (div_at<EPL>(id, a) < 0) continue;  // wave-uniform
    const float* sel = LDS ? reinterpret_cast<const float*>(div_smem) + a * (d + DIV_PAD)
                           : T + (int64_t)div_at<EPL>(tr, a) * d;
    const float na = div_at<EPL>(nrm, a);
    float acc[EPL];
    div_round<METRIC, EPL>(row, sel, d, a >= 63 ? 1 : 0, acc);
#pragma unroll
    for (int e = 0; e < EPL; ++e)
      if (id[e] >= 0 && lane + 64 * e > a) c[e] += (double)nbr_score<METRIC>(acc[e], na, nrm[e]);
  }
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    s_c[lane + 64 * e] = c[e];
    s_v[lane + 64 * e] = id[e] >= 0;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < LST_MAX_CUT; ++q) {
    if (lane != q || q >= cuts.n) continue;
    double S = 0.0;
    int L = 0;
    for (int b = 0; b < cuts.k[q]; ++b) {
      if (!s_v[b]) continue;
      S += s_c[b];
      ++L;
    }
    ils[r * cuts.n + q] = L >= 2 ? S / (double)(L * (L - 1) / 2) : 0.0;
    flag[r * cuts.n + q] = L >= 2;
  }
}

// workgroup q: the mean of column q of ils [n][ncol] over the rows whose flag [n][ncol] is set: k_lst_means'
// scheme (thread-strided partial sums, rows ascending, then evx_block_sum's fixed tree); 0.0 when none is
__global__ void __launch_bounds__(256) k_div_means(const double* __restrict__ ils, const uint8_t* __restrict__ flag,
                                                   int n, int ncol, double* __restrict__ mean) {
  __shared__ double s_red[256];
  __shared__ long long s_n[256];
  const int tid = threadIdx.x, q = blockIdx.x;
  double v = 0.0;
  long long cnt = 0;
  for (int64_t r = tid; r < n; r += 256) {
    if (!flag[r * ncol + q]) continue;
    v += ils[r * ncol + q];
    ++cnt;
  }
  s_n[tid] = cnt;
  const double sum = evx_block_sum(v, s_red);  // its barriers cover s_n
  if (tid == 0) {
    long long total = 0;
    for (int i = 0; i < 256; ++i) total += s_n[i];
    mean[q] = total > 0 ? sum / (double)total : 0.0;
  }
}

// ---------------------------------------------------------------------------
// rerank_mmr.  a_c = lam * rel_c once; per step the objective o_c (a_c at step 0,
// a_c - oml * pen_c afterwards: two products and a subtraction, each rounded),
// a wave argmax on (o_c, position) over the open positions -- larger o first,
// equal o (-0 and +0 are equal) to the lower position: a total order on finite
// values, so the butterfly gives what a scan upward with ">" gives -- then a
// round against the pick: pen_c = sim(c, pick), fmaxf of it from the second pick
// on.  The outputs collect in LDS and leave coalesced; they start as the tail's
// -1 / -inf / -inf, which is what stays once the open positions run out.
// ---------------------------------------------------------------------------
template <int METRIC, int EPL, bool LDS>
__global__ void __launch_bounds__(64) k_div_mmr(const float* __restrict__ T, int64_t rows, int d,
                                                const int32_t* __restrict__ cand, const float* __restrict__ rel,
                                                int m, int k_out, float lam, float oml,
                                                int32_t* __restrict__ items, float* __restrict__ rel_out,
                                                float* __restrict__ obj, int32_t* __restrict__ err) {
  extern __shared__ float4 div_smem[];
  __shared__ int32_t s_tr[DIV_MAX_M];
  __shared__ int32_t s_items[DIV_MAX_M];
  __shared__ float s_rel[DIV_MAX_M], s_obj[DIV_MAX_M];
  const int lane = threadIdx.x;
  const int64_t r = blockIdx.x;
  int32_t id[EPL], tr[EPL];
  const float* row[EPL];
  div_load_rows<EPL, LDS>(T, rows, d, cand + r * m, m, m, reinterpret_cast<float*>(div_smem), s_tr, id, tr, row, err);
  float rl[EPL], a[EPL], pen[EPL], nrm[EPL];
  bool open[EPL];
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const int x = lane + 64 * e;
    rl[e] = x < m ? rel[r * m + x] : 0.f;
    open[e] = id[e] >= 0 && fabsf(rl[e]) < INFINITY;  // false for a NaN
    a[e] = lam * rl[e];
    pen[e] = 0.f;
    nrm[e] = METRIC == NBR_COS ? sqrtf(seq_dot(row[e], row[e], d)) : 0.f;
    s_items[x] = -1;
    s_rel[x] = -INFINITY;
    s_obj[x] = -INFINITY;
  }
  for (int j = 0; j < k_out; ++j) {
    float bo = 0.f;
    int bp = DIV_NONE;
    float o[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      o[e] = a[e];
      if (j > 0) {
        const float t = oml * pen[e];
        o[e] = a[e] - t;
      }
      if (open[e] && (bp == DIV_NONE || o[e] > bo)) {  // slot 0 is the lower position
        bo = o[e];
        bp = lane + 64 * e;
      }
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const float oo = __shfl_xor(bo, off);
      const int op = __shfl_xor(bp, off);
      if (op != DIV_NONE && (bp == DIV_NONE || oo > bo || (oo == bo && op < bp))) {
        bo = oo;
        bp = op;
      }
    }
    if (bp == DIV_NONE) break;  // wave-uniform: the open positions ran out
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      if (bp != lane + 64 * e) continue;
      s_items[j] = id[e];
      s_rel[j] = rl[e];
      s_obj[j] = o[e];
      open[e] = false;
    }
    if (j + 1 == k_out) break;
    const float* sel = LDS ? reinterpret_cast<const float*>(div_smem) + bp * (d + DIV_PAD)
                           : T + (int64_t)div_at<EPL>(tr, bp) * d;
    const float ns = div_at<EPL>(nrm, bp);
    float acc[EPL];
    div_round<METRIC, EPL>(row, sel, d, 0, acc);
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      const float s = nbr_score<METRIC>(acc[e], nrm[e], ns);
      // fmaxf(pen, s) written as a compare and a select: the two are equal on everything but the sign of a
      // zero, which fmaxf leaves open -- hipcc uses that to feed v_max -acc for the Euclidean 0.0f - acc and
      // gives -0.0, and folds a "+ 0.0f" behind it away.  No similarity is -0.0, so no pen may be.
      pen[e] = (j == 0 || s > pen[e]) ? s : pen[e];
    }
  }
  __syncthreads();
  for (int x = lane; x < k_out; x += 64) {
    items[r * k_out + x] = s_items[x];
    rel_out[r * k_out + x] = s_rel[x];
    obj[r * k_out + x] = s_obj[x];
  }
}
