// Fold-in of new rows against frozen tables: the one kernel frame (k_fold), its
// range check and host frame, and the user side (FoldUsers, acf_fold_in_users).
// The item side is acf_fold_items.h.  Included by acf_ops.hip after its geometry
// helpers; one translation unit.  DESIGN.md §4d, §4i.
//
// Row r of a CSR (off, first) takes, for epoch e = 0..E-1 and every consecutive
// slice of at most `batch` of its positions, ONE training_batch iteration
// (APR.py:143-195) with one triplet per position; only the fitted row w_r and its
// Adagrad accumulator are kept, the tables are read-only.  A triplet reads row
// first[k] of table F (bound F1) and row neg[e][k] of Q (bound I1):
//   new users (FoldUsers): F = Q; the one-row user table [p_r] and Q, the batch
//     {(0, item_pos[k], item_neg[e][k])};
//   new items (FoldItems): F = P; the tables P and [Q ; q_r], the batch
//     {(user_pos[k], I1, item_neg[e][k])}.
//
// One workgroup of 256 lanes per fitted row (the grid strides over them); it runs
// all E epochs.  w_r and its accumulator live in the registers of lane-group 0 and
// in LDS for the whole launch; only table rows are fetched.  A slice is
//   A. per triplet (one lane-group of LPR lanes each): its two rows, x, g, loss;
//      the group's partial clean gradient of w_r (rounded products, triplet order);
//   B. (APR) the 2*Bs references (row, e) -- e < Bs the list's row of triplet e,
//      else the negative of triplet e - Bs -- sorted in LDS (bitonic, unique 64-bit
//      keys), so the references of one table row lie together, in triplet order;
//   C. lane-group 0 adds the partials in group order: the clean gradient of w_r;
//      delta_w = eps * l2_normalize(it);
//   D. (APR) per triplet again: its two rows, fetched a second time (they are in
//      L2 from A), each plus the delta of its own clean gradient, an ordered sum
//      over the row's references; the adversarial forward on w_r + delta_w and
//      them; the group's partial adversarial gradient of w_r;
//   E. lane-group 0: gradient = clean + reg + adversarial partials in group
//      order, Adagrad on (w_r, acc).
// A side supplies what differs, and nothing else: x, a triplet's term of the
// gradient of w_r, the tag of a negative's key, and D's perturbed rows.
// Workgroups never communicate; every loop is bounded by the inputs; no float
// atomics: every sum has a fixed order that depends on the inputs alone, so a
// row's outputs depend on that row's inputs only, bit for bit.

constexpr int FOLD_BS = 256;
constexpr int FOLD_KEYS = 2 * ACF_FOLD_MAX_BATCH;

__device__ __forceinline__ int32_t fold_row(int32_t x, int64_t rows) { return (x < 0 || x >= rows) ? 0 : x; }

// any index of a [na] outside [0, ra) or of b [nb] outside [0, rb): *err = 1
__global__ void __launch_bounds__(256) k_fold_check(const int32_t* __restrict__ a, int64_t na, int64_t ra,
                                                    const int32_t* __restrict__ b, int64_t nb, int64_t rb,
                                                    int32_t* __restrict__ err) {
  const int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  bool bad = false;
  if (x < na) bad = a[x] < 0 || a[x] >= ra;
  else if (x < na + nb) bad = b[x - na] < 0 || b[x - na] >= rb;
  if (bad) atomicOr(err, 1);
}

// What phase D sees of a slice: the tables, the slice's Bs list entries and
// negatives, its sorted references key[0..2*Bs) (row << 32 | e), where each
// reference went (pos[e]) and the clean g of every triplet.
struct FoldSlice {
  const float *F, *Q;
  int64_t F1, I1;
  int d;
  const int32_t *first, *neg;
  const uint64_t* key;
  const uint16_t* pos;
  const float* g;
  int Bs;

  // the table rows of triplet e (an index outside its table reads row 0)
  template <int LPR, int NV>
  __device__ __forceinline__ RowV<NV> first_row(int e, int l) const {
    return load_row<LPR, NV>(F, fold_row(first[e], F1), d, l);
  }
  template <int LPR, int NV>
  __device__ __forceinline__ RowV<NV> neg_row(int e, int l) const {
    return load_row<LPR, NV>(Q, fold_row(neg[e], I1), d, l);
  }
};

// First reference of the run of equal rows (equal high words) that key[s] is in.
// A run ends with the row or at 2*Bs: the padding behind carries a high word that
// no row has, so a scan to the padded length would visit the same references.
__device__ __forceinline__ int fold_run(const uint64_t* key, int s) {
  const uint32_t row = (uint32_t)(key[s] >> 32);
  while (s > 0 && (uint32_t)(key[s - 1] >> 32) == row) --s;
  return s;
}

struct FoldUsers {
  static constexpr uint64_t NEG_TAG = 0;  // one family: a negative can be another triplet's positive

  // w: p_r (D: p_r + delta_p); f, qj: q_i, q_j (D: perturbed)
  template <int LPR, int NV>
  static __device__ __forceinline__ float score(const RowV<NV>& w, const RowV<NV>& f, const RowV<NV>& qj) {
    return dot_row<LPR, NV>(w, f) - dot_row<LPR, NV>(w, qj);
  }

  template <int NV>
  static __device__ __forceinline__ void grad(RowV<NV>& part, float c, const RowV<NV>& f, const RowV<NV>& qj) {
    axpy_row(part, c, f);
    axpy_row(part, -c, qj);
  }

  // delta of the item row of reference s: term e of its clean gradient is +g[e] * p
  // (e < Bs) or -g[e - Bs] * p, rounded products added in reference order (the
  // IndexedSlices concat order: pos branch, then neg branch, triplet order).
  template <int LPR, int NV>
  static __device__ __forceinline__ RowV<NV> delta(const FoldSlice& sl, int s, const RowV<NV>& p, float eps) {
    const uint32_t row = (uint32_t)(sl.key[s] >> 32);
    RowV<NV> G = zero_row<NV>();
    for (int x = fold_run(sl.key, s); x < 2 * sl.Bs && (uint32_t)(sl.key[x] >> 32) == row; ++x) {
      const int e = (int)(uint32_t)sl.key[x];
      axpy_row(G, e < sl.Bs ? sl.g[e] : -sl.g[e - sl.Bs], p);
    }
    return l2_delta<LPR, NV>(G, eps);
  }

  // D: q_i + delta_i, q_j + delta_j of triplet b
  template <int LPR, int NV>
  static __device__ __forceinline__ void perturbed(const FoldSlice& sl, int b, int l, float eps, const RowV<NV>& p,
                                                   RowV<NV>& f, RowV<NV>& qj) {
    f = add_row(sl.first_row<LPR, NV>(b, l), delta<LPR, NV>(sl, sl.pos[b], p, eps));
    qj = add_row(sl.neg_row<LPR, NV>(b, l), delta<LPR, NV>(sl, sl.pos[sl.Bs + b], p, eps));
  }
};

template <int LPR, int NV, class SIDE>
__global__ void __launch_bounds__(FOLD_BS) k_fold(const float* __restrict__ F, int64_t F1,
                                                  const float* __restrict__ Q, int64_t I1, int d,
                                                  const int64_t* __restrict__ off, int64_t n, int64_t T,
                                                  const int32_t* __restrict__ first,
                                                  const int32_t* __restrict__ ineg, int E, int batch,
                                                  acf_apr_hparams hp, const float* __restrict__ init,
                                                  const float* __restrict__ acc_init, float* __restrict__ W_new,
                                                  float* __restrict__ acc_new, float* __restrict__ loss) {
  constexpr int G = FOLD_BS / LPR;   // lane-groups
  constexpr int DP = LPR * NV * 4;   // padded row length
  __shared__ uint64_t key[FOLD_KEYS];
  __shared__ uint16_t pos[FOLD_KEYS];
  __shared__ float sg[ACF_FOLD_MAX_BATCH];
  __shared__ __attribute__((aligned(16))) float red[G * DP];
  __shared__ float lred[G];
  __shared__ __attribute__((aligned(16))) float sW[DP];
  __shared__ __attribute__((aligned(16))) float sWP[DP];
  const int tid = threadIdx.x, l = tid & (LPR - 1), grp = tid / LPR;
  const bool adver = hp.adver != 0;

  for (int64_t r = blockIdx.x; r < n; r += gridDim.x) {
    int64_t b0 = off[r], b1 = off[r + 1];
    b0 = b0 < 0 ? 0 : (b0 > T ? T : b0);
    b1 = b1 < b0 ? b0 : (b1 > T ? T : b1);
    RowV<NV> w = zero_row<NV>(), a = zero_row<NV>();  // lane-group 0's copy is the row's state
    if (grp == 0) {
      if (init) w = load_row<LPR, NV>(init, r, d, l);
      if (acc_init) a = load_row<LPR, NV>(acc_init, r, d, l);
      // no acc_init, and the padding chunks of a row (c * 4 >= d; their w and gradient stay 0):
      // 0.1, so that Adagrad's rsqrt stays finite there
#pragma unroll
      for (int v = 0; v < NV; ++v)
        if (!acc_init || (l + LPR * v) * 4 >= d) a.v[v] = make_float4(0.1f, 0.1f, 0.1f, 0.1f);
      store_row<LPR, NV>(sW, 0, DP, l, w);
    }
    __syncthreads();
    for (int e = 0; e < E; ++e) {
      float eloss = 0.f;
      for (int64_t s0 = b0; s0 < b1; s0 += batch) {
        const int Bs = (int)(b1 - s0 < batch ? b1 - s0 : batch);
        const FoldSlice sl{F, Q, F1, I1, d, first + s0, ineg + (int64_t)e * T + s0, key, pos, sg, Bs};
        int n2 = 2;
        while (n2 < 2 * Bs) n2 <<= 1;
        const RowV<NV> wr = load_row<LPR, NV>(sW, 0, DP, l);
        // ---- A: clean forward, partial clean gradient of w
        RowV<NV> part = zero_row<NV>();
        float lpart = 0.f;
        for (int b = grp; b < Bs; b += G) {
          const int32_t i = fold_row(sl.first[b], F1), j = fold_row(sl.neg[b], I1);
          const RowV<NV> f = load_row<LPR, NV>(F, i, d, l), qj = load_row<LPR, NV>(Q, j, d, l);
          const float x = SIDE::template score<LPR, NV>(wr, f, qj);
          float g, ls;
          bpr_term(x, hp.clip_lo, hp.clip_hi, g, ls);
          SIDE::grad(part, g, f, qj);
          lpart = lpart + ls;
          if (l == 0) {
            sg[b] = g;
            if (adver) {
              key[b] = ((uint64_t)(uint32_t)i << 32) | (uint32_t)b;
              key[Bs + b] = SIDE::NEG_TAG | ((uint64_t)(uint32_t)j << 32) | (uint32_t)(Bs + b);
            }
          }
        }
        store_row<LPR, NV>(red, grp, DP, l, part);
        if (l == 0) lred[grp] = lpart;
        if (adver)
          for (int x = 2 * Bs + tid; x < n2; x += FOLD_BS) key[x] = ~0ull;  // padding sorts last
        __syncthreads();
        // ---- B: sort the references
        if (adver) {
          for (int k = 2; k <= n2; k <<= 1)
            for (int jj = k >> 1; jj > 0; jj >>= 1) {
              for (int t = tid; t < (n2 >> 1); t += FOLD_BS) {
                const int lo = ((t & ~(jj - 1)) << 1) | (t & (jj - 1)), hi = lo | jj;
                const uint64_t ka = key[lo], kb = key[hi];
                if ((ka > kb) == ((lo & k) == 0)) {
                  key[lo] = kb;
                  key[hi] = ka;
                }
              }
              __syncthreads();
            }
          for (int x = tid; x < 2 * Bs; x += FOLD_BS) pos[(uint32_t)key[x]] = (uint16_t)x;
        }
        // ---- C: clean gradient of w, delta_w
        RowV<NV> grad = zero_row<NV>();
        if (grp == 0) {
          float ls = 0.f;
          for (int g2 = 0; g2 < G && g2 < Bs; ++g2) {  // groups >= Bs had no triplet
            grad = add_row(grad, load_row<LPR, NV>(red, g2, DP, l));
            ls = ls + lred[g2];
          }
          eloss = eloss + ls;
          if (adver) store_row<LPR, NV>(sWP, 0, DP, l, add_row(w, l2_delta<LPR, NV>(grad, hp.eps)));
        }
        __syncthreads();
        // ---- D: adversarial forward, partial adversarial gradient of w
        if (adver) {
          const RowV<NV> wp = load_row<LPR, NV>(sWP, 0, DP, l);
          part = zero_row<NV>();
          for (int b = grp; b < Bs; b += G) {
            RowV<NV> f, qj;
            SIDE::template perturbed<LPR, NV>(sl, b, l, hp.eps, wr, f, qj);
            const float x = SIDE::template score<LPR, NV>(wp, f, qj);
            float ga, ls;
            bpr_term(x, hp.clip_lo, hp.clip_hi, ga, ls);
            SIDE::grad(part, hp.reg_adv * ga, f, qj);
          }
          store_row<LPR, NV>(red, grp, DP, l, part);
          __syncthreads();
        }
        // ---- E: reg, adversarial partials, Adagrad
        if (grp == 0) {
          if (hp.reg != 0.f) {
            const float coef = (2.0f * hp.reg / ((float)Bs * (float)d)) * (adver ? 2.0f : 1.0f);
            axpy_row(grad, coef * (float)Bs, w);
          }
          if (adver)
            for (int g2 = 0; g2 < G && g2 < Bs; ++g2) grad = add_row(grad, load_row<LPR, NV>(red, g2, DP, l));
          adagrad_apply(w, a, grad, hp.lr);
          store_row<LPR, NV>(sW, 0, DP, l, w);
        }
        __syncthreads();
      }
      if (loss && tid == 0) loss[(int64_t)e * n + r] = eloss;
    }
    if (grp == 0) {
      store_row<LPR, NV>(W_new, r, d, l, w);
      store_row<LPR, NV>(acc_new, r, d, l, a);
    }
    __syncthreads();  // sW is rewritten for the next row
  }
}

// Both entry points behind their table checks (tables_ok): the argument checks in
// the order a caller sees, the range check of first [T] against F1 and of neg
// [E*T] against I1 (one launch, before anything is written; ACF_E_RANGE without
// a message: the entry point words it), the grid cap and the launch.
template <class SIDE>
static int fold_in(const char* who, bool tables_ok, const float* F, int64_t F1, const float* Q, int64_t I1,
                   int32_t d, const int64_t* off, int64_t n, const int32_t* first, const int32_t* neg, int64_t T,
                   int32_t epochs, int32_t batch, const acf_apr_hparams* hp, const float* init,
                   const float* acc_init, float* W_new, float* acc_new, float* loss, int32_t check, void* stream) {
  ACF_RET(check_dim(d));
  ACF_CHECK(tables_ok && hp && n >= 0 && T >= 0 && epochs >= 0, ACF_E_INVALID, "%s: NULL argument or bad size", who);
  ACF_CHECK(batch >= 1 && batch <= ACF_FOLD_MAX_BATCH, ACF_E_INVALID, "%s: batch must lie in [1, %d], got %d", who,
            ACF_FOLD_MAX_BATCH, (int)batch);
  ACF_CHECK(hp->adv_mode == 0 && hp->zero_delta == 0, ACF_E_INVALID,
            "%s: only the gradient delta (adv_mode 0, zero_delta 0)", who);
  if (n == 0) return ACF_OK;
  ACF_CHECK(off && W_new && acc_new && (T == 0 || (first && (epochs == 0 || neg))), ACF_E_INVALID,
            "%s: NULL argument", who);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (check && T > 0) {
    int32_t* err = nullptr;
    int32_t herr = 0;
    HIP_TRY(hipMallocAsync((void**)&err, 16, s));
    const int64_t ET = (int64_t)epochs * T;
    const int r = [&]() -> int {
      HIP_TRY(hipMemsetAsync(err, 0, 16, s));
      k_fold_check<<<grid_for(T + ET), 256, 0, s>>>(first, T, F1, neg, ET, I1, err);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(&herr, err, sizeof(int32_t), hipMemcpyDeviceToHost, s));
      return ACF_OK;
    }();
    const hipError_t ef = hipFreeAsync(err, s);  // freed on every path
    ACF_RET(r);
    HIP_TRY(ef);
    HIP_TRY(hipStreamSynchronize(s));
    if (herr) return ACF_E_RANGE;
  }
  const unsigned grid = (unsigned)(n < (1 << 20) ? n : (1 << 20));
  OPS_GEOM(d, (k_fold<LPR, NV, SIDE><<<grid, FOLD_BS, 0, s>>>(F, F1, Q, I1, d, off, n, T, first, neg, epochs, batch,
                                                               *hp, init, acc_init, W_new, acc_new, loss)));
  HIP_TRY(hipGetLastError());
  return ACF_OK;
}

extern "C" int acf_fold_in_users(const float* Q, int64_t I1, int32_t d, const int64_t* user_off, int64_t n,
                                 const int32_t* item_pos, const int32_t* item_neg, int64_t T, int32_t epochs,
                                 int32_t batch, const acf_apr_hparams* hp, const float* init,
                                 const float* acc_init, float* P_new, float* acc_new, float* loss, int32_t check,
                                 void* stream) {
  const int r = fold_in<FoldUsers>("fold_in_users", Q && I1 > 0 && I1 <= (1ll << 31), Q, I1, Q, I1, d, user_off, n,
                                   item_pos, item_neg, T, epochs, batch, hp, init, acc_init, P_new, acc_new, loss,
                                   check, stream);
  if (r == ACF_E_RANGE) return acf_set_error(r, "fold_in_users: item index outside [0, %lld)", (long long)I1);
  return r;
}
