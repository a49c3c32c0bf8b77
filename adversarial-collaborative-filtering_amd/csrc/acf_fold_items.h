// Fold-in of new items against frozen user and item tables (k_fold_items):
// included by acf_ops.hip after acf_fold.h; one translation unit.  DESIGN.md §4i.
//
// acf_fold_in_items: new item r of a CSR (item_off, user_pos) takes, for epoch
// e = 0..E-1 and every consecutive slice of at most `batch` of its positions, ONE
// training_batch iteration (APR.py:143-195) on the tables P and [Q ; q_r] -- q_r
// appended as row I1 = num_item_rows -- with the batch
// {(user_pos[k], I1, item_neg[e][k])}.  Only q_r and its Adagrad accumulator are
// kept: P and Q are read-only, there is no accP and no accQ.
//
// A negative can never equal the new item: that item has no row in Q, negatives
// lie in [0, I1), so the i == j case of the user kernel does not exist here, and
// q_r is referenced by the pos branch of every triplet and by nothing else.
//
// One workgroup of 256 lanes per new item (the grid strides over items); it runs
// all E epochs.  q_r and its accumulator live in the registers of lane-group 0 and
// in LDS for the whole launch; rows of P and Q are fetched.  A slice is
//   A. per triplet (one lane-group of LPR lanes each): p_u, q_j, x, g, loss; the
//      group's partial clean gradient of q_r (sum of g * p_u, rounded products,
//      triplet order);
//   B. (APR) the Bs user references (u, e) and the Bs negative references
//      (j, Bs + e), the latter tagged in bit 63, sorted in LDS (bitonic, unique
//      64-bit keys): the references of one user row lie together in triplet
//      order, and so do those of one negative row;
//   C. lane-group 0 adds the partials in group order: the clean gradient of q_r;
//      delta_q = eps * l2_normalize(it);
//   D. (APR) per triplet again: the clean gradient of its user row is the ordered
//      sum of (+g_e * q_r) over the row's references, then of (-g_e * q_{j_e})
//      over them (the IndexedSlices concat order: pos branch, then neg branch);
//      that of its negative row the ordered sum of (-g_e * p_{u_e}); a delta from
//      each; the adversarial forward on p_u + delta_p, q_r + delta_q,
//      q_j + delta_j; the group's partial adversarial gradient of q_r.  Rows of
//      other triplets are fetched again (they are in L2 from A);
//   E. lane-group 0: gradient = clean + reg + adversarial partials in group
//      order, Adagrad on (q_r, acc).
// Workgroups never communicate; every loop is bounded by the inputs; no float
// atomics: every sum has a fixed order that depends on the inputs alone, so an
// item's outputs depend on that item's inputs only, bit for bit.

constexpr uint64_t FOLDI_NEG = 1ull << 63;  // indices are below 2^31: the tag keeps the two families apart

__device__ __forceinline__ int32_t foldi_row(int32_t x, int64_t rows) { return (x < 0 || x >= rows) ? 0 : x; }

// any user of user_pos [T] outside [0, U1) or negative of item_neg [E*T] outside [0, I1): *err = 1
__global__ void __launch_bounds__(256) k_fold_items_check(const int32_t* __restrict__ upos, int64_t T, int64_t U1,
                                                          const int32_t* __restrict__ ineg, int64_t ET, int64_t I1,
                                                          int32_t* __restrict__ err) {
  const int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  bool bad = false;
  if (x < T) bad = upos[x] < 0 || upos[x] >= U1;
  else if (x < T + ET) bad = ineg[x - T] < 0 || ineg[x - T] >= I1;
  if (bad) atomicOr(err, 1);
}

// First reference of the run of equal rows (equal high words) that key[s] is in.
__device__ __forceinline__ int foldi_run(const uint64_t* key, int s) {
  const uint32_t row = (uint32_t)(key[s] >> 32);
  while (s > 0 && (uint32_t)(key[s - 1] >> 32) == row) --s;
  return s;
}

// delta of the user row of triplet b: the row's references key[a..] hold
// (u << 32 | e); the clean gradient is sum_e g[e] * q_r, then sum_e -g[e] * q_{j_e},
// each in reference order.  neg: the slice's negatives; qj: q_{j_b}, already loaded.
template <int LPR, int NV>
__device__ __forceinline__ RowV<NV> foldi_user_delta(const uint64_t* key, const float* g, int s, int nk, int b,
                                                     const RowV<NV>& qr, const RowV<NV>& qj,
                                                     const float* __restrict__ Q, int64_t I1, int d,
                                                     const int32_t* __restrict__ neg, int l, float eps) {
  const int a = foldi_run(key, s);
  const uint32_t row = (uint32_t)(key[s] >> 32);
  RowV<NV> G = zero_row<NV>();
  for (int x = a; x < nk && (uint32_t)(key[x] >> 32) == row; ++x) axpy_row(G, g[(uint32_t)key[x]], qr);
  for (int x = a; x < nk && (uint32_t)(key[x] >> 32) == row; ++x) {
    const int e = (int)(uint32_t)key[x];
    axpy_row(G, -g[e], e == b ? qj : load_row<LPR, NV>(Q, foldi_row(neg[e], I1), d, l));
  }
  const float inv = __builtin_amdgcn_rsqf(fmaxf(dot_row<LPR, NV>(G, G), 1e-12f));
  return scale_row(scale_row(G, inv), eps);
}

// delta of the negative row of triplet b: references (tag | j << 32 | Bs + e); the
// clean gradient is sum_e -g[e] * p_{u_e} in reference order.  pu: p_{u_b}.
template <int LPR, int NV>
__device__ __forceinline__ RowV<NV> foldi_neg_delta(const uint64_t* key, const float* g, int s, int nk, int Bs, int b,
                                                    const RowV<NV>& pu, const float* __restrict__ P, int64_t U1,
                                                    int d, const int32_t* __restrict__ upos, int l, float eps) {
  const int a = foldi_run(key, s);
  const uint32_t row = (uint32_t)(key[s] >> 32);
  RowV<NV> G = zero_row<NV>();
  for (int x = a; x < nk && (uint32_t)(key[x] >> 32) == row; ++x) {
    const int e = (int)(uint32_t)key[x] - Bs;
    axpy_row(G, -g[e], e == b ? pu : load_row<LPR, NV>(P, foldi_row(upos[e], U1), d, l));
  }
  const float inv = __builtin_amdgcn_rsqf(fmaxf(dot_row<LPR, NV>(G, G), 1e-12f));
  return scale_row(scale_row(G, inv), eps);
}

template <int LPR, int NV>
__global__ void __launch_bounds__(FOLD_BS) k_fold_items(const float* __restrict__ P, int64_t U1,
                                                        const float* __restrict__ Q, int64_t I1, int d,
                                                        const int64_t* __restrict__ off, int64_t n, int64_t T,
                                                        const int32_t* __restrict__ upos,
                                                        const int32_t* __restrict__ ineg, int E, int batch,
                                                        acf_apr_hparams hp, const float* __restrict__ init,
                                                        const float* __restrict__ acc_init, float* __restrict__ Q_new,
                                                        float* __restrict__ acc_new, float* __restrict__ loss) {
  constexpr int G = FOLD_BS / LPR;   // lane-groups
  constexpr int DP = LPR * NV * 4;   // padded row length
  __shared__ uint64_t key[FOLD_KEYS];
  __shared__ uint16_t pos[FOLD_KEYS];
  __shared__ float sg[ACF_FOLD_MAX_BATCH];
  __shared__ __attribute__((aligned(16))) float red[G * DP];
  __shared__ float lred[G];
  __shared__ __attribute__((aligned(16))) float sQ[DP];
  __shared__ __attribute__((aligned(16))) float sQQ[DP];
  const int tid = threadIdx.x, l = tid & (LPR - 1), grp = tid / LPR;
  const bool adver = hp.adver != 0;

  for (int64_t r = blockIdx.x; r < n; r += gridDim.x) {
    int64_t b0 = off[r], b1 = off[r + 1];
    b0 = b0 < 0 ? 0 : (b0 > T ? T : b0);
    b1 = b1 < b0 ? b0 : (b1 > T ? T : b1);
    RowV<NV> q = zero_row<NV>(), a = zero_row<NV>();  // lane-group 0's copy is the item's state
    if (grp == 0) {
      if (init) q = load_row<LPR, NV>(init, r, d, l);
      if (acc_init) a = load_row<LPR, NV>(acc_init, r, d, l);
      // no acc_init, and the padding chunks of a row (c * 4 >= d; their q and gradient stay 0):
      // 0.1, so that Adagrad's rsqrt stays finite there
#pragma unroll
      for (int v = 0; v < NV; ++v)
        if (!acc_init || (l + LPR * v) * 4 >= d) a.v[v] = make_float4(0.1f, 0.1f, 0.1f, 0.1f);
      store_row<LPR, NV>(sQ, 0, DP, l, q);
    }
    __syncthreads();
    for (int e = 0; e < E; ++e) {
      const int32_t* neg = ineg + (int64_t)e * T;
      float eloss = 0.f;
      for (int64_t s0 = b0; s0 < b1; s0 += batch) {
        const int Bs = (int)(b1 - s0 < batch ? b1 - s0 : batch);
        int n2 = 2;
        while (n2 < 2 * Bs) n2 <<= 1;
        const RowV<NV> qr = load_row<LPR, NV>(sQ, 0, DP, l);
        // ---- A: clean forward, partial clean gradient of q_r
        RowV<NV> part = zero_row<NV>();
        float lpart = 0.f;
        for (int b = grp; b < Bs; b += G) {
          const int32_t u = foldi_row(upos[s0 + b], U1), j = foldi_row(neg[s0 + b], I1);
          const RowV<NV> pu = load_row<LPR, NV>(P, u, d, l), qj = load_row<LPR, NV>(Q, j, d, l);
          const float x = dot_row<LPR, NV>(pu, qr) - dot_row<LPR, NV>(pu, qj);
          float g, ls;
          bpr_term(x, hp.clip_lo, hp.clip_hi, g, ls);
          axpy_row(part, g, pu);
          lpart = lpart + ls;
          if (l == 0) {
            sg[b] = g;
            if (adver) {
              key[b] = ((uint64_t)(uint32_t)u << 32) | (uint32_t)b;
              key[Bs + b] = FOLDI_NEG | ((uint64_t)(uint32_t)j << 32) | (uint32_t)(Bs + b);
            }
          }
        }
        store_row<LPR, NV>(red, grp, DP, l, part);
        if (l == 0) lred[grp] = lpart;
        if (adver)
          for (int x = 2 * Bs + tid; x < n2; x += FOLD_BS) key[x] = ~0ull;  // padding sorts last
        __syncthreads();
        // ---- B: sort the user and the negative references
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
        // ---- C: clean gradient of q_r, delta_q
        RowV<NV> grad = zero_row<NV>();
        if (grp == 0) {
          float ls = 0.f;
          for (int g2 = 0; g2 < G && g2 < Bs; ++g2) {  // groups >= Bs had no triplet
            grad = add_row(grad, load_row<LPR, NV>(red, g2, DP, l));
            ls = ls + lred[g2];
          }
          eloss = eloss + ls;
          if (adver) {
            const float inv = __builtin_amdgcn_rsqf(fmaxf(dot_row<LPR, NV>(grad, grad), 1e-12f));
            store_row<LPR, NV>(sQQ, 0, DP, l, add_row(q, scale_row(scale_row(grad, inv), hp.eps)));
          }
        }
        __syncthreads();
        // ---- D: adversarial forward, partial adversarial gradient of q_r
        if (adver) {
          const RowV<NV> qq = load_row<LPR, NV>(sQQ, 0, DP, l);
          part = zero_row<NV>();
          for (int b = grp; b < Bs; b += G) {
            const int32_t u = foldi_row(upos[s0 + b], U1), j = foldi_row(neg[s0 + b], I1);
            const RowV<NV> pu = load_row<LPR, NV>(P, u, d, l), qj = load_row<LPR, NV>(Q, j, d, l);
            const RowV<NV> pp = add_row(pu, foldi_user_delta<LPR, NV>(key, sg, pos[b], 2 * Bs, b, qr, qj, Q, I1, d,
                                                                      neg + s0, l, hp.eps));
            const RowV<NV> qjp = add_row(qj, foldi_neg_delta<LPR, NV>(key, sg, pos[Bs + b], 2 * Bs, Bs, b, pu, P, U1,
                                                                      d, upos + s0, l, hp.eps));
            const float x = dot_row<LPR, NV>(pp, qq) - dot_row<LPR, NV>(pp, qjp);
            float ga, ls;
            bpr_term(x, hp.clip_lo, hp.clip_hi, ga, ls);
            axpy_row(part, hp.reg_adv * ga, pp);
          }
          store_row<LPR, NV>(red, grp, DP, l, part);
          __syncthreads();
        }
        // ---- E: reg, adversarial partials, Adagrad
        if (grp == 0) {
          if (hp.reg != 0.f) {
            const float coef = (2.0f * hp.reg / ((float)Bs * (float)d)) * (adver ? 2.0f : 1.0f);
            axpy_row(grad, coef * (float)Bs, q);
          }
          if (adver)
            for (int g2 = 0; g2 < G && g2 < Bs; ++g2) grad = add_row(grad, load_row<LPR, NV>(red, g2, DP, l));
#pragma unroll
          for (int v = 0; v < NV; ++v) {
            a.v[v].x = a.v[v].x + grad.v[v].x * grad.v[v].x;
            a.v[v].y = a.v[v].y + grad.v[v].y * grad.v[v].y;
            a.v[v].z = a.v[v].z + grad.v[v].z * grad.v[v].z;
            a.v[v].w = a.v[v].w + grad.v[v].w * grad.v[v].w;
            q.v[v].x = q.v[v].x - (hp.lr * grad.v[v].x) * __builtin_amdgcn_rsqf(a.v[v].x);
            q.v[v].y = q.v[v].y - (hp.lr * grad.v[v].y) * __builtin_amdgcn_rsqf(a.v[v].y);
            q.v[v].z = q.v[v].z - (hp.lr * grad.v[v].z) * __builtin_amdgcn_rsqf(a.v[v].z);
            q.v[v].w = q.v[v].w - (hp.lr * grad.v[v].w) * __builtin_amdgcn_rsqf(a.v[v].w);
          }
          store_row<LPR, NV>(sQ, 0, DP, l, q);
        }
        __syncthreads();
      }
      if (loss && tid == 0) loss[(int64_t)e * n + r] = eloss;
    }
    if (grp == 0) {
      store_row<LPR, NV>(Q_new, r, d, l, q);
      store_row<LPR, NV>(acc_new, r, d, l, a);
    }
    __syncthreads();  // sQ is rewritten for the next item
  }
}

extern "C" int acf_fold_in_items(const float* P, int64_t U1, const float* Q, int64_t I1, int32_t d,
                                 const int64_t* item_off, int64_t n, const int32_t* user_pos,
                                 const int32_t* item_neg, int64_t T, int32_t epochs, int32_t batch,
                                 const acf_apr_hparams* hp, const float* init, const float* acc_init, float* Q_new,
                                 float* acc_new, float* loss, int32_t check, void* stream) {
  int r = ops_dim(d);
  if (r) return r;
  if (!P || !Q || !hp || n < 0 || T < 0 || epochs < 0 || U1 <= 0 || U1 > (1ll << 31) || I1 <= 0 ||
      I1 >= (1ll << 31))  // the new item's own id, I1, is an int32 too
    return acf_set_error(ACF_E_INVALID, "fold_in_items: NULL argument or bad size");
  if (batch < 1 || batch > ACF_FOLD_MAX_BATCH)
    return acf_set_error(ACF_E_INVALID, "fold_in_items: batch must lie in [1, %d], got %d", ACF_FOLD_MAX_BATCH,
                         (int)batch);
  if (hp->adv_mode != 0 || hp->zero_delta != 0)
    return acf_set_error(ACF_E_INVALID, "fold_in_items: only the gradient delta (adv_mode 0, zero_delta 0)");
  if (n == 0) return ACF_OK;
  if (!item_off || !Q_new || !acc_new || (T > 0 && (!user_pos || (epochs > 0 && !item_neg))))
    return acf_set_error(ACF_E_INVALID, "fold_in_items: NULL argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (check && T > 0) {  // before anything is written
    int32_t* err = nullptr;
    int32_t herr = 0;
    OPS_TRY(hipMallocAsync((void**)&err, 16, s));
    const int64_t m = T + (int64_t)epochs * T;
    hipError_t e = hipMemsetAsync(err, 0, 16, s);
    if (e == hipSuccess) {
      k_fold_items_check<<<(unsigned)((m + 255) / 256), 256, 0, s>>>(user_pos, T, U1, item_neg, (int64_t)epochs * T,
                                                                     I1, err);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&herr, err, sizeof(int32_t), hipMemcpyDeviceToHost, s);
    const hipError_t ef = hipFreeAsync(err, s);  // freed on every path
    if (e == hipSuccess) e = ef;
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return acf_set_error(ACF_E_HIP, "fold_in_items range check: %s", hipGetErrorString(e));
    if (herr)
      return acf_set_error(ACF_E_RANGE, "fold_in_items: user outside [0, %lld) or negative outside [0, %lld)",
                           (long long)U1, (long long)I1);
  }
  const unsigned grid = (unsigned)(n < (1 << 20) ? n : (1 << 20));
  OPS_GEOM(d, (k_fold_items<LPR, NV><<<grid, FOLD_BS, 0, s>>>(P, U1, Q, I1, d, item_off, n, T, user_pos, item_neg,
                                                               epochs, batch, *hp, init, acc_init, Q_new, acc_new,
                                                               loss)));
  OPS_TRY(hipGetLastError());
  return ACF_OK;
}
