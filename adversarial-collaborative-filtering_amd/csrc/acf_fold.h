// Fold-in of new users against a frozen item table (k_fold_*): included by
// acf_ops.hip after its geometry helpers; one translation unit.  DESIGN.md §4d.
//
// acf_fold_in_users: user r of a CSR (user_off, item_pos) takes, for epoch
// e = 0..E-1 and every consecutive slice of at most `batch` of its positions, ONE
// training_batch iteration (APR.py:143-195) on the one-row user table [p_r] and Q
// with the batch {(0, item_pos[k], item_neg[e][k])}.  Only p_r and its Adagrad
// accumulator are kept: Q is read-only, there is no accQ.
//
// One workgroup of 256 lanes per user (the grid strides over users); it runs all
// E epochs.  p_r and its accumulator live in the registers of lane-group 0 and in
// LDS for the whole launch; only rows of Q are fetched.  A slice is
//   A. per triplet (one lane-group of LPR lanes each): q_i, q_j, x, g, loss; the
//      group's partial clean gradient of p (rounded products, triplet order);
//   B. (APR) the 2*Bs item references (item, e) -- e < Bs the positive of triplet
//      e, else the negative of triplet e - Bs -- sorted in LDS (bitonic, unique
//      64-bit keys), so the references of one item row lie together in the
//      IndexedSlices concat order (pos branch, then neg branch, triplet order);
//   C. lane-group 0 adds the partials in group order: the clean gradient of p;
//      delta_p = eps * l2_normalize(it);
//   D. (APR) per triplet again: the clean gradient of each of its two item rows
//      is the ordered sum of (+-g_e * p) over the row's references; delta_q from
//      it; the adversarial forward on p + delta_p, q + delta_q; the group's
//      partial adversarial gradient of p.  q_i, q_j are fetched a second time
//      (they are in L2 from A);
//   E. lane-group 0: gradient = clean + reg + adversarial partials in group
//      order, Adagrad on (p, acc).
// Workgroups never communicate; every loop is bounded by the inputs; no float
// atomics: every sum has a fixed order that depends on the inputs alone, so a
// user's outputs depend on that user's inputs only, bit for bit.

constexpr int FOLD_BS = 256;
constexpr int FOLD_KEYS = 2 * ACF_FOLD_MAX_BATCH;

__device__ __forceinline__ int32_t fold_item(int32_t x, int64_t I1) { return (x < 0 || x >= I1) ? 0 : x; }

// any item of item_pos [T] or item_neg [E*T] outside [0, I1): *err = 1
__global__ void __launch_bounds__(256) k_fold_check(const int32_t* __restrict__ ipos, int64_t T,
                                                    const int32_t* __restrict__ ineg, int64_t ET, int64_t I1,
                                                    int32_t* __restrict__ err) {
  const int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  bool bad = false;
  if (x < T) bad = ipos[x] < 0 || ipos[x] >= I1;
  else if (x < T + ET) bad = ineg[x - T] < 0 || ineg[x - T] >= I1;
  if (bad) atomicOr(err, 1);
}

// The clean gradient of item row `item` in a one-user slice: its references
// key[start..] hold (item << 32 | e); term e is +g[e] * p (e < Bs) or
// -g[e - Bs] * p, rounded products added in reference order.  s: a position of
// one of the row's references.  Then delta = eps * l2_normalize(sum).
template <int LPR, int NV>
__device__ __forceinline__ RowV<NV> fold_item_delta(const uint64_t* key, const float* g, int s, int n2, int Bs,
                                                    const RowV<NV>& p, float eps) {
  const uint32_t item = (uint32_t)(key[s] >> 32);
  int a = s;
  while (a > 0 && (uint32_t)(key[a - 1] >> 32) == item) --a;
  RowV<NV> G = zero_row<NV>();
  for (int x = a; x < n2 && (uint32_t)(key[x] >> 32) == item; ++x) {
    const int e = (int)(uint32_t)key[x];
    axpy_row(G, e < Bs ? g[e] : -g[e - Bs], p);
  }
  const float inv = __builtin_amdgcn_rsqf(fmaxf(dot_row<LPR, NV>(G, G), 1e-12f));
  return scale_row(scale_row(G, inv), eps);
}

template <int LPR, int NV>
__global__ void __launch_bounds__(FOLD_BS) k_fold(const float* __restrict__ Q, int64_t I1, int d,
                                                  const int64_t* __restrict__ off, int64_t n, int64_t T,
                                                  const int32_t* __restrict__ ipos,
                                                  const int32_t* __restrict__ ineg, int E, int batch,
                                                  acf_apr_hparams hp, const float* __restrict__ init,
                                                  const float* __restrict__ acc_init, float* __restrict__ P_new,
                                                  float* __restrict__ acc_new, float* __restrict__ loss) {
  constexpr int G = FOLD_BS / LPR;   // lane-groups
  constexpr int DP = LPR * NV * 4;   // padded row length
  __shared__ uint64_t key[FOLD_KEYS];
  __shared__ uint16_t pos[FOLD_KEYS];
  __shared__ float sg[ACF_FOLD_MAX_BATCH];
  __shared__ __attribute__((aligned(16))) float red[G * DP];
  __shared__ float lred[G];
  __shared__ __attribute__((aligned(16))) float sP[DP];
  __shared__ __attribute__((aligned(16))) float sPP[DP];
  const int tid = threadIdx.x, l = tid & (LPR - 1), grp = tid / LPR;
  const bool adver = hp.adver != 0;

  for (int64_t r = blockIdx.x; r < n; r += gridDim.x) {
    int64_t b0 = off[r], b1 = off[r + 1];
    b0 = b0 < 0 ? 0 : (b0 > T ? T : b0);
    b1 = b1 < b0 ? b0 : (b1 > T ? T : b1);
    RowV<NV> p = zero_row<NV>(), a = zero_row<NV>();  // lane-group 0's copy is the user's state
    if (grp == 0) {
      if (init) p = load_row<LPR, NV>(init, r, d, l);
      if (acc_init) a = load_row<LPR, NV>(acc_init, r, d, l);
      // no acc_init, and the padding chunks of a row (c * 4 >= d; their p and gradient stay 0):
      // 0.1, so that Adagrad's rsqrt stays finite there
#pragma unroll
      for (int v = 0; v < NV; ++v)
        if (!acc_init || (l + LPR * v) * 4 >= d) a.v[v] = make_float4(0.1f, 0.1f, 0.1f, 0.1f);
      store_row<LPR, NV>(sP, 0, DP, l, p);
    }
    __syncthreads();
    for (int e = 0; e < E; ++e) {
      const int32_t* neg = ineg + (int64_t)e * T;
      float eloss = 0.f;
      for (int64_t s0 = b0; s0 < b1; s0 += batch) {
        const int Bs = (int)(b1 - s0 < batch ? b1 - s0 : batch);
        int n2 = 2;
        while (n2 < 2 * Bs) n2 <<= 1;
        const RowV<NV> pr = load_row<LPR, NV>(sP, 0, DP, l);
        // ---- A: clean forward, partial clean gradient of p
        RowV<NV> part = zero_row<NV>();
        float lpart = 0.f;
        for (int b = grp; b < Bs; b += G) {
          const int32_t i = fold_item(ipos[s0 + b], I1), j = fold_item(neg[s0 + b], I1);
          const RowV<NV> qi = load_row<LPR, NV>(Q, i, d, l), qj = load_row<LPR, NV>(Q, j, d, l);
          const float x = dot_row<LPR, NV>(pr, qi) - dot_row<LPR, NV>(pr, qj);
          float g, ls;
          bpr_term(x, hp.clip_lo, hp.clip_hi, g, ls);
          axpy_row(part, g, qi);
          axpy_row(part, -g, qj);
          lpart = lpart + ls;
          if (l == 0) {
            sg[b] = g;
            if (adver) {
              key[b] = ((uint64_t)(uint32_t)i << 32) | (uint32_t)b;
              key[Bs + b] = ((uint64_t)(uint32_t)j << 32) | (uint32_t)(Bs + b);
            }
          }
        }
        store_row<LPR, NV>(red, grp, DP, l, part);
        if (l == 0) lred[grp] = lpart;
        if (adver)
          for (int x = 2 * Bs + tid; x < n2; x += FOLD_BS) key[x] = ~0ull;  // padding sorts last
        __syncthreads();
        // ---- B: sort the item references
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
        // ---- C: clean gradient of p, delta_p
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
            store_row<LPR, NV>(sPP, 0, DP, l, add_row(p, scale_row(scale_row(grad, inv), hp.eps)));
          }
        }
        __syncthreads();
        // ---- D: adversarial forward, partial adversarial gradient of p
        if (adver) {
          const RowV<NV> pp = load_row<LPR, NV>(sPP, 0, DP, l);
          part = zero_row<NV>();
          for (int b = grp; b < Bs; b += G) {
            const int32_t i = fold_item(ipos[s0 + b], I1), j = fold_item(neg[s0 + b], I1);
            const RowV<NV> qi = add_row(load_row<LPR, NV>(Q, i, d, l),
                                        fold_item_delta<LPR, NV>(key, sg, pos[b], n2, Bs, pr, hp.eps));
            const RowV<NV> qj = add_row(load_row<LPR, NV>(Q, j, d, l),
                                        fold_item_delta<LPR, NV>(key, sg, pos[Bs + b], n2, Bs, pr, hp.eps));
            const float x = dot_row<LPR, NV>(pp, qi) - dot_row<LPR, NV>(pp, qj);
            float ga, ls;
            bpr_term(x, hp.clip_lo, hp.clip_hi, ga, ls);
            const float c = hp.reg_adv * ga;
            axpy_row(part, c, qi);
            axpy_row(part, -c, qj);
          }
          store_row<LPR, NV>(red, grp, DP, l, part);
          __syncthreads();
        }
        // ---- E: reg, adversarial partials, Adagrad
        if (grp == 0) {
          if (hp.reg != 0.f) {
            const float coef = (2.0f * hp.reg / ((float)Bs * (float)d)) * (adver ? 2.0f : 1.0f);
            axpy_row(grad, coef * (float)Bs, p);
          }
          if (adver)
            for (int g2 = 0; g2 < G && g2 < Bs; ++g2) grad = add_row(grad, load_row<LPR, NV>(red, g2, DP, l));
#pragma unroll
          for (int v = 0; v < NV; ++v) {
            a.v[v].x = a.v[v].x + grad.v[v].x * grad.v[v].x;
            a.v[v].y = a.v[v].y + grad.v[v].y * grad.v[v].y;
            a.v[v].z = a.v[v].z + grad.v[v].z * grad.v[v].z;
            a.v[v].w = a.v[v].w + grad.v[v].w * grad.v[v].w;
            p.v[v].x = p.v[v].x - (hp.lr * grad.v[v].x) * __builtin_amdgcn_rsqf(a.v[v].x);
            p.v[v].y = p.v[v].y - (hp.lr * grad.v[v].y) * __builtin_amdgcn_rsqf(a.v[v].y);
            p.v[v].z = p.v[v].z - (hp.lr * grad.v[v].z) * __builtin_amdgcn_rsqf(a.v[v].z);
            p.v[v].w = p.v[v].w - (hp.lr * grad.v[v].w) * __builtin_amdgcn_rsqf(a.v[v].w);
          }
          store_row<LPR, NV>(sP, 0, DP, l, p);
        }
        __syncthreads();
      }
      if (loss && tid == 0) loss[(int64_t)e * n + r] = eloss;
    }
    if (grp == 0) {
      store_row<LPR, NV>(P_new, r, d, l, p);
      store_row<LPR, NV>(acc_new, r, d, l, a);
    }
    __syncthreads();  // sP is rewritten for the next user
  }
}

extern "C" int acf_fold_in_users(const float* Q, int64_t I1, int32_t d, const int64_t* user_off, int64_t n,
                                 const int32_t* item_pos, const int32_t* item_neg, int64_t T, int32_t epochs,
                                 int32_t batch, const acf_apr_hparams* hp, const float* init,
                                 const float* acc_init, float* P_new, float* acc_new, float* loss, int32_t check,
                                 void* stream) {
  int r = ops_dim(d);
  if (r) return r;
  if (!Q || !hp || n < 0 || T < 0 || epochs < 0 || I1 <= 0 || I1 > (1ll << 31))
    return acf_set_error(ACF_E_INVALID, "fold_in_users: NULL argument or bad size");
  if (batch < 1 || batch > ACF_FOLD_MAX_BATCH)
    return acf_set_error(ACF_E_INVALID, "fold_in_users: batch must lie in [1, %d], got %d", ACF_FOLD_MAX_BATCH,
                         (int)batch);
  if (hp->adv_mode != 0 || hp->zero_delta != 0)
    return acf_set_error(ACF_E_INVALID, "fold_in_users: only the gradient delta (adv_mode 0, zero_delta 0)");
  if (n == 0) return ACF_OK;
  if (!user_off || !P_new || !acc_new || (T > 0 && (!item_pos || (epochs > 0 && !item_neg))))
    return acf_set_error(ACF_E_INVALID, "fold_in_users: NULL argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (check && T > 0) {  // before anything is written
    int32_t* err = nullptr;
    int32_t herr = 0;
    OPS_TRY(hipMallocAsync((void**)&err, 16, s));
    const int64_t m = T + (int64_t)epochs * T;
    hipError_t e = hipMemsetAsync(err, 0, 16, s);
    if (e == hipSuccess) {
      k_fold_check<<<(unsigned)((m + 255) / 256), 256, 0, s>>>(item_pos, T, item_neg, (int64_t)epochs * T, I1, err);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&herr, err, sizeof(int32_t), hipMemcpyDeviceToHost, s);
    const hipError_t ef = hipFreeAsync(err, s);  // freed on every path
    if (e == hipSuccess) e = ef;
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return acf_set_error(ACF_E_HIP, "fold_in_users range check: %s", hipGetErrorString(e));
    if (herr) return acf_set_error(ACF_E_RANGE, "fold_in_users: item index outside [0, %lld)", (long long)I1);
  }
  const unsigned grid = (unsigned)(n < (1 << 20) ? n : (1 << 20));
  OPS_GEOM(d, (k_fold<LPR, NV><<<grid, FOLD_BS, 0, s>>>(Q, I1, d, user_off, n, T, item_pos, item_neg, epochs, batch,
                                                         *hp, init, acc_init, P_new, acc_new, loss)));
  OPS_TRY(hipGetLastError());
  return ACF_OK;
}
