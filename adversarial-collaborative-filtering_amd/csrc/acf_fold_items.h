// Fold-in of new items against frozen user and item tables: the item side of
// k_fold (FoldItems) and acf_fold_in_items.  Included by acf_ops.hip after
// acf_fold.h, which holds the kernel frame; one translation unit.  DESIGN.md §4i.
//
// acf_fold_in_items: new item r of a CSR (item_off, user_pos) takes, for epoch
// e = 0..E-1 and every consecutive slice of at most `batch` of its positions, ONE
// training_batch iteration (APR.py:143-195) on the tables P and [Q ; q_r] -- q_r
// appended as row I1 = num_item_rows -- with the batch
// {(user_pos[k], I1, item_neg[e][k])}.  Only q_r and its Adagrad accumulator are
// kept: P and Q are read-only, there is no accP and no accQ.
//
// A negative can never equal the new item: that item has no row in Q, negatives
// lie in [0, I1), so the i == j case of the user side does not exist here, and
// q_r is referenced by the pos branch of every triplet and by nothing else.
//
// The frame's stages with this side's rows:
//   A. p_u, q_j, x = p_u.q_r - p_u.q_j; the partial clean gradient of q_r is the
//      sum of g * p_u;
//   B. the Bs user references (u, e) and the Bs negative references (j, Bs + e),
//      the latter tagged in bit 63: the references of one user row lie together
//      in triplet order, and so do those of one negative row;
//   D. the clean gradient of a triplet's user row is the ordered sum of
//      (+g_e * q_r) over the row's references, then of (-g_e * q_{j_e}) over them
//      (the IndexedSlices concat order: pos branch, then neg branch); that of its
//      negative row the ordered sum of (-g_e * p_{u_e}); a delta from each; the
//      adversarial forward on p_u + delta_p, q_r + delta_q, q_j + delta_j; the
//      partial adversarial gradient of q_r is the sum of (reg_adv * g_a) *
//      (p_u + delta_p).  Rows of other triplets are fetched again (they are in L2
//      from A).

struct FoldItems {
  static constexpr uint64_t NEG_TAG = 1ull << 63;  // indices are below 2^31: the tag keeps the two families apart

  // w: q_r (D: q_r + delta_q); f, qj: p_u, q_j (D: perturbed)
  template <int LPR, int NV>
  static __device__ __forceinline__ float score(const RowV<NV>& w, const RowV<NV>& f, const RowV<NV>& qj) {
    return dot_row<LPR, NV>(f, w) - dot_row<LPR, NV>(f, qj);
  }

  template <int NV>
  static __device__ __forceinline__ void grad(RowV<NV>& part, float c, const RowV<NV>& f, const RowV<NV>&) {
    axpy_row(part, c, f);
  }

  // delta of the user row of triplet b (reference s): the row's references hold
  // (u << 32 | e); the clean gradient is sum_e g[e] * q_r, then sum_e -g[e] * q_{j_e},
  // each in reference order.  qj: q_{j_b}, already loaded.
  template <int LPR, int NV>
  static __device__ __forceinline__ RowV<NV> user_delta(const FoldSlice& sl, int s, int b, int l, float eps,
                                                        const RowV<NV>& qr, const RowV<NV>& qj) {
    const int a = fold_run(sl.key, s);
    const uint32_t row = (uint32_t)(sl.key[s] >> 32);
    RowV<NV> G = zero_row<NV>();
    for (int x = a; x < 2 * sl.Bs && (uint32_t)(sl.key[x] >> 32) == row; ++x)
      axpy_row(G, sl.g[(uint32_t)sl.key[x]], qr);
    for (int x = a; x < 2 * sl.Bs && (uint32_t)(sl.key[x] >> 32) == row; ++x) {
      const int e = (int)(uint32_t)sl.key[x];
      axpy_row(G, -sl.g[e], e == b ? qj : sl.neg_row<LPR, NV>(e, l));
    }
    return l2_delta<LPR, NV>(G, eps);
  }

  // delta of the negative row of triplet b (reference s): references
  // (tag | j << 32 | Bs + e); the clean gradient is sum_e -g[e] * p_{u_e} in
  // reference order.  pu: p_{u_b}, already loaded.
  template <int LPR, int NV>
  static __device__ __forceinline__ RowV<NV> neg_delta(const FoldSlice& sl, int s, int b, int l, float eps,
                                                       const RowV<NV>& pu) {
    const uint32_t row = (uint32_t)(sl.key[s] >> 32);
    RowV<NV> G = zero_row<NV>();
    for (int x = fold_run(sl.key, s); x < 2 * sl.Bs && (uint32_t)(sl.key[x] >> 32) == row; ++x) {
      const int e = (int)(uint32_t)sl.key[x] - sl.Bs;
      axpy_row(G, -sl.g[e], e == b ? pu : sl.first_row<LPR, NV>(e, l));
    }
    return l2_delta<LPR, NV>(G, eps);
  }

  // D: p_u + delta_p, q_j + delta_j of triplet b
  template <int LPR, int NV>
  static __device__ __forceinline__ void perturbed(const FoldSlice& sl, int b, int l, float eps, const RowV<NV>& qr,
                                                   RowV<NV>& f, RowV<NV>& qj) {
    const RowV<NV> pu = sl.first_row<LPR, NV>(b, l), q = sl.neg_row<LPR, NV>(b, l);
    f = add_row(pu, user_delta<LPR, NV>(sl, sl.pos[b], b, l, eps, qr, q));
    qj = add_row(q, neg_delta<LPR, NV>(sl, sl.pos[sl.Bs + b], b, l, eps, pu));
  }
};

extern "C" int acf_fold_in_items(const float* P, int64_t U1, const float* Q, int64_t I1, int32_t d,
                                 const int64_t* item_off, int64_t n, const int32_t* user_pos,
                                 const int32_t* item_neg, int64_t T, int32_t epochs, int32_t batch,
                                 const acf_apr_hparams* hp, const float* init, const float* acc_init, float* Q_new,
                                 float* acc_new, float* loss, int32_t check, void* stream) {
  const bool tables = P && Q && U1 > 0 && U1 <= (1ll << 31) && I1 > 0 &&
                      I1 < (1ll << 31);  // the new item's own id, I1, is an int32 too
  const int r = fold_in<FoldItems>("fold_in_items", tables, P, U1, Q, I1, d, item_off, n, user_pos, item_neg, T,
                                   epochs, batch, hp, init, acc_init, Q_new, acc_new, loss, check, stream);
  if (r == ACF_E_RANGE)
    return acf_set_error(r, "fold_in_items: user outside [0, %lld) or negative outside [0, %lld)", (long long)U1,
                         (long long)I1);
  return r;
}
