// acf_grid.hip — grid training of libacf_apr.so: M APR/BPR models ("members") over ONE triplet
// stream in one call (acf_apr_grid_workspace, acf_apr_grid_train, and their _pgd siblings with a
// K-step inner attack per member).  The members
// share the plan, which depends on the triplets alone, and differ in their tables
// ([M][rows][dim], member-major) and in their hyper-parameters.  Context-free: everything
// lives in the caller's workspace.  Nothing here touches the step kernels, k_stream or the
// plans of acf_apr.hip / acf_plan.hip, and they launch nothing of this unit.
//
// Plan (k_grid_plan, one workgroup per batch, once per call).  Every triplet t of a batch
// contributes four terms e = br * B + t, numbered in the concat order of the reference's
// IndexedSlices (acf_adv_direction's order, per batch):
//   br 0  row user[t] of P:  +g_t * q_i      br 2  row ipos[t] of Q:  +g_t * p_u
//   br 1  row user[t] of P:  -g_t * q_j      br 3  row ineg[t] of Q:  -g_t * p_u
// The 4B terms are sorted by the 64-bit key (table, row, e) in a workgroup radix sort (the keys
// are distinct, so the order is total); a run of equal (table, row) is a "slot", one unique row
// of the batch, its terms in ascending e.  Per batch the plan holds the slot count, per slot its
// row key and first term, the sorted e, and per triplet the slots of its three rows.
//
// Schedule: three launches per batch, a lane-group of LPR lanes per (member, slot), members of
// a slot adjacent in the grid (unit = slot * M + member), so a slot's records are read by
// neighbouring lane-groups of one workgroup.
//   k_grid_sum<GRID_CLEAN>  reads the tables; per unit the clean gradient G0 of the row (terms in
//                        plan order, 256 at a time) and delta = eps * l2norm(G0) go to scratch;
//                        the user-row owner writes the triplets' clean loss.  A BPR member's G
//                        (with its reg term) is final here.
//   k_grid_sum<GRID_ADV>  adversarial (APR members only): reads the tables and every delta of the
//                        batch; G = G0 + reg term + reg_adv * G_adv over its own scratch row.
//   k_grid_apply         Adagrad on the unit's own table row: the only writes to the tables.
// K-step members (acf_apr_grid_train_pgd, K = adv_iters[m] > 1, alpha = adv_step[m]): the clean
// launch leaves delta_1 = project(alpha * l2norm(G0)), and max(K) - 1 launches of
//   k_grid_sum<GRID_INNER>  (launch k = 1 .. max(K) - 1) follow it: the batch gradient at
//                        (P + delta_k, Q + delta_k), summed as above, normalised, and
//                        delta_{k+1} = project(delta_k + alpha * n) onto the eps ball
//                        (k_adv_pgd_step's arithmetic, restated for a lane-group).
// Delta is double-buffered with a PER-MEMBER PARITY: delta_k of member m lives in buffer
// (k - 1) & 1 of m's own scratch slice.  Inner launch k reads the member's buffer (k - 1) & 1 and
// writes its buffer k & 1; a unit whose member has K < k + 1 returns at once and touches nothing,
// and the adversarial launch reads buffer (K - 1) & 1 of each member, where its delta_K was left.
// A unit reads deltas of its own member only, so members of different K never meet in a buffer.
// K = 1 is today's member: one buffer, eps * l2norm(G0), alpha unread; acf_apr_grid_train launches
// instances compiled without the K-step branches (PGD = false), the same arithmetic.
// No launch reads a table row or a delta that a workgroup of the same launch writes; a unit
// writes only its own scratch row and, in k_grid_apply, its own table row.  No float atomics:
// every sum's order is the plan's.  A unit's arithmetic depends on LPR (that is, on dim) alone,
// never on M, on the other members' K or on the unit's place in the grid.
// Build: one hipcc line with acf_apr.hip and the library's other units, same flags.

#include <hip/hip_runtime.h>
#include <rocprim/block/block_radix_sort.hpp>
#include <rocprim/block/block_scan.hpp>

#include "acf_apr.h"
#include "acf_host.h"  // HIP_TRY, ACF_CHECK, ACF_RET, DISPATCH_LPR, read_range_err
#include "acf_rows.h"  // load_row, dot_row, bpr_term, l2_delta, adagrad_apply

namespace {

constexpr int GRID_CHUNK = 256;      // terms per partial sum: part of the bit contract, not a knob
constexpr int GRID_EBITS = 12;       // e < 4 * ACF_GRID_MAX_BATCH = 2^12
constexpr int GRID_WG = 256;

struct GridHP {  // what a member's kernels read of its acf_apr_hparams
  float lr, eps, reg, reg_adv, lo, hi;
  int32_t iters;  // 0: a BPR member; else K, the steps of the attack (1: the one-step delta)
  float alpha;    // the step size of a K > 1 member
};

struct GridHPs {  // by value to k_grid_hp: 2 KiB of kernel arguments
  GridHP h[ACF_GRID_MAX_MODELS];
};

// The members' hyper-parameters, from kernel arguments to the workspace (the caller's hp is host
// memory; a copy from pageable memory would wait on the stream).  Static indices only: the
// arguments stay in scalar registers.
__global__ void __launch_bounds__(64) k_grid_hp(GridHPs a, int32_t M, GridHP* __restrict__ out) {
#pragma unroll
  for (int k = 0; k < ACF_GRID_MAX_MODELS; ++k)
    if ((int)threadIdx.x == k && k < M) out[k] = a.h[k];
}

__device__ __forceinline__ int32_t grid_clamp(int32_t x, int64_t rows) { return (x < 0 || x >= rows) ? 0 : x; }

// One batch's plan records inside the workspace (S = 3B slots at most).
struct GridPlan {
  int32_t* hdr;    // [nb]            slots of batch b
  uint32_t* srow;  // [nb][S]         row key of a slot: user row r -> r, item row r -> U1 + r
  int32_t* soff;   // [nb][S + 1]     first sorted term of a slot; soff[slots] = 4B
  uint16_t* te;    // [nb][4B]        sorted terms e
  uint16_t* ts;    // [nb][3][B]      slot of user[t], ipos[t], ineg[t]
};

template <int IPT>
__global__ void __launch_bounds__(GRID_WG) k_grid_plan(const int32_t* __restrict__ user,
                                                       const int32_t* __restrict__ ipos,
                                                       const int32_t* __restrict__ ineg, int32_t B, int64_t U1,
                                                       int64_t I1, int end_bit, GridPlan pl,
                                                       int32_t* __restrict__ err) {
  using Sort = rocprim::block_radix_sort<uint64_t, GRID_WG, IPT>;
  using Scan = rocprim::block_scan<int32_t, GRID_WG>;
  __shared__ union {
    typename Sort::storage_type sort;
    uint64_t key[GRID_WG * IPT];
  } sm;
  __shared__ typename Scan::storage_type scan_st;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int32_t T = 4 * B, S = 3 * B;
  const int32_t* ub = user + b * B;
  const int32_t* ib = ipos + b * B;
  const int32_t* jb = ineg + b * B;
  uint64_t keys[IPT];
#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    const int32_t e = tid * IPT + k;
    keys[k] = ~0ull;  // padding: above every term
    if (e < T) {
      const int br = e / B;
      const int32_t t = e - br * B;
      int32_t r = br < 2 ? ub[t] : (br == 2 ? ib[t] : jb[t]);
      const int64_t rows = br < 2 ? U1 : I1;
      if (r < 0 || r >= rows) {
        atomicOr(err, br < 2 ? 1 : 2);
        r = 0;
      }
      keys[k] = ((uint64_t)(br < 2 ? r : U1 + r) << GRID_EBITS) | (uint64_t)e;
    }
  }
  Sort().sort(keys, sm.sort, 0u, (unsigned)end_bit);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < IPT; ++k) sm.key[tid * IPT + k] = keys[k];
  __syncthreads();
  bool head[IPT];
  int32_t cnt = 0;
#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    const int q = tid * IPT + k;
    head[k] = q < T && (q == 0 || (sm.key[q - 1] >> GRID_EBITS) != (keys[k] >> GRID_EBITS));
    cnt += head[k] ? 1 : 0;
  }
  int32_t run, total;
  Scan().exclusive_scan(cnt, run, 0, total, scan_st);
  uint32_t* srow = pl.srow + b * S;
  int32_t* soff = pl.soff + b * (S + 1);
  uint16_t* te = pl.te + b * T;
  uint16_t* ts = pl.ts + b * S;
#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    const int q = tid * IPT + k;
    if (q >= T) continue;
    if (head[k]) {
      if (run < S) {  // always true: a batch has at most 3B distinct rows
        srow[run] = (uint32_t)(keys[k] >> GRID_EBITS);
        soff[run] = q;
      }
      ++run;
    }
    const int32_t e = (int32_t)(keys[k] & ((1u << GRID_EBITS) - 1));
    const int br = e / B;
    const int32_t t = e - br * B;
    te[q] = (uint16_t)e;
    if (br != 1 && t < B) ts[(br == 0 ? 0 : br - 1) * B + t] = (uint16_t)(run - 1);
  }
  if (tid == 0) {
    pl.hdr[b] = total < S ? total : S;
    soff[total < S ? total : S] = T;
  }
}

// What the step launches of one batch read (by value).
struct GridArgs {
  float *P, *Q, *accP, *accQ;                 // [M][rows][d]
  const int32_t *user, *ipos, *ineg;          // this batch's triplets
  const GridHP* hp;                           // [M]
  const int32_t* hdr;                         // this batch's plan records
  const uint32_t* srow;
  const int32_t* soff;
  const uint16_t* te;
  const uint16_t* ts;
  float *delta[2], *G;                        // scratch [M][S][d]; delta[1]: K-step members only
  float *lc, *la;                             // member 0's losses of this batch, or NULL
  int64_t U1, I1, nloss;                      // nloss: a member's stride in lc / la
  int32_t M, B, d, S;
  int32_t it;                                 // GRID_INNER: the launch k, which makes delta_{k+1}
};

// Unit (member m, slot s) of this lane-group; false: none.
template <int LPR>
__device__ __forceinline__ bool grid_unit(const GridArgs& a, int& m, int& s, int& l) {
  const int64_t unit = (blockIdx.x * (int64_t)GRID_WG + threadIdx.x) / LPR;
  l = threadIdx.x & (LPR - 1);
  const int64_t sl = unit / a.M;
  if (sl >= a.hdr[0]) return false;
  s = (int)sl;
  m = (int)(unit - sl * a.M);
  return true;
}

enum { GRID_CLEAN = 0, GRID_ADV = 1, GRID_INNER = 2 };

// delta' = project(delta + alpha * n) onto the L2 ball of radius eps, n = l2norm(g):
// v = delta + alpha * n (the product rounded, then the sum), s = sqrt(dot_row(v, v)),
// delta' = v when s <= eps (s = 0 included), else v * (eps / s).
template <int LPR>
__device__ __forceinline__ RowV<1> grid_pgd_step(const RowV<1>& delta, const RowV<1>& g, float alpha, float eps) {
  RowV<1> v = add_row(delta, scale_row(l2_delta<LPR, 1>(g, 1.0f), alpha));
  const float s = sqrtf(dot_row<LPR, 1>(v, v));
  if (!(s <= eps)) v = scale_row(v, eps / s);
  return v;
}

// PGD: an instance of acf_apr_grid_train_pgd, where a member may have K > 1.  The instances of
// acf_apr_grid_train (every K = 1, one delta buffer) are compiled without any of it.
template <int LPR, int MODE, bool PGD>
__global__ void __launch_bounds__(GRID_WG) k_grid_sum(GridArgs a) {
  static_assert(PGD || MODE != GRID_INNER, "the inner launch belongs to the K-step entry");
  constexpr bool ADV = MODE != GRID_CLEAN;  // the triplets' rows are taken at the perturbed point
  int m, s, l;
  if (!grid_unit<LPR>(a, m, s, l)) return;
  const GridHP h = a.hp[m];
  const bool adver = h.iters != 0;
  if (ADV && !adver) return;
  if (MODE == GRID_INNER && h.iters < a.it + 1) return;  // this member's delta_K is already in place
  const int d = a.d, B = a.B;
  const float* Pm = a.P + (int64_t)m * a.U1 * d;
  const float* Qm = a.Q + (int64_t)m * a.I1 * d;
  // the member's delta_k is in buffer (k - 1) & 1: GRID_INNER k reads that and writes k & 1,
  // GRID_ADV reads delta_K, GRID_CLEAN writes delta_1
  const int src = MODE == GRID_INNER ? (a.it - 1) & 1 : (PGD && MODE == GRID_ADV ? (h.iters - 1) & 1 : 0);
  float* dl = a.delta[src] + (int64_t)m * a.S * d;
  float* Gm = a.G + (int64_t)m * a.S * d;
  float* loss = MODE == GRID_ADV ? a.la : (MODE == GRID_CLEAN ? a.lc : nullptr);
  const uint32_t key = a.srow[s];
  const bool is_user = (int64_t)key < a.U1;
  const int32_t o = a.soff[s], cnt = a.soff[s + 1] - o;
  RowV<1> tot = zero_row<1>();
  for (int32_t c0 = 0; c0 < cnt; c0 += GRID_CHUNK) {  // partial sums of 256 terms, added in order
    const int32_t c1 = c0 + GRID_CHUNK < cnt ? c0 + GRID_CHUNK : cnt;
    RowV<1> acc = zero_row<1>();
    for (int32_t x = c0; x < c1; ++x) {
      const int32_t e = a.te[o + x];
      const int br = e / B;
      const int32_t t = e - br * B;
      const int32_t u = grid_clamp(a.user[t], a.U1), i = grid_clamp(a.ipos[t], a.I1),
                    j = grid_clamp(a.ineg[t], a.I1);
      RowV<1> p = load_row<LPR, 1>(Pm, u, d, l);
      RowV<1> qi = load_row<LPR, 1>(Qm, i, d, l);
      RowV<1> qj = load_row<LPR, 1>(Qm, j, d, l);
      if (ADV) {
        p = add_row(p, load_row<LPR, 1>(dl, a.ts[t], d, l));
        qi = add_row(qi, load_row<LPR, 1>(dl, a.ts[B + t], d, l));
        qj = add_row(qj, load_row<LPR, 1>(dl, a.ts[2 * B + t], d, l));
      }
      const float sc = dot_row<LPR, 1>(p, qi) - dot_row<LPR, 1>(p, qj);
      float g, ls;
      bpr_term(sc, h.lo, h.hi, g, ls);
      if (br == 0 && l == 0 && loss) loss[(int64_t)m * a.nloss + t] = ls;
      axpy_row(acc, (br & 1) ? -g : g, br == 0 ? qi : (br == 1 ? qj : p));
    }
    tot = c0 == 0 ? acc : add_row(tot, acc);
  }
  // reg: 2 reg w / (B d) per occurrence, twice in the APR graph
  const float coef = (2.0f * h.reg / ((float)B * (float)d)) * (adver ? 2.0f : 1.0f) *
                     (float)(is_user ? cnt / 2 : cnt);
  if (MODE == GRID_INNER) {
    float* dn = a.delta[src ^ 1] + (int64_t)m * a.S * d;
    store_row<LPR, 1>(dn, s, d, l, grid_pgd_step<LPR>(load_row<LPR, 1>(dl, s, d, l), tot, h.alpha, h.eps));
    return;
  }
  const int64_t row = is_user ? (int64_t)key : (int64_t)key - a.U1;
  if (MODE == GRID_CLEAN) {
    if (adver) {
      store_row<LPR, 1>(dl, s, d, l,
                        PGD && h.iters > 1 ? grid_pgd_step<LPR>(zero_row<1>(), tot, h.alpha, h.eps)
                                    : l2_delta<LPR, 1>(tot, h.eps));
    } else if (h.reg != 0.f) {
      axpy_row(tot, coef, load_row<LPR, 1>(is_user ? Pm : Qm, row, d, l));
    }
    store_row<LPR, 1>(Gm, s, d, l, tot);
  } else {
    RowV<1> G = load_row<LPR, 1>(Gm, s, d, l);
    if (h.reg != 0.f) axpy_row(G, coef, load_row<LPR, 1>(is_user ? Pm : Qm, row, d, l));
    axpy_row(G, h.reg_adv, tot);
    store_row<LPR, 1>(Gm, s, d, l, G);
  }
}

template <int LPR>
__global__ void __launch_bounds__(GRID_WG) k_grid_apply(GridArgs a) {
  int m, s, l;
  if (!grid_unit<LPR>(a, m, s, l)) return;
  const int d = a.d;
  const uint32_t key = a.srow[s];
  const bool is_user = (int64_t)key < a.U1;
  const int64_t row = is_user ? (int64_t)key : (int64_t)key - a.U1;
  const int64_t base = (int64_t)m * (is_user ? a.U1 : a.I1) * d;
  float* W = (is_user ? a.P : a.Q) + base;
  float* A = (is_user ? a.accP : a.accQ) + base;
  const RowV<1> G = load_row<LPR, 1>(a.G + (int64_t)m * a.S * d, s, d, l);
  RowV<1> w = load_row<LPR, 1>(W, row, d, l);
  RowV<1> acc = load_row<LPR, 1>(A, row, d, l);
  adagrad_apply(w, acc, G, a.hp[m].lr);
  store_row<LPR, 1>(W, row, d, l, w);
  store_row<LPR, 1>(A, row, d, l, acc);
}

template <int LPR>
void launch_clean(const GridArgs& a, unsigned grid, hipStream_t s) {
  hipLaunchKernelGGL((k_grid_sum<LPR, GRID_CLEAN, false>), dim3(grid), dim3(GRID_WG), 0, s, a);
}
template <int LPR>
void launch_clean_pgd(const GridArgs& a, unsigned grid, hipStream_t s) {
  hipLaunchKernelGGL((k_grid_sum<LPR, GRID_CLEAN, true>), dim3(grid), dim3(GRID_WG), 0, s, a);
}
template <int LPR>
void launch_adv(const GridArgs& a, unsigned grid, hipStream_t s) {
  hipLaunchKernelGGL((k_grid_sum<LPR, GRID_ADV, false>), dim3(grid), dim3(GRID_WG), 0, s, a);
}
template <int LPR>
void launch_adv_pgd(const GridArgs& a, unsigned grid, hipStream_t s) {
  hipLaunchKernelGGL((k_grid_sum<LPR, GRID_ADV, true>), dim3(grid), dim3(GRID_WG), 0, s, a);
}
template <int LPR>
void launch_inner(const GridArgs& a, unsigned grid, hipStream_t s) {
  hipLaunchKernelGGL((k_grid_sum<LPR, GRID_INNER, true>), dim3(grid), dim3(GRID_WG), 0, s, a);
}
template <int LPR>
void launch_apply(const GridArgs& a, unsigned grid, hipStream_t s) {
  hipLaunchKernelGGL((k_grid_apply<LPR>), dim3(grid), dim3(GRID_WG), 0, s, a);
}

// ---- host: workspace layout --------------------------------------------------
struct GridLayout {
  size_t err, hp, hdr, srow, soff, te, ts, delta, G, delta2, total;
};

inline size_t grid_up(size_t x) { return (x + 255) & ~(size_t)255; }

// pgd: the second delta buffer of K-step members, after everything else
GridLayout grid_layout(int32_t M, int32_t B, int32_t nb, int32_t d, bool pgd) {
  GridLayout L;
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t a = at;
    at += grid_up(bytes);
    return a;
  };
  const size_t S = (size_t)3 * B, n = (size_t)nb;
  L.err = take(sizeof(int32_t));
  L.hp = take(sizeof(GridHP) * ACF_GRID_MAX_MODELS);
  L.hdr = take(n * 4);
  L.srow = take(n * S * 4);
  L.soff = take(n * (S + 1) * 4);
  L.te = take(n * 4 * B * 2);
  L.ts = take(n * S * 2);
  L.delta = take((size_t)M * S * d * sizeof(float));
  L.G = take((size_t)M * S * d * sizeof(float));
  L.delta2 = pgd ? take((size_t)M * S * d * sizeof(float)) : 0;
  L.total = at;
  return L;
}

int grid_check_shape(int32_t M, int32_t B, int32_t nb, int64_t U1, int64_t I1, int32_t d) {
  ACF_CHECK(M >= 1 && M <= ACF_GRID_MAX_MODELS, ACF_E_INVALID, "n_models must be in [1, %d], got %d",
            ACF_GRID_MAX_MODELS, (int)M);
  ACF_CHECK(d >= 4 && d <= 256 && d % 4 == 0, ACF_E_INVALID, "grid dim must be a multiple of 4 in [4, 256], got %d",
            (int)d);
  ACF_CHECK(B >= 1 && B <= ACF_GRID_MAX_BATCH, ACF_E_INVALID, "batch_size must be in [1, %d], got %d",
            ACF_GRID_MAX_BATCH, (int)B);
  ACF_CHECK(nb >= 0 && (int64_t)nb * B < ((int64_t)1 << 31), ACF_E_INVALID,
            "n_batches must be >= 0 with fewer than 2^31 triplets, got %d", (int)nb);
  ACF_CHECK(U1 >= 1 && I1 >= 1 && U1 + I1 <= ((int64_t)1 << 31), ACF_E_INVALID,
            "table rows must be positive with at most 2^31 rows in all, got %lld + %lld", (long long)U1,
            (long long)I1);
  return ACF_OK;
}

int grid_workspace(int32_t M, int32_t B, int32_t nb, int64_t U1, int64_t I1, int32_t d, bool pgd, size_t* bytes) {
  ACF_CHECK(bytes, ACF_E_INVALID, "bytes is NULL");
  ACF_RET(grid_check_shape(M, B, nb, U1, I1, d));
  *bytes = grid_layout(M, B, nb, d, pgd).total;
  return ACF_OK;
}

// Both entries.  pgd: acf_apr_grid_train_pgd (adv_iters, adv_step and the second delta buffer);
// else every member has K = 1.
int grid_train(float* P, float* Q, float* accP, float* accQ, int32_t M, int64_t U1, int64_t I1, int32_t d,
               const acf_apr_hparams* hp, bool pgd, const int32_t* adv_iters, const float* adv_step,
               const int32_t* user, const int32_t* item_pos, const int32_t* item_neg, int32_t B, int32_t nb,
               float* loss_clean, float* loss_adv, void* workspace, size_t workspace_bytes, int32_t check,
               void* stream);

}  // namespace

extern "C" int acf_apr_grid_workspace(int32_t n_models, int32_t batch_size, int32_t n_batches,
                                      int64_t num_user_rows, int64_t num_item_rows, int32_t dim, size_t* bytes) {
  return grid_workspace(n_models, batch_size, n_batches, num_user_rows, num_item_rows, dim, false, bytes);
}

extern "C" int acf_apr_grid_pgd_workspace(int32_t n_models, int32_t batch_size, int32_t n_batches,
                                          int64_t num_user_rows, int64_t num_item_rows, int32_t dim,
                                          size_t* bytes) {
  return grid_workspace(n_models, batch_size, n_batches, num_user_rows, num_item_rows, dim, true, bytes);
}

extern "C" int acf_apr_grid_train(float* P, float* Q, float* accP, float* accQ, int32_t n_models,
                                  int64_t num_user_rows, int64_t num_item_rows, int32_t dim,
                                  const acf_apr_hparams* hp, const int32_t* user, const int32_t* item_pos,
                                  const int32_t* item_neg, int32_t batch_size, int32_t n_batches,
                                  float* loss_clean, float* loss_adv, void* workspace, size_t workspace_bytes,
                                  int32_t check, void* stream) {
  return grid_train(P, Q, accP, accQ, n_models, num_user_rows, num_item_rows, dim, hp, false, nullptr, nullptr, user,
                    item_pos, item_neg, batch_size, n_batches, loss_clean, loss_adv, workspace, workspace_bytes,
                    check, stream);
}

extern "C" int acf_apr_grid_train_pgd(float* P, float* Q, float* accP, float* accQ, int32_t n_models,
                                      int64_t num_user_rows, int64_t num_item_rows, int32_t dim,
                                      const acf_apr_hparams* hp, const int32_t* adv_iters, const float* adv_step,
                                      const int32_t* user, const int32_t* item_pos, const int32_t* item_neg,
                                      int32_t batch_size, int32_t n_batches, float* loss_clean, float* loss_adv,
                                      void* workspace, size_t workspace_bytes, int32_t check, void* stream) {
  return grid_train(P, Q, accP, accQ, n_models, num_user_rows, num_item_rows, dim, hp, true, adv_iters, adv_step,
                    user, item_pos, item_neg, batch_size, n_batches, loss_clean, loss_adv, workspace,
                    workspace_bytes, check, stream);
}

namespace {

int grid_train(float* P, float* Q, float* accP, float* accQ, int32_t M, int64_t U1, int64_t I1, int32_t d,
               const acf_apr_hparams* hp, bool pgd, const int32_t* adv_iters, const float* adv_step,
               const int32_t* user, const int32_t* item_pos, const int32_t* item_neg, int32_t B, int32_t nb,
               float* loss_clean, float* loss_adv, void* workspace, size_t workspace_bytes, int32_t check,
               void* stream) {
  ACF_CHECK(P && Q && accP && accQ, ACF_E_INVALID, "a table pointer is NULL");
  ACF_CHECK(hp, ACF_E_INVALID, "hp is NULL");
  ACF_CHECK(!pgd || (adv_iters && adv_step), ACF_E_INVALID, "adv_iters or adv_step is NULL");
  ACF_RET(grid_check_shape(M, B, nb, U1, I1, d));
  ACF_CHECK(nb == 0 || (user && item_pos && item_neg), ACF_E_INVALID, "a triplet pointer is NULL");
  bool any_adv = false;
  int32_t max_iters = 1;  // over the APR members: a BPR member has no delta
  GridHPs hps;
  for (int m = 0; m < ACF_GRID_MAX_MODELS; ++m) hps.h[m] = GridHP{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0, 0.f};
  for (int m = 0; m < M; ++m) {
    ACF_CHECK(hp[m].adv_mode == 0, ACF_E_INVALID, "member %d: adv_mode %d (random delta) is not a grid mode", m,
              (int)hp[m].adv_mode);
    ACF_CHECK(hp[m].zero_delta == 0, ACF_E_INVALID, "member %d: zero_delta is not a grid mode", m);
    const int32_t K = pgd ? adv_iters[m] : 1;
    const float alpha = pgd ? adv_step[m] : 0.f;
    ACF_CHECK(K >= 1 && K <= ACF_GRID_MAX_ADV_ITERS, ACF_E_INVALID, "member %d: adv_iters must be in [1, %d], got %d",
              m, ACF_GRID_MAX_ADV_ITERS, (int)K);
    ACF_CHECK(alpha >= 0.f && alpha <= 3.402823466e38f, ACF_E_INVALID,
              "member %d: adv_step must be finite and >= 0, got %g", m, (double)alpha);
    hps.h[m] = GridHP{hp[m].lr, hp[m].eps, hp[m].reg, hp[m].reg_adv, hp[m].clip_lo, hp[m].clip_hi,
                      hp[m].adver ? K : 0, alpha};
    any_adv = any_adv || hp[m].adver;
    if (hp[m].adver && K > max_iters) max_iters = K;
  }
  const GridLayout L = grid_layout(M, B, nb, d, pgd);
  ACF_CHECK(workspace, ACF_E_INVALID, "workspace is NULL");
  ACF_CHECK(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, ACF_E_INVALID, "workspace must be 16-byte aligned");
  ACF_CHECK(workspace_bytes >= L.total, ACF_E_INVALID, "workspace of %zu bytes, %zu needed", workspace_bytes,
            L.total);
  if (nb == 0) return ACF_OK;
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int32_t* err = (int32_t*)(ws + L.err);
  GridHP* dhp = (GridHP*)(ws + L.hp);
  GridPlan pl{(int32_t*)(ws + L.hdr), (uint32_t*)(ws + L.srow), (int32_t*)(ws + L.soff), (uint16_t*)(ws + L.te),
              (uint16_t*)(ws + L.ts)};
  const int32_t S = 3 * B, T = 4 * B;

  // plan: once, from the triplets alone
  HIP_TRY(hipMemsetAsync(err, 0, sizeof(int32_t), s));
  int rb = 1;
  while (((int64_t)1 << rb) < U1 + I1) ++rb;
  const int end_bit = GRID_EBITS + rb + 1;  // the padding key's next bit is set: it sorts last
  if (T <= GRID_WG)
    hipLaunchKernelGGL(k_grid_plan<1>, dim3(nb), dim3(GRID_WG), 0, s, user, item_pos, item_neg, B, U1, I1, end_bit,
                       pl, err);
  else if (T <= GRID_WG * 4)
    hipLaunchKernelGGL(k_grid_plan<4>, dim3(nb), dim3(GRID_WG), 0, s, user, item_pos, item_neg, B, U1, I1, end_bit,
                       pl, err);
  else if (T <= GRID_WG * 8)
    hipLaunchKernelGGL(k_grid_plan<8>, dim3(nb), dim3(GRID_WG), 0, s, user, item_pos, item_neg, B, U1, I1, end_bit,
                       pl, err);
  else
    hipLaunchKernelGGL(k_grid_plan<16>, dim3(nb), dim3(GRID_WG), 0, s, user, item_pos, item_neg, B, U1, I1, end_bit,
                       pl, err);
  HIP_TRY(hipGetLastError());
  if (check) ACF_RET(read_range_err(err, s));  // one sync, before any table is written
  hipLaunchKernelGGL(k_grid_hp, dim3(1), dim3(64), 0, s, hps, M, dhp);
  HIP_TRY(hipGetLastError());

  GridArgs a;
  a.P = P, a.Q = Q, a.accP = accP, a.accQ = accQ;
  a.hp = dhp;
  a.delta[0] = (float*)(ws + L.delta), a.delta[1] = pgd ? (float*)(ws + L.delta2) : nullptr;
  a.G = (float*)(ws + L.G);
  a.it = 0;
  a.U1 = U1, a.I1 = I1, a.nloss = (int64_t)nb * B;
  a.M = M, a.B = B, a.d = d, a.S = S;
  int lpr = 1;
  while (lpr * 4 < d) lpr <<= 1;
  const unsigned grid = (unsigned)(((int64_t)S * M * lpr + GRID_WG - 1) / GRID_WG);
  for (int64_t b = 0; b < nb; ++b) {
    a.user = user + b * B, a.ipos = item_pos + b * B, a.ineg = item_neg + b * B;
    a.hdr = pl.hdr + b, a.srow = pl.srow + b * S, a.soff = pl.soff + b * (S + 1);
    a.te = pl.te + b * T, a.ts = pl.ts + b * S;
    a.lc = loss_clean ? loss_clean + b * B : nullptr;
    a.la = loss_adv ? loss_adv + b * B : nullptr;
    if (pgd) {
      ACF_RET(DISPATCH_LPR(d, launch_clean_pgd, a, grid, s));
      for (a.it = 1; a.it < max_iters; ++a.it) ACF_RET(DISPATCH_LPR(d, launch_inner, a, grid, s));
      if (any_adv) ACF_RET(DISPATCH_LPR(d, launch_adv_pgd, a, grid, s));
    } else {
      ACF_RET(DISPATCH_LPR(d, launch_clean, a, grid, s));
      if (any_adv) ACF_RET(DISPATCH_LPR(d, launch_adv, a, grid, s));
    }
    ACF_RET(DISPATCH_LPR(d, launch_apply, a, grid, s));
  }
  HIP_TRY(hipGetLastError());
  return ACF_OK;
}

}  // namespace
