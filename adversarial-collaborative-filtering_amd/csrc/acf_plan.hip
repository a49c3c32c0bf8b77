// acf_plan.hip — the plan of libacf_apr.so's training engine: from a call's triplets to the
// records the step kernels (acf_apr.hip) read — per-batch unique rows ("slots"), ordered
// occurrence records, fused-triplet records, slot / hot / task lists (acf_plan.h).  Four
// builders write the same records: the sort plan (device-wide radix sort; every shape), the
// batch-local plan (B <= 1,024: one workgroup per batch), the one-workgroup shard plan and the
// hash plan of triplet-centric steps (acf_hplan.h); acf_apr_plan chooses.  Nothing here launches
// a step kernel, and the step launches nothing of this unit.
// Build: one hipcc line with acf_apr.hip and the library's other units, same flags.

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/block/block_radix_sort.hpp>
#include <rocprim/block/block_scan.hpp>

#include <algorithm>
#include <vector>

#include "acf_apr.h"
#include "acf_host.h"  // HIP_TRY, ACF_CHECK, ACF_RET, grid_for
#include "acf_plan.h"  // the records, the context, resolve

// ---------------------------------------------------------------------------
// plan kernels
// ---------------------------------------------------------------------------
// The plan sorts every occurrence by its segment (t, row) — users and items in
// one sort, items after users — with the occurrence index as tie-break so the
// order inside a segment is the occurrence order.  Two key layouts:
//   Key64: (segment << ob | occurrence) in one 64-bit key;
//   Key32: 32-bit segment key, occurrence as the sort value (fewer radix passes;
//          used when batches x rows fits 31 bits).
struct Key64 {
  const uint64_t* k;
  uint32_t ob;
  uint64_t kmask;  // clears the item bit
  __device__ uint64_t seg(int64_t x) const { return (k[x] & kmask) >> ob; }
  __device__ int32_t occ(int64_t x) const { return (int32_t)(k[x] & ((1ull << ob) - 1)); }
};
struct Key32 {
  const uint32_t* k;
  const int32_t* v;
  uint32_t kmask;
  __device__ uint64_t seg(int64_t x) const { return k[x] & kmask; }
  __device__ int32_t occ(int64_t x) const { return v[x]; }
};

template <bool PAIRS>
__global__ void k_stage(const int32_t* __restrict__ user, const int32_t* __restrict__ ipos,
                        const int32_t* __restrict__ ineg, int64_t E, int32_t B, int64_t U1,
                        int64_t I1, void* __restrict__ keys, int32_t* __restrict__ vals,
                        uint32_t ob_u, uint32_t ob_i, uint64_t item_bit, int32_t* __restrict__ err) {
  int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (x >= E) return;
  int64_t t = x / B;
  int32_t u = user[x], i = ipos[x], j = ineg[x];
  if (u < 0 || u >= U1) { atomicOr(err, 1); u = 0; }
  if (i < 0 || i >= I1) { atomicOr(err, 2); i = 0; }
  if (j < 0 || j >= I1) { atomicOr(err, 2); j = 0; }
  // [E user keys | 2E item keys]; item_bit (above both key ranges) puts every
  // item key after every user key
  if (PAIRS) {
    uint32_t* k = static_cast<uint32_t*>(keys);
    k[x] = (uint32_t)(t * U1 + u);
    k[E + 2 * x] = (uint32_t)item_bit | (uint32_t)(t * I1 + i);
    k[E + 2 * x + 1] = (uint32_t)item_bit | (uint32_t)(t * I1 + j);
    vals[x] = (int32_t)x;
    vals[E + 2 * x] = (int32_t)(2 * x);
    vals[E + 2 * x + 1] = (int32_t)(2 * x + 1);
  } else {
    uint64_t* k = static_cast<uint64_t*>(keys);
    k[x] = ((uint64_t)(t * U1 + u) << ob_u) | (uint64_t)x;
    k[E + 2 * x] = item_bit | ((uint64_t)(t * I1 + i) << ob_i) | (uint64_t)(2 * x);
    k[E + 2 * x + 1] = item_bit | ((uint64_t)(t * I1 + j) << ob_i) | (uint64_t)(2 * x + 1);
  }
}

// head flags over the sorted [E user keys | 2E item keys]
template <class KT>
__global__ void k_heads(KT ku, KT ki, int64_t E, int32_t* __restrict__ flag) {
  int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (x >= 3 * E) return;
  bool h;
  if (x < E) h = x == 0 || ku.seg(x) != ku.seg(x - 1);
  else h = x == E || ki.seg(x - E) != ki.seg(x - E - 1);
  flag[x] = h ? 1 : 0;
}

// After an inclusive scan of the head flags: unique rows, occurrence offsets,
// per-batch unique ranges, and for every triplet the slots and CSR positions of
// its occurrences.  Item side: the scan ran over users and items together,
// *sbase = user uniques.
template <class KT>
__global__ void k_compact(KT key, const int32_t* __restrict__ inc, const int32_t* __restrict__ sbase,
                          int64_t n, int64_t R, int32_t nb, int32_t* __restrict__ uniq,
                          int32_t* __restrict__ off, int32_t* __restrict__ bstart,
                          int32_t* __restrict__ tsl, int32_t* __restrict__ tpos, int32_t item_side) {
  int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (x >= n) return;
  const uint64_t seg = key.seg(x);
  const int32_t v = key.occ(x);
  const int32_t s = inc[x] - 1 - (sbase ? *sbase : 0);
  // tsl[e] = {user slot, positive-item slot, negative-item slot, -}; tpos alike
  const int64_t at = item_side ? (int64_t)(v >> 1) * 4 + 1 + (v & 1) : (int64_t)v * 4;
  tsl[at] = s;
  tpos[at] = (int32_t)x;
  const bool head = (x == 0) || key.seg(x - 1) != seg;
  if (head) {
    uniq[s] = (int32_t)(seg % (uint64_t)R);
    off[s] = (int32_t)x;
    int64_t t = (int64_t)(seg / (uint64_t)R);
    bool bhead = (x == 0) || (key.seg(x - 1) / (uint64_t)R) != (uint64_t)t;
    if (bhead) bstart[t] = s;
  }
  if (x == n - 1) {
    off[s + 1] = (int32_t)n;
    bstart[nb] = s + 1;
  }
}

// local slot in batch tb of the row (binary search of tb's sorted unique rows), or -1
__device__ __forceinline__ int find_local(const int32_t* __restrict__ uniq, const int32_t* __restrict__ ubs,
                                          const int32_t* __restrict__ bstart, int tb, int32_t row,
                                          int item_side) {
  int a = bstart[tb], b = bstart[tb + 1];
  while (a < b) {
    int mid = (a + b) >> 1;
    if (uniq[mid] < row) a = mid + 1; else b = mid;
  }
  if (a < bstart[tb + 1] && uniq[a] == row) {
    const int nU = ubs[tb + 1] - ubs[tb];
    return item_side ? nU + (a - bstart[tb]) : (a - bstart[tb]);
  }
  return -1;
}

// inplace (triplet-centric plans, every row updated in its table): every row is
// read from its table and nothing depends on the next batch, so no search.
__global__ void k_slot_info(const int32_t* __restrict__ uniq, const int32_t* __restrict__ off,
                            const int32_t* __restrict__ ubs, const int32_t* __restrict__ bstart,
                            int32_t n_uniq, int32_t nb, int32_t item_side, int32_t kb,
                            int4* __restrict__ info, int32_t inplace) {
  int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (g >= n_uniq || g >= bstart[nb]) return;  // bstart[nb] = unique rows of the plan
  if (inplace) {
    const int32_t row = uniq[g], o = off[g];
    info[g] = make_int4(row, row, off[g + 1] - o, o);
    return;
  }
  // batch of g: last t with bstart[t] <= g
  int lo = 0, hi = nb;  // answer in [0, nb)
  while (hi - lo > 1) {
    int mid = (lo + hi) >> 1;
    if (bstart[mid] <= g) lo = mid; else hi = mid;
  }
  const int t = lo;
  const int32_t row = uniq[g];
  int32_t s = row;
  if (t > 0) {
    const int local = find_local(uniq, ubs, bstart, t - 1, row, item_side);
    if (local >= 0) s = make_src(1, local, kb);
  }
  int32_t in_next = 0;
  if (t + 1 < nb) {
    int a = bstart[t + 1], b = bstart[t + 2];
    while (a < b) {
      int mid = (a + b) >> 1;
      if (uniq[mid] < row) a = mid + 1; else b = mid;
    }
    in_next = (a < bstart[t + 2] && uniq[a] == row) ? 1 : 0;
  }
  const int32_t o = off[g];
  info[g] = make_int4(row, s, (off[g + 1] - o) | (in_next ? ACF_INFO_NEXT : 0), o);
}

// One-wave-per-slot plans: the previous and next batch that touch each unique
// row, at any distance, from one sort of the unique (side, row, batch) keys.
// Entry x < E names user unique x, entry E + x item unique x; entries past a
// side's unique count sort last (all-ones key).  The key layout:
//   32-bit (VK32): side << (rb + tb) | row << tb | t, the entry as the value;
//   64-bit: (side << (rb + tb) | row << tb | t) << 30 | entry.
struct VKeys {
  int32_t rb, tb, k32;
  __device__ uint64_t key(int32_t side, int32_t row, int32_t t) const {
    return ((uint64_t)side << (rb + tb)) | ((uint64_t)row << tb) | (uint64_t)t;
  }
};

__device__ __forceinline__ int batch_of(const int32_t* __restrict__ bstart, int nb, int64_t g) {
  int lo = 0, hi = nb;  // last t with bstart[t] <= g
  while (hi - lo > 1) {
    int mid = (lo + hi) >> 1;
    if (bstart[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ void k_vkeys(const int32_t* __restrict__ uuniq, const int32_t* __restrict__ iuniq,
                        const int32_t* __restrict__ ubs, const int32_t* __restrict__ ibs, int64_t E,
                        int32_t nb, VKeys vk, void* __restrict__ keys, int32_t* __restrict__ vals) {
  const int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (x >= 3 * E) return;
  const int32_t side = x >= E ? 1 : 0;
  const int64_t g = side ? x - E : x;
  const int32_t* bs = side ? ibs : ubs;
  const bool valid = g < bs[nb];
  uint64_t k = ~0ull;
  if (valid) k = vk.key(side, (side ? iuniq : uuniq)[g], batch_of(bs, nb, g));
  if (vk.k32) {
    static_cast<uint32_t*>(keys)[x] = valid ? (uint32_t)k : ~0u;
    vals[x] = (int32_t)x;
  } else {
    static_cast<uint64_t*>(keys)[x] = valid ? (k << 30) | (uint64_t)x : ~0ull;
  }
}

// Over the sorted keys: info[g] of each unique row (src from the previous batch
// that touches it, NEXT when batch t+1 does) and nextt[t][slot] = the next batch
// that touches it (0x7fffffff: none in the plan).
__global__ void k_prev_next(const void* __restrict__ keys, const int32_t* __restrict__ vals, int64_t E,
                            VKeys vk, const int32_t* __restrict__ uoff, const int32_t* __restrict__ ioff,
                            const int32_t* __restrict__ ubs, const int32_t* __restrict__ ibs, int32_t S,
                            int32_t kb, int4* __restrict__ uinfo, int4* __restrict__ iinfo,
                            int32_t* __restrict__ nextt) {
  const int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (p >= 3 * E) return;
  const uint64_t tmask = (1ull << vk.tb) - 1;
  auto rd = [&](int64_t q, uint64_t& k, int64_t& x) {  // (side,row,t) key and entry at sorted q
    if (vk.k32) {
      const uint32_t v = static_cast<const uint32_t*>(keys)[q];
      k = v == ~0u ? ~0ull : (uint64_t)v;
      x = vals[q];
    } else {
      const uint64_t v = static_cast<const uint64_t*>(keys)[q];
      k = v == ~0ull ? ~0ull : (v >> 30);
      x = (int64_t)(v & ((1ull << 30) - 1));
    }
  };
  uint64_t k;
  int64_t x;
  rd(p, k, x);
  if (k == ~0ull) return;
  const int32_t side = x >= E ? 1 : 0;
  const int64_t g = side ? x - E : x;
  const int32_t t = (int32_t)(k & tmask);
  const uint64_t rowkey = k >> vk.tb;  // side | row
  const int32_t row = (int32_t)(rowkey & ((1ull << vk.rb) - 1));
  auto local = [&](int32_t s, int64_t gg, int32_t tt) -> int32_t {
    return s ? (ubs[tt + 1] - ubs[tt]) + (int32_t)(gg - ibs[tt]) : (int32_t)(gg - ubs[tt]);
  };
  int32_t src = row;
  if (p > 0) {
    uint64_t kp;
    int64_t xp;
    rd(p - 1, kp, xp);
    if (kp != ~0ull && (kp >> vk.tb) == rowkey) {
      const int32_t tp = (int32_t)(kp & tmask);
      src = make_src(t - tp, local(side, side ? xp - E : xp, tp), kb);
    }
  }
  int32_t tn = 0x7fffffff;
  if (p + 1 < 3 * E) {
    uint64_t kn;
    int64_t xn;
    rd(p + 1, kn, xn);
    if (kn != ~0ull && (kn >> vk.tb) == rowkey) tn = (int32_t)(kn & tmask);
  }
  const int32_t* off = side ? ioff : uoff;
  const int32_t o = off[g];
  (side ? iinfo : uinfo)[g] = make_int4(row, src, (off[g + 1] - o) | (tn == t + 1 ? ACF_INFO_NEXT : 0), o);
  nextt[(int64_t)t * S + local(side, g, t)] = tn;
}

// A triplet is FUSED when its user, positive and negative item each occur once
// in the batch (so i != j): its rows' batch-aggregated gradients are its own
// contributions, and the whole APR step for it runs in one lane-group with no
// batch-wide reduction (k_single).  A fused row is written straight to its table
// ("in place") unless the next batch touches it or it is pending from the
// previous batch; otherwise it goes through the W scratch like any other row.
struct FuseInfo {
  int fused, in_u, in_i, in_j;
};

__device__ __forceinline__ int info_count(const int4& f) { return f.z & (ACF_INFO_NEXT - 1); }

__device__ __forceinline__ FuseInfo fuse_info(const int4& U, const int4& I, const int4& J, int kb) {
  FuseInfo f;
  f.fused = info_count(U) == 1 && info_count(I) == 1 && info_count(J) == 1;
  f.in_u = f.fused && !pend1(U.y, kb) && !(U.z & ACF_INFO_NEXT);
  f.in_i = f.fused && !pend1(I.y, kb) && !(I.z & ACF_INFO_NEXT);
  f.in_j = f.fused && !pend1(J.y, kb) && !(J.z & ACF_INFO_NEXT);
  return f;
}

// Fused-triplet record (same 48-B shape as OccRec; fields by position):
//  a = {u, i, j, local slot of u}, b = {slot i, slot j, src u, src i},
//  c = {src j, flags (1 fused | 2 in-place u | 4 in-place i | 8 in-place j), e, gen}

// item occurrence record: own = the item's slot info, oth = the triplet's other item
__device__ __forceinline__ OccRec item_rec(const int4& own, const int4& oth, const int4& U, int32_t v,
                                           int32_t ku, int32_t k_oth, int fused, int in_place,
                                           int32_t gen) {
  OccRec r;
  r.own_row = own.x;
  r.own_src = own.y;
  r.meta = info_count(own) | ACF_ITEM_BIT | (fused ? ACF_SINGLE_BIT : 0) |
           (in_place ? ACF_INPLACE_BIT : 0);
  r.ovf = own.w;
  r.e_role = v;
  r.pa_row = U.x;
  r.pb_row = oth.x;
  r.pa_src = U.y;
  r.pb_src = oth.y;
  r.pa_slot = ku | (info_count(U) == 1 ? ACF_SOLO_BIT : 0);
  r.pb_slot = k_oth | (info_count(oth) == 1 ? ACF_SOLO_BIT : 0);
  r.gen = gen;
  return r;
}

// One thread per triplet: its user and two item occurrence records and, when
// fused, its fused-triplet record.  The first R records of a slot go inline
// only (that is the only place they are read from), later ones to the CSR.
// Per-slot flags of packed plans (non-fused and not hot << 32 | row stays in W
// scratch), written by k_records for the slot's first occurrence (the hot
// lists likewise); scanned into the per-batch slot and write-back lists.
// csr: the slot's local CSR base | item << 31 (the triplet-centric combine's piece waves read it beside the piece)
__device__ __forceinline__ void slot_flag(uint64_t* __restrict__ sflags, const HotLists& hl, int64_t t, int32_t S,
                                          int32_t k, int32_t count, bool single, bool inplace, int32_t csr) {
  const bool hot = !single && count > ACF_HOT_MIN;
  sflags[t * S + k] = ((uint64_t)(!single && !hot) << 32) | (uint64_t)(!inplace);
  if (hot) {
    const int32_t np = hot_pieces(count);
    const int32_t h = atomicAdd(hl.cnt + t, 1);
    const int32_t base = atomicAdd(hl.pcnt + t, np);
    hl.list[t * hl.hot_stride + h] = make_int4(k, np, base, count);
    for (int32_t p = 0; p < np; ++p) {
      hl.piece[t * hl.piece_stride + base + p] = make_int4(k, p, np, base);
      hl.paux[t * hl.piece_stride + base + p] = make_int2(count, csr);
    }
  }
}

// tri (triplet-centric list plans, see k_tri_*): every row that occurs once in
// its batch is "single" (its triplet's lane-group steps it: SINGLE bit, and
// INPLACE by fuse_info's rule), and every triplet gets a record in trec with
// the single bits 16 / 32 / 64 (u / i / j) beside the fused / in-place flags.
// the records of triplet e of batch t (its user slots start at ub0, its item slots
// at ib0, nU user slots); shared by k_records and the one-workgroup shard plan
__device__ __forceinline__ void records_one(int64_t e, int32_t t, int32_t ub0, int32_t nU, int32_t ib0, int32_t S,
                                            int32_t R, int32_t gen, int32_t kb, int32_t no_fuse, int32_t tri,
                                            const int4* tsl, const int4* tpos, const int4* uinfo, const int4* iinfo,
                                            OccRec* urec, OccRec* irec, OccRec* inl, OccRec* trec,
                                            uint64_t* sflags, const HotLists& hl) {
  const int4 sl = tsl[e], ps = tpos[e];
  const int4 U = uinfo[sl.x], I = iinfo[sl.y], J = iinfo[sl.z];
  const int32_t k = sl.x - ub0, ki = nU + (sl.y - ib0), kj = nU + (sl.z - ib0);
  FuseInfo f = fuse_info(U, I, J, kb);
  if (no_fuse) f.fused = f.in_u = f.in_i = f.in_j = 0;  // shard mode: item counts are rank-local
  const int su = info_count(U) == 1, si = info_count(I) == 1, sj = info_count(J) == 1;
  if (tri) {  // single rows step in their triplet; in place by the fused rule
    f.in_u = su && !pend1(U.y, kb) && !(U.z & ACF_INFO_NEXT);
    f.in_i = si && !pend1(I.y, kb) && !(I.z & ACF_INFO_NEXT);
    f.in_j = sj && !pend1(J.y, kb) && !(J.z & ACF_INFO_NEXT);
  }
  const int xu = tri ? su : f.fused, xi = tri ? si : f.fused, xj = tri ? sj : f.fused;
  OccRec r;
  r.own_row = U.x;
  r.own_src = U.y;
  r.meta = info_count(U) | (xu ? ACF_SINGLE_BIT : 0) | (f.in_u ? ACF_INPLACE_BIT : 0);
  r.ovf = U.w;
  r.e_role = (int32_t)e;
  r.pa_row = I.x;
  r.pb_row = J.x;
  r.pa_src = I.y;
  r.pb_src = J.y;
  r.pa_slot = ki | (info_count(I) == 1 ? ACF_SOLO_BIT : 0);
  r.pb_slot = kj | (info_count(J) == 1 ? ACF_SOLO_BIT : 0);
  r.gen = gen;
  // the CSR records (occurrences past the first R) are read by the slot kernels
  // only: the triplet-centric step reads a shared slot's first record (its
  // combine) and trec -- a single row's slot is read by nothing (its triplet
  // steps it from trec), so tri plans write neither its record nor its slot
  // flags (0, the cleared value: not listed, written in place), ~60% of
  // k_records' scattered 48-B stores at configs[4]
  const int64_t base = (int64_t)t * S;
  int32_t rr = ps.x - U.w;
  if (rr < R) { if (!(tri && su)) inl[(base + k) * R + rr] = r; }
  else if (!tri) urec[ps.x] = r;
  const OccRec ri = item_rec(I, J, U, (int32_t)(2 * e), k, kj, xi, f.in_i, gen);
  rr = ps.y - I.w;
  if (rr < R) { if (!(tri && si)) inl[(base + ki) * R + rr] = ri; }
  else if (!tri) irec[ps.y] = ri;
  const OccRec rj = item_rec(J, I, U, (int32_t)(2 * e + 1), k, ki, xj, f.in_j, gen);
  rr = ps.z - J.w;
  if (rr < R) { if (!(tri && sj)) inl[(base + kj) * R + rr] = rj; }
  else if (!tri) irec[ps.z] = rj;
  if (sflags) {  // packed plans: the slot flags and hot lists, from each slot's first occurrence
    // local CSR bases (users: t * B + x, items: t * 2B + x; t is 0 in the shard plan's batch)
    const int32_t Bt = S / 3;
    if (ps.x == U.w && !(tri && su)) slot_flag(sflags, hl, t, S, k, info_count(U), xu, f.in_u, U.w - (int32_t)t * Bt);
    if (ps.y == I.w && !(tri && si))
      slot_flag(sflags, hl, t, S, ki, info_count(I), xi, f.in_i, (I.w - (int32_t)t * 2 * Bt) | (int32_t)0x80000000);
    if (ps.z == J.w && !(tri && sj))
      slot_flag(sflags, hl, t, S, kj, info_count(J), xj, f.in_j, (J.w - (int32_t)t * 2 * Bt) | (int32_t)0x80000000);
  }
  if (f.fused || tri) {  // other triplets' records read as absent (older generation)
    OccRec q;
    q.own_row = U.x; q.own_src = I.x; q.meta = J.x; q.ovf = k;
    q.e_role = ki; q.pa_row = kj; q.pb_row = U.y; q.pa_src = I.y;
    q.pb_src = J.y;
    q.pa_slot = (f.fused ? 1 : 0) | (f.in_u ? 2 : 0) | (f.in_i ? 4 : 0) | (f.in_j ? 8 : 0) |
                (su ? 16 : 0) | (si ? 32 : 0) | (sj ? 64 : 0);
    q.pb_slot = (int32_t)e; q.gen = gen;
    trec[e] = q;
  }
}

__global__ void k_records(int64_t E, int32_t B, int32_t S, int32_t R, int32_t gen, int32_t kb, int32_t no_fuse,
                          int32_t tri,
                          const int4* __restrict__ tsl, const int4* __restrict__ tpos,
                          const int4* __restrict__ uinfo, const int4* __restrict__ iinfo,
                          const int32_t* __restrict__ ubs, const int32_t* __restrict__ ibs,
                          OccRec* __restrict__ urec, OccRec* __restrict__ irec,
                          OccRec* __restrict__ inl, OccRec* __restrict__ trec,
                          int32_t* __restrict__ gen_ptr, uint64_t* __restrict__ sflags, HotLists hl) {
  const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (e == 0) *gen_ptr = gen;
  if (e >= E) return;
  const int32_t t = (int32_t)(e / B);
  records_one(e, t, ubs[t], ubs[t + 1] - ubs[t], ibs[t], S, R, gen, kb, no_fuse, tri, tsl, tpos, uinfo, iinfo,
              urec, irec, inl, trec, sflags, hl);
}

__global__ void k_slot_lists(const uint64_t* __restrict__ flags, const uint64_t* __restrict__ incl,
                             int64_t n, int32_t S, int32_t* __restrict__ slot_list,
                             int32_t* __restrict__ flush_list, int32_t* __restrict__ slot_cnt,
                             int32_t* __restrict__ flush_cnt) {
  const int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (x >= n) return;
  const int64_t t = x / S;
  const int32_t k = (int32_t)(x - t * S);
  const uint64_t base = t > 0 ? incl[t * S - 1] : 0;
  const uint64_t f = flags[x], v = incl[x] - base;  // inclusive counts inside batch t
  if (f >> 32) slot_list[t * S + (int64_t)(v >> 32) - 1] = k;
  if (f & 0xFFFFFFFFull) flush_list[t * S + (int64_t)(v & 0xFFFFFFFFull) - 1] = k;
  if (k == S - 1) {
    slot_cnt[t] = (int32_t)(v >> 32);
    flush_cnt[t] = (int32_t)(v & 0xFFFFFFFFull);
  }
}

// Streamed-step task lists (one-wave-per-slot plans): per batch its non-fused
// slots (slot order), then the groups of `opw` consecutive triplets that hold a
// fused one (as S + group).  Flags over [nb][S + G], scanned into the lists.
__global__ void k_task_flags(const OccRec* __restrict__ inl, const OccRec* __restrict__ trec, int64_t n,
                             int32_t S, int32_t G, int32_t B, int32_t R, int32_t opw, int32_t gen,
                             int32_t* __restrict__ flags) {
  const int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (x >= n) return;
  const int64_t t = x / (S + G);
  const int32_t y = (int32_t)(x - t * (S + G));
  int32_t f = 0;
  if (y < S) {
    const OccRec* r = inl + (t * S + y) * R;
    f = r->gen == gen && (r->meta & ACF_COUNT_MASK) != 0 && !(r->meta & ACF_SINGLE_BIT);
  } else {
    const int32_t b0 = (y - S) * opw, b1 = min(b0 + opw, B);
    for (int32_t b = b0; b < b1; ++b) {
      const OccRec* q = trec + t * B + b;
      f |= (q->gen == gen && (q->pa_slot & 1)) ? 1 : 0;
    }
  }
  flags[x] = f;
}

__global__ void k_task_list(const int32_t* __restrict__ flags, const int32_t* __restrict__ incl, int64_t n,
                            int32_t stride, int32_t* __restrict__ list, int32_t* __restrict__ cnt) {
  const int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (x >= n) return;
  const int64_t t = x / stride;
  const int32_t y = (int32_t)(x - t * stride);
  const int32_t base = t > 0 ? incl[t * stride - 1] : 0;
  if (flags[x]) list[t * stride + incl[x] - base - 1] = y;
  if (y == stride - 1) cnt[t] = incl[x] - base;
}

#include "acf_hplan.h"  // the hash plan (k_hplan_*): DESIGN.md §3

// ---------------------------------------------------------------------------
// Batch-local plan (one-wave-per-slot plans, B <= 1024): the same records,
// task lists and next-batch table as the sort plan above, in TWO launches with
// one workgroup per batch instead of ~30 launches of device-wide sorts/scans.
//  - k_bplan_sort: the batch's 3B occurrences sorted by (side, row) in LDS
//    (rocPRIM block radix sort, stable: occurrence order inside a row), its
//    unique rows, their CSR starts, each occurrence's (slot, rank); each unique
//    row marks batch t in its row's batch bitmap and records its local slot.
//  - k_bplan_build: per unique row, the previous / next batch that touches the
//    row from the bitmap (any distance: the streamed step's version source) and
//    the previous batch's local slot; then k_records' occurrence / fused-triplet
//    records and k_task_flags/k_task_list's task list, from LDS.
// The occurrence order, slot order (users by row, then items by row) and CSR
// positions (t*B + position in the sorted user part, t*2B + position in the
// item part) are the sort plan's, so the records are bit-identical
// (test_batch_plan_matches_sort_plan).  The bitmaps come in two buffers by
// plan generation parity: a plan sets bits in one and clears the other, which
// the previous plan used.
// ---------------------------------------------------------------------------
struct BPlanArgs {
  const int32_t* user;
  const int32_t* ipos;
  const int32_t* ineg;
  int64_t U1, I1;
  int32_t B, S, nb, rb, kb, W, nbs;  // nbs: batch stride of slot_of (max batches)
  int32_t R, opw, stride, gen;
  unsigned long long* mask;        // [U1 + I1][W] batches touching each row (this plan)
  unsigned long long* mask_clear;  // the other bitmap buffer: cleared here
  int64_t clear_words;
  uint16_t* slot_of;  // [U1 + I1][nbs] local slot of the row in batch t (valid where mask has t)
  uint32_t* bkey;     // [nb][S] sorted unique keys (side << rb | row)
  int32_t* bstart;    // [nb][S + 1] CSR start of each unique row in the sorted batch
  int32_t* bocc;      // [nb][S] occurrence o -> slot | rank << 16
  int2* bn;           // [nb] {unique rows, unique user rows}
  int32_t* berr;      // [nb] range-check bits of the batch
  int32_t* err;       // err[0] = OR of berr
  int32_t* gen_ptr;
  OccRec *urec, *irec, *inl, *trec;
  int32_t* nextt;
  int32_t* task_list;
  int32_t* task_cnt;
  int2* final_list;   // slots no later batch of the plan touches (k_stream's tail write-back)
  int32_t* final_cnt;
};

// Workgroup barrier for LDS data only.  __syncthreads() also waits for every
// outstanding global store and atomic of the wave (vmcnt(0)): after a phase of
// scattered global writes that is a full memory round trip (≈2-4 us per barrier
// in the plan kernels, tools/diag_plan.py) for data no other thread of the
// workgroup reads back.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// The plan of chunk c+1 runs beside chunk c's k_stream (PlanPipeline): a CU
// that holds one k_stream workgroup (one wave of 240 VGPRs per SIMD) has 272
// VGPRs per SIMD left, and a 1,024-thread plan workgroup puts 4 waves on each
// SIMD, so it fits at <= 64 VGPRs per wave (allocated in eights).  The plan
// kernels use 38 (sort) and 56 / 61 (build): they fit, and nothing pins that.
// Capping them (__launch_bounds__(BS, 8): HIP's second argument is waves per
// SIMD) also caps the SGPRs and spilled 33-52 of them in the build kernels, so
// it was not taken; re-read the counts (tools/kernel_resources.py) after an
// edit that costs registers.
template <int BS, int IPT>
__global__ void __launch_bounds__(BS) k_bplan_sort(BPlanArgs p) {
  constexpr int N = BS * IPT;
  using Sort = rocprim::block_radix_sort<uint32_t, BS, IPT, int32_t>;
  using Scan = rocprim::block_scan<int32_t, BS>;
  __shared__ union {
    typename Sort::storage_type sort;
    struct {
      uint32_t key[N];
      int32_t val[N];
      int32_t start[N + 1];
    } a;
  } sm;
  __shared__ typename Scan::storage_type scan_st;
  __shared__ int32_t s_err, s_nu;
  const int t = blockIdx.x, tid = threadIdx.x, B = p.B, S3 = 3 * B;
  STAMP(t, tid >> 6, 0);
  if (tid == 0) { s_err = 0; s_nu = -1; }
  if (t == 0 && tid == 0) *p.final_cnt = 0;  // k_bplan_build appends to it
  const uint32_t side_bit = 1u << p.rb;
  uint32_t keys[IPT];
  int32_t vals[IPT];
  int err = 0;
  // all loads first, the range checks after them: a check right behind its load
  // made the compiler wait for each load in turn (IPT serial round trips)
  int32_t raw[IPT];
#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    const int o = tid * IPT + k;  // occurrence: users [0, B), items B + 2e + role
    raw[k] = 0;
    if (o < B) {
      raw[k] = p.user[(int64_t)t * B + o];
    } else if (o < S3) {
      const int v = o - B;
      raw[k] = ((v & 1) ? p.ineg : p.ipos)[(int64_t)t * B + (v >> 1)];
    }
  }
#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    const int o = tid * IPT + k;
    uint32_t key = ~0u;  // padding sorts after every key (stable: after equal ones too)
    int32_t x = raw[k];
    if (o < B) {
      if (x < 0 || x >= p.U1) { err |= 1; x = 0; }
      key = (uint32_t)x;
    } else if (o < S3) {
      if (x < 0 || x >= p.I1) { err |= 2; x = 0; }
      key = side_bit | (uint32_t)x;
    }
    keys[k] = key;
    vals[k] = o;
  }
  __syncthreads();
  STAMP(t, tid >> 6, 1);
  if (err) atomicOr(&s_err, err);
  Sort().sort(keys, vals, sm.sort, 0, p.rb + 1);
  __syncthreads();
  STAMP(t, tid >> 6, 2);
#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    sm.a.key[tid * IPT + k] = keys[k];
    sm.a.val[tid * IPT + k] = vals[k];
  }
  __syncthreads();
  int cnt = 0;
#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    const int q = tid * IPT + k;
    cnt += (q < S3 && (q == 0 || keys[k] != sm.a.key[q - 1])) ? 1 : 0;
  }
  int32_t excl = 0, total = 0;
  Scan().exclusive_scan(cnt, excl, 0, total, scan_st);
  STAMP(t, tid >> 6, 3);
  int32_t sl[IPT];
  int32_t s = excl - 1;
  const int64_t rbase = (int64_t)t * p.S;
#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    const int q = tid * IPT + k;
    sl[k] = -1;
    if (q >= S3) continue;
    const uint32_t key = keys[k];
    if (q == 0 || key != sm.a.key[q - 1]) {
      ++s;
      sm.a.start[s] = q;
      const int side = (key & side_bit) ? 1 : 0;
      const int64_t row = (int64_t)(key & (side_bit - 1));
      const int64_t rid = side ? p.U1 + row : row;
      p.bkey[rbase + s] = key;
      p.bstart[(int64_t)t * (p.S + 1) + s] = q;
      p.slot_of[rid * p.nbs + t] = (uint16_t)s;
      atomicOr(p.mask + rid * p.W + (t >> 6), 1ull << (t & 63));
      if (side && (q == 0 || !(sm.a.key[q - 1] & side_bit))) s_nu = s;
    }
    sl[k] = s;
  }
  lds_barrier();  // run starts and s_nu (LDS); the row writes above stay in flight
#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    const int q = tid * IPT + k;
    if (q < S3) p.bocc[rbase + vals[k]] = sl[k] | ((q - sm.a.start[sl[k]]) << 16);
  }
  if (tid == 0) {
    p.bstart[(int64_t)t * (p.S + 1) + total] = S3;
    p.bn[t] = make_int2(total, s_nu < 0 ? total : s_nu);
    p.berr[t] = s_err;
  }
  STAMP(t, tid >> 6, 4);
}

// ---------------------------------------------------------------------------
// One-workgroup shard plan (shard mode, one batch of B <= 1,024 triplets:
// distributed.ShardedAPR's per-step plan).  It writes what the device-wide sort
// plan writes for nb = 1 -- unique rows and CSR offsets, slot info, the triplets'
// slots and CSR positions, occurrence records, slot flags, hot lists and the
// slot / write-back lists -- in ONE launch instead of ~17 (stage, radix sort,
// head flags, two scans, compaction, slot info, four clears, records, list
// scan), which a captured split step replays every step.  Same keys and the
// same stable order (users by row, then items by row, occurrence order inside a
// row), so the records are the sort plan's bit for bit
// (test_shard_plan_small_matches_sort_plan).
// ---------------------------------------------------------------------------
struct SPlanArgs {
  const int32_t* user;
  const int32_t* ipos;
  const int32_t* ineg;
  int64_t U1, I1;
  int32_t B, rb, kb, gen;
  int32_t *uuniq, *uoff, *ubs, *iuniq, *ioff, *ibs;
  int32_t *tsl, *tpos;  // [E][4]
  int4 *uinfo, *iinfo;
  OccRec *urec, *irec, *inl, *trec;
  int32_t *gen_ptr, *err;
  uint64_t* sflags;
  HotLists hl;
  int32_t *slot_list, *flush_list, *slot_cnt, *flush_cnt;
};

template <int BS, int IPT>
__global__ void __launch_bounds__(BS) k_shard_plan(SPlanArgs p) {
  constexpr int N = BS * IPT;
  using Sort = rocprim::block_radix_sort<uint32_t, BS, IPT, int32_t>;
  using Scan = rocprim::block_scan<int32_t, BS>;
  using Scan64 = rocprim::block_scan<uint64_t, BS>;
  __shared__ union {
    typename Sort::storage_type sort;
    struct {
      uint32_t key[N];
      int32_t start[N + 1];
    } a;
    typename Scan64::storage_type scan64;
  } sm;
  __shared__ typename Scan::storage_type scan_st;
  __shared__ int32_t s_err, s_nu;
  const int tid = threadIdx.x, B = p.B, S3 = 3 * B;
  // what the sort plan clears: slot flags, inline records (shard plans), hot counters
  for (int x = tid; x < S3; x += BS) {
    p.sflags[x] = 0;
    p.inl[x] = OccRec{};
  }
  for (int x = tid; x < p.hl.piece_stride; x += BS) p.hl.arrive[x] = 0;
  if (tid == 0) {
    p.hl.cnt[0] = 0;
    p.hl.pcnt[0] = 0;
    *p.gen_ptr = p.gen;
    s_err = 0;
    s_nu = 0;
  }
  // keys: users [0, B) by row, items B + 2e + role after them (side bit)
  const uint32_t side_bit = 1u << p.rb;
  uint32_t keys[IPT];
  int32_t vals[IPT], raw[IPT];
  int err = 0;
#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    const int o = tid * IPT + k;
    raw[k] = 0;
    if (o < B) {
      raw[k] = p.user[o];
    } else if (o < S3) {
      const int v = o - B;
      raw[k] = ((v & 1) ? p.ineg : p.ipos)[v >> 1];
    }
  }
#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    const int o = tid * IPT + k;
    uint32_t key = ~0u;  // padding sorts after every key (stable: after equal ones too)
    int32_t x = raw[k];
    if (o < B) {
      if (x < 0 || x >= p.U1) { err |= 1; x = 0; }
      key = (uint32_t)x;
    } else if (o < S3) {
      if (x < 0 || x >= p.I1) { err |= 2; x = 0; }
      key = side_bit | (uint32_t)x;
    }
    keys[k] = key;
    vals[k] = o;
  }
  __syncthreads();
  if (err) atomicOr(&s_err, err);
  Sort().sort(keys, vals, sm.sort, 0, p.rb + 1);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < IPT; ++k) sm.a.key[tid * IPT + k] = keys[k];
  __syncthreads();
  int cnt = 0;
#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    const int q = tid * IPT + k;
    cnt += (q < S3 && (q == 0 || keys[k] != sm.a.key[q - 1])) ? 1 : 0;
  }
  int32_t excl = 0, total = 0;
  Scan().exclusive_scan(cnt, excl, 0, total, scan_st);
  int32_t sl[IPT];
  int32_t s = excl - 1;
#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    const int q = tid * IPT + k;
    sl[k] = -1;
    if (q >= S3) continue;
    if (q == 0 || keys[k] != sm.a.key[q - 1]) {
      ++s;
      sm.a.start[s] = q;
      if (q == B) s_nu = s;  // position B holds the first item occurrence: a head
    }
    sl[k] = s;
  }
  if (tid == 0) sm.a.start[total] = S3;
  __syncthreads();
  const int nU = s_nu, nI = total - nU;
  // unique rows, CSR offsets and slot info (user part [0, B), item part [0, 2B));
  // every triplet's slots and CSR positions
#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    const int q = tid * IPT + k;
    if (q >= S3) continue;
    const int32_t sk = sl[k];
    const int32_t row = (int32_t)(keys[k] & (side_bit - 1));
    if (sm.a.start[sk] == q) {
      const int32_t c = sm.a.start[sk + 1] - q;
      if (q < B) {
        p.uuniq[sk] = row;
        p.uoff[sk] = q;
        p.uinfo[sk] = make_int4(row, row, c, q);
      } else {
        p.iuniq[sk - nU] = row;
        p.ioff[sk - nU] = q - B;
        p.iinfo[sk - nU] = make_int4(row, row, c, q - B);
      }
    }
    const int o = vals[k];
    if (o < B) {
      p.tsl[o * 4] = sk;
      p.tpos[o * 4] = q;
    } else {
      const int v = o - B;
      const int at = (v >> 1) * 4 + 1 + (v & 1);
      p.tsl[at] = sk - nU;
      p.tpos[at] = q - B;
    }
  }
  if (tid == 0) {
    p.uoff[nU] = B;
    p.ioff[nI] = 2 * B;
    p.ubs[0] = 0;
    p.ubs[1] = nU;
    p.ibs[0] = 0;
    p.ibs[1] = nI;
    *p.err = s_err;
  }
  __syncthreads();  // the slot info and triplet slots above, for the records
  for (int e = tid; e < B; e += BS)
    records_one(e, 0, 0, nU, 0, S3, 1, p.gen, p.kb, 1, 0, reinterpret_cast<const int4*>(p.tsl),
                reinterpret_cast<const int4*>(p.tpos), p.uinfo, p.iinfo, p.urec, p.irec, p.inl, p.trec,
                p.sflags, p.hl);
  __syncthreads();  // the slot flags, for the lists
  uint64_t f[IPT], inc[IPT];
#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    const int x = tid * IPT + k;
    f[k] = x < S3 ? p.sflags[x] : 0ull;
  }
  Scan64().inclusive_scan(f, inc, sm.scan64, rocprim::plus<uint64_t>());
#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    const int x = tid * IPT + k;
    if (x >= S3) continue;
    if (f[k] >> 32) p.slot_list[(inc[k] >> 32) - 1] = x;
    if (f[k] & 0xFFFFFFFFull) p.flush_list[(inc[k] & 0xFFFFFFFFull) - 1] = x;
    if (x == S3 - 1) {
      *p.slot_cnt = (int32_t)(inc[k] >> 32);
      *p.flush_cnt = (int32_t)(inc[k] & 0xFFFFFFFFull);
    }
  }
}

template <int BS, int MAXB>
__global__ void __launch_bounds__(BS) k_bplan_build(BPlanArgs p) {
  using Scan = rocprim::block_scan<int32_t, BS>;
  __shared__ int4 info[3 * MAXB];
  __shared__ uint8_t single[3 * MAXB];
  __shared__ uint8_t gflag[MAXB];
  __shared__ typename Scan::storage_type scan_st;
  __shared__ int32_t s_fin, s_fbase;
  const int t = blockIdx.x, tid = threadIdx.x, B = p.B, S = p.S;
  const int G = (B + p.opw - 1) / p.opw;
  STAMP(t, 16 + (tid >> 6), 0);
  if (tid == 0) s_fin = 0;
  const int2 n = p.bn[t];
  const int64_t rbase = (int64_t)t * S;
  // the triplet's occurrence slots, loaded now (k_bplan_sort wrote them): off
  // the dependent chain of the slot pass below (B <= MAXB <= BS: one triplet per thread)
  int32_t ou = 0, oi = 0, oj = 0;
  if (tid < B) {
    ou = p.bocc[rbase + tid];
    oi = p.bocc[rbase + B + 2 * tid];
    oj = p.bocc[rbase + B + 2 * tid + 1];
  }
  // per unique row: key and CSR bounds, then the row's batch bitmap word, then
  // the previous batch's local slot.  The SPT slots of a thread go through each
  // stage together, so their dependent loads overlap (three round trips, not 3 SPT).
  constexpr int SPT = (3 * MAXB + BS - 1) / BS;
  const uint32_t side_bit = 1u << p.rb;
  uint32_t key[SPT];
  int32_t st[SPT], en[SPT];
  unsigned long long mw[SPT];
#pragma unroll
  for (int q = 0; q < SPT; ++q) {
    const int s = tid + q * BS;
    if (s < S) single[s] = 0;
    if (s < n.x) {
      key[q] = p.bkey[rbase + s];
      st[q] = p.bstart[(int64_t)t * (S + 1) + s];
      en[q] = p.bstart[(int64_t)t * (S + 1) + s + 1];
    }
  }
  auto rid_of = [&](uint32_t k) -> int64_t {
    const int32_t row = (int32_t)(k & (side_bit - 1));
    return (k & side_bit) ? p.U1 + row : (int64_t)row;
  };
  STAMP(t, 16 + (tid >> 6), 1);
#pragma unroll
  for (int q = 0; q < SPT; ++q)
    if (tid + q * BS < n.x) mw[q] = p.mask[rid_of(key[q]) * p.W + (t >> 6)];
  int32_t tp[SPT], prev_slot[SPT], tn[SPT];
#pragma unroll
  for (int q = 0; q < SPT; ++q) {
    tp[q] = -1;
    tn[q] = 0x7fffffff;
    if (tid + q * BS >= n.x) continue;
    const unsigned long long* m = p.mask + rid_of(key[q]) * p.W;
    // previous batch touching the row: highest bit below t
    int w = t >> 6;
    unsigned long long bits = mw[q] & ((1ull << (t & 63)) - 1);
    while (!bits && w > 0) bits = m[--w];
    if (bits) tp[q] = w * 64 + 63 - __clzll((long long)bits);
    // next batch touching the row: lowest bit above t
    w = t >> 6;
    bits = (t & 63) == 63 ? 0ull : (mw[q] & ~((2ull << (t & 63)) - 1));
    const int wl = (p.nb - 1) >> 6;
    while (!bits && w < wl) bits = m[++w];
    if (bits) tn[q] = w * 64 + __ffsll((long long)bits) - 1;
  }
  STAMP(t, 16 + (tid >> 6), 2);
#pragma unroll
  for (int q = 0; q < SPT; ++q)
    if (tp[q] >= 0) prev_slot[q] = p.slot_of[rid_of(key[q]) * p.nbs + tp[q]];
#pragma unroll
  for (int q = 0; q < SPT; ++q) {
    const int s = tid + q * BS;
    if (s >= n.x) continue;
    const int side = (key[q] & side_bit) ? 1 : 0;
    const int32_t row = (int32_t)(key[q] & (side_bit - 1));
    const int32_t cnt = en[q] - st[q];
    const int32_t ovf = side ? t * 2 * B + st[q] - B : t * B + st[q];
    const int32_t src = tp[q] >= 0 ? make_src(t - tp[q], prev_slot[q], p.kb) : row;
    info[s] = make_int4(row, src, cnt | (tn[q] == t + 1 ? ACF_INFO_NEXT : 0), ovf);
  }
  for (int g = tid; g < G; g += BS) gflag[g] = 0;
  lds_barrier();  // info (LDS); the nextt stores stay in flight
  // final slots (no later batch of the plan touches the row): their place in
  // this batch's share of the final-slot list
  int32_t fidx[SPT];
#pragma unroll
  for (int q = 0; q < SPT; ++q) {
    fidx[q] = -1;
    if (tid + q * BS < n.x && tn[q] == 0x7fffffff) fidx[q] = atomicAdd(&s_fin, 1);
  }
  const int gen = p.gen;
  STAMP(t, 16 + (tid >> 6), 3);
  static_assert(MAXB <= BS, "k_bplan_build: one triplet per thread");
  // records: formed now (the fused flags feed the task list), stored after it,
  // so no barrier waits for them
  OccRec r, ri, rj, q;
  int64_t ar = 0, ai = 0, aj = 0;  // destinations: >= 0 inline index, < 0 CSR index - 1
  bool fused = false;
  int64_t e = 0;
  if (tid < B) {
    const int b = tid;
    e = (int64_t)t * B + b;
    const int32_t k = ou & 0xFFFF, ki = oi & 0xFFFF, kj = oj & 0xFFFF;
    const int4 U = info[k], I = info[ki], J = info[kj];
    const FuseInfo f = fuse_info(U, I, J, p.kb);
    r.own_row = U.x;
    r.own_src = U.y;
    r.meta = info_count(U) | (f.fused ? ACF_SINGLE_BIT : 0) | (f.in_u ? ACF_INPLACE_BIT : 0);
    r.ovf = U.w;
    r.e_role = (int32_t)e;
    r.pa_row = I.x;
    r.pb_row = J.x;
    r.pa_src = I.y;
    r.pb_src = J.y;
    r.pa_slot = ki | (info_count(I) == 1 ? ACF_SOLO_BIT : 0);
    r.pb_slot = kj | (info_count(J) == 1 ? ACF_SOLO_BIT : 0);
    r.gen = gen;
    int32_t rr = ou >> 16;
    ar = rr < p.R ? (rbase + k) * p.R + rr : -1 - ((int64_t)U.w + rr);
    ri = item_rec(I, J, U, (int32_t)(2 * e), k, kj, f.fused, f.in_i, gen);
    rr = oi >> 16;
    ai = rr < p.R ? (rbase + ki) * p.R + rr : -1 - ((int64_t)I.w + rr);
    rj = item_rec(J, I, U, (int32_t)(2 * e + 1), k, ki, f.fused, f.in_j, gen);
    rr = oj >> 16;
    aj = rr < p.R ? (rbase + kj) * p.R + rr : -1 - ((int64_t)J.w + rr);
    fused = f.fused;
    if (f.fused) {
      q.own_row = U.x; q.own_src = I.x; q.meta = J.x; q.ovf = k;
      q.e_role = ki; q.pa_row = kj; q.pb_row = U.y; q.pa_src = I.y;
      q.pb_src = J.y;
      q.pa_slot = 1 | (f.in_u ? 2 : 0) | (f.in_i ? 4 : 0) | (f.in_j ? 8 : 0);
      q.pb_slot = (int32_t)e; q.gen = gen;
      single[k] = single[ki] = single[kj] = 1;  // the fused triplet's slots are its own
      gflag[b / p.opw] = 1;
    }
  }
  lds_barrier();
  STAMP(t, 16 + (tid >> 6), 4);
  // the batch's share of the final-slot list: the atomic stays in flight over
  // the task-list scans below (they wait on LDS only)
  int32_t fret = 0;
  if (tid == 0 && s_fin > 0) fret = atomicAdd(p.final_cnt, s_fin);
  // task list: the non-fused slots in slot order, then the groups holding a fused triplet
  int32_t base = 0;
  for (int y0 = 0; y0 < S + G; y0 += BS) {
    const int y = y0 + tid;
    int32_t f = 0;
    if (y < S) f = (y < n.x && !single[y]) ? 1 : 0;
    else if (y < S + G) f = gflag[y - S];
    int32_t excl = 0, tot = 0;
    Scan().exclusive_scan(f, excl, 0, tot, scan_st);
    if (f) p.task_list[(int64_t)t * p.stride + base + excl] = y;
    base += tot;
    lds_barrier();  // scan storage reuse
  }
  STAMP(t, 16 + (tid >> 6), 5);
  if (tid == 0) s_fbase = fret;
  lds_barrier();
  // every global store of the kernel from here on: on gfx950 vmcnt counts stores
  // too, so an earlier store would have held up the loads the phases above wait for
#pragma unroll
  for (int q = 0; q < SPT; ++q) {
    const int s = tid + q * BS;
    if (s < S) p.nextt[rbase + s] = s < n.x ? tn[q] : 0;  // 0: no row, never written back
    if (fidx[q] >= 0)
      p.final_list[s_fbase + fidx[q]] =
          make_int2((int32_t)(rbase + s), (int32_t)(key[q] & (side_bit - 1)) | ((key[q] & side_bit) ? (int32_t)0x80000000 : 0));
  }
  if (tid < B) {
    (ar >= 0 ? p.inl[ar] : p.urec[-1 - ar]) = r;
    (ai >= 0 ? p.inl[ai] : p.irec[-1 - ai]) = ri;
    (aj >= 0 ? p.inl[aj] : p.irec[-1 - aj]) = rj;
    if (fused) p.trec[e] = q;
  }
  if (tid == 0) {
    p.task_cnt[t] = base;
    if (t == 0) {
      int32_t e = 0;
      for (int x = 0; x < p.nb; ++x) e |= p.berr[x];
      p.err[0] = e;
      *p.gen_ptr = gen;
    }
  }
  // clear the other bitmap buffer (used by the previous plan), a stripe per batch
  const int64_t w0 = p.clear_words * t / p.nb, w1 = p.clear_words * (t + 1) / p.nb;
  for (int64_t x = w0 + tid; x < w1; x += BS) p.mask_clear[x] = 0ull;
  STAMP(t, 16 + (tid >> 6), 6);
}

#ifdef ACF_DIAG
int plan_set_stamps(uint64_t* buf, int32_t cap) {
  HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), &buf, sizeof(buf)));
  HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_cap), &cap, sizeof(cap)));
  return ACF_OK;
}

#endif
// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// Batch-local plan buffers, allocated at first use: the two batch bitmaps, the
// per-row local slots and the per-batch sort outputs.  Off (sort plan) when
// the bitmaps or slot table would be large (big tables: packed plans anyway).
static bool bplan_ready(acf_apr_ctx* c) {
  if (c->bplan_ok >= 0) return c->bplan_ok == 1;
  c->bplan_ok = 0;
  const int64_t rows = c->U1 + c->I1;
  const int32_t W = (c->maxNB + 63) / 64;
  const size_t mask_words = (size_t)rows * W;
  const size_t S = (size_t)3 * c->maxB;
  if (c->maxB > 1024 || mask_words * 8 > ((size_t)64 << 20) ||
      (size_t)rows * c->maxNB * 2 > ((size_t)256 << 20))
    return false;
  std::vector<void*> got;
  auto A = [&](auto** p, size_t n) -> bool {
    if (dalloc(c, p, n) != ACF_OK) return false;
    got.push_back(*p);
    return true;
  };
  bool ok = A(&c->bmask[0], mask_words) && A(&c->bmask[1], mask_words) &&
            A(&c->slot_of, (size_t)rows * c->maxNB) && A(&c->bkey, (size_t)c->maxNB * S) &&
            A(&c->bstart, (size_t)c->maxNB * (S + 1)) && A(&c->bocc, (size_t)c->maxNB * S) &&
            A(&c->bn, (size_t)c->maxNB) && A(&c->berr, (size_t)c->maxNB) &&
            A(&c->final_list, (size_t)std::min<int64_t>(rows, (int64_t)c->maxNB * S)) && A(&c->final_cnt, 4);
  ok = ok && hipMemset(c->bmask[0], 0, mask_words * 8) == hipSuccess &&
       hipMemset(c->bmask[1], 0, mask_words * 8) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
  if (!ok) {  // give back what was allocated; the sort plan stays in use
    (void)hipGetLastError();
    for (void* p : got) {
      (void)hipFree(p);
      c->allocs.erase(std::find(c->allocs.begin(), c->allocs.end(), p));
    }
    c->bmask[0] = c->bmask[1] = nullptr;
    c->final_list = nullptr;
    c->final_cnt = nullptr;
    return false;
  }
  c->bmask_words = mask_words;
  c->bmask_dirty[0] = c->bmask_dirty[1] = 0;
  c->bplan_ok = 1;
  return true;
}

// partition bits of a batch of B triplets: 2^pb partitions of <= ACF_HPLAN_PART occurrences on average
static int32_t hplan_pbits(int32_t B, int32_t part) {
  const uint64_t parts = ((uint64_t)3 * B + part - 1) / part;
  return parts <= 1 ? 0 : (int32_t)bits_for(parts - 1);
}

static bool hplan_ready(acf_apr_ctx* c) {
  if (c->hplan_ok >= 0) return c->hplan_ok == 1;
  c->hplan_ok = 0;
  if (c->maxB > ACF_HPLAN_MAXB) return false;
  const int32_t pb = hplan_pbits(c->maxB, ACF_HPLAN_PART);
  if (pb + (int32_t)bits_for((uint64_t)c->maxNB) > 32) return false;
  const size_t n3 = (size_t)3 * c->maxE;
  const size_t ncnt = ((size_t)c->maxNB << pb) * (((size_t)3 * c->maxB + ACF_HPLAN_PTILE - 1) / ACF_HPLAN_PTILE);
  const size_t ntt = (size_t)c->maxNB * ((c->maxB + 255) / 256) + 1;  // triplet tiles (+ a zero)
  size_t tb = 0;
  size_t tb2 = 0;
  if (rocprim::exclusive_scan(nullptr, tb, c->flag, c->inc, 0, ncnt, rocprim::plus<int32_t>()) != hipSuccess ||
      rocprim::exclusive_scan(nullptr, tb2, (unsigned long long*)nullptr, (unsigned long long*)nullptr, 0ull, ntt,
                              rocprim::plus<unsigned long long>()) != hipSuccess)
    return false;
  tb = std::max(tb, tb2);
  std::vector<void*> got;
  auto A = [&](auto** p, size_t m) -> bool {
    if (dalloc(c, p, m) != ACF_OK) return false;
    got.push_back(*p);
    return true;
  };
  bool ok = A(&c->hplan_occ, n3) && A(&c->hplan_pcnt, 2 * ncnt) && A(&c->hplan_claims, n3 / 2 + 1) &&
            A(&c->hplan_ptot, ((size_t)c->maxNB << pb) * 2 * ACF_HPLAN_TOT) &&
            A(&c->hplan_cnt, (size_t)3 * c->maxNB) && A(&c->hplan_haux, (size_t)c->maxNB * c->hot.hot_stride) &&
            A(&c->hplan_perm, (size_t)c->maxE) && A(&c->hplan_tcnt, (size_t)c->maxNB) &&
            A(&c->hplan_ttc, 2 * ntt);
  c->hplan_tmp_bytes = tb;
  if (ok && tb > c->tmp_bytes) ok = A(reinterpret_cast<char**>(&c->hplan_tmp), tb);
  if (!ok) {
    (void)hipGetLastError();
    for (void* p : got) {
      (void)hipFree(p);
      c->allocs.erase(std::find(c->allocs.begin(), c->allocs.end(), p));
    }
    c->hplan_occ = nullptr;
    c->hplan_pcnt = nullptr;
    c->hplan_claims = nullptr;
    c->hplan_ptot = nullptr;
    c->hplan_cnt = nullptr;
    c->hplan_haux = nullptr;
    c->hplan_perm = nullptr;
    c->hplan_tcnt = nullptr;
    c->hplan_ttc = nullptr;
    c->hplan_tmp = nullptr;
    return false;
  }
  c->hplan_ok = 1;
  return true;
}

// triplet-centric plans (see k_hplan_*): the same step inputs as the sort plan's
// tri branch, slot ids and CSR ranges numbered in allocation order
static int hash_plan(acf_apr_ctx* c, const int32_t* user, const int32_t* ipos, const int32_t* ineg, int32_t B,
                     int32_t nb, int32_t gen, int32_t kb, int32_t check, hipStream_t s) {
  const int32_t pb = hplan_pbits(B, ACF_HPLAN_PART);
  HIP_TRY(hipMemsetAsync(c->err, 0, sizeof(int32_t), s));  // the other counters: k_hplan_keys
  HPlanArgs p;
  p.user = user; p.ipos = ipos; p.ineg = ineg;
  p.U1 = c->U1; p.I1 = c->I1;
  p.B = B; p.S = 3 * B; p.nb = nb; p.gen = gen; p.pb = pb;
  p.tpb = (3 * B + ACF_HPLAN_PTILE - 1) / ACF_HPLAN_PTILE;
  p.ppr = reinterpret_cast<uint32_t*>(c->flag);
  p.pstage = reinterpret_cast<unsigned long long*>(c->key_in);
  p.pval = reinterpret_cast<unsigned long long*>(c->key_out);
  const int64_t ncnt = ((int64_t)nb << pb) * p.tpb;
  p.pcnt = c->hplan_pcnt;
  p.poff = c->hplan_pcnt + ((size_t)c->maxNB << hplan_pbits(c->maxB, ACF_HPLAN_PART)) *
                               (((size_t)3 * c->maxB + ACF_HPLAN_PTILE - 1) / ACF_HPLAN_PTILE);
  p.occ = c->hplan_occ; p.csr = c->tsl;
  p.claims = c->hplan_claims;
  p.ptot = c->hplan_ptot;
  p.pbase = c->hplan_ptot + ((size_t)c->maxNB << hplan_pbits(c->maxB, ACF_HPLAN_PART)) * ACF_HPLAN_TOT;
  p.scnt = c->hplan_cnt; p.ucsr = c->hplan_cnt + c->maxNB; p.icsr = c->hplan_cnt + 2 * c->maxNB;
  p.inl = c->inl; p.trec = c->trec; p.tpos = c->tpos;
  p.perm = c->hplan_perm; p.tcnt = c->hplan_tcnt;
  p.ttiles = (B + 255) / 256;
  p.ttc = c->hplan_ttc;
  p.tto = c->hplan_ttc + (size_t)c->maxNB * ((c->maxB + 255) / 256) + 1;
  p.slot_list = c->slot_list; p.slot_cnt = c->slot_cnt; p.flush_cnt = c->flush_cnt;
  p.saux = c->flush_list;  // unused by in-place plans
  p.haux = c->hplan_haux;
  p.hl = c->hot;
  p.err = c->err; p.gen_ptr = c->gen_dev;
  p.shard = c->shard;
  const unsigned tiles = (unsigned)(nb * p.tpb);
  k_hplan_keys<<<tiles, 256, 0, s>>>(p);
  HIP_TRY(hipGetLastError());
  {
    void* tmp = c->hplan_tmp ? c->hplan_tmp : c->tmp;
    size_t tb = c->hplan_tmp ? c->hplan_tmp_bytes : c->tmp_bytes;
    HIP_TRY(rocprim::exclusive_scan(tmp, tb, p.pcnt, p.poff, 0, (size_t)ncnt, rocprim::plus<int32_t>(), s));
  }
  k_hplan_scatter<<<tiles, 256, 0, s>>>(p);
  k_hplan_dedup<ACF_HPLAN_BUCKETS><<<(unsigned)(nb << pb), 256, 0, s>>>(p);
  k_hplan_bases<<<(unsigned)nb, 1024, 0, s>>>(p);
  k_hplan_emit<<<(unsigned)(nb << pb), 256, 0, s>>>(p);
  {  // the triplets' places (fused first): per-tile counts, their scan, the records
    const unsigned ttl = (unsigned)(nb * p.ttiles);
    k_hplan_tcount<<<ttl, 256, 0, s>>>(p);
    void* tmp = c->hplan_tmp ? c->hplan_tmp : c->tmp;
    size_t tb = c->hplan_tmp ? c->hplan_tmp_bytes : c->tmp_bytes;
    HIP_TRY(rocprim::exclusive_scan(tmp, tb, p.ttc, p.tto, 0ull, (size_t)ttl + 1, rocprim::plus<unsigned long long>(),
                                    s));
    k_hplan_trip<<<ttl, 256, 0, s>>>(p);
  }
  // (a one-batch plan, the split step's, gets more workgroups per batch)
  const unsigned rx = (unsigned)std::max(64, 1024 / nb);
  k_hplan_rank_small<<<dim3(rx, nb), 256, 0, s>>>(p);
  k_hplan_rank_hot<<<dim3(rx, nb), 256, (size_t)2 * ((2 * B + 31) / 32) * sizeof(uint32_t), s>>>(p);
  HIP_TRY(hipGetLastError());
  c->plan_R = 1;
  c->plan_kind2 = 0;
  c->plan_kb = kb;
  c->tri = 1;
  c->plan_kind = 3;
  c->task_lists = 0;
  c->lists = 1;
  if (check) {
    int32_t herr = 0;
    HIP_TRY(hipMemcpyAsync(&herr, c->err, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    ACF_CHECK(herr == 0, ACF_E_RANGE, "triplet index out of range (%s%s)",
              (herr & 1) ? "user >= num_user_rows " : "", (herr & 2) ? "item >= num_item_rows" : "");
  }
  c->B = B;
  c->nb = nb;
  return ACF_OK;
}

static int batch_plan(acf_apr_ctx* c, const int32_t* user, const int32_t* ipos, const int32_t* ineg,
                      int32_t B, int32_t nb, int32_t gen, int32_t kb, int32_t check, hipStream_t s) {
  const int cur = gen & 1, oth = cur ^ 1;
  if (c->bmask_dirty[cur])  // a plan used it and no later batch plan cleared it
    HIP_TRY(hipMemsetAsync(c->bmask[cur], 0, c->bmask_words * 8, s));
  BPlanArgs p;
  p.user = user; p.ipos = ipos; p.ineg = ineg;
  p.U1 = c->U1; p.I1 = c->I1;
  p.B = B; p.S = 3 * B; p.nb = nb;
  p.rb = (int32_t)bits_for((uint64_t)std::max(c->U1, c->I1));
  p.kb = kb;
  p.W = (c->maxNB + 63) / 64;
  p.nbs = c->maxNB;
  p.R = c->R;
  p.opw = 64 / c->lpr;
  p.stride = 3 * B + (B + p.opw - 1) / p.opw;
  p.gen = gen;
  p.mask = c->bmask[cur];
  p.mask_clear = c->bmask[oth];
  p.clear_words = c->bmask_dirty[oth] ? (int64_t)c->bmask_words : 0;
  p.slot_of = c->slot_of;
  p.bkey = c->bkey; p.bstart = c->bstart; p.bocc = c->bocc; p.bn = c->bn; p.berr = c->berr;
  p.err = c->err; p.gen_ptr = c->gen_dev;
  p.urec = c->urec; p.irec = c->irec; p.inl = c->inl; p.trec = c->trec;
  p.nextt = c->nextt;
  p.task_list = c->task_list; p.task_cnt = c->task_cnt;
  p.final_list = c->final_list; p.final_cnt = c->final_cnt;
  // 3 occurrences per thread in the sort, one thread per slot / triplet in the
  // build: ~24 us for a 20-batch plan against ~32 us for 6 per thread / 256-thread
  // builds (per-thread loops serialise the build's dependent loads)
  if (B <= 512) {
    k_bplan_sort<512, 3><<<nb, 512, 0, s>>>(p);
    k_bplan_build<1024, 512><<<nb, 1024, 0, s>>>(p);
  } else {
    k_bplan_sort<1024, 3><<<nb, 1024, 0, s>>>(p);
    k_bplan_build<1024, 1024><<<nb, 1024, 0, s>>>(p);
  }
  HIP_TRY(hipGetLastError());
  c->bmask_dirty[cur] = 1;
  c->bmask_dirty[oth] = 0;
  c->plan_R = c->R;
  c->tri = 0;
  c->plan_kind = 1;
  c->plan_kind2 = 1;
  c->plan_kb = kb;
  c->task_lists = 1;
  c->task_stride = p.stride;
  c->lists = 0;
  c->final_ok = (int64_t)c->maxNB * 3 * c->maxB < (1ll << 31) ? 1 : 0;
  if (check) {
    int32_t herr = 0;
    HIP_TRY(hipMemcpyAsync(&herr, c->err, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    ACF_CHECK(herr == 0, ACF_E_RANGE, "triplet index out of range (%s%s)",
              (herr & 1) ? "user >= num_user_rows " : "", (herr & 2) ? "item >= num_item_rows" : "");
  }
  c->B = B;
  c->nb = nb;
  return ACF_OK;
}

// shard mode, one batch of B <= 1,024: the one-workgroup plan (k_shard_plan)
static int shard_plan_small(acf_apr_ctx* c, const int32_t* user, const int32_t* ipos, const int32_t* ineg,
                            int32_t B, int32_t gen, int32_t check, hipStream_t s) {
  const int32_t kb = (int32_t)bits_for((uint64_t)3 * B + 1);
  SPlanArgs p;
  p.user = user; p.ipos = ipos; p.ineg = ineg;
  p.U1 = c->U1; p.I1 = c->I1;
  p.B = B;
  p.rb = (int32_t)bits_for((uint64_t)std::max(c->U1, c->I1));
  p.kb = kb;
  p.gen = gen;
  p.uuniq = c->uuniq; p.uoff = c->uoff; p.ubs = c->ubs;
  p.iuniq = c->iuniq; p.ioff = c->ioff; p.ibs = c->ibs;
  p.tsl = c->tsl; p.tpos = c->tpos;
  p.uinfo = c->uinfo; p.iinfo = c->iinfo;
  p.urec = c->urec; p.irec = c->irec; p.inl = c->inl; p.trec = c->trec;
  p.gen_ptr = c->gen_dev; p.err = c->err;
  p.sflags = c->key_in;
  p.hl = c->hot;
  p.slot_list = c->slot_list; p.flush_list = c->flush_list;
  p.slot_cnt = c->slot_cnt; p.flush_cnt = c->flush_cnt;
  k_shard_plan<1024, 3><<<1, 1024, 0, s>>>(p);
  HIP_TRY(hipGetLastError());
  c->plan_R = 1;
  c->plan_kind2 = 0;
  c->plan_kb = kb;
  c->tri = 0;
  c->plan_kind = 2;
  c->task_lists = 0;
  c->lists = 1;
  if (check) {
    int32_t herr = 0;
    HIP_TRY(hipMemcpyAsync(&herr, c->err, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    ACF_CHECK(herr == 0, ACF_E_RANGE, "triplet index out of range (%s%s)",
              (herr & 1) ? "user >= num_user_rows " : "", (herr & 2) ? "item >= num_item_rows" : "");
  }
  c->B = B;
  c->nb = 1;
  return ACF_OK;
}

// sorted keys -> head flags -> one scan -> per-side compaction
template <class KT>
static int plan_groups(acf_apr_ctx* c, const KT& ku, const KT& ki, int64_t E, int32_t nb,
                       hipStream_t s) {
  k_heads<KT><<<grid_for(3 * E), 256, 0, s>>>(ku, ki, E, c->flag);
  size_t tb = c->tmp_bytes;
  HIP_TRY(rocprim::inclusive_scan(c->tmp, tb, c->flag, c->inc, (size_t)(3 * E), rocprim::plus<int32_t>(), s));
  k_compact<KT><<<grid_for(E), 256, 0, s>>>(ku, c->inc, nullptr, E, c->U1, nb, c->uuniq, c->uoff, c->ubs,
                                            c->tsl, c->tpos, 0);
  k_compact<KT><<<grid_for(2 * E), 256, 0, s>>>(ki, c->inc + E, c->inc + E - 1, 2 * E, c->I1, nb, c->iuniq,
                                                c->ioff, c->ibs, c->tsl, c->tpos, 1);
  HIP_TRY(hipGetLastError());
  return ACF_OK;
}

extern "C" int acf_apr_plan(acf_apr_ctx* c, const int32_t* user, const int32_t* ipos,
                            const int32_t* ineg, int32_t B, int32_t nb, int32_t check,
                            void* stream_) {
  ACF_CHECK(c, ACF_E_INVALID, "ctx is NULL");
  ACF_CHECK(user && ipos && ineg, ACF_E_INVALID, "triplet pointers must be non-NULL");
  ACF_CHECK(B > 0 && B <= c->maxB, ACF_E_INVALID, "batch_size %d outside (0, %d]", B, c->maxB);
  ACF_CHECK(nb > 0 && nb <= c->maxNB, ACF_E_INVALID, "n_batches %d outside (0, %d]", nb, c->maxNB);
  hipStream_t s = static_cast<hipStream_t>(stream_);
  const int64_t E = (int64_t)B * nb;
  const uint32_t ob_u = bits_for((uint64_t)E), ob_i = bits_for((uint64_t)(2 * E));
  const uint32_t eb_u = ob_u + bits_for((uint64_t)nb * (uint64_t)c->U1);
  const uint32_t eb_i = ob_i + bits_for((uint64_t)nb * (uint64_t)c->I1);
  const uint32_t eb = std::max(eb_u, eb_i);  // item keys carry bit eb
  ACF_CHECK(eb < 64, ACF_E_INVALID, "plan key does not fit 64 bits");
  ACF_RET(resolve(c, 1));  // a queued streamed call of this context still needs its plan
  if (c->replay_dirty) {
    // a settling point replayed a call of this context on its own stream (the
    // two-kernel schedule reads the records this plan overwrites): a plan on
    // another stream -- PlanPipeline's side stream -- starts after that replay
    c->replay_dirty = false;
    HIP_TRY(hipStreamWaitEvent(s, c->replay_ev, 0));
  }
  c->B = 0;
  c->nb = 0;
  c->last_delta_batch = -1;
  c->final_ok = 0;  // set by the batch plan
  const int32_t gen = ++c->gen;
  {
    const int packed = is_packed(c, B);
    const int32_t kb = (int32_t)bits_for((uint64_t)3 * B + 1);
    if (!packed && c->plan_mode == 0 && B <= 1024 && kb + bits_for((uint64_t)nb + 1) <= 31 && bplan_ready(c))
      return batch_plan(c, user, ipos, ineg, B, nb, gen, kb, check, s);
  }
  if (c->shard && nb == 1 && B <= 1024 && c->plan_mode == 0 &&
      bits_for((uint64_t)std::max(c->U1, c->I1)) <= 30)
    return shard_plan_small(c, user, ipos, ineg, B, gen, check, s);
  // triplet-centric plans (r05: in shard mode too, from B = 1,025)
  if (is_packed(c, B) && c->fusion && c->plan_mode == 0 && B <= ACF_HPLAN_MAXB && hplan_ready(c))
    return hash_plan(c, user, ipos, ineg, B, nb, gen, (int32_t)bits_for((uint64_t)3 * B + 1), check, s);
  HIP_TRY(hipMemsetAsync(c->err, 0, sizeof(int32_t), s));
  // 32-bit keys (segment only, occurrence as the sort value) when they fit
  const uint32_t sb = std::max(bits_for((uint64_t)nb * (uint64_t)c->U1),
                               bits_for((uint64_t)nb * (uint64_t)c->I1));
  const bool pairs = sb < 32;
  const uint64_t item_bit = 1ull << (pairs ? sb : eb);
  const int64_t n3 = 3 * E;
  size_t tb = c->tmp_bytes;
  if (pairs) {
    uint32_t* kin = reinterpret_cast<uint32_t*>(c->key_in);
    int32_t* vin = reinterpret_cast<int32_t*>(kin + n3);
    uint32_t* kout = reinterpret_cast<uint32_t*>(c->key_out);
    int32_t* vout = reinterpret_cast<int32_t*>(kout + n3);
    k_stage<true><<<grid_for(E), 256, 0, s>>>(user, ipos, ineg, E, B, c->U1, c->I1, kin, vin, 0, 0,
                                              item_bit, c->err);
    HIP_TRY(hipGetLastError());
    HIP_TRY(rocprim::radix_sort_pairs(c->tmp, tb, kin, kout, vin, vout, (size_t)n3, 0, sb + 1, s));
    const Key32 ku{kout, vout, ~0u}, ki{kout + E, vout + E, ~(uint32_t)item_bit};
    ACF_RET(plan_groups(c, ku, ki, E, nb, s));
  } else {
    k_stage<false><<<grid_for(E), 256, 0, s>>>(user, ipos, ineg, E, B, c->U1, c->I1, c->key_in,
                                               nullptr, ob_u, ob_i, item_bit, c->err);
    HIP_TRY(hipGetLastError());
    HIP_TRY(rocprim::radix_sort_keys(c->tmp, tb, c->key_in, c->key_out, (size_t)n3, 0, eb + 1, s));
    const Key64 ku{c->key_out, ob_u, ~0ull}, ki{c->key_out + E, ob_i, ~item_bit};
    ACF_RET(plan_groups(c, ku, ki, E, nb, s));
  }
  // where each unique row's value lives at batch start, then the records; one
  // lane-group per slot (large batches) reads only a slot's first record inline
  // (one-wave-per-slot plans encode every earlier batch, below)
  const int packed = is_packed(c, B);
  const int32_t kb = (int32_t)bits_for((uint64_t)3 * B + 1);
  // one-wave-per-slot plans encode every earlier batch (dt < nb must fit the src)
  const VKeys vk{(int32_t)bits_for((uint64_t)std::max(c->U1, c->I1)), (int32_t)bits_for((uint64_t)nb), 0};
  const int all_dt = !packed && kb + bits_for((uint64_t)nb + 1) <= 31 && vk.rb + vk.tb <= 32;
  if (all_dt) {
    // slots k_prev_next does not name (no row) read as "next batch 0": never flushed
    HIP_TRY(hipMemsetAsync(c->nextt, 0, (size_t)n3 * sizeof(int32_t), s));
    VKeys v = vk;
    v.k32 = 1 + vk.rb + vk.tb <= 31;
    uint32_t* k32 = reinterpret_cast<uint32_t*>(c->key_in);
    int32_t* v32 = reinterpret_cast<int32_t*>(k32 + n3);
    uint32_t* o32 = reinterpret_cast<uint32_t*>(c->key_out);
    int32_t* w32 = reinterpret_cast<int32_t*>(o32 + n3);
    k_vkeys<<<grid_for(n3), 256, 0, s>>>(c->uuniq, c->iuniq, c->ubs, c->ibs, E, nb, v,
                                         v.k32 ? (void*)k32 : (void*)c->key_in, v32);
    HIP_TRY(hipGetLastError());
    size_t tb3 = c->tmp_bytes;
    const int bits = 1 + vk.rb + vk.tb;
    if (v.k32) {
      // padding keys are all ones: past every valid key in the sorted bits (ties keep input order)
      HIP_TRY(rocprim::radix_sort_pairs(c->tmp, tb3, k32, o32, v32, w32, (size_t)n3, 0, bits, s));
    } else {
      HIP_TRY(rocprim::radix_sort_keys(c->tmp, tb3, c->key_in, c->key_out, (size_t)n3, 0, bits + 30, s));
    }
    k_prev_next<<<grid_for(n3), 256, 0, s>>>(v.k32 ? (const void*)o32 : (const void*)c->key_out, w32, E, v,
                                             c->uoff, c->ioff, c->ubs, c->ibs, 3 * B, kb, c->uinfo, c->iinfo,
                                             c->nextt);
  } else {
    // triplet-centric plans (packed, fusion on, not shard mode) update every row in
    // its table: no source / next-batch search (k_slot_info inplace)
    const int32_t tri_plan = packed && !c->shard && c->fusion;
    k_slot_info<<<grid_for(E), 256, 0, s>>>(c->uuniq, c->uoff, c->ubs, c->ubs, (int32_t)E, nb, 0, kb,
                                            c->uinfo, tri_plan);
    k_slot_info<<<grid_for(2 * E), 256, 0, s>>>(c->iuniq, c->ioff, c->ubs, c->ibs, (int32_t)(2 * E), nb, 1,
                                                kb, c->iinfo, tri_plan);
  }
  HIP_TRY(hipGetLastError());
  c->plan_R = packed ? 1 : c->R;
  c->plan_kind = 0;
  c->plan_kind2 = all_dt;
  c->plan_kb = kb;
  c->tri = packed && !c->shard && c->fusion;
  if (c->shard) {
    // Shard plans are replayed inside captured step graphs (distributed.ShardedAPR),
    // where a step's generation repeats from one replay to the next: clear the
    // inline records so that a slot this plan does not write never reads as
    // current (k_flush scans every slot of the batch).
    HIP_TRY(hipMemsetAsync(c->inl, 0, (size_t)nb * 3 * B * sizeof(OccRec), s));
  }
  if (packed) {  // k_records writes the slot flags of the slots it finds; the rest read 0
    HIP_TRY(hipMemsetAsync(c->key_in, 0, (size_t)3 * E * sizeof(uint64_t), s));
    HIP_TRY(hipMemsetAsync(c->hot.cnt, 0, 2 * (size_t)c->maxNB * sizeof(int32_t), s));
    HIP_TRY(hipMemsetAsync(c->hot.arrive, 0, (size_t)nb * c->hot.piece_stride * sizeof(int32_t), s));
  }
  k_records<<<grid_for(E), 256, 0, s>>>(E, B, 3 * B, c->plan_R, gen, kb, c->shard, c->tri,
                                        reinterpret_cast<const int4*>(c->tsl),
                                        reinterpret_cast<const int4*>(c->tpos), c->uinfo, c->iinfo,
                                        c->ubs, c->ibs, c->urec, c->irec, c->inl, c->trec, c->gen_dev,
                                        packed ? c->key_in : nullptr, c->hot);
  HIP_TRY(hipGetLastError());
  c->task_lists = 0;
  if (all_dt) {  // streamed-step task lists
    const int32_t opw = 64 / c->lpr, G = (B + opw - 1) / opw, stride = 3 * B + G;
    const int64_t n = (int64_t)nb * stride;
    int32_t* fl = reinterpret_cast<int32_t*>(c->key_in);
    int32_t* inc = reinterpret_cast<int32_t*>(c->key_out);
    k_task_flags<<<grid_for(n), 256, 0, s>>>(c->inl, c->trec, n, 3 * B, G, B, c->plan_R, opw, gen, fl);
    size_t tb4 = c->tmp_bytes;
    HIP_TRY(rocprim::inclusive_scan(c->tmp, tb4, fl, inc, (size_t)n, rocprim::plus<int32_t>(), s));
    k_task_list<<<grid_for(n), 256, 0, s>>>(fl, inc, n, stride, c->task_list, c->task_cnt);
    HIP_TRY(hipGetLastError());
    c->task_lists = 1;
    c->task_stride = stride;
  }
  c->lists = 0;
  if (packed) {  // per-batch lists of non-fused slots and of rows left in W scratch
    const int64_t n = (int64_t)nb * 3 * B;
    size_t tb2 = c->tmp_bytes;
    HIP_TRY(rocprim::inclusive_scan(c->tmp, tb2, c->key_in, c->key_out, (size_t)n, rocprim::plus<uint64_t>(), s));
    k_slot_lists<<<grid_for(n), 256, 0, s>>>(c->key_in, c->key_out, n, 3 * B, c->slot_list, c->flush_list,
                                             c->slot_cnt, c->flush_cnt);
    HIP_TRY(hipGetLastError());
    c->lists = 1;
  }
  if (check) {
    int32_t herr = 0;
    HIP_TRY(hipMemcpyAsync(&herr, c->err, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    ACF_CHECK(herr == 0, ACF_E_RANGE, "triplet index out of range (%s%s)",
              (herr & 1) ? "user >= num_user_rows " : "",
              (herr & 2) ? "item >= num_item_rows" : "");
  }
  c->B = B;
  c->nb = nb;
  return ACF_OK;
}

extern "C" int acf_apr_set_plan_mode(acf_apr_ctx* c, int32_t mode) {
  ACF_CHECK(c, ACF_E_INVALID, "ctx is NULL");
  ACF_RET(resolve(c, 2));  // settle queued streamed calls first (FailGroup)
  ACF_CHECK(mode == 0 || mode == 1, ACF_E_INVALID, "plan mode must be 0 (auto) or 1 (sort plan)");
  c->plan_mode = mode;
  return ACF_OK;
}

extern "C" int acf_apr_plan_kind(const acf_apr_ctx* c) { return c ? c->plan_kind : -1; }
