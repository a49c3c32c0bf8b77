// What the VALU score sweeps of libacf_apr.so share (k_eval_all, k_topk_valu,
// k_evx_sweep; seq_dot: every ranking kernel): included by acf_rank.hip before
// acf_eval.h; one translation unit.  __device__ __forceinline__ pieces and two
// host helpers, no kernels.  DESIGN.md §4.
#pragma once

// ---------------------------------------------------------------------------
// score(u,c) = sequential sum over k of round(P[u][k]*Q[c][k]) (_eval_by_user,
// utils.py:244-254; TF's product rounding).  Every score that is stored or
// compared anywhere in the ranking kernels comes out of seq_step, in ascending k
// from +0.f, so that equal pairs give equal bits on every path and ">=" ties
// are decided exactly.  The chain never yields -0.0: it starts at +0.0 and a
// round-to-nearest sum is -0.0 only from two negative zeros.
// The sweeps keep their own loop over k around seq_step (8 rows of a tile in LDS
// against one candidate row, q read once): moved into a function here, hipcc
// schedules the same loop differently and k_evx_sweep measured 2.6-3.7x slower,
// k_topk_valu 4-7 %.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float seq_step(float s, const float4 pv, const float4 qv) {
  s = s + pv.x * qv.x;
  s = s + pv.y * qv.y;
  s = s + pv.z * qv.z;
  s = s + pv.w * qv.w;
  return s;
}

__device__ __forceinline__ float seq_dot(const float* __restrict__ p, const float* __restrict__ q,
                                         int d) {
  float s = 0.f;
  for (int k = 0; k < d; k += 4) {
    const float4 qv = *reinterpret_cast<const float4*>(q + k);
    const float4 pv = *reinterpret_cast<const float4*>(p + k);
    s = seq_step(s, pv, qv);
  }
  return s;
}

// rows[UB][d] (LDS) = rows users[u0 .. u0 + nu) of P, zeros past nu; a workgroup
// of 256, no barrier inside.  CHECK: a row outside [0, U1) is read as row 0 and
// bit 1 is ORed into *err; without it the caller has validated users on the host.
template <int UB, bool CHECK>
__device__ __forceinline__ void sweep_load_rows(float* rows, const float* __restrict__ P, int d,
                                                const int32_t* __restrict__ users, int u0, int nu, int64_t U1,
                                                int32_t* err) {
  for (int idx = threadIdx.x; idx < UB * d; idx += 256) {
    const int uu = idx / d, k = idx - uu * d;
    float v = 0.f;
    if (uu < nu) {
      int64_t row = users[u0 + uu];
      if (CHECK && (row < 0 || row >= U1)) {
        row = 0;
        if (k == 0) atomicOr(err, 1);
      }
      v = P[row * d + k];
    }
    rows[idx] = v;
  }
}

// ---- exclusion bitmap -------------------------------------------------------
// bits[uu] = the SET of user uu's exclusion entries inside [c0, c0 + n), n <=
// BITS, as bit (entry - c0), one strided pass per user: unsorted, repeated and
// out-of-range entries need no preparation.  off[0 .. nu] (LDS) are the tile's
// offsets into excl.  Barrier contract, a workgroup of 256: the caller has
// synchronised every earlier read of bits (off may still be unsynchronised: the
// barrier after the clear covers it); on return the bits are NOT synchronised,
// the caller's next barrier publishes them.
template <int UB, int BITS>
__device__ __forceinline__ void sweep_excl_strided(uint32_t (&bits)[UB][BITS / 32], const int64_t* off, int nu,
                                                   const int32_t* __restrict__ excl, int64_t c0, int64_t n) {
  const int tid = threadIdx.x;
  for (int x = tid; x < UB * (BITS / 32); x += 256) (&bits[0][0])[x] = 0u;
  __syncthreads();
  for (int uu = 0; uu < nu; ++uu) {
    for (int64_t x = off[uu] + tid; x < off[uu + 1]; x += 256) {
      const int64_t it = (int64_t)excl[x] - c0;
      if (it >= 0 && it < n) atomicOr(&bits[uu][it >> 5], 1u << (it & 31));
    }
  }
}

// ---- host -------------------------------------------------------------------
// the MFMA sweeps' error band (k_eval_fused's comment): eb = 4 (d + 2) 2^-24, and
// 4 d FLT_MIN for the denormal products that MFMA flushes
static void mfma_err_band(int d, float* eb, float* floor_e) {
  *eb = 4.0f * (float)(d + 2) * 5.9604645e-8f;
  *floor_e = (float)d * 1.1754944e-38f * 4.0f;
}

// Cut [0, num_cand) into S strips of wper whole windows of `win` candidates, one
// workgroup per (tile of `ub` users, strip): enough strips that about `target`
// workgroups fill the device when there are few users, no more than there are
// windows, and few enough that the strips' partial results (strip_bytes each)
// stay under 48 MiB.
static void sweep_strips(int64_t num_cand, int win, int64_t n_users, int ub, int64_t target, int64_t strip_bytes,
                         int* wper, int* S) {
  const int64_t W = std::max<int64_t>(1, (num_cand + win - 1) / win);  // windows
  const int64_t tiles = std::max<int64_t>(1, (n_users + ub - 1) / ub);
  int64_t s = (target + tiles - 1) / tiles;
  s = std::min(s, ((int64_t)48 << 20) / strip_bytes);
  s = std::max<int64_t>(1, std::min(s, W));
  const int64_t per = (W + s - 1) / s;
  *wper = (int)per;
  *S = (int)((W + per - 1) / per);
}
