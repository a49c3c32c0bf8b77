// All-items ranking kernels of libacf_neumf.so (k_nmf_rank, k_nmf_rank_pos):
// included by acf_neumf.hip after acf_topk_select.h (topk_key, topk_prune,
// k_topk_merge) and acf_neumf_step.h (the layout, MR, mfma_panel, inst_block's
// forward); one translation unit.  The strips, the workspace and the entry points
// are host code in acf_neumf.hip.  DESIGN.md §4e.
//
// acf_neumf_rank_all: positions and top-K lists of whole users
// with no pair list and no U x I score array.  A work item is (entry r of `users`,
// strip of the candidate range); a workgroup stages the weights once and takes
// work items blockIdx.x, + gridDim.x, ...  Per work item it loads the user's two
// rows once, builds the strip's exclusion bitmap in LDS (set semantics: unsorted,
// repeated and out-of-range entries need no preparation) and walks the strip MR
// candidates a block: the block's item rows are one contiguous span of MF_I /
// MLP_I (the next block's in flight while this one computes), the forward is
// inst_block<2>'s, statement for statement -- the same LDS images, the same
// mfma_panel calls, the same 16-lane head and sigmoid -- and an MFMA tile's row
// depends on its own A row only, so score(u, c) has acf_neumf_predict's bits
// whatever the other 15 rows hold.  The 16 scores never leave the workgroup: a
// counter per head lane (score >= the test item's score, which the prologue
// k_nmf_inst<2> launch computed) and acf_topk_select.h's bounded key buffer
// (RK_CAP keys, at most MR appended a block, pruned above RK_CAP - MR).  The
// strips' partial lists go through k_topk_merge, the strips' counts are summed by
// k_nmf_rank_pos.  Integer atomics in LDS only; every result is exact.
#pragma once

constexpr int RK_CAP = 256;          // keys of a work item's buffer (>= TOPK_MAX_K + MR)
constexpr int RK_STRIP_MIN = 4096;   // candidates of a strip, at least (more strips only to fill the device)
constexpr int RK_STRIP_MAX = 32768;  // ... at most: the exclusion bitmap is RK_STRIP_MAX / 8 bytes of LDS
constexpr int RK_TARGET_WG = 1024;   // work items wanted before strips stop being cut
static_assert(RK_CAP >= TOPK_MAX_K + MR && RK_CAP % 64 == 0, "key buffer");

struct RankArgs {
  const float* P;
  int64_t off[S_COUNT];
  int64_t U1;
  int32_t d;
  const int32_t* users;
  int32_t n_users, nc;
  const int64_t* excl_off;  // NULL: no exclusions
  const int32_t* excl;
  const float* tscore;      // [n_users] score of each entry's test item; NULL: no positions
  int32_t K, S, strip_len;  // strip_len % MR == 0
  uint64_t* keys;           // [n_users][S][K] partial lists
  int32_t* cnt;             // [n_users][S] partial counts
  int32_t* err;
};

// LDS of k_nmf_rank in bytes: keys | bitmap | h0, a1, f | b1, b2, Wo, bo | MF_U[u] | W1, W2
__host__ __device__ __forceinline__ int64_t rank_smem(int d) {
  int64_t f = (int64_t)3 * MR * (2 * d + 1) + 5 * d + 4 + d;
  if (weights_in_lds(d)) f += (int64_t)2 * d * (2 * d + 1) + (int64_t)2 * d * (d + 1);
  return (int64_t)RK_CAP * 8 + RK_STRIP_MAX / 8 + f * 4;
}

template <int DC>
__global__ void __launch_bounds__(256) k_nmf_rank(RankArgs a) {
  extern __shared__ float sm[];
  __shared__ int s_cnt[1];
  __shared__ uint64_t s_thr[1];
  __shared__ int s_pc[MR];
  const int d = DC ? DC : a.d, d2 = 2 * d, tid = threadIdx.x;
  const int L2 = d2 + 1, L1 = d + 1;
  uint64_t* buf = reinterpret_cast<uint64_t*>(sm);           // [RK_CAP]
  uint32_t* s_ex = reinterpret_cast<uint32_t*>(buf + RK_CAP);  // [RK_STRIP_MAX / 32]
  float* s_x = reinterpret_cast<float*>(s_ex + RK_STRIP_MAX / 32);  // [MR][L2] h0 = MLP_U[u] | MLP_I[c]
  float* s_a1 = s_x + MR * L2;   // [MR][L2]
  float* s_f = s_a1 + MR * L2;   // [MR][L2] MF_U[u] * MF_I[c] | a2
  float* s_vec = s_f + MR * L2;  // b1 [2d] | b2 [d] | Wo [2d] | bo (+3)
  float* s_b1 = s_vec, *s_b2 = s_vec + d2, *s_wo = s_b2 + d, *s_bo = s_wo + d2;
  float* s_mu = s_bo + 4;        // [d] MF_U[u]
  float* s_w1 = s_mu + d;        // [2d][2d+1] (weights_in_lds)
  float* s_w2 = s_w1 + d2 * L2;  // [2d][d+1]
  const bool wl = weights_in_lds(d);
  // once per workgroup: biases, head and (d <= 64) the two weight panels
  for (int x = tid; x < 5 * d + 1; x += 256) {
    const int64_t src = x < d2 ? a.off[S_B1] + x
                               : x < 3 * d ? a.off[S_B2] + (x - d2)
                                           : x < 5 * d ? a.off[S_WO] + (x - 3 * d) : a.off[S_BO];
    s_vec[x] = a.P[src];
  }
  if (wl) {
    const float4* g1 = reinterpret_cast<const float4*>(a.P + a.off[S_W1]);
    const float4* g2 = reinterpret_cast<const float4*>(a.P + a.off[S_W2]);
    for (int x = tid; x < d2 * d2 / 4; x += 256) {
      const float4 v = g1[x];
      const int e = 4 * x, rr = e / d2, cc = e - rr * d2;
      float* dst = s_w1 + rr * L2 + cc;
      dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
    }
    for (int x = tid; x < d2 * d / 4; x += 256) {
      const float4 v = g2[x];
      const int e = 4 * x, rr = e / d, cc = e - rr * d;
      float* dst = s_w2 + rr * L1 + cc;
      dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
    }
  }
  const float* W1 = wl ? s_w1 : a.P + a.off[S_W1];
  const float* W2 = wl ? s_w2 : a.P + a.off[S_W2];
  const int ld1 = wl ? L2 : d2, ld2 = wl ? L1 : d;
  // a block's item rows: float4 x = tid + 256 q of the MR x d span starting at row c0
  constexpr int QG = MR * 128 / 4 / 256;  // d <= 128
  const int n4 = MR * d / 4;
  float4 gm[QG], gl[QG];
  auto gather = [&](int c0) {
    const float4* mi = reinterpret_cast<const float4*>(a.P + a.off[S_MF_I] + (int64_t)c0 * d);
    const float4* li = reinterpret_cast<const float4*>(a.P + a.off[S_MLP_I] + (int64_t)c0 * d);
#pragma unroll
    for (int q = 0; q < QG; ++q) {
      const int x = tid + 256 * q;
      const bool ok = x < n4 && c0 + (4 * x) / d < a.nc;  // rows past the candidates: zeros, never consumed
      gm[q] = ok ? mi[x] : make_float4(0.f, 0.f, 0.f, 0.f);
      gl[q] = ok ? li[x] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  int bad = 0;
  const int64_t total = (int64_t)a.n_users * a.S;
  for (int64_t w = blockIdx.x; w < total; w += gridDim.x) {
    const int64_t r = w / a.S;
    const int strip = (int)(w - r * a.S);
    const int c_lo = strip * a.strip_len, c_hi = min(a.nc, c_lo + a.strip_len);
    __syncthreads();  // the previous work item's reads (first pass: the staged weights)
    int32_t u = a.users[r];
    if (u < 0 || u >= a.U1) {
      bad = 1;
      u = 0;
    }
    for (int k = tid; k < d; k += 256) {
      s_mu[k] = a.P[a.off[S_MF_U] + (int64_t)u * d + k];
      const float lu = a.P[a.off[S_MLP_U] + (int64_t)u * d + k];
      for (int t = 0; t < MR; ++t) s_x[t * L2 + k] = lu;
    }
    for (int x = tid; x < (a.strip_len + 31) / 32; x += 256) s_ex[x] = 0u;
    if (tid == 0) {
      s_cnt[0] = 0;
      s_thr[0] = 0;
    }
    __syncthreads();
    if (a.excl_off) {
      const int64_t e1 = a.excl_off[r + 1];
      for (int64_t x = a.excl_off[r] + tid; x < e1; x += 256) {
        const int32_t it = a.excl[x];
        if (it >= c_lo && it < c_hi) atomicOr(&s_ex[(it - c_lo) >> 5], 1u << ((it - c_lo) & 31));
      }
    }
    const float ts = a.tscore ? a.tscore[r] : 0.f;
    int npos = 0;
    gather(c_lo);
    for (int c0 = c_lo; c0 < c_hi; c0 += MR) {
#pragma unroll
      for (int q = 0; q < QG; ++q) {
        const int x = tid + 256 * q;
        if (x < n4) {
          const int e = 4 * x, t = e / d, k = e - t * d;
          float* hx = s_x + t * L2 + d + k;
          float* hf = s_f + t * L2 + k;
          hx[0] = gl[q].x; hx[1] = gl[q].y; hx[2] = gl[q].z; hx[3] = gl[q].w;
          hf[0] = s_mu[k] * gm[q].x;  // GMF tower
          hf[1] = s_mu[k + 1] * gm[q].y;
          hf[2] = s_mu[k + 2] * gm[q].z;
          hf[3] = s_mu[k + 3] * gm[q].w;
        }
      }
      __syncthreads();  // (first block: also the bitmap)
      if (c0 + MR < c_hi) gather(c0 + MR);
      // layer 1: a1 = relu(h0 W1 + b1)
      mfma_panel<false>(s_x, L2, W1, ld1, d2, d2, [&](int row, int col, float v) {
        const float z = v + s_b1[col];
        s_a1[row * L2 + col] = z > 0.f ? z : 0.f;
      });
      __syncthreads();
      // layer 2: a2 = relu(a1 W2 + b2) -> f[d:2d]
      mfma_panel<false>(s_a1, L2, W2, ld2, d2, d, [&](int row, int col, float v) {
        const float z = v + s_b2[col];
        s_f[row * L2 + d + col] = z > 0.f ? z : 0.f;
      });
      __syncthreads();
      // head: 16 lanes per candidate, p = sigmoid(f Wo + bo); the score is consumed here
      {
        const int row = tid >> 4, part = tid & 15;
        float sacc = 0.f;
        for (int k = part; k < d2; k += 16) sacc = sacc + s_f[row * L2 + k] * s_wo[k];
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) sacc += __shfl_xor(sacc, m, 64);
        if (part == 0) {
          const float logit = sacc + s_bo[0];
          const float p = 1.0f / (1.0f + expf(-logit));
          const int c = c0 + row, wbit = c - c_lo;
          if (c < c_hi && !((s_ex[wbit >> 5] >> (wbit & 31)) & 1u)) {
            if (a.tscore && p >= ts) ++npos;
            if (a.K > 0) {
              const uint64_t key = topk_key(p, c);
              if (key > s_thr[0]) {
                const int pos = atomicAdd(&s_cnt[0], 1);
                if (pos < RK_CAP) buf[pos] = key;
              }
            }
          }
        }
      }
      if (a.K > 0) topk_prune<1, RK_CAP / 64>(buf, s_cnt, s_thr, nullptr, RK_CAP, a.K, RK_CAP - MR);
      else __syncthreads();
    }
    if (a.K > 0) {
      __syncthreads();
      topk_prune<1, RK_CAP / 64>(buf, s_cnt, s_thr, nullptr, RK_CAP, a.K, -1);
      topk_store_partial(a.keys, buf, s_cnt[0], a.K, r, strip, a.S, tid, 256);
    }
    if (a.tscore) {
      if ((tid & 15) == 0) s_pc[tid >> 4] = npos;
      __syncthreads();
      if (tid == 0) {
        int sum = 0;
        for (int t = 0; t < MR; ++t) sum += s_pc[t];
        a.cnt[r * a.S + strip] = sum;
      }
    }
  }
  if (bad) atomicOr(a.err, bad);
}

// positions[r] = the sum of entry r's strip counts
__global__ void __launch_bounds__(256) k_nmf_rank_pos(const int32_t* __restrict__ cnt, int S, int n,
                                                      int32_t* __restrict__ pos) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  int sum = 0;
  for (int s = 0; s < S; ++s) sum += cnt[r * S + s];
  pos[r] = sum;
}
