// The NeuMF training step of libacf_neumf.so (k_nmf_inst, k_nmf_step, k_nmf_wsum,
// k_nmf_rows), with the parameter layout and NArgs that host and device share:
// included by acf_neumf.hip after hip_runtime.h, first of its three kernel
// headers; one translation unit.  DESIGN.md §9.
//
// One training step (Keras train_on_batch):
//   k_nmf_inst<CLEAN>   workgroups looping over blocks of 16 instances: gather
//                       MF_U[u], MF_I[i], MLP_U[u], MLP_I[i]; MLP [2d -> 2d -> d]
//                       relu on f32 MFMA (16x16x4, exact f32 products); head;
//                       BCE (prediction clipped to [1e-7, 1-1e-7]); backward
//                       through head and MLP; per-instance row contributions;
//                       the weight gradients of the block (outer products over
//                       its 16 instances on MFMA) into the workgroup's slot
//   k_nmf_rows          one wave per (instance, side): the row's first
//                       occurrence owns it and sums every occurrence's
//                       contribution in instance order into the gradient row;
//                       with adver also delta = eps * g / |g| of that row.  The
//                       step's last k_nmf_rows launch also sums the weight-
//                       gradient slots in slot order (deterministic, no atomics)
//   (adver) k_nmf_inst<ADV>, k_nmf_rows on the perturbed rows, scaled by reg_adv
//
// Batches of <= FR_MAXB instances sum their rows in line instead: one
// k_nmf_step launch per adversarial step (k_nmf_inst<MODE, DC, true> per pass
// otherwise) holds the instance workgroups, which take their weight-gradient
// tiles from LDS and count arrivals at their rows, and the row waves, whose
// owners wait for the arrivals and sum the rows in k_nmf_rows' order.
//
// The MLP is tiny per instance (2d x 2d and 2d x d at d = 64); the step is a
// latency-bound chain (gather -> 4 MFMA layers -> weight gradients -> rows).
// acf_neumf_predict is k_nmf_inst's forward half (MODE 2).
#pragma once

// parameter segments, in Keras order
enum { S_MF_U = 0, S_MF_I, S_MLP_U, S_MLP_I, S_W1, S_B1, S_W2, S_B2, S_WO, S_BO, S_COUNT };

struct Layout {
  int64_t off[S_COUNT];
  int64_t total;
};

static Layout make_layout(int64_t U1, int64_t I1, int64_t d) {
  Layout L;
  L.off[S_MF_U] = 0;
  L.off[S_MF_I] = U1 * d;
  L.off[S_MLP_U] = (U1 + I1) * d;
  L.off[S_MLP_I] = (2 * U1 + I1) * d;
  L.off[S_W1] = 2 * (U1 + I1) * d;
  L.off[S_B1] = L.off[S_W1] + 4 * d * d;
  L.off[S_W2] = L.off[S_B1] + 2 * d;
  L.off[S_B2] = L.off[S_W2] + 2 * d * d;
  L.off[S_WO] = L.off[S_B2] + d;
  L.off[S_BO] = L.off[S_WO] + 2 * d;
  L.total = L.off[S_BO] + 4;  // bo + pad: every segment starts 16-B aligned
  return L;
}

struct NArgs {
  const float* P;
  float* G;
  int64_t off[S_COUNT];
  const int32_t* u;
  const int32_t* i;
  const float* y;
  int64_t U1, I1;
  int32_t B, d;
  float scale_over_B;    // 1/B (clean) or reg_adv/B (adversarial)
  float* contrib;        // [B][4][d] per-instance row contributions
  // the activations the weight gradients need (k_nmf_inst -> k_nmf_rows' gradient workgroups)
  float *h0, *a1, *dz1, *dz2;  // [B][2d], [B][2d], [B][2d], [B][d]
  float* wpart;          // [gridDim.x][nout] this pass's weight-gradient partials (one slot per workgroup)
  const float* delta;    // [B][4][d], rows written at their owner instance
  const int32_t* owner;  // [B][2] first occurrence of the instance's user / item
  // rows in line (k_nmf_inst<.., .., true>, B <= FR_MAXB): arrivals at each row
  // (users, then items; zero between passes), and the clean pass's delta
  int32_t* rcnt;         // [U1 + I1]
  int32_t with_delta;
  float eps;
  // both passes in one launch (k_nmf_step): per row, (gen << 32 | its first
  // occurrence) once the clean pass's owner has stored the row's delta and gradient
  unsigned long long* rdone;  // [U1 + I1]
  int32_t gen;
  // polls a rows-in-line wait makes before it gives up (err bit 512; 0: give up at
  // once -- acf_neumf_set_spin_limit, the failsafe's forcing test)
  int32_t spin;
  float* pred;
  int32_t* err;
};

__device__ __forceinline__ int32_t clamp_idx(int32_t r, int64_t n) { return (r < 0 || r >= n) ? 0 : r; }

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int MR = 16;        // instances per block = the MFMA tile height
constexpr int NSLOT = 256;    // workgroups (= weight-gradient partial slots) per training pass, at most
constexpr int DFAST = 64;     // the dimension with a compile-time specialisation of k_nmf_inst
constexpr int MAX_Q = 2;      // d <= 128: each lane holds up to 2 of a row's elements
// occurrences whose contributions are loaded together: most rows have few, and the
// unrolled predicated loads of a wider batch cost more than the round trips save
// (profiles/r05/neumf_rbatch_ab.txt; DESIGN.md §9, knob table)
constexpr int RBATCH = 4;
// rows in line (k_nmf_inst<MODE, DC, true>) up to this batch: one block of MR
// instances per workgroup, the batch's indices in LDS
constexpr int FR_MAXB = 1024;

// device-scope write-through store / load of one float (the contributions a row's
// last arrival in another workgroup reads in the same launch; MI355X guide,
// Guideline 16: no L2 write-back or invalidate)
__device__ __forceinline__ void st_wt(float* p, float v) {
  asm volatile("global_store_dword %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ float ld_dev(const float* p) {
  return __uint_as_float(__hip_atomic_load((const __attribute__((address_space(1))) uint32_t*)p, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT));
}

// Weight-gradient partial vector of one workgroup: the parameter buffer's tail from
// S_W1 on, element for element -- W1 [2d][2d] | b1 [2d] | W2 [2d][d] | b2 [d] |
// Wo [2d] | bo | (pad: the loss sum, 2 spare) -- so slot element x is the gradient
// of parameter off[S_W1] + x, and the slot sum can ride on the Adam stream.
struct WOut {
  int64_t w1, b1, w2, b2, wo, bo, loss, n;
};

__host__ __device__ __forceinline__ WOut wout(int64_t d) {
  WOut o;
  o.w1 = 0;
  o.b1 = 4 * d * d;
  o.w2 = o.b1 + 2 * d;
  o.b2 = o.w2 + 2 * d * d;
  o.wo = o.b2 + d;
  o.bo = o.wo + 2 * d;
  o.loss = o.bo + 1;
  o.n = o.bo + 4;  // = Layout total - off[S_W1], a multiple of 4
  return o;
}

// W1 and W2 are staged in LDS (row stride +1 float: the transposed reads of the
// backward products are then conflict-free) when they fit beside the activations
__host__ __device__ __forceinline__ bool weights_in_lds(int d) { return d <= 64; }

// k_nmf_inst's LDS in floats (the rows-in-line batch indices come after it)
__host__ __device__ __forceinline__ int64_t inst_floats(int d) {
  int64_t f = (int64_t)3 * MR * (2 * d + 1) + 3 * MR * (d + 1) + 2 * MR + 5 * d + 4;
  if (weights_in_lds(d)) f += (int64_t)2 * d * (2 * d + 1) + (int64_t)2 * d * (d + 1);
  return f;
}

// C[MR x N] = A[MR x K] . w(k, n) on v_mfma_f32_16x16x4_f32 (exact f32 products,
// k-ordered fma chain).  A: LDS, row-major with leading dimension lda (padded so
// the 16 lanes reading one k hit different banks); w(k, n) = W[k*ldw + n], or
// W[n*ldw + k] with TRANS (the backward products with W^T).  The 4 waves take
// 32-column panels (two 16x16 tiles, two independent accumulators) round-robin;
// epi(row, col, value) consumes every output element.  With a compile-time d
// every bound and offset folds to an immediate.
// Lane maps (cdna_hip_programming.md §3): A[l&15][k0 + (l>>4)], B[k0 + (l>>4)][l&15],
// C/D: col = l&15, row = 4*(l>>4) + reg.
template <bool TRANS>
__device__ __forceinline__ float w_at(const float* __restrict__ W, int ldw, int k, int col) {
  return TRANS ? W[(int64_t)col * ldw + k] : W[(int64_t)k * ldw + col];
}

template <bool TRANS, class Epi>
__device__ __forceinline__ void mfma_panel(const float* sA, int lda, const float* __restrict__ W, int ldw,
                                           int K, int N, Epi epi) {
  constexpr int KB = 8;  // k-steps whose operands are read before their MFMAs issue
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = lane & 15, h = lane >> 4;
  if (N > 64) {
    // two 16-column tiles per wave (independent accumulators), 32-column panels
    for (int n0 = wave * 32; n0 < N; n0 += 4 * 32) {
      f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
      const int ca = n0 + r, cb = n0 + 16 + r;
      for (int kb = 0; kb < K; kb += 4 * KB) {
        float av[KB], ba[KB], bb[KB];
#pragma unroll
        for (int j = 0; j < KB; ++j) {
          const int k = kb + 4 * j + h;
          const bool ok = k < K;
          av[j] = ok ? sA[r * lda + k] : 0.f;
          ba[j] = (ok && ca < N) ? w_at<TRANS>(W, ldw, k, ca) : 0.f;
          bb[j] = (ok && cb < N) ? w_at<TRANS>(W, ldw, k, cb) : 0.f;
        }
#pragma unroll
        for (int j = 0; j < KB; ++j) {
          c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], ba[j], c0, 0, 0, 0);
          c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bb[j], c1, 0, 0, 0);
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (ca < N) epi(4 * h + q, ca, c0[q]);
        if (cb < N) epi(4 * h + q, cb, c1[q]);
      }
    }
  } else {
    // N <= 64: one 16-column tile per wave, K split over two accumulators
    const int c = wave * 16 + r;
    if (wave * 16 >= N) return;
    f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
    for (int kb = 0; kb < K; kb += 8 * KB) {
      float a0[KB], a1[KB], w0[KB], w1[KB];
#pragma unroll
      for (int j = 0; j < KB; ++j) {
        const int k = kb + 8 * j + h, k1 = k + 4;
        a0[j] = k < K ? sA[r * lda + k] : 0.f;
        a1[j] = k1 < K ? sA[r * lda + k1] : 0.f;
        w0[j] = (k < K && c < N) ? w_at<TRANS>(W, ldw, k, c) : 0.f;
        w1[j] = (k1 < K && c < N) ? w_at<TRANS>(W, ldw, k1, c) : 0.f;
      }
#pragma unroll
      for (int j = 0; j < KB; ++j) {
        c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[j], w0[j], c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[j], w1[j], c1, 0, 0, 0);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (c < N) epi(4 * h + q, c, c0[q] + c1[q]);
  }
}

// Weight gradients of a block over its MR instances, 16x16 output tiles:
// W1 += h0^T dz1 [2d][2d], then W2 += a1^T dz2 [2d][d];
// out[k][n] (+)= sum_t A[t][k] * Bm[t][n] with A / Bm in LDS (row t), a t-ordered
// chain of 4 MFMAs per tile; each wave takes OG tiles at a time (independent
// chains).  The slot is accumulated across the workgroup's blocks (ACC: add to what
// this lane stored for the previous block -- the same lane, the same address).
constexpr int OG = 4;

// one weight gradient [K][N] (A rows with leading dimension lda, Bm rows ldb),
// its tiles [tlo, thi) (row-major over 16x16 tiles); EXACT: K and N multiples of
// 16 (no bounds); tiles tt = tlo + wave + 4 * (OG*i + g)
template <bool ACC, bool EXACT>
__device__ __forceinline__ void outer_mat(const float* A, int lda, const float* Bm, int ldb, int K, int N,
                                          float* __restrict__ out, int tlo, int thi) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, h = lane >> 4;
  const int tn = (N + 15) / 16, T = thi;
  const float* Ar = A + h * lda + r;   // lane's element of row t = h, column r
  const float* Br = Bm + h * ldb + r;
  for (int tb = tlo + wave; tb < T; tb += 4 * OG) {
    float av[OG][MR / 4], bv[OG][MR / 4];
    int k0[OG], n0[OG];
#pragma unroll
    for (int g = 0; g < OG; ++g) {
      const int tt = tb + 4 * g;  // wave-uniform
      k0[g] = (tt / tn) * 16;
      n0[g] = (tt % tn) * 16;
#pragma unroll
      for (int j = 0; j < MR / 4; ++j) {
        const bool okA = tt < T && (EXACT || k0[g] + r < K), okB = tt < T && (EXACT || n0[g] + r < N);
        av[g][j] = okA ? Ar[4 * j * lda + k0[g]] : 0.f;
        bv[g][j] = okB ? Br[4 * j * ldb + n0[g]] : 0.f;
      }
    }
    f32x4 c[OG];
#pragma unroll
    for (int g = 0; g < OG; ++g) c[g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < MR / 4; ++j)
#pragma unroll
      for (int g = 0; g < OG; ++g) c[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[g][j], bv[g][j], c[g], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < OG; ++g) {
      if (tb + 4 * g >= T) break;
      float* o = out + (int64_t)(k0[g] + 4 * h) * N + n0[g] + r;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (EXACT || (k0[g] + 4 * h + q < K && n0[g] + r < N)) {
          float* p = o + (int64_t)q * N;
          *p = ACC ? *p + c[g][q] : c[g][q];  // (ACC a template: no speculative load of the slot)
        }
      }
    }
  }
}

// tiles [lo, hi) of the two gradients' tile space (W1's T1 tiles, then W2's)
__host__ __device__ __forceinline__ int wtiles1(int d) { return ((2 * d + 15) / 16) * ((2 * d + 15) / 16); }
__host__ __device__ __forceinline__ int wtiles(int d) { return wtiles1(d) + ((2 * d + 15) / 16) * ((d + 15) / 16); }

template <bool ACC, bool EXACT>
__device__ __forceinline__ void outer_tiles(const float* s_h0, const float* s_dz1, const float* s_a1,
                                            const float* s_dz2, int d, float* __restrict__ w1,
                                            float* __restrict__ w2, int lo, int hi) {
  const int d2 = 2 * d, T1 = wtiles1(d);
  if (lo < T1) outer_mat<ACC, EXACT>(s_h0, d2 + 1, s_dz1, d2 + 1, d2, d2, w1, lo, min(hi, T1));
  if (hi > T1) outer_mat<ACC, EXACT>(s_a1, d2 + 1, s_dz2, d + 1, d2, d, w2, max(lo, T1) - T1, hi - T1);
}

// k_nmf_rows' weight-gradient workgroups take the tiles in groups of one wave round
constexpr int WG_TILES = 4 * OG;

// Weight-gradient workgroup (slot w, tile group g) -- extra workgroups of the NEXT
// launch after k_nmf_inst (the adversarial k_nmf_inst for the clean pass, the last
// k_nmf_rows for the adversarial pass), which leave most CUs idle: for the blocks
// w, w + nslot, ... of k_nmf_inst's 16 instances, stage h0, dz1, a1, dz2 in LDS
// (padded rows; instances past the batch are zero) and add tiles
// [g WG_TILES, (g+1) WG_TILES) of W1 += h0^T dz1, W2 += a1^T dz2 to slot w (the
// slot k_nmf_inst's workgroup w writes the vector partials of).
#ifdef NMF_DIAG
__device__ uint64_t g_nmf_wstamps[8];  // weight-gradient workgroup (0, 0) of the last launch that ran one
#define WSTAMP(i)                                                                          \
  do {                                                                                     \
    uint64_t t_;                                                                           \
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");         \
    if (w == 0 && g == 0 && threadIdx.x == 0) g_nmf_wstamps[i] = t_;                      \
  } while (0)
#else
#define WSTAMP(i) \
  do {            \
  } while (0)
#endif

template <bool EXACT>
__device__ __forceinline__ void wgrad_group(const NArgs& a, int w, int g, int nslot, float* sm) {
  WSTAMP(0);
  const int d = a.d, d2 = 2 * d, L2 = d2 + 1, L1 = d + 1, tid = threadIdx.x;
  float* s_h0 = sm;
  float* s_dz1 = s_h0 + MR * L2;
  float* s_a1 = s_dz1 + MR * L2;
  float* s_dz2 = s_a1 + MR * L2;
  const WOut o = wout(d);
  float* slot = a.wpart + (int64_t)w * o.n;
  const int64_t nblk = ((int64_t)a.B + MR - 1) / MR;
  const int lo = g * WG_TILES, hi = min(lo + WG_TILES, wtiles(d));
  for (int64_t blk = w; blk < nblk; blk += nslot) {
    const int64_t b0 = blk * MR;
    const int nt = (int)min((int64_t)MR, (int64_t)a.B - b0);
    if (blk != w) __syncthreads();  // the previous block's tiles are done with LDS
    // every load first (one round trip), the LDS stores after them
    constexpr int QA = MR * 256 / 256, QB = MR * 128 / 256;  // d <= 128
    float v0[QA], v1[QA], v2[QA], v3[QB];
#pragma unroll
    for (int q = 0; q < QA; ++q) {
      const int x = tid + 256 * q, t = x / d2, k = x - t * d2;
      if (256 * q < MR * d2) {  // uniform (MR d2 is a multiple of 64)
        const int64_t gi = (b0 + (x < MR * d2 && t < nt ? t : 0)) * d2 + (x < MR * d2 ? k : 0);
        v0[q] = a.h0[gi];
        v1[q] = a.dz1[gi];
        v2[q] = a.a1[gi];
      }
    }
#pragma unroll
    for (int q = 0; q < QB; ++q) {
      const int x = tid + 256 * q, t = x / d, k = x - t * d;
      if (256 * q < MR * d) v3[q] = a.dz2[(b0 + (x < MR * d && t < nt ? t : 0)) * d + (x < MR * d ? k : 0)];
    }
    WSTAMP(1);
#pragma unroll
    for (int q = 0; q < QA; ++q) {
      const int x = tid + 256 * q, t = x / d2, k = x - t * d2;
      if (x < MR * d2) {
        const bool ok = t < nt;
        s_h0[t * L2 + k] = ok ? v0[q] : 0.f;
        s_dz1[t * L2 + k] = ok ? v1[q] : 0.f;
        s_a1[t * L2 + k] = ok ? v2[q] : 0.f;
      }
    }
#pragma unroll
    for (int q = 0; q < QB; ++q) {
      const int x = tid + 256 * q, t = x / d, k = x - t * d;
      if (x < MR * d) s_dz2[t * L1 + k] = t < nt ? v3[q] : 0.f;
    }
    __syncthreads();
    WSTAMP(2);
    if (blk == w)
      outer_tiles<false, EXACT>(s_h0, s_dz1, s_a1, s_dz2, d, slot + o.w1, slot + o.w2, lo, hi);
    else
      outer_tiles<true, EXACT>(s_h0, s_dz1, s_a1, s_dz2, d, slot + o.w1, slot + o.w2, lo, hi);
    WSTAMP(3);
  }
}

static size_t wgrad_smem(int d) { return (size_t)MR * (3 * (2 * d + 1) + (d + 1)) * sizeof(float); }

#ifndef ACF_SPIN_LIMIT
#define ACF_SPIN_LIMIT (1 << 22)
#endif

// Rows in line (k_nmf_inst<MODE, DC, true>): the last arrival at a row (side s,
// row r, first occurrence f; L = the side's clamped batch indices in LDS) sums
// every occurrence's contribution in instance order -- k_nmf_rows' sum, bit for
// bit -- adds it to the gradient rows and (with_delta) writes delta at f.  One wave;
// the contributions are loaded RB occurrences at a time.
// MG (both passes in one launch): the clean pass stores the row write-through and
// then publishes it (rdone); the adversarial pass reads the gradient row that way.
template <int MODE, bool MG>
__device__ __forceinline__ void row_finish(const NArgs& a, const int32_t* L, int s, int32_t r, int f) {
  constexpr int RB = RBATCH;
  const int lane = threadIdx.x & 63, B = a.B, d = a.d;
  const int tA = s ? S_MF_I : S_MF_U, tB = s ? S_MLP_I : S_MLP_U;
  float gA[MAX_Q], gB[MAX_Q], oA[MAX_Q], oB[MAX_Q];
#pragma unroll
  for (int q = 0; q < MAX_Q; ++q) {
    const int k = lane + 64 * q;
    gA[q] = gB[q] = 0.f;
    const float* pA = a.G + a.off[tA] + (int64_t)r * d + k;
    const float* pB = a.G + a.off[tB] + (int64_t)r * d + k;
    oA[q] = k < d ? (MG && MODE == 1 ? ld_dev(pA) : *pA) : 0.f;
    oB[q] = k < d ? (MG && MODE == 1 ? ld_dev(pB) : *pB) : 0.f;
  }
  // occurrences in instance order, RB per round trip across 64-instance chunks
  // (a row's occurrences are spread over the batch: one chunk at a time would be
  // one round trip per chunk)
  int base = f & ~63;
  uint64_t mask = __ballot(base + lane < B && base + lane >= f && L[base + lane] == r);
  while (true) {
    int js[RB];
#pragma unroll
    for (int e = 0; e < RB; ++e) {
      while (!mask && base + 64 < B) {
        base += 64;
        mask = __ballot(base + lane < B && L[base + lane] == r);
      }
      js[e] = -1;
      if (mask) {
        js[e] = base + __ffsll((unsigned long long)mask) - 1;
        mask &= mask - 1;
      }
    }
    if (js[0] < 0) break;
    {
      float va[RB][MAX_Q], vb[RB][MAX_Q];
#pragma unroll
      for (int e = 0; e < RB; ++e)
#pragma unroll
        for (int q = 0; q < MAX_Q; ++q) {
          const int k = lane + 64 * q;
          const bool ok = js[e] >= 0 && k < d;
          va[e][q] = ok ? ld_dev(a.contrib + ((int64_t)js[e] * 4 + tA) * d + k) : 0.f;
          vb[e][q] = ok ? ld_dev(a.contrib + ((int64_t)js[e] * 4 + tB) * d + k) : 0.f;
        }
#pragma unroll
      for (int e = 0; e < RB; ++e)
        if (js[e] >= 0)
#pragma unroll
          for (int q = 0; q < MAX_Q; ++q) {
            gA[q] = gA[q] + va[e][q];
            gB[q] = gB[q] + vb[e][q];
          }
    }
  }
  float ssA = 0.f, ssB = 0.f;
#pragma unroll
  for (int q = 0; q < MAX_Q; ++q) {
    const int k = lane + 64 * q;
    if (k < d) {
      float* pA = a.G + a.off[tA] + (int64_t)r * d + k;
      float* pB = a.G + a.off[tB] + (int64_t)r * d + k;
      if (MG && MODE == 0) {
        st_wt(pA, oA[q] + gA[q]);
        st_wt(pB, oB[q] + gB[q]);
      } else {
        *pA = oA[q] + gA[q];
        *pB = oB[q] + gB[q];
      }
      ssA = ssA + gA[q] * gA[q];
      ssB = ssB + gB[q] * gB[q];
    }
  }
  if (!a.with_delta) return;
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    ssA += __shfl_xor(ssA, m, 64);
    ssB += __shfl_xor(ssB, m, 64);
  }
  const float invA = 1.0f / sqrtf(fmaxf(ssA, 1e-12f)), invB = 1.0f / sqrtf(fmaxf(ssB, 1e-12f));
  float* delta = const_cast<float*>(a.delta);
#pragma unroll
  for (int q = 0; q < MAX_Q; ++q) {
    const int k = lane + 64 * q;
    if (k < d) {
      float* dA = delta + ((int64_t)f * 4 + tA) * d + k;
      float* dB = delta + ((int64_t)f * 4 + tB) * d + k;
      if (MG) {
        st_wt(dA, gA[q] * invA * a.eps);
        st_wt(dB, gB[q] * invB * a.eps);
      } else {
        *dA = gA[q] * invA * a.eps;
        *dB = gB[q] * invB * a.eps;
      }
    }
  }
  if (MG && MODE == 0) {  // the row is out: publish it to the adversarial pass
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0)
      __hip_atomic_store(a.rdone + (s ? a.U1 : 0) + r, ((unsigned long long)(uint32_t)a.gen << 32) | (uint32_t)f,
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

#ifdef NMF_DIAG  // diagnostic build only: phase stamps (100 MHz) of workgroup 0, clean pass
__device__ uint64_t g_nmf_stamps[16];
__device__ uint64_t g_nmf_rstamps[8];  // k_nmf_rows, workgroup 0 wave 0 (owner of u[0]), clean pass
#define RSTAMP(i)                                                                          \
  do {                                                                                     \
    uint64_t t_;                                                                           \
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");         \
    if (with_delta && blockIdx.x == 0 && threadIdx.x == 0) g_nmf_rstamps[i] = t_;          \
  } while (0)
#define NSTAMP(i)                                                                          \
  do {                                                                                     \
    uint64_t t_;                                                                           \
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");         \
    if (MODE == 0 && blockIdx.x == 0 && threadIdx.x == 0) g_nmf_stamps[i] = t_;           \
  } while (0)
#else
#define NSTAMP(i) \
  do {            \
  } while (0)
#define RSTAMP(i) \
  do {            \
  } while (0)
#endif

// Row waves of a rows-in-line launch (k_nmf_inst workgroups past the instance
// workgroups): k_nmf_rows' wave per (instance, side) -- find the pair's first
// occurrence (the clean pass records it for the adversarial pass's delta
// gathers) -- then the row's owner counts the row's occurrences, waits until that
// many arrivals are in (no wave of the instance workgroups ever waits for a row
// wave, and they are dispatched first), re-arms the counter and sums the row
// (row_finish).
template <int MODE, bool MG>
__device__ __forceinline__ void row_wait_finish_one(const NArgs& a, const int32_t* s_idx, int b, int s) {
  const int lane = threadIdx.x & 63, B = a.B;
  const int32_t* L = s_idx + s * B;
  const int32_t r = L[b];
  int first = b;
  for (int base = 0; base <= b; base += 64) {
    const int j = base + lane;
    const uint64_t mask = __ballot(j <= b && L[j] == r);
    if (mask) {
      first = base + __ffsll((unsigned long long)mask) - 1;
      break;
    }
  }
  if (MODE == 0 && lane == 0) const_cast<int32_t*>(a.owner)[2 * b + s] = first;
  if (first != b) return;
  int cnt = 0;
  for (int base = b & ~63; base < B; base += 64) {
    const int j = base + lane;
    cnt += __popcll(__ballot(j < B && j >= b && L[j] == r));
  }
  int32_t* ctr = a.rcnt + (s ? a.U1 : 0) + r;
  // a give-up leaves the launch's results undefined (never its addresses: every
  // index is clamped) and its counters stale: the host resets them and, with the
  // failsafe on, replays the call on the row-sum path (acf_neumf_train / _grad)
  if (a.spin == 0 && lane == 0) atomicOr(a.err, 512);  // forced: every owner reports a give-up
  for (int it = 0; __hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < cnt;) {
    if (++it > a.spin) {
      if (lane == 0) atomicOr(a.err, 512);
      break;
    }
    __builtin_amdgcn_s_sleep(8);
  }
  if (lane == 0) __hip_atomic_store(ctr, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // every arrival is in
  // (a hot row's contributions 8 or 16 at a time measured the same as RBATCH:
  // profiles/r05/neumf_rows_in_line_ab.txt)
  row_finish<MODE, MG>(a, L, s, r, b);
}

// a row workgroup: the batch's indices into LDS, then its waves' pairs (strided
// over the row workgroups)
template <int MODE, bool MG>
__device__ __forceinline__ void row_wait_finish(const NArgs& a, unsigned fb, unsigned nrow, int32_t* s_idx) {
  const int tid = threadIdx.x, wave = tid >> 6, B = a.B;
  {
    int32_t su[FR_MAXB / 256], si[FR_MAXB / 256];
#pragma unroll
    for (int q = 0; q < FR_MAXB / 256; ++q) {
      const int x = tid + 256 * q;
      su[q] = x < B ? a.u[x] : 0;
      si[q] = x < B ? a.i[x] : 0;
    }
#pragma unroll
    for (int q = 0; q < FR_MAXB / 256; ++q) {
      const int x = tid + 256 * q;
      if (x < B) {
        s_idx[x] = clamp_idx(su[q], a.U1);
        s_idx[B + x] = clamp_idx(si[q], a.I1);
      }
    }
  }
  __syncthreads();
  for (int64_t item = (int64_t)fb * 4 + wave; item < 2 * (int64_t)B; item += 4 * (int64_t)nrow)
    row_wait_finish_one<MODE, MG>(a, s_idx, (int)(item >> 1), (int)(item & 1));
}

// One workgroup per slot, looping over blocks of MR instances (blk = blockIdx.x,
// + gridDim.x, ...): the MLP forward (and, MODE 0 / 1, the backward) of a block on
// MFMA with every operand in LDS, the row contributions to global scratch, and the
// block's weight gradients accumulated into the workgroup's slot of a.wpart
// (outer products on MFMA; bias / head / loss sums per owning thread).  MODE 2 is
// prediction only.  DC = compile-time d (0: a.d at run time).
// FR (rows in line, B <= FR_MAXB: one block per workgroup): no k_nmf_rows launch
// and no weight-gradient workgroups.  The block's weight-gradient tiles are taken
// from LDS by the workgroup itself; once the block's contributions are out
// (write-through) each (instance, side) counts its arrival at its row.  Workgroups
// past inst_blocks are the row waves (row_wait_finish, a wave per (instance,
// side) as in k_nmf_rows): the owner of a row waits for all its arrivals and sums
// the row.  Same sums in the same order: bit-identical to the k_nmf_rows path
// (test_neumf_rows_in_line_matches_rows_kernel).
// (instance workgroup bx of the pass; MG: the clean and adversarial passes share
// one launch, k_nmf_step)
template <int MODE, int DC, bool FR, bool MG>
__device__ __forceinline__ void inst_block(const NArgs& a, unsigned bx, unsigned inst_blocks, float* sm) {
  __shared__ int32_t s_own[MG && MODE == 1 ? 2 * MR : 1];  // the block's pairs' owners (first occurrences)
  NSTAMP(0);
  const int d = DC ? DC : a.d, d2 = 2 * d, tid = threadIdx.x;
  const int L2 = d2 + 1, L1 = d + 1;  // padded leading dimensions
  const int64_t nblk = ((int64_t)a.B + MR - 1) / MR;
  float* s_x = sm;                 // [MR][L2]  h0 = MLP_U[u] | MLP_I[i]
  float* s_a1 = s_x + MR * L2;     // [MR][L2]
  float* s_f = s_a1 + MR * L2;     // [MR][L2]  MF_U*MF_I | a2; later dz1
  float* s_mu = s_f + MR * L2;     // [MR][L1]
  float* s_mi = s_mu + MR * L1;    // [MR][L1]
  float* s_dz2 = s_mi + MR * L1;   // [MR][L1]
  float* s_dl = s_dz2 + MR * L1;   // [MR] d loss / d logit
  float* s_ls = s_dl + MR;         // [MR] per-instance loss
  float* s_vec = s_ls + MR;        // b1 [2d] | b2 [d] | Wo [2d] | bo (+3)
  float* s_b1 = s_vec, *s_b2 = s_vec + d2, *s_wo = s_b2 + d, *s_bo = s_wo + d2;
  float* s_w1 = s_bo + 4;          // [2d][2d+1] (weights_in_lds)
  float* s_w2 = s_w1 + d2 * L2;    // [2d][d+1]
  const bool wl = weights_in_lds(d);
  // Prologue, in issue order: the first block's indices (and owners), its row
  // gathers, the weights, biases and head (once per workgroup), and only then the
  // LDS stores -- the weights stream in behind the row gathers.
  // Row gathers of a block: one round trip for the indices (and owners), one for
  // every row element; no branch on the data (a bad index is clamped to row 0 and
  // flagged once at the end).
  constexpr int QG = MR * 128 / 256;  // gather elements per thread (d <= 128)
  // element x = tid + 256 q of the block's MR x d; with a compile-time d that is a
  // multiple of 16 the live q are known and the gathers need no branch
  auto live = [&](int q) { return (MR * d) % 256 == 0 ? q < MR * d / 256 : tid + 256 * q < MR * d; };
  float g[QG][4];
  int bad = 0;
  int32_t uu[QG], ii[QG], ou[QG], oi[QG];
  auto gather_idx = [&](int64_t blk) {
    const int64_t b0 = blk * MR;
    const int nt = (int)min((int64_t)MR, (int64_t)a.B - b0);
#pragma unroll
    for (int q = 0; q < QG; ++q) {
      const int x = tid + 256 * q, t = x / d;
      const int64_t b = b0 + ((x < MR * d && t < nt) ? t : 0);
      uu[q] = a.u[b];
      ii[q] = a.i[b];
      if (MODE == 1 && MG) {
        ou[q] = s_own[2 * (b - b0)];
        oi[q] = s_own[2 * (b - b0) + 1];
      } else if (MODE == 1) {
        ou[q] = a.owner[2 * b];
        oi[q] = a.owner[2 * b + 1];
      }
    }
  };
  auto gather_rows = [&](int64_t blk) {
    const int64_t b0 = blk * MR;
    const int nt = (int)min((int64_t)MR, (int64_t)a.B - b0);
#pragma unroll
    for (int q = 0; q < QG; ++q) {
      const int x = tid + 256 * q;
      if (live(q)) {
        const int t = x / d, k = x - t * d;
        const bool ok = t < nt;
        const bool ub = uu[q] < 0 || uu[q] >= a.U1, ib = ii[q] < 0 || ii[q] >= a.I1;
        bad |= (ok && ub ? 1 : 0) | (ok && ib ? 2 : 0);
        const int64_t ru = (int64_t)(ub ? 0 : uu[q]) * d + k, ri = (int64_t)(ib ? 0 : ii[q]) * d + k;
        float v0 = a.P[a.off[S_MF_U] + ru], v1_ = a.P[a.off[S_MF_I] + ri];
        float v2_ = a.P[a.off[S_MLP_U] + ru], v3 = a.P[a.off[S_MLP_I] + ri];
        if (MODE == 1) {
          const float* du = a.delta + (int64_t)ou[q] * 4 * d;
          const float* di = a.delta + (int64_t)oi[q] * 4 * d;
          if (MG) {  // stored in this launch (write-through)
            v0 = v0 + ld_dev(du + 0 * d + k);
            v1_ = v1_ + ld_dev(di + 1 * d + k);
            v2_ = v2_ + ld_dev(du + 2 * d + k);
            v3 = v3 + ld_dev(di + 3 * d + k);
          } else {
            v0 = v0 + du[0 * d + k];
            v1_ = v1_ + di[1 * d + k];
            v2_ = v2_ + du[2 * d + k];
            v3 = v3 + di[3 * d + k];
          }
        }
        g[q][0] = ok ? v0 : 0.f;
        g[q][1] = ok ? v1_ : 0.f;
        g[q][2] = ok ? v2_ : 0.f;
        g[q][3] = ok ? v3 : 0.f;
      }
    }
  };
  int64_t blk = bx;
  // FR: the row of the block's pair tid (instance tid >> 1; user, item), for its arrival
  int32_t prow = 0;
  if constexpr (FR) {
    const int64_t b = blk * MR + (tid >> 1);
    if (tid < 2 * MR && b < a.B) prow = (tid & 1) ? clamp_idx(a.i[b], a.I1) : clamp_idx(a.u[b], a.U1);
  }
  if (!(MG && MODE == 1) && blk < nblk) {
    gather_idx(blk);
    gather_rows(blk);
  }
  constexpr int Q1 = 64 * 64 * 4 / 4 / 256, Q2 = 64 * 64 * 2 / 4 / 256;  // weights_in_lds: d <= 64
  const int n1 = wl ? d2 * d2 / 4 : 0, n2 = wl ? d2 * d / 4 : 0;
  float4 v1[Q1], v2[Q2];
  {
    const float4* g1 = reinterpret_cast<const float4*>(a.P + a.off[S_W1]);
    const float4* g2 = reinterpret_cast<const float4*>(a.P + a.off[S_W2]);
#pragma unroll
    for (int q = 0; q < Q1; ++q) if (tid + 256 * q < n1) v1[q] = g1[tid + 256 * q];
#pragma unroll
    for (int q = 0; q < Q2; ++q) if (tid + 256 * q < n2) v2[q] = g2[tid + 256 * q];
  }
  const int nvec = 5 * d + 1;  // b1, b2, Wo, bo
  constexpr int QV = (5 * 128 + 1 + 255) / 256;  // d <= 128
  float vv[QV];
#pragma unroll
  for (int q = 0; q < QV; ++q) {
    const int x = tid + 256 * q;
    vv[q] = 0.f;
    if (x < nvec) {
      const int64_t src = x < d2 ? a.off[S_B1] + x
                                 : x < 3 * d ? a.off[S_B2] + (x - d2)
                                             : x < 5 * d ? a.off[S_WO] + (x - 3 * d) : a.off[S_BO];
      vv[q] = a.P[src];
    }
  }
#pragma unroll
  for (int q = 0; q < QV; ++q)
    if (tid + 256 * q < nvec) s_vec[tid + 256 * q] = vv[q];
#pragma unroll
  for (int q = 0; q < Q1; ++q) {
    const int x = tid + 256 * q;
    if (x < n1) {
      const int e = 4 * x, rr = e / d2, cc = e - rr * d2;
      float* dst = s_w1 + rr * L2 + cc;
      dst[0] = v1[q].x; dst[1] = v1[q].y; dst[2] = v1[q].z; dst[3] = v1[q].w;
    }
  }
#pragma unroll
  for (int q = 0; q < Q2; ++q) {
    const int x = tid + 256 * q;
    if (x < n2) {
      const int e = 4 * x, rr = e / d, cc = e - rr * d;
      float* dst = s_w2 + rr * L1 + cc;
      dst[0] = v2[q].x; dst[1] = v2[q].y; dst[2] = v2[q].z; dst[3] = v2[q].w;
    }
  }
  if constexpr (MG && MODE == 1) {
    // the adversarial pass beside the clean one: the block's rows wait for their
    // clean owners (delta and gradient stored, owner index in the flag), then gather
    if (tid < 2 * MR) {
      const int64_t b = blk * MR + (tid >> 1);
      int32_t own = 0;
      if (b < a.B) {
        unsigned long long* fl = a.rdone + ((tid & 1) ? a.U1 : 0) + prow;
        unsigned long long v = 0;
        for (int it = 0;; ++it) {
          v = __hip_atomic_load(fl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if ((int32_t)(v >> 32) == a.gen) break;
          if (it >= a.spin) {
            atomicOr(a.err, 512);
            break;
          }
          __builtin_amdgcn_s_sleep(4);
        }
        own = (int32_t)(v & 0xFFFFFFFFull);
      }
      s_own[tid] = own;
    }
    __syncthreads();
    if (blk < nblk) {
      gather_idx(blk);
      gather_rows(blk);
    }
  }
  NSTAMP(1);
  const float* W1 = wl ? s_w1 : a.P + a.off[S_W1];
  const float* W2 = wl ? s_w2 : a.P + a.off[S_W2];
  const int ld1 = wl ? L2 : d2, ld2 = wl ? L1 : d;
  const float* Wo = s_wo;
  const float* b1 = s_b1;
  const float* b2 = s_b2;
  const WOut wo_ = wout(d);
  float* slot = MODE == 2 ? nullptr : a.wpart + (int64_t)bx * wo_.n;
  // vector partials owned by threads across the workgroup's blocks
  float acc_wo = 0.f, acc_b1 = 0.f, acc_b2 = 0.f, acc_bo = 0.f, acc_ls = 0.f;
  for (; blk < nblk; blk += inst_blocks) {
    const int64_t b0 = blk * MR;
    const int nt = (int)min((int64_t)MR, (int64_t)a.B - b0);
#pragma unroll
    for (int q = 0; q < QG; ++q) {
      const int x = tid + 256 * q;
      if (live(q)) {
        const int t = x / d, k = x - t * d;
        const float mu = g[q][0], mi = g[q][1], lu = g[q][2], li = g[q][3];
        s_mu[t * L1 + k] = mu;
        s_mi[t * L1 + k] = mi;
        s_x[t * L2 + k] = lu;
        s_x[t * L2 + d + k] = li;
        s_f[t * L2 + k] = mu * mi;  // GMF tower
      }
    }
    __syncthreads();
    // the next block's rows fly while this one computes
    if (blk + inst_blocks < nblk) {
      gather_idx(blk + inst_blocks);
      gather_rows(blk + inst_blocks);
    }
    NSTAMP(2);
    // layer 1: a1 = relu(h0 W1 + b1)
    mfma_panel<false>(s_x, L2, W1, ld1, d2, d2, [&](int row, int col, float v) {
      const float z = v + b1[col];
      s_a1[row * L2 + col] = z > 0.f ? z : 0.f;
    });
    __syncthreads();
    NSTAMP(3);
    // layer 2: a2 = relu(a1 W2 + b2) -> f[d:2d]
    mfma_panel<false>(s_a1, L2, W2, ld2, d2, d, [&](int row, int col, float v) {
      const float z = v + b2[col];
      s_f[row * L2 + d + col] = z > 0.f ? z : 0.f;
    });
    __syncthreads();
    NSTAMP(4);
    // head: 16 lanes per instance, p = sigmoid(f Wo + bo); Keras BCE on clip(p)
    {
      const int row = tid >> 4, part = tid & 15;
      float sacc = 0.f;
      for (int k = part; k < d2; k += 16) sacc = sacc + s_f[row * L2 + k] * Wo[k];
#pragma unroll
      for (int m = 1; m < 16; m <<= 1) sacc += __shfl_xor(sacc, m, 64);
      if (part == 0) {
        const float logit = sacc + s_bo[0];
        const float p = 1.0f / (1.0f + expf(-logit));
        if (MODE == 2) {
          if (row < nt) a.pred[b0 + row] = p;
        } else {
          const float y = row < nt ? a.y[b0 + row] : 0.f;
          const bool inside = p >= 1e-7f && p <= 1.0f - 1e-7f;  // clip_by_value's gradient
          const float pc = fminf(fmaxf(p, 1e-7f), 1.0f - 1e-7f);
          s_dl[row] = (row < nt && inside) ? (p - y) * a.scale_over_B : 0.f;
          s_ls[row] = row < nt ? -(y * logf(pc) + (1.0f - y) * logf(1.0f - pc)) : 0.f;
        }
      }
    }
    __syncthreads();
    if (MODE == 2) continue;
    NSTAMP(5);
    // dz2 = (dl * Wo[d:2d]) * (a2 > 0); GMF row contributions dmf * MF_I / dmf * MF_U;
    // the head's weight gradients (f^T dl, sum dl) and the loss sum
    for (int x = tid; x < MR * d; x += 256) {
      const int t = x / d, k = x - t * d;
      const float dl = s_dl[t];
      const float dz = s_f[t * L2 + d + k] > 0.f ? dl * Wo[d + k] : 0.f;
      s_dz2[t * L1 + k] = dz;
      if (t < nt) {
        const float dmf = dl * Wo[k];
        float* cu = a.contrib + ((b0 + t) * 4 + S_MF_U) * d + k;
        float* ci = a.contrib + ((b0 + t) * 4 + S_MF_I) * d + k;
        if constexpr (FR) {
          st_wt(cu, dmf * s_mi[t * L1 + k]);
          st_wt(ci, dmf * s_mu[t * L1 + k]);
        } else {
          *cu = dmf * s_mi[t * L1 + k];
          *ci = dmf * s_mu[t * L1 + k];
        }
      }
    }
    if (tid < d2)
      for (int t = 0; t < nt; ++t) acc_wo = acc_wo + s_f[t * L2 + tid] * s_dl[t];
    if (tid == 0)
      for (int t = 0; t < nt; ++t) {
        acc_bo = acc_bo + s_dl[t];
        acc_ls = acc_ls + s_ls[t];
      }
    __syncthreads();
    NSTAMP(6);
    // dz1 = (dz2 W2^T) * (a1 > 0) -> s_f (f is spent)
    mfma_panel<true>(s_dz2, L1, W2, ld2, d, d2, [&](int row, int col, float v) {
      s_f[row * L2 + col] = s_a1[row * L2 + col] > 0.f ? v : 0.f;
    });
    __syncthreads();
    NSTAMP(7);
    // dh0 = dz1 W1^T -> MLP_U / MLP_I row contributions
    mfma_panel<true>(s_f, L2, W1, ld1, d2, d2, [&](int row, int col, float v) {
      if (row < nt) {
        const int tab = col < d ? S_MLP_U : S_MLP_I, kk = col < d ? col : col - d;
        float* cp = a.contrib + ((b0 + row) * 4 + tab) * d + kk;
        if constexpr (FR) st_wt(cp, v);
        else *cp = v;
      }
    });
    NSTAMP(8);
    if constexpr (FR) {
      if (tid < d2)
        for (int t = 0; t < nt; ++t) acc_b1 = acc_b1 + s_f[t * L2 + tid];
      if (tid < d)
        for (int t = 0; t < nt; ++t) acc_b2 = acc_b2 + s_dz2[t * L1 + tid];
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's contributions are out
      __syncthreads();
      if (tid < 2 * nt)  // arrival at the row (its owner's row wave waits for all of them)
        __hip_atomic_fetch_add(a.rcnt + ((tid & 1) ? a.U1 : 0) + prow, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (nt < MR) {  // a partial block: rows past the batch zero, as wgrad_group stages them
        for (int x = tid; x < (MR - nt) * L2; x += 256) {
          s_a1[nt * L2 + x] = 0.f;
          s_f[nt * L2 + x] = 0.f;
        }
        for (int x = tid; x < (MR - nt) * L1; x += 256) s_dz2[nt * L1 + x] = 0.f;
        __syncthreads();
      }
      // the block's weight gradients into the slot (wgrad_group's tiles, from LDS)
      if (d % 16 == 0) outer_tiles<false, true>(s_x, s_f, s_a1, s_dz2, d, slot + wo_.w1, slot + wo_.w2, 0, wtiles(d));
      else outer_tiles<false, false>(s_x, s_f, s_a1, s_dz2, d, slot + wo_.w1, slot + wo_.w2, 0, wtiles(d));
      continue;
    }
    // the weight gradients' operands -> k_nmf_rows' gradient workgroups (W1 += h0^T dz1,
    // W2 += a1^T dz2 on MFMA there, beside the row sums); b1 += sum dz1, b2 += sum dz2 here
    for (int x = tid; x < MR * d2; x += 256) {
      const int t = x / d2, k = x - t * d2;
      if (t < nt) {
        const int64_t g = (b0 + t) * d2 + k;
        a.h0[g] = s_x[t * L2 + k];
        a.a1[g] = s_a1[t * L2 + k];
        a.dz1[g] = s_f[t * L2 + k];
      }
    }
    for (int x = tid; x < MR * d; x += 256) {
      const int t = x / d, k = x - t * d;
      if (t < nt) a.dz2[(b0 + t) * d + k] = s_dz2[t * L1 + k];
    }
    if (tid < d2)
      for (int t = 0; t < nt; ++t) acc_b1 = acc_b1 + s_f[t * L2 + tid];
    if (tid < d)
      for (int t = 0; t < nt; ++t) acc_b2 = acc_b2 + s_dz2[t * L1 + tid];
    NSTAMP(9);
    __syncthreads();
    NSTAMP(10);
  }
  if (MODE != 2) {
    if (tid < d2) {
      slot[wo_.wo + tid] = acc_wo;
      slot[wo_.b1 + tid] = acc_b1;
    }
    if (tid < d) slot[wo_.b2 + tid] = acc_b2;
    if (tid == 0) {
      slot[wo_.bo] = acc_bo;
      slot[wo_.loss] = acc_ls;
    }
  }
  if (bad) atomicOr(a.err, bad);
}

template <int MODE, int DC, bool FR = false>
__global__ void __launch_bounds__(256) k_nmf_inst(NArgs a, NArgs wg, unsigned inst_blocks) {
  extern __shared__ float sm[];
  if (FR && blockIdx.x >= inst_blocks) {  // the pass's row waves
    row_wait_finish<MODE, false>(a, blockIdx.x - inst_blocks, gridDim.x - inst_blocks, reinterpret_cast<int32_t*>(sm));
    return;
  }
  if (blockIdx.x >= inst_blocks) {  // the previous pass's weight-gradient workgroups
    const int x = (int)(blockIdx.x - inst_blocks), ns = (int)inst_blocks;
    if (wg.d % 16 == 0) wgrad_group<true>(wg, x % ns, x / ns, ns, sm);
    else wgrad_group<false>(wg, x % ns, x / ns, ns, sm);
    return;
  }
  inst_block<MODE, DC, FR, false>(a, blockIdx.x, inst_blocks, sm);
}

// Both passes of an adversarial rows-in-line step in ONE launch, in dispatch
// order: the clean instance workgroups (a), the clean row waves, the adversarial
// instance workgroups (b: each waits for its rows' clean owners, rdone), the
// adversarial row waves.  Every wait is on workgroups earlier in the grid, and
// the first ones never wait.  Bit-identical to the two launches.  (r05: the
// adversarial instance workgroups second, staging their weights at once and
// then waiting, measured 3-5% slower: they hold CUs the clean row waves need.)
template <int DC>
__global__ void __launch_bounds__(256) k_nmf_step(NArgs a, NArgs b, unsigned gi, unsigned gr) {
  extern __shared__ float sm[];
  unsigned x = blockIdx.x;
  if (x < gi) return inst_block<0, DC, true, true>(a, x, gi, sm);
  x -= gi;
  if (x < gr) return row_wait_finish<0, true>(a, x, gr, reinterpret_cast<int32_t*>(sm));
  x -= gr;
  if (x < gi) return inst_block<1, DC, true, true>(b, x, gi, sm);
  x -= gi;
  row_wait_finish<1, true>(b, x, gr, reinterpret_cast<int32_t*>(sm));
}

// Weight gradients of the step: slot element x summed over the passes' slots
// (deterministic, no atomics): groups of SB consecutive slots summed in slot
// order, then the group sums in group order; G += clean sum, then += adversarial
// sum; the loss element gives the passes' mean losses.  acf_neumf_train does the
// same sums with a lane per group (k_nmf_adam_next), so train == grad + adam bit
// for bit.
constexpr int SB = 8;

__device__ __forceinline__ float slot_sum(const float* part, int p, int nslot, int64_t nout, int64_t x) {
  float acc = 0.f;
  const float* q = part + (int64_t)p * nslot * nout + x;
  for (int s0 = 0; s0 < nslot; s0 += SB) {
    float v[SB];
#pragma unroll
    for (int j = 0; j < SB; ++j) v[j] = s0 + j < nslot ? q[(int64_t)(s0 + j) * nout] : 0.f;
    float gs = 0.f;
#pragma unroll
    for (int j = 0; j < SB; ++j)
      if (s0 + j < nslot) gs = gs + v[j];
    acc = acc + gs;
  }
  return acc;
}

// group gi's sum of four consecutive elements (x a multiple of 4, nout a multiple of 4)
__device__ __forceinline__ float4 slot_group4(const float* part, int p, int nslot, int64_t nout, int64_t x, int gi) {
  const float4* q = reinterpret_cast<const float4*>(part + (int64_t)p * nslot * nout + x);
  const int64_t st = nout / 4;
  const int s0 = gi * SB;
  float4 v[SB];
#pragma unroll
  for (int j = 0; j < SB; ++j) v[j] = s0 + j < nslot ? q[(s0 + j) * st] : make_float4(0.f, 0.f, 0.f, 0.f);
  float4 gs = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int j = 0; j < SB; ++j)
    if (s0 + j < nslot) {
      gs.x = gs.x + v[j].x;
      gs.y = gs.y + v[j].y;
      gs.z = gs.z + v[j].z;
      gs.w = gs.w + v[j].w;
    }
  return gs;
}

__device__ __forceinline__ float4 slot_sum4(const float* part, int p, int nslot, int64_t nout, int64_t x) {
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int gi = 0; gi * SB < nslot; ++gi) {
    const float4 gs = slot_group4(part, p, nslot, nout, x, gi);
    acc.x = acc.x + gs.x;
    acc.y = acc.y + gs.y;
    acc.z = acc.z + gs.z;
    acc.w = acc.w + gs.w;
  }
  return acc;
}

__device__ __forceinline__ void wsum_one(const NArgs& a, int64_t x, int nslot, int npass, const float* part,
                                         float* loss_out) {
  const WOut o = wout(a.d);
  if (x > o.loss) return;
  const float acc0 = slot_sum(part, 0, nslot, o.n, x);
  const float acc1 = npass > 1 ? slot_sum(part, 1, nslot, o.n, x) : 0.f;
  if (x == o.loss) {
    if (loss_out) {
      loss_out[0] = acc0 / (float)a.B;
      loss_out[1] = npass > 1 ? acc1 / (float)a.B : 0.f;
    }
    return;
  }
  float* dst = a.G + a.off[S_W1] + x;
  float v = *dst + acc0;
  if (npass > 1) v = v + acc1;
  *dst = v;
}

// acf_neumf_grad: the passes' slots summed into G (acf_neumf_train does it on the Adam stream)
__global__ void __launch_bounds__(256) k_nmf_wsum(NArgs a, int nslot, int npass, const float* __restrict__ part,
                                                  float* loss_out) {
  wsum_one(a, blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nslot, npass, part, loss_out);
}

constexpr int RCH = 2048;  // batch indices staged in LDS per round

// One wave per (instance b, side s): s = 0 the user's MF_U / MLP_U rows, s = 1
// the item's MF_I / MLP_I rows.  The first occurrence of the row in the batch
// owns it: sums all its occurrences' contributions in instance order, adds the
// sum to the gradient rows and (with_delta) writes delta = eps*g/|g| per table.
// The workgroup stages the batch's indices in LDS (rounds of RCH); an owner's
// occurrences are loaded RBATCH at a time and added in order.  Workgroups past
// the rows' (blockIdx.x >= rows_blocks) are the pass's weight-gradient
// workgroups (wgrad_group; nslot slots x tile groups): latency-bound row sums
// leave the CUs free for their MFMA tiles.
__global__ void __launch_bounds__(256) k_nmf_rows(NArgs a, int32_t* __restrict__ owner,
                                                  float* __restrict__ delta, int with_delta, float eps,
                                                  unsigned rows_blocks, int nslot) {
  extern __shared__ float sm_w[];
  if (blockIdx.x >= rows_blocks) {
    const int x = (int)(blockIdx.x - rows_blocks);
    if (a.d % 16 == 0) wgrad_group<true>(a, x % nslot, x / nslot, nslot, sm_w);
    else wgrad_group<false>(a, x % nslot, x / nslot, nslot, sm_w);
    return;
  }
  __shared__ int32_t s_idx[2][RCH];
  RSTAMP(0);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int B = a.B, d = a.d;
  const int64_t item = (int64_t)blockIdx.x * 4 + wave;
  const bool live = item < 2 * (int64_t)B;
  const int b = live ? (int)(item >> 1) : 0, s = (int)(item & 1);
  const int64_t nrows = s ? a.I1 : a.U1;
  const int32_t r = clamp_idx((s ? a.i : a.u)[b], nrows);
  const int tA = s ? S_MF_I : S_MF_U, tB = s ? S_MLP_I : S_MLP_U;
  int first = -1;
  float gA[MAX_Q], gB[MAX_Q], oA[MAX_Q], oB[MAX_Q];
  // the row's gradient, fetched now (used if this wave owns the row)
#pragma unroll
  for (int q = 0; q < MAX_Q; ++q) {
    const int k = lane + 64 * q;
    gA[q] = gB[q] = 0.f;
    oA[q] = live && k < d ? a.G[a.off[tA] + (int64_t)r * d + k] : 0.f;
    oB[q] = live && k < d ? a.G[a.off[tB] + (int64_t)r * d + k] : 0.f;
  }
  for (int c0 = 0; c0 < B; c0 += RCH) {
    const int n = min(RCH, B - c0);
    if (c0 > 0) __syncthreads();
    int32_t su[RCH / 256], si[RCH / 256];
#pragma unroll
    for (int q = 0; q < RCH / 256; ++q) {
      const int x = threadIdx.x + 256 * q;
      su[q] = x < n ? a.u[c0 + x] : 0;
      si[q] = x < n ? a.i[c0 + x] : 0;
    }
#pragma unroll
    for (int q = 0; q < RCH / 256; ++q) {
      const int x = threadIdx.x + 256 * q;
      if (x < n) {
        s_idx[0][x] = clamp_idx(su[q], a.U1);
        s_idx[1][x] = clamp_idx(si[q], a.I1);
      }
    }
    __syncthreads();
    RSTAMP(1);
    if (!live) continue;
    const int32_t* L = s_idx[s];
    if (first < 0) {  // the first occurrence (b itself at the latest)
      for (int base = 0; base < n && c0 + base <= b; base += 64) {
        const int j = base + lane;
        const uint64_t mask = __ballot(j < n && c0 + j <= b && L[j] == r);
        if (mask) {
          first = c0 + base + __ffsll((unsigned long long)mask) - 1;
          break;
        }
      }
    }
    RSTAMP(2);
    if (first != b) continue;
    for (int base = max(b - c0, 0) & ~63; base < n; base += 64) {
      const int j = base + lane;
      uint64_t mask = __ballot(j < n && c0 + j >= b && L[j] == r);
      while (mask) {
        int js[RBATCH];
#pragma unroll
        for (int e = 0; e < RBATCH; ++e) {
          js[e] = -1;
          if (mask) {
            js[e] = c0 + base + __ffsll((unsigned long long)mask) - 1;
            mask &= mask - 1;
          }
        }
        float va[RBATCH][MAX_Q], vb[RBATCH][MAX_Q];
#pragma unroll
        for (int e = 0; e < RBATCH; ++e)
#pragma unroll
          for (int q = 0; q < MAX_Q; ++q) {
            const int k = lane + 64 * q;
            const bool ok = js[e] >= 0 && k < d;
            va[e][q] = ok ? a.contrib[((int64_t)js[e] * 4 + tA) * d + k] : 0.f;
            vb[e][q] = ok ? a.contrib[((int64_t)js[e] * 4 + tB) * d + k] : 0.f;
          }
#pragma unroll
        for (int e = 0; e < RBATCH; ++e)
          if (js[e] >= 0)
#pragma unroll
            for (int q = 0; q < MAX_Q; ++q) {
              gA[q] = gA[q] + va[e][q];
              gB[q] = gB[q] + vb[e][q];
            }
      }
    }
  }
  RSTAMP(3);
  if (!live) return;
  if (lane == 0) owner[2 * b + s] = first;
  if (first != b) return;
  float ssA = 0.f, ssB = 0.f;
#pragma unroll
  for (int q = 0; q < MAX_Q; ++q) {
    const int k = lane + 64 * q;
    if (k < d) {
      a.G[a.off[tA] + (int64_t)r * d + k] = oA[q] + gA[q];
      a.G[a.off[tB] + (int64_t)r * d + k] = oB[q] + gB[q];
      ssA = ssA + gA[q] * gA[q];
      ssB = ssB + gB[q] * gB[q];
    }
  }
  RSTAMP(4);
  if (!with_delta) return;
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    ssA += __shfl_xor(ssA, m, 64);
    ssB += __shfl_xor(ssB, m, 64);
  }
  const float invA = 1.0f / sqrtf(fmaxf(ssA, 1e-12f)), invB = 1.0f / sqrtf(fmaxf(ssB, 1e-12f));
#pragma unroll
  for (int q = 0; q < MAX_Q; ++q) {
    const int k = lane + 64 * q;
    if (k < d) {
      delta[((int64_t)b * 4 + tA) * d + k] = gA[q] * invA * eps;
      delta[((int64_t)b * 4 + tB) * d + k] = gB[q] * invB * eps;
    }
  }
  RSTAMP(5);
}
