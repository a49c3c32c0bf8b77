// The Adam kernels of libacf_neumf.so: the dense stream (k_nmf_adam) and
// acf_neumf_train's lazy form of it (k_nmf_adam_next, k_nmf_adam_catchup), with
// k_nmf_fill_i32: included by acf_neumf.hip after acf_neumf_step.h (SB, NSLOT,
// slot_sum4, slot_group4); one translation unit.  DESIGN.md §9.
//
//   k_nmf_adam          Keras 2.2 Adam over the WHOLE flat parameter buffer
//                       (Keras densifies the embedding IndexedSlices, so every
//                       row's moments decay and every row moves): one HBM
//                       stream of p, g, m, v, zeroing g behind it.
// acf_neumf_train runs that Adam lazily (k_nmf_adam_next, k_nmf_adam_catchup; the
// comment above LAZY_S), so a step moves the rows it touches, not the whole tables.
#pragma once

// NeuMF's weight-gradient slots handed to k_nmf_adam (acf_neumf_train): the
// float4s from base4 on get the slot sums of k_nmf_inst (wsum_one's arithmetic)
// added to their gradient first; the loss element goes to loss_out.
struct AdamSlots {
  const float* part = nullptr;  // nullptr: plain Adam
  int nslot = 0, npass = 0;
  int64_t base4 = 0, nout = 0;  // first float4 of the slot range; slot length (floats)
  float* loss_out = nullptr;
  float B = 1.f;  // the batch, for the mean losses
};

// Keras 2.2 Adam (keras/optimizers.py Adam.get_updates) of float4 x:
// m = b1*m + (1-b1)*g; v = b2*v + (1-b2)*g^2; p -= lr_t*m / (sqrt(v) + eps); g = 0.
// With slots (ws.part) the float4s from base4 on first get the slot sums of
// k_nmf_inst added to their gradient (wsum_one's arithmetic); the loss element
// goes to loss_out.
struct AdamK {
  float b1, b2, lr_t, eps;
};

// the float4's operands, loaded together (a wave issues them before its slot
// sums or its row claim resolve)
struct Adam4V {
  float4 g, m, v, p;
};

__device__ __forceinline__ Adam4V adam4_load(const float4* p, const float4* g, const float4* m, const float4* v,
                                             int64_t x) {
  return Adam4V{g[x], m[x], v[x], p[x]};
}

// the slot sums s4[pass] of float4 x (x >= ws.base4) added to its gradient; the loss element
__device__ __forceinline__ void adam4_fold(float4& gg, int64_t x, const AdamSlots& ws, const float4* s4) {
  const int64_t e0 = 4 * (x - ws.base4);
  const int64_t loss_x = ws.nout - 3;
  const float sum[2][4] = {{s4[0].x, s4[0].y, s4[0].z, s4[0].w}, {s4[1].x, s4[1].y, s4[1].z, s4[1].w}};
  float* gc = &gg.x;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    if (e0 + c < loss_x) {
      float t = gc[c] + sum[0][c];
      if (ws.npass > 1) t = t + sum[1][c];
      gc[c] = t;
    } else if (e0 + c == loss_x && ws.loss_out) {
      ws.loss_out[0] = sum[0][c] / ws.B;
      ws.loss_out[1] = ws.npass > 1 ? sum[1][c] / ws.B : 0.f;
    }
  }
}

// one Adam iteration of the float4 with learning rate lr_t (every path's arithmetic)
__device__ __forceinline__ void adam_math(Adam4V& a, const AdamK& k, float lr_t) {
  const float c1 = 1.0f - k.b1, c2 = 1.0f - k.b2;
#define ACF_ADAM(c)                                          \
  a.m.c = k.b1 * a.m.c + c1 * a.g.c;                         \
  a.v.c = k.b2 * a.v.c + c2 * (a.g.c * a.g.c);               \
  a.p.c = a.p.c - (lr_t * a.m.c) / (sqrtf(a.v.c) + k.eps);
  ACF_ADAM(x) ACF_ADAM(y) ACF_ADAM(z) ACF_ADAM(w)
#undef ACF_ADAM
}

__device__ __forceinline__ void adam4_store(float4* p, float4* g, float4* m, float4* v, int64_t x, const AdamK& k,
                                            Adam4V a) {
  adam_math(a, k, k.lr_t);
  m[x] = a.m;
  v[x] = a.v;
  p[x] = a.p;
  g[x] = make_float4(0.f, 0.f, 0.f, 0.f);
}

__device__ __forceinline__ void adam4(float4* __restrict__ p, float4* __restrict__ g, float4* __restrict__ m,
                                      float4* __restrict__ v, int64_t x, const AdamK& k, const AdamSlots& ws) {
  Adam4V a = adam4_load(p, g, m, v, x);
  if (ws.part && x >= ws.base4) {
    const int64_t e0 = 4 * (x - ws.base4);
    float4 s4[2];
    s4[0] = slot_sum4(ws.part, 0, ws.nslot, ws.nout, e0);
    s4[1] = ws.npass > 1 ? slot_sum4(ws.part, 1, ws.nslot, ws.nout, e0) : make_float4(0.f, 0.f, 0.f, 0.f);
    adam4_fold(a.g, x, ws, s4);
  }
  adam4_store(p, g, m, v, x, k, a);
}

// dense, float4 stream; with slots the stream runs from the top down: the slot
// range (the buffer's tail) is summed in the first sweep, under the rest of it
__global__ void __launch_bounds__(256) k_nmf_adam(float4* __restrict__ p, float4* __restrict__ g,
                                                  float4* __restrict__ m, float4* __restrict__ v,
                                                  int64_t n4, float b1, float b2, float lr_t,
                                                  float eps, AdamSlots ws = AdamSlots()) {
  const AdamK k{b1, b2, lr_t, eps};
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4;
       i += (int64_t)gridDim.x * blockDim.x)
    adam4(p, g, m, v, ws.part ? n4 - 1 - i : i, k, ws);
}

// acf_neumf_train runs Keras's dense Adam lazily with the same per-element
// arithmetic, so train == grad + adam bit for bit.  Each row holds in G the
// gradient of at most one pending iteration pend[r] (the step that gathered it);
// at every other iteration its gradient is 0, and such an iteration (m = b1 m,
// v = b2 v, p -= lr_t m / (sqrt(v) + eps)) depends on (p, m, v) and lr_t only.
// So a row's iterations can run later, in order, all at once, as long as that
// happens before anything reads the row or adds to its G:
//  k_nmf_adam_next    (caller's stream, after step k's gradients: iteration t)
//                     the rows of batch k+1, which step k+1 gathers and adds
//                     gradients to: a wave per (instance, side) claims its user /
//                     item row (atomicExch of the row's last iteration: the first
//                     claimer runs it) and runs the row's iterations up to t in
//                     both of its tables (MF_x, MLP_x), the pending one with G;
//                     pend = t + 1.  And the parameter tail (MLP / head) with the
//                     slot sums and the losses, every iteration;
//  k_nmf_adam_catchup (side stream, beside step k+1's kernels) slice k % LAZY_S
//                     of the rows brought to iteration t, so no row is more than
//                     LAZY_S iterations behind; after the call's last step, every
//                     row (caller's stream).
// catch-up period (acf_neumf_ctx::lazy_s = LAZY_S):
// a row is at most lazy_s iterations behind; a step's slice is 1/lazy_s of the
// rows, so a longer period is a smaller slice beside each step.  8 measured best
// beside the one-launch step (profiles/r05/neumf_catchup_wg_ab.txt; DESIGN.md §9,
// knob table)
constexpr int LAZY_S = 8;
constexpr int LAZY_W = 32;  // lr_t window (> the catch-up period)
// workgroups of a step's catch-up slice, beside the step's kernels: too few and
// the slice outlasts the step, and above 512 nothing more is gained
// (profiles/r05/neumf_catchup_wg_ab.txt; DESIGN.md §9, knob table)
constexpr int64_t CATCHUP_WG = 512;
static_assert(LAZY_W > LAZY_S, "lr window");

struct AdamLazy {
  int64_t U1, I1, d4;
  int32_t* last_u;   // [U1] the last Adam iteration the user's rows have taken
  int32_t* last_i;   // [I1]
  int32_t* pend_u;   // [U1] the iteration whose gradient G holds for the user's rows (<= last: none)
  int32_t* pend_i;   // [I1]
  int32_t* err;      // bit 8: a row more than LAZY_W - 1 iterations behind (never, by construction)
  int32_t t;         // this step's Adam iteration
  float lr[LAZY_W];  // lr[x] = lr_t of iteration t - (LAZY_W - 1) + x

  // the row's float4 q (q < d4: MF table, else MLP table)
  __device__ int64_t at(int side, int64_t r, int64_t q) const {
    if (q < d4) return side ? U1 * d4 + r * d4 + q : r * d4 + q;                            // S_MF_U / S_MF_I
    return side ? (2 * U1 + I1) * d4 + r * d4 + (q - d4) : (U1 + I1) * d4 + r * d4 + (q - d4);  // S_MLP_x
  }
};

// iterations (from, t] of a float4 (from >= t - LAZY_W), a.g the gradient of
// iteration gp, 0 at the others; unrolled so that every lr[x] is a kernel-argument load
__device__ __forceinline__ void lazy_iters(Adam4V& a, const AdamK& k, const AdamLazy& z, int32_t from,
                                           int32_t gp) {
  const float4 g = a.g;
#pragma unroll
  for (int x = 0; x < LAZY_W; ++x) {
    const int32_t tau = z.t - (LAZY_W - 1) + x;
    if (tau > from) {
      a.g = tau == gp ? g : make_float4(0.f, 0.f, 0.f, 0.f);
      adam_math(a, k, z.lr[x]);
    }
  }
}

__global__ void __launch_bounds__(256) k_nmf_adam_next(float4* __restrict__ p, float4* __restrict__ g,
                                                       float4* __restrict__ m, float4* __restrict__ v,
                                                       int64_t n4, int64_t emb4, AdamK k, AdamSlots ws,
                                                       AdamLazy z, const int32_t* __restrict__ un,
                                                       const int32_t* __restrict__ in, int32_t Bn,
                                                       unsigned row_blocks) {
  if (blockIdx.x >= row_blocks) {
    // the parameter tail: a lane per (float4, pass, slot group), 64 / (2 gp) float4s
    // per wave (gp = slot groups rounded up to a power of two)
    const int64_t t4 = n4 - emb4;
    const int lane = threadIdx.x & 63;
    const int ng = (ws.nslot + SB - 1) / SB;  // <= 32 (nslot <= NSLOT)
    int gp = 1;
    while (gp < ng) gp <<= 1;
    const int fpw = 32 / gp;  // float4s per wave
    const int f = lane / (2 * gp), pass = (lane / gp) & 1, gi = lane & (gp - 1);
    const int lead = f * 2 * gp;  // the float4's pass-0 leader; pass 1's is lead + gp
    const int64_t w0 = ((blockIdx.x - row_blocks) * (int64_t)blockDim.x + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)(gridDim.x - row_blocks) * blockDim.x) >> 6;
    for (int64_t i0 = w0 * fpw; i0 < t4; i0 += nw * fpw) {
      const int64_t i = i0 + f;
      const int64_t x = emb4 + i;
      const bool live = i < t4;
      Adam4V a{};
      if (live && lane == lead) a = adam4_load(p, g, m, v, x);
      float4 gs = make_float4(0.f, 0.f, 0.f, 0.f);
      if (live && gi < ng && pass < ws.npass) gs = slot_group4(ws.part, pass, ws.nslot, ws.nout, 4 * i, gi);
      // the group sums in group order (slot_sum4's arithmetic), by the pass leaders
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int j = 0; j < ng; ++j) {
        const int src = (lane & ~(gp - 1)) + j;
        acc.x = acc.x + __shfl(gs.x, src, 64);
        acc.y = acc.y + __shfl(gs.y, src, 64);
        acc.z = acc.z + __shfl(gs.z, src, 64);
        acc.w = acc.w + __shfl(gs.w, src, 64);
      }
      float4 sums[2];
      sums[0] = acc;
      sums[1] = make_float4(__shfl(acc.x, lead + gp, 64), __shfl(acc.y, lead + gp, 64),
                            __shfl(acc.z, lead + gp, 64), __shfl(acc.w, lead + gp, 64));
      if (ws.npass < 2) sums[1] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (live && lane == lead) {
        adam4_fold(a.g, x, ws, sums);
        adam4_store(p, g, m, v, x, k, a);
      }
    }
    return;
  }
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (wave >= 2 * (int64_t)Bn) return;
  const int b = (int)(wave >> 1), side = (int)(wave & 1);
  const int64_t nrows = side ? z.I1 : z.U1;
  int32_t r = side ? in[b] : un[b];
  if (r < 0 || r >= nrows) r = 0;  // the step flags bad indices; row 0 stays a valid address
  int32_t* lst = (side ? z.last_i : z.last_u) + r;
  int32_t* pnd = (side ? z.pend_i : z.pend_u) + r;
  int32_t old = 0;
  if (lane == 0) old = atomicExch(lst, z.t);
  const int32_t gp = *pnd;
  // the row's float4s, loaded beside the claim: nothing else writes the row
  // before the claimer's stores
  const int64_t d4 = z.d4;
  for (int64_t q = lane; q < 2 * d4; q += 64) {
    const int64_t x = z.at(side, r, q);
    Adam4V a = adam4_load(p, g, m, v, x);
    const int32_t from = __shfl(old, 0, 64);
    if (from == z.t) return;  // another occurrence claimed the row
    if (z.t - from > LAZY_W) {
      if (lane == 0) atomicOr(z.err, 256);
      return;
    }
    lazy_iters(a, k, z, from, gp);
    m[x] = a.m;
    v[x] = a.v;
    p[x] = a.p;
    g[x] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (lane == 0) *pnd = z.t + 1;  // step k+1's gradient
}

// rows [lo, hi) of the (users, then items) row space brought to iteration t; a
// lane-group of 32 (2 d4 <= 32) or 64 lanes per row, CR rows per lane-group in
// flight (2: 103 VGPRs and no faster beside the step)
constexpr int CR = 1;

__global__ void __launch_bounds__(256) k_nmf_adam_catchup(float4* __restrict__ p, float4* __restrict__ g,
                                                          float4* __restrict__ m, float4* __restrict__ v,
                                                          AdamK k, AdamLazy z, int64_t lo, int64_t hi) {
  const int64_t d4 = z.d4;
  const int lpr = 2 * d4 <= 32 ? 32 : 64;
  const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t groups = (int64_t)gridDim.x * blockDim.x / lpr;
  const int l = (int)(threadIdx.x & (lpr - 1));
  for (int64_t r0 = lo + gid / lpr; r0 < hi; r0 += CR * groups) {
    int32_t from[CR], gp[CR];
    int64_t rr[CR];
#pragma unroll
    for (int j = 0; j < CR; ++j) {
      rr[j] = r0 + j * groups;
      from[j] = z.t;
      gp[j] = 0;
      if (rr[j] < hi) {
        const int side = rr[j] >= z.U1 ? 1 : 0;
        const int64_t r = side ? rr[j] - z.U1 : rr[j];
        from[j] = (side ? z.last_i : z.last_u)[r];
        gp[j] = (side ? z.pend_i : z.pend_u)[r];
      }
    }
    for (int64_t q = l; q < 2 * d4; q += lpr) {
      Adam4V a[CR];
      int64_t x[CR];
#pragma unroll
      for (int j = 0; j < CR; ++j) {  // all loads first
        if (from[j] >= z.t || z.t - from[j] > LAZY_W) continue;  // claimed at t / (never) too far behind
        const int side = rr[j] >= z.U1 ? 1 : 0;
        x[j] = z.at(side, side ? rr[j] - z.U1 : rr[j], q);
        const bool wg = gp[j] > from[j] && gp[j] <= z.t;  // G holds a gradient of the range
        a[j] = Adam4V{wg ? g[x[j]] : make_float4(0.f, 0.f, 0.f, 0.f), m[x[j]], v[x[j]], p[x[j]]};
      }
#pragma unroll
      for (int j = 0; j < CR; ++j) {
        if (from[j] >= z.t || z.t - from[j] > LAZY_W) continue;
        lazy_iters(a[j], k, z, from[j], gp[j]);
        m[x[j]] = a[j].m;
        v[x[j]] = a[j].v;
        p[x[j]] = a[j].p;
        if (gp[j] > from[j] && gp[j] <= z.t) g[x[j]] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    if (l == 0) {
#pragma unroll
      for (int j = 0; j < CR; ++j) {
        if (from[j] >= z.t) continue;
        if (z.t - from[j] > LAZY_W) {
          atomicOr(z.err, 256);
          continue;
        }
        const int side = rr[j] >= z.U1 ? 1 : 0;
        (side ? z.last_i : z.last_u)[side ? rr[j] - z.U1 : rr[j]] = z.t;  // read again only after this launch
      }
    }
  }
}

__global__ void k_nmf_fill_i32(int32_t* __restrict__ a, int64_t n, int32_t val) {
  const int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (x < n) a[x] = val;
}
