// acf_keras_mf.hip — MI355X (gfx950) kernels + C-ABI of the two flat-buffer
// dot-product engines of libacf_neumf.so (include/acf_neumf.h "Keras BPR" and
// "FastAdversarialMF"): acf_kbpr_*, the reference's Keras BPR (pairwise loss on
// u.p - u.n), and acf_amf_*, its FastAdversarialMF (u.i with MSE, plus two
// popularity discriminators on embedding rows).  Both keep parameters, gradient
// and Adam moments in one flat float32 buffer each that starts with [user table |
// item table], score a pair with k_kbpr_predict, sum a batch's row gradients per
// table row in occurrence order, and end every batch in the dense Keras Adam
// k_nmf_adam, which stays in acf_neumf.hip (acf_dense_adam, acf_neumf_adam.h).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <initializer_list>
#include <utility>
#include <vector>

#include "acf_apr.h"
#include "acf_neumf.h"
#include "acf_host.h"
#include "acf_neumf_adam.h"

// What both engines' contexts hold; each adds its own per-batch scratch.
struct FlatCtx {
  int64_t U1 = 0, I1 = 0;
  int32_t d = 0, maxB = 0;
  int32_t* err = nullptr;
  std::vector<void*> allocs;
};

template <class C>
static int flat_destroy(C* c) {
  if (!c) return ACF_OK;
  for (void* p : c->allocs) (void)hipFree(p);
  delete c;
  return ACF_OK;
}

// scratch: the context's float buffers and their floats per instance of a full batch
template <class C>
static int flat_create(C** out, int64_t U1, int64_t I1, int32_t d, int32_t maxB,
                       std::initializer_list<std::pair<float * C::*, size_t>> scratch) {
  ACF_CHECK(out != nullptr, ACF_E_INVALID, "out is NULL");
  *out = nullptr;
  ACF_CHECK(U1 > 0 && I1 > 0 && U1 < (1ll << 31) && I1 < (1ll << 31), ACF_E_INVALID, "bad table rows");
  ACF_CHECK(d >= 4 && d <= 256 && d % 4 == 0, ACF_E_INVALID, "dim must be a multiple of 4 in [4, 256], got %d", d);
  ACF_CHECK(maxB > 0 && maxB <= (1 << 24), ACF_E_INVALID, "max_batch must be in (0, 2^24], got %d", maxB);
  C* c = new C();
  c->U1 = U1; c->I1 = I1; c->d = d; c->maxB = maxB;
  auto alloc = [c](void** p, size_t bytes) -> int {
    if (hipMalloc(p, bytes) != hipSuccess) {
      (void)hipGetLastError();
      flat_destroy(c);
      return acf_set_error(ACF_E_NOMEM, "hipMalloc of %zu bytes failed", bytes);
    }
    c->allocs.push_back(*p);
    return ACF_OK;
  };
  for (const auto& b : scratch) ACF_RET(alloc((void**)&(c->*b.first), (size_t)maxB * b.second * sizeof(float)));
  ACF_RET(alloc((void**)&c->err, 16));
  if (hipMemset(c->err, 0, 16) != hipSuccess) {
    flat_destroy(c);
    return acf_set_error(ACF_E_HIP, "hipMemset failed");
  }
  *out = c;
  return ACF_OK;
}

// ---------------------------------------------------------------------------
// Keras BPR (BPR.py:23-99; run.py --model bpr, BASELINE configs[0]).
// params = [uEmb (U1 x d) | iEmb (I1 x d)] (BPR.py:35-36), gradient and Adam
// moments in the same layout.  Per batch of B triplets:
//   x = u.p - u.n (Dot layers, BPR.py:42-43); loss = 1 - log(sigmoid(x))
//   (bpr_triplet_loss, BPR.py:11-16); Keras loss = mean over the batch
//   (identity_loss, BPR.py:19-20), so d loss / d x = SigmoidGrad(LogGrad(-1/B)).
//   The gathered rows' gradients are summed per table row in occurrence order
//   (users: batch order; items: the positive gathers, then the negative ones:
//   TF's IndexedSlices densified), then Keras 2.2 Adam over the whole buffer.
// ---------------------------------------------------------------------------
template <int LPR>
__device__ __forceinline__ float kb_sum(float s) {
#pragma unroll
  for (int m = 1; m < LPR; m <<= 1) s += __shfl_xor(s, m, 64);
  return s;
}

// one lane-group of LPR lanes (one float4 each, d <= 4 LPR) per triplet
template <int LPR>
__global__ void __launch_bounds__(256) k_kbpr_inst(const float* __restrict__ P, const int32_t* __restrict__ u,
                                                   const int32_t* __restrict__ ip, const int32_t* __restrict__ in,
                                                   int32_t B, int32_t d, int64_t U1, int64_t I1,
                                                   float* __restrict__ contrib, float* __restrict__ loss,
                                                   int32_t* __restrict__ err) {
  const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int b = (int)(gid / LPR), l = (int)(threadIdx.x & (LPR - 1));
  if (b >= B) return;
  int32_t ru = u[b], rp = ip[b], rn = in[b];
  if (l == 0 && (ru < 0 || ru >= U1)) atomicOr(err, 1);
  if (l == 0 && (rp < 0 || rp >= I1 || rn < 0 || rn >= I1)) atomicOr(err, 2);
  ru = (ru < 0 || ru >= U1) ? 0 : ru;
  rp = (rp < 0 || rp >= I1) ? 0 : rp;
  rn = (rn < 0 || rn >= I1) ? 0 : rn;
  const float* Q = P + U1 * (int64_t)d;
  const bool on = l * 4 < d;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 pu = on ? *reinterpret_cast<const float4*>(P + (int64_t)ru * d + 4 * l) : z;
  const float4 pp = on ? *reinterpret_cast<const float4*>(Q + (int64_t)rp * d + 4 * l) : z;
  const float4 pn = on ? *reinterpret_cast<const float4*>(Q + (int64_t)rn * d + 4 * l) : z;
  const float dp = kb_sum<LPR>(pu.x * pp.x + pu.y * pp.y + pu.z * pp.z + pu.w * pp.w);
  const float dn = kb_sum<LPR>(pu.x * pn.x + pu.y * pn.y + pu.z * pn.z + pu.w * pn.w);
  const float x = dp - dn;
  const float sg = 1.0f / (1.0f + expf(-x));           // K.sigmoid
  if (l == 0) loss[b] = 1.0f - logf(sg);               // 1 - K.log(.)
  const float up = -1.0f / (float)B;                   // d mean / d loss_b, through "1 - ."
  const float g = (up * (1.0f / sg)) * sg * (1.0f - sg);  // LogGrad, then SigmoidGrad
  if (!on) return;
  float4 gu, gp, gn;
  gu.x = g * pp.x + (-g) * pn.x; gu.y = g * pp.y + (-g) * pn.y;
  gu.z = g * pp.z + (-g) * pn.z; gu.w = g * pp.w + (-g) * pn.w;
  gp = make_float4(g * pu.x, g * pu.y, g * pu.z, g * pu.w);
  gn = make_float4(-g * pu.x, -g * pu.y, -g * pu.z, -g * pu.w);
  float* c = contrib + (int64_t)b * 3 * d + 4 * l;
  *reinterpret_cast<float4*>(c) = gu;
  *reinterpret_cast<float4*>(c + d) = gp;
  *reinterpret_cast<float4*>(c + 2 * d) = gn;
}

// one wave per gathered row occurrence: occurrence o < B is user b = o, o >= B
// is item slot o - B of [positives | negatives].  The first occurrence of a
// table row owns it and adds every occurrence's contribution in order.
__global__ void __launch_bounds__(256) k_kbpr_rows(const int32_t* __restrict__ u, const int32_t* __restrict__ ip,
                                                   const int32_t* __restrict__ in, int32_t B, int32_t d,
                                                   int64_t U1, int64_t I1, const float* __restrict__ contrib,
                                                   float* __restrict__ G) {
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (wave >= 3 * (int64_t)B) return;
  const int o = (int)wave;
  const bool item = o >= B;
  const int n = item ? 2 * B : B;  // occurrences of this table
  auto row_of = [&](int k) -> int32_t {  // table row of occurrence k of this table
    int32_t r = item ? (k < B ? ip[k] : in[k - B]) : u[k];
    const int64_t rows = item ? I1 : U1;
    return (r < 0 || r >= rows) ? 0 : r;
  };
  auto contrib_of = [&](int k) -> const float* {  // its gradient row
    return item ? contrib + ((int64_t)(k < B ? k : k - B) * 3 + (k < B ? 1 : 2)) * d
                : contrib + (int64_t)k * 3 * d;
  };
  const int me = item ? o - B : o;
  const int32_t r = row_of(me);
  for (int base = 0; base < me; base += 64) {  // an earlier occurrence owns the row
    const int k = base + lane;
    if (__any(k < me && row_of(k) == r)) return;
  }
  float acc[4] = {0.f, 0.f, 0.f, 0.f};  // d <= 256: lane holds elements lane + 64 q
  for (int base = me; base < n; base += 64) {
    const int k = base + lane;
    uint64_t mask = __ballot(k < n && row_of(k) == r);
    while (mask) {
      const int kk = base + __ffsll((unsigned long long)mask) - 1;
      mask &= mask - 1;
      const float* c = contrib_of(kk);
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (lane + 64 * q < d) acc[q] = acc[q] + c[lane + 64 * q];
    }
  }
  float* g = G + (item ? U1 * (int64_t)d : 0) + (int64_t)r * d;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (lane + 64 * q < d) g[lane + 64 * q] = g[lane + 64 * q] + acc[q];
}

struct acf_kbpr_ctx : FlatCtx {
  float* contrib = nullptr;
};

extern "C" int acf_kbpr_destroy(acf_kbpr_ctx* c) { return flat_destroy(c); }

extern "C" int acf_kbpr_create(acf_kbpr_ctx** out, int64_t U1, int64_t I1, int32_t d, int32_t maxB) {
  return flat_create(out, U1, I1, d, maxB, {{&acf_kbpr_ctx::contrib, (size_t)3 * d}});
}

template <int LPR>
static void launch_kbpr_inst(const acf_kbpr_ctx* c, const float* P, const int32_t* u, const int32_t* ip,
                             const int32_t* in, int32_t B, float* loss, hipStream_t s) {
  k_kbpr_inst<LPR><<<(unsigned)(((int64_t)B * LPR + 255) / 256), 256, 0, s>>>(P, u, ip, in, B, c->d, c->U1,
                                                                              c->I1, c->contrib, loss, c->err);
}

extern "C" int acf_kbpr_train(acf_kbpr_ctx* c, float* P, float* G, float* m, float* v, const int32_t* u,
                              const int32_t* ip, const int32_t* in, int64_t n, int32_t batch, int64_t t_first,
                              const acf_neumf_hparams* hp, float* losses, void* stream_) {
  ACF_CHECK(c && P && G && m && v && u && ip && in && hp && losses, ACF_E_INVALID, "NULL argument");
  ACF_CHECK(batch > 0 && batch <= c->maxB, ACF_E_INVALID, "batch %d outside (0, %d]", batch, c->maxB);
  ACF_CHECK(n >= 0 && t_first >= 1, ACF_E_INVALID, "bad triplet count or Adam iteration");
  hipStream_t s = static_cast<hipStream_t>(stream_);
  HIP_TRY(hipMemsetAsync(c->err, 0, sizeof(int32_t), s));
  const int64_t n4 = (c->U1 + c->I1) * (int64_t)c->d / 4;
  int64_t k = 0;
  for (int64_t o = 0; o < n; o += batch, ++k) {
    const int32_t B = (int32_t)std::min<int64_t>(batch, n - o);
    ACF_RET(DISPATCH_LPR(c->d, launch_kbpr_inst, c, P, u + o, ip + o, in + o, B, losses + o, s));
    k_kbpr_rows<<<(unsigned)((3 * (int64_t)B * 64 + 255) / 256), 256, 0, s>>>(u + o, ip + o, in + o, B, c->d,
                                                                             c->U1, c->I1, c->contrib, G);
    ACF_RET(acf_dense_adam(P, G, m, v, n4, t_first + k, hp, s));
  }
  return read_range_err(c->err, s);
}

// predictor = Model([user, item], pDot) (BPR.py:57): u . i per pair
template <int LPR>
__global__ void __launch_bounds__(256) k_kbpr_predict(const float* __restrict__ P, const int32_t* __restrict__ u,
                                                      const int32_t* __restrict__ it, int64_t n, int32_t d,
                                                      int64_t U1, int64_t I1, float* __restrict__ out,
                                                      int32_t* __restrict__ err) {
  const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t b = gid / LPR;
  const int l = (int)(threadIdx.x & (LPR - 1));
  if (b >= n) return;
  int32_t ru = u[b], ri = it[b];
  if (l == 0 && (ru < 0 || ru >= U1 || ri < 0 || ri >= I1)) atomicOr(err, (ru < 0 || ru >= U1) ? 1 : 2);
  ru = (ru < 0 || ru >= U1) ? 0 : ru;
  ri = (ri < 0 || ri >= I1) ? 0 : ri;
  const bool on = l * 4 < d;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 a = on ? *reinterpret_cast<const float4*>(P + (int64_t)ru * d + 4 * l) : z;
  const float4 q = on ? *reinterpret_cast<const float4*>(P + (U1 + ri) * (int64_t)d + 4 * l) : z;
  const float s = kb_sum<LPR>(a.x * q.x + a.y * q.y + a.z * q.z + a.w * q.w);
  if (l == 0) out[b] = s;
}

template <int LPR>
static void launch_pair_predict(const FlatCtx* c, const float* P, const int32_t* u, const int32_t* it, int64_t n,
                                float* out, hipStream_t s) {
  k_kbpr_predict<LPR><<<(unsigned)((n * LPR + 255) / 256), 256, 0, s>>>(P, u, it, n, c->d, c->U1, c->I1, out,
                                                                       c->err);
}

// acf_kbpr_predict and acf_amf_predict: both buffers start with [user table | item table]
static int pair_predict(FlatCtx* c, const float* P, const int32_t* u, const int32_t* it, int64_t n, float* out,
                        void* stream_) {
  ACF_CHECK(c && P && u && it && out, ACF_E_INVALID, "NULL argument");
  ACF_CHECK(n >= 0, ACF_E_INVALID, "negative count");
  if (n == 0) return ACF_OK;
  hipStream_t s = static_cast<hipStream_t>(stream_);
  HIP_TRY(hipMemsetAsync(c->err, 0, sizeof(int32_t), s));
  ACF_RET(DISPATCH_LPR(c->d, launch_pair_predict, c, P, u, it, n, out, s));
  HIP_TRY(hipGetLastError());
  return read_range_err(c->err, s);
}

extern "C" int acf_kbpr_predict(acf_kbpr_ctx* c, const float* P, const int32_t* u, const int32_t* it, int64_t n,
                                float* out, void* stream_) {
  return pair_predict(c, P, u, it, n, out, stream_);
}

// ---------------------------------------------------------------------------
// FastAdversarialMF (FastAdversarialMF.py:13-144; run.py --model amf2).
// params = [P (U1 x d) | Q (I1 x d) | D_u | D_i], a discriminator block being
// [W1 (d x d, Keras [in, out]) | b1 (d) | W2 (d) | b2 (1) | 3 pad]; gradient and
// Adam moments in the same layout.  Per batch of B instances (u, i, y) with the
// adversarial indices (ua, ia) and the players' popularity targets:
//   pred = P[u] . Q[i]; MSE vs y                                   (:48, :74)
//   D(e) = sigmoid(relu(e W1 + b1) . W2 + b2) on e = P[ua] / Q[ia]  (:119-127)
//   player mf (P, Q): MSE + BCE(D_u, tu) + BCE(D_i, ti), the discriminators
//   frozen; players disc_u / disc_i: BCE(D, du) / BCE(D, di), the embeddings
//   frozen; all at the same pre-step parameters (AdversarialOptimizerSimultaneous),
//   then one dense Keras Adam over the whole buffer (every player steps each batch).
// Kernels: k_amf_inst (one lane-group per instance: gathers, MSE, both
// discriminators forward and backward, row contributions + the per-instance
// factors of the weight gradients), k_amf_rows (per-row sums in occurrence
// order: P gets the u then the ua gathers, Q the i then the ia gathers),
// k_amf_wgrad (one thread per discriminator parameter, instances in order),
// k_nmf_adam.  Parity with the reference is unpinned (oracle/amf_oracle.py).
// ---------------------------------------------------------------------------
__host__ __device__ __forceinline__ int64_t amf_disc_block(int64_t d) { return d * d + 2 * d + 4; }

struct AmfArgs {
  const float* params;
  float* grad;
  const int32_t *u, *i, *ua, *ia;
  const float *y, *tu, *ti, *du, *di;
  int32_t B, d;
  int64_t U1, I1;
  float* contrib;  // [B][4][d]: MSE -> P[u], MSE -> Q[i], D_u -> P[ua], D_i -> Q[ia]
  float* dscr;     // [2][B][3d + 4]: e, relu'(h) * dz_d * W2, relu(h), dz_d
  float* loss;     // [B][3]: squared error, BCE(D_u, tu), BCE(D_i, ti)
  int32_t* err;
};

__device__ __forceinline__ float4 f4_or0(const float* p, bool on) {
  return on ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
}

template <int LPR>
__global__ void __launch_bounds__(256) k_amf_inst(AmfArgs a) {
  const int64_t gid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int b = (int)(gid / LPR), l = (int)(threadIdx.x & (LPR - 1));
  if (b >= a.B) return;
  const int d = a.d;
  int32_t ru = a.u[b], ri = a.i[b], rua = a.ua[b], ria = a.ia[b];
  if (l == 0 && (ru < 0 || ru >= a.U1 || rua < 0 || rua >= a.U1)) atomicOr(a.err, 1);
  if (l == 0 && (ri < 0 || ri >= a.I1 || ria < 0 || ria >= a.I1)) atomicOr(a.err, 2);
  ru = (ru < 0 || ru >= a.U1) ? 0 : ru;
  rua = (rua < 0 || rua >= a.U1) ? 0 : rua;
  ri = (ri < 0 || ri >= a.I1) ? 0 : ri;
  ria = (ria < 0 || ria >= a.I1) ? 0 : ria;
  const float* P = a.params;
  const float* Q = P + a.U1 * (int64_t)d;
  const bool on = l * 4 < d;
  const float invB = 1.0f / (float)a.B;
  // prediction and MSE (the Dot layer's gradient: dpred * the other row)
  const float4 pu = f4_or0(P + (int64_t)ru * d + 4 * l, on), qi = f4_or0(Q + (int64_t)ri * d + 4 * l, on);
  const float pred = kb_sum<LPR>(pu.x * qi.x + pu.y * qi.y + pu.z * qi.z + pu.w * qi.w);
  const float diff = pred - a.y[b];
  if (l == 0) a.loss[(int64_t)b * 3] = diff * diff;
  const float dpred = (diff * 2.0f) * invB;  // mean's 1/B times SquareGrad's 2x
  float* c = a.contrib + (int64_t)b * 4 * d + 4 * l;
  if (on) {
    *reinterpret_cast<float4*>(c) = make_float4(dpred * qi.x, dpred * qi.y, dpred * qi.z, dpred * qi.w);
    *reinterpret_cast<float4*>(c + d) = make_float4(dpred * pu.x, dpred * pu.y, dpred * pu.z, dpred * pu.w);
  }
  const float* const D0 = P + (a.U1 + a.I1) * (int64_t)d;
#pragma unroll 1
  for (int X = 0; X < 2; ++X) {
    const float* W1 = D0 + X * amf_disc_block(d);
    const float* b1 = W1 + (int64_t)d * d;
    const float* W2 = b1 + d;
    const float b2 = W2[d];
    const float4 e = f4_or0((X ? Q + (int64_t)ria * d : P + (int64_t)rua * d) + 4 * l, on);
    // h = e W1 + b1: lane l holds outputs 4l..4l+3; e_k broadcast inside the lane-group
    float4 h = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int kk = 0; kk < d / 4; ++kk) {
      const float ek[4] = {__shfl(e.x, kk, LPR), __shfl(e.y, kk, LPR), __shfl(e.z, kk, LPR),
                           __shfl(e.w, kk, LPR)};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 w = f4_or0(W1 + (int64_t)(4 * kk + q) * d + 4 * l, on);
        h.x = fmaf(ek[q], w.x, h.x); h.y = fmaf(ek[q], w.y, h.y);
        h.z = fmaf(ek[q], w.z, h.z); h.w = fmaf(ek[q], w.w, h.w);
      }
    }
    const float4 bb = f4_or0(b1 + 4 * l, on), w2 = f4_or0(W2 + 4 * l, on);
    h = make_float4(h.x + bb.x, h.y + bb.y, h.z + bb.z, h.w + bb.w);
    const float4 act = make_float4(fmaxf(h.x, 0.f), fmaxf(h.y, 0.f), fmaxf(h.z, 0.f), fmaxf(h.w, 0.f));
    const float z = kb_sum<LPR>(act.x * w2.x + act.y * w2.y + act.z * w2.z + act.w * w2.w) + b2;
    const float s = 1.0f / (1.0f + expf(-z));
    const bool inside = s >= 1e-7f && s <= 1.0f - 1e-7f;  // clip_by_value's gradient
    const float tm = (X ? a.ti : a.tu)[b], td = (X ? a.di : a.du)[b];
    if (l == 0) {
      const float sc = fminf(fmaxf(s, 1e-7f), 1.0f - 1e-7f);
      a.loss[(int64_t)b * 3 + 1 + X] = -(tm * logf(sc) + (1.0f - tm) * logf(1.0f - sc));
    }
    const float dzm = inside ? (s - tm) * invB : 0.f, dzd = inside ? (s - td) * invB : 0.f;
    const float4 dhm = make_float4(h.x > 0.f ? dzm * w2.x : 0.f, h.y > 0.f ? dzm * w2.y : 0.f,
                                   h.z > 0.f ? dzm * w2.z : 0.f, h.w > 0.f ? dzm * w2.w : 0.f);
    // de = W1 dh_m: lane l holds rows 4l..4l+3 of W1, dh_m broadcast
    float4 de = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int nn = 0; nn < d / 4; ++nn) {
      const float4 g = make_float4(__shfl(dhm.x, nn, LPR), __shfl(dhm.y, nn, LPR), __shfl(dhm.z, nn, LPR),
                                   __shfl(dhm.w, nn, LPR));
      float* dst[4] = {&de.x, &de.y, &de.z, &de.w};
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 w = f4_or0(W1 + (int64_t)(4 * l + q) * d + 4 * nn, on);
        float acc = *dst[q];
        acc = fmaf(w.x, g.x, acc); acc = fmaf(w.y, g.y, acc);
        acc = fmaf(w.z, g.z, acc); acc = fmaf(w.w, g.w, acc);
        *dst[q] = acc;
      }
    }
    if (on) {
      *reinterpret_cast<float4*>(c + (2 + X) * d) = de;
      float* sc = a.dscr + ((int64_t)X * a.B + b) * (3 * d + 4);
      *reinterpret_cast<float4*>(sc + 4 * l) = e;
      *reinterpret_cast<float4*>(sc + d + 4 * l) =
          make_float4(h.x > 0.f ? dzd * w2.x : 0.f, h.y > 0.f ? dzd * w2.y : 0.f, h.z > 0.f ? dzd * w2.z : 0.f,
                      h.w > 0.f ? dzd * w2.w : 0.f);
      *reinterpret_cast<float4*>(sc + 2 * d + 4 * l) = act;
      if (l == 0) sc[3 * d] = dzd;
    }
  }
}

// one wave per gathered row occurrence, 4B of them: P's [u_0..u_{B-1}, ua_0..],
// then Q's [i_0.., ia_0..].  The first occurrence of a row owns it and adds every
// occurrence's contribution in that order.
__global__ void __launch_bounds__(256) k_amf_rows(AmfArgs a) {
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  const int B = a.B, d = a.d;
  if (wave >= 4 * (int64_t)B) return;
  const bool item = wave >= 2 * B;
  const int me = (int)(item ? wave - 2 * B : wave), n = 2 * B;
  auto row_of = [&](int k) -> int32_t {
    int32_t r = item ? (k < B ? a.i[k] : a.ia[k - B]) : (k < B ? a.u[k] : a.ua[k - B]);
    const int64_t rows = item ? a.I1 : a.U1;
    return (r < 0 || r >= rows) ? 0 : r;
  };
  auto contrib_of = [&](int k) -> const float* {
    const int b = k < B ? k : k - B, slot = (k < B ? 0 : 2) + (item ? 1 : 0);
    return a.contrib + ((int64_t)b * 4 + slot) * d;
  };
  const int32_t r = row_of(me);
  for (int base = 0; base < me; base += 64) {
    const int k = base + lane;
    if (__any(k < me && row_of(k) == r)) return;
  }
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int base = me; base < n; base += 64) {
    const int k = base + lane;
    uint64_t mask = __ballot(k < n && row_of(k) == r);
    while (mask) {
      const int kk = base + __ffsll((unsigned long long)mask) - 1;
      mask &= mask - 1;
      const float* cc = contrib_of(kk);
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (lane + 64 * q < d) acc[q] = acc[q] + cc[lane + 64 * q];
    }
  }
  float* g = a.grad + (item ? a.U1 * (int64_t)d : 0) + (int64_t)r * d;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (lane + 64 * q < d) g[lane + 64 * q] = g[lane + 64 * q] + acc[q];
}

// one thread per discriminator parameter: W1[k][n] = sum_b e_b[k] dh_b[n],
// b1 = sum_b dh_b, W2 = sum_b relu(h_b) dz_b, b2 = sum_b dz_b (instances in order)
__global__ void __launch_bounds__(256) k_amf_wgrad(AmfArgs a) {
  const int64_t d = a.d, DB = amf_disc_block(d);
  const int64_t x = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (x >= 2 * DB) return;
  const int X = (int)(x / DB);
  const int64_t j = x - X * DB;
  const float* sc = a.dscr + (int64_t)X * a.B * (3 * d + 4);
  const int64_t S = 3 * d + 4;
  float acc = 0.f;
  if (j < d * d) {
    const int64_t k = j / d, n = j - k * d;
    for (int b = 0; b < a.B; ++b) acc = acc + sc[b * S + k] * sc[b * S + d + n];
  } else if (j < d * d + d) {
    const int64_t n = j - d * d;
    for (int b = 0; b < a.B; ++b) acc = acc + sc[b * S + d + n];
  } else if (j < d * d + 2 * d) {
    const int64_t n = j - d * d - d;
    for (int b = 0; b < a.B; ++b) acc = acc + sc[b * S + 2 * d + n] * sc[b * S + 3 * d];
  } else if (j == d * d + 2 * d) {
    for (int b = 0; b < a.B; ++b) acc = acc + sc[b * S + 3 * d];
  } else {
    return;  // padding
  }
  float* g = a.grad + (a.U1 + a.I1) * d + x;
  *g = *g + acc;
}

struct acf_amf_ctx : FlatCtx {
  float *contrib = nullptr, *dscr = nullptr;
};

extern "C" int64_t acf_amf_param_count(int64_t U1, int64_t I1, int32_t d) {
  return (U1 + I1) * (int64_t)d + 2 * amf_disc_block(d);
}

extern "C" int acf_amf_destroy(acf_amf_ctx* c) { return flat_destroy(c); }

extern "C" int acf_amf_create(acf_amf_ctx** out, int64_t U1, int64_t I1, int32_t d, int32_t maxB) {
  return flat_create(out, U1, I1, d, maxB, {{&acf_amf_ctx::contrib, (size_t)4 * d},
                                            {&acf_amf_ctx::dscr, (size_t)2 * (3 * d + 4)}});
}

template <int LPR>
static void launch_amf_inst(const AmfArgs& a, hipStream_t s) {
  k_amf_inst<LPR><<<(unsigned)(((int64_t)a.B * LPR + 255) / 256), 256, 0, s>>>(a);
}

static int amf_batch(const AmfArgs& a, hipStream_t s) {
  ACF_RET(DISPATCH_LPR(a.d, launch_amf_inst, a, s));
  k_amf_rows<<<(unsigned)((4 * (int64_t)a.B * 64 + 255) / 256), 256, 0, s>>>(a);
  k_amf_wgrad<<<(unsigned)((2 * amf_disc_block(a.d) + 255) / 256), 256, 0, s>>>(a);
  HIP_TRY(hipGetLastError());
  return ACF_OK;
}

extern "C" int acf_amf_grad(acf_amf_ctx* c, const float* params, float* grad, const int32_t* u, const int32_t* i,
                            const float* y, const int32_t* ua, const int32_t* ia, const float* tu, const float* ti,
                            const float* du, const float* di, int32_t B, float* loss, void* stream_) {
  ACF_CHECK(c && params && grad && u && i && y && ua && ia && tu && ti && du && di && loss, ACF_E_INVALID,
            "NULL argument");
  ACF_CHECK(B > 0 && B <= c->maxB, ACF_E_INVALID, "batch %d outside (0, %d]", B, c->maxB);
  hipStream_t s = static_cast<hipStream_t>(stream_);
  HIP_TRY(hipMemsetAsync(c->err, 0, sizeof(int32_t), s));
  const AmfArgs a{params, grad, u, i, ua, ia, y, tu, ti, du, di, B, c->d, c->U1, c->I1, c->contrib, c->dscr,
                  loss, c->err};
  ACF_RET(amf_batch(a, s));
  return read_range_err(c->err, s);
}

extern "C" int acf_amf_train(acf_amf_ctx* c, float* params, float* grad, float* m, float* v, const int32_t* u,
                             const int32_t* i, const float* y, const int32_t* ua, const int32_t* ia, const float* tu,
                             const float* ti, const float* du, const float* di, int64_t n, int32_t batch,
                             int64_t t_first, const acf_neumf_hparams* hp, float* losses, void* stream_) {
  ACF_CHECK(c && params && grad && m && v && u && i && y && ua && ia && tu && ti && du && di && hp && losses,
            ACF_E_INVALID, "NULL argument");
  ACF_CHECK(batch > 0 && batch <= c->maxB, ACF_E_INVALID, "batch %d outside (0, %d]", batch, c->maxB);
  ACF_CHECK(n >= 0 && t_first >= 1, ACF_E_INVALID, "bad instance count or Adam iteration");
  hipStream_t s = static_cast<hipStream_t>(stream_);
  HIP_TRY(hipMemsetAsync(c->err, 0, sizeof(int32_t), s));
  const int64_t n4 = acf_amf_param_count(c->U1, c->I1, c->d) / 4;
  int64_t k = 0;
  for (int64_t o = 0; o < n; o += batch, ++k) {
    const int32_t B = (int32_t)std::min<int64_t>(batch, n - o);
    const AmfArgs a{params, grad, u + o, i + o, ua + o, ia + o, y + o, tu + o, ti + o, du + o, di + o,
                    B, c->d, c->U1, c->I1, c->contrib, c->dscr, losses + 3 * o, c->err};
    ACF_RET(amf_batch(a, s));
    ACF_RET(acf_dense_adam(params, grad, m, v, n4, t_first + k, hp, s));
  }
  return read_range_err(c->err, s);
}

// model = Model([user, item], pred) (FastAdversarialMF.py:51; MF.py:38-40): u . i per pair
extern "C" int acf_amf_predict(acf_amf_ctx* c, const float* params, const int32_t* u, const int32_t* it, int64_t n,
                               float* out, void* stream_) {
  return pair_predict(c, params, u, it, n, out, stream_);
}
