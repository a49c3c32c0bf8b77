// acf_torch.cpp — PyTorch custom ops (TORCH_LIBRARY(acf, m)) over the C-ABI of
// libacf_apr.so: the APR hot path as torch.ops.acf.* on HIP tensors, the
// interface SURVEY.md §8(b) proposes.  Each op validates device / dtype /
// contiguity / shape with TORCH_CHECK, runs on the current HIP stream, and
// mutates its (a!) arguments in place.  No computation happens here: every op
// is one or two calls of the C-ABI (include/acf_apr.h).
//
//   acf::bpr_apr_step          one training_batch iteration (utils.py:114-119;
//                              APR.py:143-195): the fused streamed step
//   acf::apr_train             training_batch over n_batches (utils.py:113-119)
//   acf::gather_bpr_fwd_bwd    gathers + BPR loss + IndexedSlices grads (APR.py:121-150,183)
//   acf::row_segment_sum       IndexedSlices dedup (APR.py:183-187,195)
//   acf::l2norm_perturb        delta = eps * l2_normalize(g) (APR.py:186-191)
//   acf::sparse_adagrad_apply  SparseApplyAdagrad (APR.py:193-195)
//   acf::score_rank            _eval_by_user positions over candidate lists (utils.py:244-254)
//   acf::score_rank_all        the same over all items minus exclusions (utils.py:211-254)
//   acf::recommend_topk        the k best items per user and their scores (no reference counterpart)
//   acf::adv_direction         adv_update's direction over a whole triplet stream (utils.py:145-154)
//   acf::adv_apply             delta = N * eps and W + delta (APR.py:130-141,190)
//   acf::adv_pgd               iterated projected gradient attack on the whole stream
//   acf::fold_in_users         rows for new users against a frozen Q (no reference counterpart)
//   acf::fold_in_items         rows for new items against frozen P and Q (no reference counterpart)
//   acf::eval_positions_multi  positions of several held-out items per user, one sweep per user
//   acf::rank_metrics          hit / recall / precision / ndcg / map @K, mrr, auc of such positions (fp64)
//   acf::eval_positions_worst  certified worst-case positions under an eps attack on the user or the item rows
//   acf::eval_radius           certified radius: per entry the k smallest eps at which a candidate breaks the top-K
#include <torch/library.h>
#include <ATen/ATen.h>
// ROCm builds of PyTorch keep the "cuda" device type: the guard and stream
// wrappers that accept it are the *MasqueradingAsCUDA ones
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <cmath>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>

#include "acf_apr.h"

namespace {

void ok(int rc, const char* what) {
  TORCH_CHECK(rc == ACF_OK, what, " failed (code ", rc, "): ", acf_apr_last_error());
}

void* stream_of(const at::Tensor& t) {
  return c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream();
}

void need(const at::Tensor& t, const char* name, at::ScalarType dt, int64_t dim) {
  TORCH_CHECK(t.is_cuda(), name, " must be a HIP tensor (there is no CPU path)");
  TORCH_CHECK(t.scalar_type() == dt, name, " must be ", dt, ", got ", t.scalar_type());
  TORCH_CHECK(t.dim() == dim, name, " must be ", dim, "-D, got ", t.dim(), "-D");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

void need_table(const at::Tensor& t, const char* name, const at::Tensor& like) {
  need(t, name, at::kFloat, 2);
  TORCH_CHECK(t.device() == like.device(), name, " is on ", t.device(), ", expected ", like.device());
  const int64_t d = t.size(1);
  TORCH_CHECK(d >= 4 && d <= 1024 && d % 4 == 0, name, ": dim must be a multiple of 4 in [4, 1024], got ", d);
}

at::Tensor idx32(const at::Tensor& t, const char* name, const at::Tensor& like) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device(), name, " must live on ", like.device());
  TORCH_CHECK(t.scalar_type() == at::kInt || t.scalar_type() == at::kLong, name, " must be int32 or int64");
  return t.reshape({-1}).to(at::kInt).contiguous();
}

acf_apr_hparams hparams(double lr, double eps, double reg, double reg_adv, bool adver, double clip_lo,
                        double clip_hi) {
  acf_apr_hparams h;
  h.lr = (float)lr; h.eps = (float)eps; h.reg = (float)reg; h.reg_adv = (float)reg_adv;
  h.clip_lo = (float)clip_lo; h.clip_hi = (float)clip_hi;
  h.adver = adver ? 1 : 0; h.adv_mode = 0; h.seed = 0; h.zero_delta = 0; h.reserved = 0;
  return h;
}

// contexts (plan workspace + version buffers) by (device, tables, batch shape);
// one MF graph owns one in the reference (APR.py:197-202).  A context is shared
// (reference-counted) and carries its own lock, held for a whole
// train / copy_losses / step_errors sequence, so a concurrent call that evicts
// it from the cache cannot destroy it under a running op.
struct CtxKey {
  int dev;
  int64_t U1, I1;
  int32_t d, B, nb;
  bool operator<(const CtxKey& o) const {
    return std::tie(dev, U1, I1, d, B, nb) < std::tie(o.dev, o.U1, o.I1, o.d, o.B, o.nb);
  }
};
struct Ctx {
  acf_apr_ctx* c = nullptr;
  std::mutex mu;
  ~Ctx() {
    if (c) acf_apr_destroy(c);
  }
};
struct Entry {
  std::shared_ptr<Ctx> ctx;
  uint64_t last_use;
};
std::mutex g_mu;
std::map<CtxKey, Entry> g_ctx;
uint64_t g_clock = 0;
constexpr size_t kMaxContexts = 8;

std::shared_ptr<Ctx> context(const at::Tensor& P, const at::Tensor& Q, int32_t B, int32_t nb) {
  const CtxKey k{P.device().index(), P.size(0), Q.size(0), (int32_t)P.size(1), B, nb};
  std::lock_guard<std::mutex> lock(g_mu);
  auto it = g_ctx.find(k);
  if (it != g_ctx.end()) {
    it->second.last_use = ++g_clock;
    return it->second.ctx;
  }
  if (g_ctx.size() >= kMaxContexts) {  // bounded: drop the least recently used context
    auto lru = g_ctx.begin();
    for (auto e = g_ctx.begin(); e != g_ctx.end(); ++e)
      if (e->second.last_use < lru->second.last_use) lru = e;
    g_ctx.erase(lru);  // destroyed when the last running op lets go of it
  }
  auto h = std::make_shared<Ctx>();
  ok(acf_apr_create(&h->c, k.U1, k.I1, k.d, B, nb), "acf_apr_create");
  g_ctx.emplace(k, Entry{h, ++g_clock});
  return h;
}

// releases every cached context (plan workspace and k_stream version buffers,
// linear in d and batches per call); contexts still in use by a running op are
// destroyed when it returns.  Returns how many were dropped from the cache.
int64_t release_contexts() {
  std::lock_guard<std::mutex> lock(g_mu);
  const int64_t n = (int64_t)g_ctx.size();
  g_ctx.clear();
  return n;
}

// an index tensor must lie in [0, rows): TF Gather's InvalidArgument, checked
// before any kernel reads a row through it (one aminmax + one host sync)
void check_range(const at::Tensor& idx, int64_t rows, const char* name) {
  if (idx.numel() == 0) return;
  auto mm = idx.aminmax();
  const int64_t lo = std::get<0>(mm).item<int64_t>(), hi = std::get<1>(mm).item<int64_t>();
  TORCH_CHECK_INDEX(lo >= 0 && hi < rows, name, ": index ", lo < 0 ? lo : hi, " is outside [0, ", rows, ")");
}

void check_tables(const at::Tensor& P, const at::Tensor& Q, const at::Tensor& aP, const at::Tensor& aQ) {
  need_table(P, "embedding_P", P);
  need_table(Q, "embedding_Q", P);
  need_table(aP, "accumulator_P", P);
  need_table(aQ, "accumulator_Q", P);
  TORCH_CHECK(Q.size(1) == P.size(1), "embedding_P and embedding_Q dims differ");
  TORCH_CHECK(aP.sizes() == P.sizes() && aQ.sizes() == Q.sizes(), "accumulators must match their tables");
}

// training_batch over nb batches of B triplets; per-triplet losses
std::tuple<at::Tensor, at::Tensor> train(at::Tensor& P, at::Tensor& Q, at::Tensor& aP, at::Tensor& aQ,
                                         const at::Tensor& u_, const at::Tensor& i_, const at::Tensor& j_,
                                         int64_t B, double lr, double eps, double reg, double reg_adv, bool adver,
                                         double clip_lo, double clip_hi) {
  check_tables(P, Q, aP, aQ);
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(P.device());
  at::Tensor u = idx32(u_, "user", P), i = idx32(i_, "item_pos", P), j = idx32(j_, "item_neg", P);
  const int64_t n = u.numel();
  TORCH_CHECK(i.numel() == n && j.numel() == n, "triplet lengths differ");
  TORCH_CHECK(B > 0 && n > 0 && n % B == 0, n, " triplets is not a positive multiple of batch_size ", B);
  const int32_t nb = (int32_t)(n / B);
  std::shared_ptr<Ctx> held = context(P, Q, (int32_t)B, nb);
  std::lock_guard<std::mutex> ctx_lock(held->mu);
  acf_apr_ctx* c = held->c;
  acf_apr_tables tb{P.data_ptr<float>(), Q.data_ptr<float>(), aP.data_ptr<float>(), aQ.data_ptr<float>()};
  const acf_apr_hparams h = hparams(lr, eps, reg, reg_adv, adver, clip_lo, clip_hi);
  void* s = stream_of(P);
  // check = 1: an index outside its table raises (TF Gather's InvalidArgument)
  ok(acf_apr_train(c, &tb, &h, u.data_ptr<int32_t>(), i.data_ptr<int32_t>(), j.data_ptr<int32_t>(), (int32_t)B,
                   nb, 1, 1, s),
     "acf_apr_train");
  at::Tensor lc = at::empty({n}, P.options()), la = at::empty({n}, P.options());
  ok(acf_apr_copy_losses(c, lc.data_ptr<float>(), la.data_ptr<float>(), s), "acf_apr_copy_losses");
  int32_t err = 0;
  ok(acf_apr_step_errors(c, &err, s), "acf_apr_step_errors");
  TORCH_CHECK(err == 0, "the streamed step gave up waiting for a row version (step error ", err,
              "): the tables of this call are not trustworthy");
  if (!adver) la.zero_();
  return {lc, la};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> bpr_apr_step(at::Tensor& P, at::Tensor& Q, at::Tensor& aP,
                                                            at::Tensor& aQ, const at::Tensor& u, const at::Tensor& i,
                                                            const at::Tensor& j, double lr, double eps, double reg,
                                                            double reg_adv, bool adver, double clip_lo,
                                                            double clip_hi) {
  check_tables(P, Q, aP, aQ);
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(P.device());
  at::Tensor uu = idx32(u, "user", P), ii = idx32(i, "item_pos", P), jj = idx32(j, "item_neg", P);
  const int64_t B = uu.numel();
  TORCH_CHECK(B > 0 && ii.numel() == B && jj.numel() == B, "user / item_pos / item_neg must be equal, non-empty");
  // the forward below gathers rows before train()'s device-side check runs
  check_range(uu, P.size(0), "user");
  check_range(ii, Q.size(0), "item_pos");
  check_range(jj, Q.size(0), "item_neg");
  // pairwise accuracy of the batch (training_loss_acc's ACC, utils.py:159-175) before the step
  at::Tensor corr = at::empty({1}, P.options().dtype(at::kInt));
  ok(acf_bpr_forward(P.data_ptr<float>(), Q.data_ptr<float>(), P.size(0), Q.size(0), (int32_t)P.size(1),
                     uu.data_ptr<int32_t>(), ii.data_ptr<int32_t>(), jj.data_ptr<int32_t>(), (int32_t)B, 1,
                     (float)clip_lo, (float)clip_hi, nullptr, corr.data_ptr<int32_t>(), nullptr, nullptr,
                     stream_of(P)),
     "acf_bpr_forward");
  auto [lc, la] = train(P, Q, aP, aQ, uu, ii, jj, B, lr, eps, reg, reg_adv, adver, clip_lo, clip_hi);
  return {lc.sum(), la.sum(), corr.reshape({})};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor> gather_bpr_fwd_bwd(
    const at::Tensor& P, const at::Tensor& Q, const at::Tensor& u_, const at::Tensor& i_, const at::Tensor& j_,
    double clip_lo, double clip_hi) {
  need_table(P, "embedding_P", P);
  need_table(Q, "embedding_Q", P);
  TORCH_CHECK(Q.size(1) == P.size(1), "embedding_P and embedding_Q dims differ");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(P.device());
  at::Tensor u = idx32(u_, "user", P), i = idx32(i_, "item_pos", P), j = idx32(j_, "item_neg", P);
  const int64_t n = u.numel(), d = P.size(1);
  TORCH_CHECK(i.numel() == n && j.numel() == n, "triplet lengths differ");
  check_range(u, P.size(0), "user");
  check_range(i, Q.size(0), "item_pos");
  check_range(j, Q.size(0), "item_neg");
  at::Tensor loss = at::empty({n}, P.options()), x = at::empty({n}, P.options());
  at::Tensor pi = at::empty({2 * n}, u.options()), qi = at::empty({2 * n}, u.options());
  at::Tensor pv = at::empty({2 * n, d}, P.options()), qv = at::empty({2 * n, d}, P.options());
  if (n == 0) return {loss, x, pi, pv, qi, qv};  // empty tensors have no storage: NULL to the C ABI
  ok(acf_gather_bpr_fwd_bwd(P.data_ptr<float>(), Q.data_ptr<float>(), P.size(0), Q.size(0), (int32_t)d,
                            u.data_ptr<int32_t>(), i.data_ptr<int32_t>(), j.data_ptr<int32_t>(), n, (float)clip_lo,
                            (float)clip_hi, loss.data_ptr<float>(), x.data_ptr<float>(), pi.data_ptr<int32_t>(),
                            pv.data_ptr<float>(), qi.data_ptr<int32_t>(), qv.data_ptr<float>(), stream_of(P)),
     "acf_gather_bpr_fwd_bwd");
  return {loss, x, pi, pv, qi, qv};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> row_segment_sum(const at::Tensor& idx_, const at::Tensor& vals,
                                                               int64_t num_rows) {
  need(vals, "values", at::kFloat, 2);
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(vals.device());
  at::Tensor idx = idx32(idx_, "indices", vals);
  const int64_t m = idx.numel(), d = vals.size(1);
  TORCH_CHECK(vals.size(0) == m, "indices and values disagree: ", m, " vs ", vals.size(0), " rows");
  TORCH_CHECK(d >= 4 && d <= 1024 && d % 4 == 0, "values: dim must be a multiple of 4 in [4, 1024]");
  if (m > 0) {
    auto mm = idx.aminmax();
    TORCH_CHECK(std::get<0>(mm).item<int32_t>() >= 0 && std::get<1>(mm).item<int32_t>() < num_rows,
                "row_segment_sum: an index is outside [0, ", num_rows, ")");
  }
  TORCH_CHECK(num_rows > 0 && num_rows <= (1ll << 31), "row_segment_sum: num_rows outside (0, 2^31]");
  if (m == 0)  // empty tensors have no storage: NULL to the C ABI
    return {at::empty({0}, idx.options()), at::empty({0, d}, vals.options()), at::empty({0}, idx.options())};
  size_t ws = 0;
  ok(acf_row_segment_sum_workspace(m, &ws), "acf_row_segment_sum_workspace");
  at::Tensor work = at::empty({(int64_t)ws}, vals.options().dtype(at::kByte));
  at::Tensor uniq = at::empty({m}, idx.options()), cnt = at::empty({m}, idx.options());
  at::Tensor sum = at::empty({m, d}, vals.options());
  at::Tensor k = at::empty({1}, idx.options().dtype(at::kLong));
  ok(acf_row_segment_sum(idx.data_ptr<int32_t>(), vals.data_ptr<float>(), m, (int32_t)d, num_rows,
                         work.data_ptr(), ws, uniq.data_ptr<int32_t>(), sum.data_ptr<float>(),
                         cnt.data_ptr<int32_t>(), k.data_ptr<int64_t>(), stream_of(vals)),
     "acf_row_segment_sum");
  const int64_t kk = k.item<int64_t>();  // the unique count sizes the outputs (one sync)
  return {uniq.narrow(0, 0, kk), sum.narrow(0, 0, kk), cnt.narrow(0, 0, kk)};
}

at::Tensor l2norm_perturb(const at::Tensor& g, double eps) {
  need(g, "g_rows", at::kFloat, 2);
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(g.device());
  const int64_t d = g.size(1);
  TORCH_CHECK(d >= 4 && d <= 1024 && d % 4 == 0, "g_rows: dim must be a multiple of 4 in [4, 1024], got ", d);
  at::Tensor out = at::empty_like(g);
  if (g.size(0) == 0) return out;  // an empty tensor has no storage: NULL to the C ABI
  ok(acf_l2norm_perturb(g.data_ptr<float>(), g.size(0), (int32_t)g.size(1), (float)eps, out.data_ptr<float>(),
                        stream_of(g)),
     "acf_l2norm_perturb");
  return out;
}

void sparse_adagrad_apply(at::Tensor& W, at::Tensor& acc, const at::Tensor& idx_, const at::Tensor& g, double lr) {
  need_table(W, "W", W);
  need_table(acc, "accumulator", W);
  need(g, "g_rows", at::kFloat, 2);
  TORCH_CHECK(acc.sizes() == W.sizes(), "accumulator must match W");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(W.device());
  at::Tensor idx = idx32(idx_, "unique indices", W);
  TORCH_CHECK(g.size(0) == idx.numel() && g.size(1) == W.size(1), "g_rows must be [len(indices), dim]");
  check_range(idx, W.size(0), "unique indices");
  if (idx.numel() == 0) return;  // empty tensors have no storage: NULL to the C ABI
  ok(acf_sparse_adagrad_apply(W.data_ptr<float>(), acc.data_ptr<float>(), W.size(0), (int32_t)W.size(1),
                              idx.data_ptr<int32_t>(), g.data_ptr<float>(), idx.numel(), (float)lr, stream_of(W)),
     "acf_sparse_adagrad_apply");
}

at::Tensor score_rank(const at::Tensor& P, const at::Tensor& Q, const at::Tensor& users_, const at::Tensor& tests_,
                      const at::Tensor& cand_off, const at::Tensor& cand_items_) {
  need_table(P, "embedding_P", P);
  need_table(Q, "embedding_Q", P);
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(P.device());
  at::Tensor users = idx32(users_, "users", P), tests = idx32(tests_, "test_items", P);
  at::Tensor cands = idx32(cand_items_, "cand_items", P);
  need(cand_off, "cand_off", at::kLong, 1);
  TORCH_CHECK(cand_off.numel() == users.numel() + 1 && tests.numel() == users.numel(),
              "cand_off must have len(users) + 1 entries and test_items len(users)");
  check_range(users, P.size(0), "users");
  check_range(tests, Q.size(0), "test_items");
  check_range(cands, Q.size(0), "cand_items");
  if (cands.numel() == 0) cands = at::zeros({1}, users.options());
  at::Tensor pos = at::empty({users.numel()}, users.options());
  ok(acf_eval_positions_list(P.data_ptr<float>(), Q.data_ptr<float>(), P.size(0), Q.size(0), (int32_t)P.size(1),
                             users.data_ptr<int32_t>(), tests.data_ptr<int32_t>(), (int32_t)users.numel(),
                             cand_off.data_ptr<int64_t>(), cands.data_ptr<int32_t>(), pos.data_ptr<int32_t>(),
                             stream_of(P)),
     "acf_eval_positions_list");
  return pos;
}

at::Tensor score_rank_all(const at::Tensor& P, const at::Tensor& Q, const at::Tensor& users_,
                          const at::Tensor& tests_, int64_t num_candidates, const at::Tensor& excl_off,
                          const at::Tensor& excl_items_) {
  need_table(P, "embedding_P", P);
  need_table(Q, "embedding_Q", P);
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(P.device());
  at::Tensor users = idx32(users_, "users", P), tests = idx32(tests_, "test_items", P);
  at::Tensor excl = idx32(excl_items_, "excl_items", P);
  need(excl_off, "excl_off", at::kLong, 1);
  TORCH_CHECK(excl_off.numel() == users.numel() + 1 && tests.numel() == users.numel(),
              "excl_off must have len(users) + 1 entries and test_items len(users)");
  TORCH_CHECK(num_candidates >= 0 && num_candidates <= Q.size(0), "num_candidates exceeds item rows");
  check_range(users, P.size(0), "users");
  check_range(tests, Q.size(0), "test_items");
  check_range(excl, Q.size(0), "excl_items");
  if (excl.numel() == 0) excl = at::zeros({1}, users.options());
  at::Tensor pos = at::empty({users.numel()}, users.options());
  ok(acf_eval_positions_all(P.data_ptr<float>(), Q.data_ptr<float>(), P.size(0), Q.size(0), (int32_t)P.size(1),
                            users.data_ptr<int32_t>(), tests.data_ptr<int32_t>(), (int32_t)users.numel(),
                            (int32_t)num_candidates, excl_off.data_ptr<int64_t>(), excl.data_ptr<int32_t>(),
                            pos.data_ptr<int32_t>(), stream_of(P)),
     "acf_eval_positions_all");
  return pos;
}

// the k best candidates per user and their scores (acf_recommend_topk, kernel auto).  An
// exclusion list is a set and may hold entries outside [0, num_candidates), which
// are ignored: unlike score_rank_all's, its entries are not range-checked.
std::tuple<at::Tensor, at::Tensor> recommend_topk(const at::Tensor& P, const at::Tensor& Q, const at::Tensor& users_,
                                                  int64_t k, int64_t num_candidates, const at::Tensor& excl_off,
                                                  const at::Tensor& excl_items_) {
  need_table(P, "embedding_P", P);
  need_table(Q, "embedding_Q", P);
  TORCH_CHECK(P.size(1) == Q.size(1), "embedding_P and embedding_Q dims differ");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(P.device());
  at::Tensor users = idx32(users_, "users", P);
  at::Tensor excl = idx32(excl_items_, "excl_items", P);
  need(excl_off, "excl_off", at::kLong, 1);
  TORCH_CHECK(excl_off.device() == P.device(), "excl_off must live on ", P.device());
  TORCH_CHECK(excl_off.numel() == users.numel() + 1, "excl_off must have len(users) + 1 entries");
  TORCH_CHECK(k >= 1 && k <= 128, "k must be in [1, 128], got ", k);
  TORCH_CHECK(num_candidates >= 0 && num_candidates <= Q.size(0), "num_candidates exceeds item rows");
  check_range(users, P.size(0), "users");
  if (excl.numel() == 0) excl = at::zeros({1}, users.options());
  const int32_t n = (int32_t)users.numel();
  size_t ws = 0;
  ok(acf_recommend_topk_workspace(n, (int32_t)num_candidates, (int32_t)k, 0, &ws), "acf_recommend_topk_workspace");
  at::Tensor work = at::empty({(int64_t)((ws + 7) / 8)}, users.options().dtype(at::kLong));
  at::Tensor items = at::empty({n, k}, users.options());
  at::Tensor scores = at::empty({n, k}, P.options());
  ok(acf_recommend_topk(P.data_ptr<float>(), Q.data_ptr<float>(), P.size(0), Q.size(0), (int32_t)P.size(1),
                        users.data_ptr<int32_t>(), n, (int32_t)num_candidates, excl_off.data_ptr<int64_t>(),
                        excl.data_ptr<int32_t>(), (int32_t)k, items.data_ptr<int32_t>(), scores.data_ptr<float>(),
                        work.data_ptr(), ws, 0, stream_of(P)),
     "acf_recommend_topk");
  return {items, scores};
}

// unit-direction tables (nP, nQ) over all the triplets as one batch (acf_adv_direction,
// indices range-checked by the call); adv: "grad" or "random"
std::tuple<at::Tensor, at::Tensor> adv_direction(const at::Tensor& P, const at::Tensor& Q, const at::Tensor& user_,
                                                 const at::Tensor& item_pos_, const at::Tensor& item_neg_,
                                                 c10::string_view adv, int64_t seed, int64_t call, int64_t t,
                                                 double clip_lo, double clip_hi) {
  need_table(P, "embedding_P", P);
  need_table(Q, "embedding_Q", P);
  TORCH_CHECK(P.size(1) == Q.size(1), "embedding_P and embedding_Q dims differ");
  TORCH_CHECK(adv == "grad" || adv == "random", "adv must be 'grad' or 'random'");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(P.device());
  at::Tensor u = idx32(user_, "user", P), i = idx32(item_pos_, "item_pos", P), j = idx32(item_neg_, "item_neg", P);
  const int64_t n = u.numel();
  TORCH_CHECK(i.numel() == n && j.numel() == n, "user, item_pos and item_neg must have equal lengths");
  const int32_t mode = adv == "grad" ? 0 : 1;
  size_t ws = 0;
  if (mode == 0 && n > 0)
    ok(acf_adv_direction_workspace(n, P.size(0), Q.size(0), (int32_t)P.size(1), &ws), "acf_adv_direction_workspace");
  at::Tensor work = at::empty({(int64_t)((ws + 7) / 8)}, u.options().dtype(at::kLong));
  at::Tensor nP = at::empty_like(P), nQ = at::empty_like(Q);
  ok(acf_adv_direction(P.data_ptr<float>(), Q.data_ptr<float>(), P.size(0), Q.size(0), (int32_t)P.size(1),
                       n ? u.data_ptr<int32_t>() : nullptr, n ? i.data_ptr<int32_t>() : nullptr,
                       n ? j.data_ptr<int32_t>() : nullptr, n, (float)clip_lo, (float)clip_hi, mode, (uint64_t)seed,
                       (uint32_t)call, (int32_t)t, nP.data_ptr<float>(), nQ.data_ptr<float>(),
                       ws ? work.data_ptr() : nullptr, ws, 1, stream_of(P)),
     "acf_adv_direction");
  return {nP, nQ};
}

// (W + N * eps, N * eps): two separately rounded fp32 operations (acf_adv_apply)
std::tuple<at::Tensor, at::Tensor> adv_apply(const at::Tensor& W, const at::Tensor& N, double eps) {
  need(W, "W", at::kFloat, 2);
  need(N, "N", at::kFloat, 2);
  TORCH_CHECK(N.device() == W.device(), "N is on ", N.device(), ", expected ", W.device());
  TORCH_CHECK(W.sizes() == N.sizes(), "W and N differ in shape");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(W.device());
  at::Tensor sum = at::empty_like(W), delta = at::empty_like(W);
  ok(acf_adv_apply(W.data_ptr<float>(), N.data_ptr<float>(), W.size(0), (int32_t)W.size(1), (float)eps,
                   delta.data_ptr<float>(), sum.data_ptr<float>(), stream_of(W)),
     "acf_adv_apply");
  return {sum, delta};
}

// `iters` projected gradient steps on the whole stream's clean loss (acf_adv_pgd, planned once
// inside the call, indices range-checked): (delta_P, delta_Q, losses float64 [iters + 1])
std::tuple<at::Tensor, at::Tensor, at::Tensor> adv_pgd(const at::Tensor& P, const at::Tensor& Q,
                                                       const at::Tensor& user_, const at::Tensor& item_pos_,
                                                       const at::Tensor& item_neg_, double eps, int64_t iters,
                                                       c10::optional<double> alpha_, c10::string_view side,
                                                       const c10::optional<at::Tensor>& dP0,
                                                       const c10::optional<at::Tensor>& dQ0, double clip_lo,
                                                       double clip_hi) {
  need_table(P, "embedding_P", P);
  need_table(Q, "embedding_Q", P);
  TORCH_CHECK(P.size(1) == Q.size(1), "embedding_P and embedding_Q dims differ");
  TORCH_CHECK(iters >= 1 && iters <= ACF_ADV_PGD_MAX_ITERS, "iters must lie in [1, ", ACF_ADV_PGD_MAX_ITERS, "]");
  TORCH_CHECK(std::isfinite(eps) && eps >= 0, "eps must be finite and >= 0");
  const double alpha = alpha_.has_value() ? *alpha_ : 2.5 * eps / (double)iters;
  TORCH_CHECK(std::isfinite(alpha) && alpha >= 0, "alpha must be finite and >= 0");
  TORCH_CHECK(side == "both" || side == "user" || side == "item", "side must be 'both', 'user' or 'item'");
  const int32_t sd = side == "both" ? ACF_ADV_SIDE_BOTH : side == "user" ? ACF_ADV_SIDE_USER : ACF_ADV_SIDE_ITEM;
  auto need_start = [&](const c10::optional<at::Tensor>& t, const at::Tensor& w, const char* name) {
    if (!t.has_value()) return;
    need_table(*t, name, P);
    TORCH_CHECK(t->sizes() == w.sizes(), name, " must have its table's shape");
  };
  need_start(dP0, P, "delta_P0");
  need_start(dQ0, Q, "delta_Q0");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(P.device());
  at::Tensor u = idx32(user_, "user", P), i = idx32(item_pos_, "item_pos", P), j = idx32(item_neg_, "item_neg", P);
  const int64_t n = u.numel();
  TORCH_CHECK(i.numel() == n && j.numel() == n, "user, item_pos and item_neg must have equal lengths");
  size_t ws = 0;
  ok(acf_adv_pgd_workspace(n, P.size(0), Q.size(0), (int32_t)P.size(1), &ws), "acf_adv_pgd_workspace");
  at::Tensor work = at::empty({(int64_t)((ws + 7) / 8)}, u.options().dtype(at::kLong));
  at::Tensor dP = at::empty_like(P), dQ = at::empty_like(Q);
  at::Tensor losses = at::empty({iters + 1}, P.options().dtype(at::kDouble));
  ok(acf_adv_pgd(P.data_ptr<float>(), Q.data_ptr<float>(), P.size(0), Q.size(0), (int32_t)P.size(1),
                 n ? u.data_ptr<int32_t>() : nullptr, n ? i.data_ptr<int32_t>() : nullptr,
                 n ? j.data_ptr<int32_t>() : nullptr, n, (float)clip_lo, (float)clip_hi, nullptr, 0, (float)eps,
                 (float)alpha, (int32_t)iters, sd, dP0.has_value() ? dP0->data_ptr<float>() : nullptr,
                 dQ0.has_value() ? dQ0->data_ptr<float>() : nullptr, dP.data_ptr<float>(), dQ.data_ptr<float>(),
                 losses.data_ptr<double>(), work.data_ptr(), ws, 1, stream_of(P)),
     "acf_adv_pgd");
  return {dP, dQ, losses};
}

// a CSR's offsets: int64 [n + 1] on `like`'s device, 0 = off[0] <= ... <= off[n] = total (read back once)
void need_csr(const at::Tensor& off, const char* name, int64_t n, int64_t total, const at::Tensor& like) {
  need(off, name, at::kLong, 1);
  TORCH_CHECK(off.device() == like.device(), name, " must live on ", like.device());
  TORCH_CHECK(off.numel() == n + 1, name, " must have ", n + 1, " entries, got ", off.numel());
  const at::Tensor h = off.cpu();
  const int64_t* o = h.data_ptr<int64_t>();
  TORCH_CHECK(o[0] == 0 && o[n] == total, name, " must start at 0 and end at ", total);
  for (int64_t r = 0; r < n; ++r) TORCH_CHECK(o[r] <= o[r + 1], name, " must be non-decreasing");
}

// What the two fold-in ops share: the CSR (off, first) and the negatives checked and as int32, init /
// acc_init [n, d] or None, the outputs; a pointer is null where the C ABI takes no array (an empty one).
struct FoldArgs {
  int64_t n, T, d;
  at::Tensor first, neg, rows, acc, loss;
  const int32_t *first_p, *neg_p;
  const float *init_p = nullptr, *acc_init_p = nullptr;
  float *rows_p, *acc_p, *loss_p;
};

FoldArgs fold_args(const at::Tensor& Q, const at::Tensor& off, const char* off_name, const at::Tensor& first_,
                   const char* first_name, const at::Tensor& neg_, int64_t epochs, int64_t batch,
                   const c10::optional<at::Tensor>& init, const c10::optional<at::Tensor>& acc_init) {
  TORCH_CHECK(off.numel() >= 1, off_name, " must have n + 1 entries");
  TORCH_CHECK(epochs >= 0 && epochs < (1ll << 31), "epochs must be >= 0");
  TORCH_CHECK(batch >= 1 && batch <= ACF_FOLD_MAX_BATCH, "batch must lie in [1, ", ACF_FOLD_MAX_BATCH, "], got ", batch);
  FoldArgs a;
  a.first = idx32(first_, first_name, Q);
  a.n = off.numel() - 1, a.T = a.first.numel(), a.d = Q.size(1);
  TORCH_CHECK(neg_.dim() == 2 && neg_.size(0) == epochs && neg_.size(1) == a.T,
              "item_neg must have shape (epochs, len(", first_name, "))");
  a.neg = idx32(neg_, "item_neg", Q);
  need_csr(off, off_name, a.n, a.T, Q);
  const auto start = [&](const c10::optional<at::Tensor>& t, const char* name) -> const float* {
    if (!t.has_value()) return nullptr;
    need(*t, name, at::kFloat, 2);
    TORCH_CHECK(t->device() == Q.device() && t->size(0) == a.n && t->size(1) == a.d, name, " must be [n, dim] on ",
                Q.device());
    return t->data_ptr<float>();
  };
  a.init_p = start(init, "init"), a.acc_init_p = start(acc_init, "acc_init");
  a.rows = at::empty({a.n, a.d}, Q.options()), a.acc = at::empty({a.n, a.d}, Q.options());
  a.loss = at::empty({epochs, a.n}, Q.options());
  a.first_p = a.T ? a.first.data_ptr<int32_t>() : nullptr;
  a.neg_p = a.T && epochs ? a.neg.data_ptr<int32_t>() : nullptr;
  a.rows_p = a.n ? a.rows.data_ptr<float>() : nullptr;
  a.acc_p = a.n ? a.acc.data_ptr<float>() : nullptr;
  a.loss_p = a.n && epochs ? a.loss.data_ptr<float>() : nullptr;
  return a;
}

// rows, accumulators and per-epoch losses of n new users fitted against a frozen Q
// (acf_fold_in_users, items range-checked by the call); init / acc_init: [n, d] or None
std::tuple<at::Tensor, at::Tensor, at::Tensor> fold_in_users(
    const at::Tensor& Q, const at::Tensor& user_off, const at::Tensor& item_pos, const at::Tensor& item_neg,
    int64_t epochs, int64_t batch, const c10::optional<at::Tensor>& init, const c10::optional<at::Tensor>& acc_init,
    double lr, double eps, double reg, double reg_adv, bool adver, double clip_lo, double clip_hi) {
  need_table(Q, "embedding_Q", Q);
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(Q.device());
  const FoldArgs a = fold_args(Q, user_off, "user_off", item_pos, "item_pos", item_neg, epochs, batch, init, acc_init);
  const acf_apr_hparams hp = hparams(lr, eps, reg, reg_adv, adver, clip_lo, clip_hi);
  ok(acf_fold_in_users(Q.data_ptr<float>(), Q.size(0), (int32_t)a.d, user_off.data_ptr<int64_t>(), a.n, a.first_p,
                       a.neg_p, a.T, (int32_t)epochs, (int32_t)batch, &hp, a.init_p, a.acc_init_p, a.rows_p, a.acc_p,
                       a.loss_p, 1, stream_of(Q)),
     "acf_fold_in_users");
  return {a.rows, a.acc, a.loss};
}

// rows, accumulators and per-epoch losses of n new items fitted against frozen P and Q
// (acf_fold_in_items, users and negatives range-checked by the call); init / acc_init: [n, d] or None
std::tuple<at::Tensor, at::Tensor, at::Tensor> fold_in_items(
    const at::Tensor& P, const at::Tensor& Q, const at::Tensor& item_off, const at::Tensor& user_pos,
    const at::Tensor& item_neg, int64_t epochs, int64_t batch, const c10::optional<at::Tensor>& init,
    const c10::optional<at::Tensor>& acc_init, double lr, double eps, double reg, double reg_adv, bool adver,
    double clip_lo, double clip_hi) {
  need_table(P, "embedding_P", P);
  need_table(Q, "embedding_Q", P);
  TORCH_CHECK(P.size(1) == Q.size(1), "embedding_P and embedding_Q differ in dim: ", P.size(1), " and ", Q.size(1));
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(Q.device());
  const FoldArgs a = fold_args(Q, item_off, "item_off", user_pos, "user_pos", item_neg, epochs, batch, init, acc_init);
  const acf_apr_hparams hp = hparams(lr, eps, reg, reg_adv, adver, clip_lo, clip_hi);
  ok(acf_fold_in_items(P.data_ptr<float>(), P.size(0), Q.data_ptr<float>(), Q.size(0), (int32_t)a.d,
                       item_off.data_ptr<int64_t>(), a.n, a.first_p, a.neg_p, a.T, (int32_t)epochs, (int32_t)batch, &hp,
                       a.init_p, a.acc_init_p, a.rows_p, a.acc_p, a.loss_p, 1, stream_of(Q)),
     "acf_fold_in_items");
  return {a.rows, a.acc, a.loss};
}

// positions of every test item of every entry's list (acf_eval_positions_multi).  users and
// test items are range-checked here, before any gather; an exclusion list is a set and may
// hold entries outside [0, num_candidates) (ignored).  Empty excl_off and excl_items: no exclusions.
at::Tensor eval_positions_multi(const at::Tensor& P, const at::Tensor& Q, const at::Tensor& users_,
                                const at::Tensor& test_off, const at::Tensor& test_items_, int64_t num_candidates,
                                const at::Tensor& excl_off, const at::Tensor& excl_items_) {
  need_table(P, "embedding_P", P);
  need_table(Q, "embedding_Q", P);
  TORCH_CHECK(P.size(1) == Q.size(1), "embedding_P and embedding_Q dims differ");
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(P.device());
  at::Tensor users = idx32(users_, "users", P), tests = idx32(test_items_, "test_items", P);
  at::Tensor excl = idx32(excl_items_, "excl_items", P);
  const int64_t n = users.numel(), T = tests.numel();
  TORCH_CHECK(n < (1ll << 31) && T < (1ll << 31), "too many users or test items");
  TORCH_CHECK(num_candidates >= 1 && num_candidates <= Q.size(0), "num_candidates must lie in [1, item rows]");
  need_csr(test_off, "test_off", n, T, P);
  const bool no_excl = excl_off.numel() == 0 && excl.numel() == 0;
  if (!no_excl) need_csr(excl_off, "excl_off", n, excl.numel(), P);
  check_range(users, P.size(0), "users");
  check_range(tests, Q.size(0), "test_items");
  if (excl.numel() == 0) excl = at::zeros({1}, users.options());
  at::Tensor pos = at::empty({T}, users.options());
  if (n == 0 || T == 0) return pos;
  size_t ws = 0;
  ok(acf_eval_positions_multi_workspace((int32_t)n, T, (int32_t)num_candidates, &ws),
     "acf_eval_positions_multi_workspace");
  at::Tensor work = at::empty({(int64_t)((ws + 3) / 4)}, users.options());
  ok(acf_eval_positions_multi(P.data_ptr<float>(), Q.data_ptr<float>(), P.size(0), Q.size(0), (int32_t)P.size(1),
                              users.data_ptr<int32_t>(), test_off.data_ptr<int64_t>(), tests.data_ptr<int32_t>(),
                              (int32_t)n, T, (int32_t)num_candidates,
                              no_excl ? nullptr : excl_off.data_ptr<int64_t>(),
                              no_excl ? nullptr : excl.data_ptr<int32_t>(), pos.data_ptr<int32_t>(),
                              work.data_ptr(), ws, 0, stream_of(P)),
     "acf_eval_positions_multi");
  return pos;
}

// (per_user [n, n_cut, 5], per_user_free [n, 2], mean_cut [n_cut, 5], mean_free [2], n_scored [1]) in fp64
// (acf_eval_rank_metrics); columns: hit, recall, precision, ndcg, map / mrr, auc
std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor, at::Tensor> rank_metrics(
    const at::Tensor& positions, const at::Tensor& test_off, const at::Tensor& n_neg, at::IntArrayRef cutoffs) {
  need(positions, "positions", at::kInt, 1);
  need(n_neg, "n_neg", at::kInt, 1);
  TORCH_CHECK(n_neg.device() == positions.device(), "n_neg must live on ", positions.device());
  const c10::hip::HIPGuardMasqueradingAsCUDA guard(positions.device());
  const int64_t n = n_neg.numel(), T = positions.numel(), nc = (int64_t)cutoffs.size();
  TORCH_CHECK(n < (1ll << 31), "too many users");
  TORCH_CHECK(nc <= 8, "at most 8 cutoffs, got ", nc);
  int32_t cuts[8] = {0};
  for (int64_t c = 0; c < nc; ++c) {
    TORCH_CHECK(cutoffs[c] >= 1 && cutoffs[c] <= 1024, "a cutoff must lie in [1, 1024], got ", cutoffs[c]);
    cuts[c] = (int32_t)cutoffs[c];
  }
  need_csr(test_off, "test_off", n, T, positions);
  const auto f64 = positions.options().dtype(at::kDouble);
  at::Tensor per_user = at::empty({n, nc, 5}, f64), per_free = at::empty({n, 2}, f64);
  at::Tensor mean_cut = at::empty({nc, 5}, f64), mean_free = at::empty({2}, f64);
  at::Tensor n_scored = at::empty({1}, positions.options().dtype(at::kLong));
  const at::Tensor pos = T ? positions : at::zeros({1}, positions.options());  // never read, never NULL
  ok(acf_eval_rank_metrics(pos.data_ptr<int32_t>(), test_off.data_ptr<int64_t>(), (int32_t)n,
                           n ? n_neg.data_ptr<int32_t>() : nullptr, cuts, (int32_t)nc,
                           n && nc ? per_user.data_ptr<double>() : nullptr, n ? per_free.data_ptr<double>() : nullptr,
                           nc ? mean_cut.data_ptr<double>() : nullptr, mean_free.data_ptr<double>(),
                           n_scored.data_ptr<int64_t>(), stream_of(positions)),
     "acf_eval_rank_metrics");
  return {per_user, per_free, mean_cut, mean_free, n_scored};
}

// Entries with one test item each, as eval_positions_worst and eval_radius take them: the tables and the
// side checked, the tables' device guarded while this lives, users and test items int32 on it and
// range-checked here, before any gather; empty excl_off and excl_items: no exclusions (NULL, NULL).
struct CertEntries {
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard;
  at::Tensor users, tests, excl;
  int64_t n;
  int32_t side;
  const int64_t* eoff;
  const int32_t* ex;

  CertEntries(const at::Tensor& P, const at::Tensor& Q, const at::Tensor& users_, const at::Tensor& test_items_,
              int64_t num_candidates, const at::Tensor& excl_off, const at::Tensor& excl_items_,
              c10::string_view side_) {
    need_table(P, "embedding_P", P);
    need_table(Q, "embedding_Q", P);
    TORCH_CHECK(P.size(1) == Q.size(1), "embedding_P and embedding_Q dims differ");
    TORCH_CHECK(side_ == "user" || side_ == "item", "side must be \"user\" or \"item\", got \"", side_, "\"");
    side = side_ == "user" ? 0 : 1;
    guard.set_device(P.device());
    users = idx32(users_, "users", P), tests = idx32(test_items_, "test_items", P);
    excl = idx32(excl_items_, "excl_items", P);
    n = users.numel();
    TORCH_CHECK(n < (1ll << 31), "too many users");
    TORCH_CHECK(tests.numel() == n, "test_items must have one entry per user");
    TORCH_CHECK(num_candidates >= 1 && num_candidates <= Q.size(0), "num_candidates must lie in [1, item rows]");
    const bool no_excl = excl_off.numel() == 0 && excl.numel() == 0;
    if (!no_excl) need_csr(excl_off, "excl_off", n, excl.numel(), P);
    check_range(users, P.size(0), "users");
    check_range(tests, Q.size(0), "test_items");
    if (excl.numel() == 0) excl = at::zeros({1}, users.options());
    eoff = no_excl ? nullptr : excl_off.data_ptr<int64_t>();
    ex = no_excl ? nullptr : excl.data_ptr<int32_t>();
  }
};

// worst-case positions [n_eps, n] of every entry's test item under an attack of budget eps on the
// side's rows (acf_eval_positions_worst; side: "user" | "item").
at::Tensor eval_positions_worst(const at::Tensor& P, const at::Tensor& Q, const at::Tensor& users,
                                const at::Tensor& test_items, int64_t num_candidates, const at::Tensor& excl_off,
                                const at::Tensor& excl_items, at::ArrayRef<double> eps, c10::string_view side) {
  const int64_t ne = (int64_t)eps.size();
  TORCH_CHECK(ne >= 1 && ne <= 8, "1 to 8 eps, got ", ne);
  float ev[8] = {0};
  for (int64_t e = 0; e < ne; ++e) {
    ev[e] = (float)eps[e];
    TORCH_CHECK(std::isfinite(ev[e]) && ev[e] >= 0.f, "eps must be finite and >= 0, got ", eps[e]);
  }
  const CertEntries c(P, Q, users, test_items, num_candidates, excl_off, excl_items, side);
  at::Tensor worst = at::empty({ne, c.n}, c.users.options());
  if (c.n == 0) return worst;
  size_t ws = 0;
  ok(acf_eval_positions_worst_workspace((int32_t)c.n, (int32_t)num_candidates, (int32_t)ne, &ws),
     "acf_eval_positions_worst_workspace");
  at::Tensor work = at::empty({(int64_t)((ws + 3) / 4)}, c.users.options());
  ok(acf_eval_positions_worst(P.data_ptr<float>(), Q.data_ptr<float>(), P.size(0), Q.size(0), (int32_t)P.size(1),
                              c.users.data_ptr<int32_t>(), c.tests.data_ptr<int32_t>(), (int32_t)c.n,
                              (int32_t)num_candidates, c.eoff, c.ex, ev, (int32_t)ne, c.side,
                              worst.data_ptr<int32_t>(), work.data_ptr(), ws, 0, stream_of(P)),
     "acf_eval_positions_worst");
  return worst;
}

// the k smallest (eps_c, c) per entry, eps [n, k] ascending and items [n, k] (acf_eval_radius; side:
// "user" | "item"): eps[r][j] is the certified radius at j + 1.
std::tuple<at::Tensor, at::Tensor> eval_radius(const at::Tensor& P, const at::Tensor& Q, const at::Tensor& users,
                                               const at::Tensor& test_items, int64_t num_candidates,
                                               const at::Tensor& excl_off, const at::Tensor& excl_items, int64_t k,
                                               c10::string_view side) {
  TORCH_CHECK(k >= 1 && k <= 128, "k must lie in [1, 128], got ", k);
  const CertEntries c(P, Q, users, test_items, num_candidates, excl_off, excl_items, side);
  at::Tensor eps = at::empty({c.n, k}, P.options()), items = at::empty({c.n, k}, c.users.options());
  if (c.n == 0) return {eps, items};
  size_t ws = 0;
  ok(acf_eval_radius_workspace((int32_t)c.n, (int32_t)num_candidates, (int32_t)k, &ws), "acf_eval_radius_workspace");
  at::Tensor work = at::empty({(int64_t)((ws + 7) / 8)}, c.users.options().dtype(at::kLong));
  ok(acf_eval_radius(P.data_ptr<float>(), Q.data_ptr<float>(), P.size(0), Q.size(0), (int32_t)P.size(1),
                     c.users.data_ptr<int32_t>(), c.tests.data_ptr<int32_t>(), (int32_t)c.n, (int32_t)num_candidates,
                     c.eoff, c.ex, (int32_t)k, c.side, eps.data_ptr<float>(), items.data_ptr<int32_t>(),
                     work.data_ptr(), ws, 0, stream_of(P)),
     "acf_eval_radius");
  return {eps, items};
}

}  // namespace

#ifndef ACF_BUILD_HASH
#define ACF_BUILD_HASH "unhashed"
#endif
// "ACF_BUILD_HASH=<32 hex>" of this library's sources (build_native.source_hash)
extern "C" const char* acf_torch_build_hash(void) { return "ACF_BUILD_HASH=" ACF_BUILD_HASH; }

TORCH_LIBRARY(acf, m) {
  m.def("bpr_apr_step(Tensor(a!) P, Tensor(b!) Q, Tensor(c!) accP, Tensor(d!) accQ, Tensor u, Tensor i, "
        "Tensor j, float lr=0.05, float eps=0.5, float reg=0., float reg_adv=1., bool adver=True, "
        "float clip_lo=-80., float clip_hi=100000000.) -> (Tensor loss_clean, Tensor loss_adv, Tensor n_correct)");
  m.def("apr_train(Tensor(a!) P, Tensor(b!) Q, Tensor(c!) accP, Tensor(d!) accQ, Tensor u, Tensor i, Tensor j, "
        "int batch_size, float lr=0.05, float eps=0.5, float reg=0., float reg_adv=1., bool adver=True, "
        "float clip_lo=-80., float clip_hi=100000000.) -> (Tensor loss_clean, Tensor loss_adv)");
  m.def("gather_bpr_fwd_bwd(Tensor P, Tensor Q, Tensor u, Tensor i, Tensor j, float clip_lo=-80., "
        "float clip_hi=100000000.) -> (Tensor loss, Tensor x, Tensor p_idx, Tensor p_val, Tensor q_idx, "
        "Tensor q_val)");
  m.def("row_segment_sum(Tensor idx, Tensor vals, int num_rows) -> (Tensor uniq_idx, Tensor summed, Tensor count)");
  m.def("l2norm_perturb(Tensor g_rows, float eps) -> Tensor");
  m.def("sparse_adagrad_apply(Tensor(a!) W, Tensor(b!) acc, Tensor uniq_idx, Tensor g_rows, float lr) -> ()");
  m.def("score_rank(Tensor P, Tensor Q, Tensor users, Tensor test_items, Tensor cand_off, Tensor cand_items) "
        "-> Tensor");
  m.def("release_contexts() -> int", &release_contexts);
  m.def("score_rank_all(Tensor P, Tensor Q, Tensor users, Tensor test_items, int num_candidates, "
        "Tensor excl_off, Tensor excl_items) -> Tensor");
  m.def("recommend_topk(Tensor P, Tensor Q, Tensor users, int k, int num_candidates, Tensor excl_off, "
        "Tensor excl_items) -> (Tensor items, Tensor scores)");
  m.def("adv_direction(Tensor P, Tensor Q, Tensor user, Tensor item_pos, Tensor item_neg, str adv=\"grad\", "
        "int seed=0, int call=1, int t=0, float clip_lo=-80.0, float clip_hi=1e8) -> (Tensor nP, Tensor nQ)");
  m.def("adv_apply(Tensor W, Tensor N, float eps) -> (Tensor sum, Tensor delta)");
  m.def("adv_pgd(Tensor P, Tensor Q, Tensor user, Tensor item_pos, Tensor item_neg, float eps, int iters=10, "
        "float? alpha=None, str side=\"both\", Tensor? delta_P0=None, Tensor? delta_Q0=None, float clip_lo=-80.0, "
        "float clip_hi=1e8) -> (Tensor delta_P, Tensor delta_Q, Tensor losses)");
  m.def("fold_in_users(Tensor Q, Tensor user_off, Tensor item_pos, Tensor item_neg, int epochs, int batch=512, "
        "Tensor? init=None, Tensor? acc_init=None, float lr=0.05, float eps=0.5, float reg=0., float reg_adv=1., "
        "bool adver=True, float clip_lo=-80., float clip_hi=100000000.) -> (Tensor P_new, Tensor acc_new, Tensor loss)");
  m.def("fold_in_items(Tensor P, Tensor Q, Tensor item_off, Tensor user_pos, Tensor item_neg, int epochs, "
        "int batch=512, Tensor? init=None, Tensor? acc_init=None, float lr=0.05, float eps=0.5, float reg=0., "
        "float reg_adv=1., bool adver=True, float clip_lo=-80., float clip_hi=100000000.) -> "
        "(Tensor Q_new, Tensor acc_new, Tensor loss)");
  m.def("eval_positions_multi(Tensor P, Tensor Q, Tensor users, Tensor test_off, Tensor test_items, "
        "int num_candidates, Tensor excl_off, Tensor excl_items) -> Tensor");
  m.def("rank_metrics(Tensor positions, Tensor test_off, Tensor n_neg, int[] cutoffs) -> "
        "(Tensor per_user, Tensor per_user_free, Tensor mean_cut, Tensor mean_free, Tensor n_scored)");
  m.def("eval_positions_worst(Tensor P, Tensor Q, Tensor users, Tensor test_items, int num_candidates, "
        "Tensor excl_off, Tensor excl_items, float[] eps, str side=\"user\") -> Tensor");
  m.def("eval_radius(Tensor P, Tensor Q, Tensor users, Tensor test_items, int num_candidates, Tensor excl_off, "
        "Tensor excl_items, int k=10, str side=\"user\") -> (Tensor eps, Tensor items)");
}

TORCH_LIBRARY_IMPL(acf, CUDA, m) {
  m.impl("bpr_apr_step", &bpr_apr_step);
  m.impl("apr_train", &train);
  m.impl("gather_bpr_fwd_bwd", &gather_bpr_fwd_bwd);
  m.impl("row_segment_sum", &row_segment_sum);
  m.impl("l2norm_perturb", &l2norm_perturb);
  m.impl("sparse_adagrad_apply", &sparse_adagrad_apply);
  m.impl("score_rank", &score_rank);
  m.impl("score_rank_all", &score_rank_all);
  m.impl("recommend_topk", &recommend_topk);
  m.impl("adv_direction", &adv_direction);
  m.impl("adv_apply", &adv_apply);
  m.impl("adv_pgd", &adv_pgd);
  m.impl("fold_in_users", &fold_in_users);
  m.impl("fold_in_items", &fold_in_items);
  m.impl("eval_positions_multi", &eval_positions_multi);
  m.impl("rank_metrics", &rank_metrics);
  m.impl("eval_positions_worst", &eval_positions_worst);
  m.impl("eval_radius", &eval_radius);
}
