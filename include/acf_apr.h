/*
 * acf_apr.h — C-ABI of the MI355X-native adversarial BPR-MF (APR) hot path.
 *
 * The reference (feay1234/Adversarial-Collaborative-Filtering) has no FFI: its hot
 * path is a TensorFlow-1 graph driven from Python through `sess.run`.  Every entry
 * point below replaces one such `sess.run` call site (or the op group behind it);
 * the citation on each names the reference line it stands in for.  Python binds
 * these with ctypes (adversarial-collaborative-filtering_amd/_native.py); the
 * binding a maintainer would add to the reference is shown in INTEGRATION.md.
 *
 * Conventions
 *   - All array arguments are DEVICE pointers (HIP, gfx950) unless noted.
 *   - Tables are fp32, row-major, contiguous, [rows, dim]; indices are int32.
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy null stream).
 *   - Every call is asynchronous on `stream` unless documented otherwise.
 *   - Return value: ACF_OK (0) or an ACF_E_* code; acf_last_error() gives a
 *     thread-local message for the last failing call.
 *   - dim must be a multiple of 4 and <= 1024 (all configurations the reference
 *     runs use dim in {8,16,32,64,128}).
 */
#ifndef ACF_APR_H
#define ACF_APR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACF_APR_ABI_VERSION 2

enum {
  ACF_OK = 0,
  ACF_E_INVALID = 1,     /* bad argument (shape, null pointer, unsupported dim) */
  ACF_E_RANGE = 2,       /* index out of range (TF Gather's InvalidArgument)     */
  ACF_E_HIP = 3,         /* HIP runtime error                                    */
  ACF_E_NOMEM = 4,       /* device allocation failed                             */
  ACF_E_STATE = 5        /* call out of order (e.g. step before plan)            */
};

/* Opaque per-model context: owns the device workspace, the batch plans and the
 * cached hipGraph executables.  One context per (process, device, model). */
typedef struct acf_apr_ctx acf_apr_ctx;

/* Trainable state of MF (APR.py:105-119) plus its Adagrad slots
 * (APR.py:193-195, TF initial_accumulator_value = 0.1). */
typedef struct acf_apr_tables {
  float* P;    /* embedding_P  [num_user_rows, dim] */
  float* Q;    /* embedding_Q  [num_item_rows, dim] */
  float* accP; /* Adagrad accumulator of P, same shape */
  float* accQ; /* Adagrad accumulator of Q, same shape */
} acf_apr_tables;

/* Hyper-parameters read by MF.__init__ (APR.py:86-97) and the graph constants. */
typedef struct acf_apr_hparams {
  float lr;        /* args.lr       (run_adv_ori.py:42, default 0.05)  */
  float eps;       /* args.eps      (run_adv_ori.py:54, default 0.5)   */
  float reg;       /* args.reg      (run_adv_ori.py:40, default 0)     */
  float reg_adv;   /* args.reg_adv  (run_adv_ori.py:44, default 1)     */
  float clip_lo;   /* clip_by_value lower bound, -80  (APR.py:148)     */
  float clip_hi;   /* clip_by_value upper bound, 1e8  (APR.py:148)     */
  int32_t adver;   /* 0: BPR graph, 1: APR graph (APR.py:156)          */
  int32_t adv_mode;/* 0: "grad" (APR.py:180-191); 1: "random" (APR.py:170-177) */
  uint64_t seed;   /* counter-based RNG seed for adv_mode = 1          */
  int32_t zero_delta; /* 1: adversarial terms use delta = 0 (the dns>1 branch of
                         utils.py:121-139 never runs update_P/update_Q)  */
  int32_t reserved;
} acf_apr_hparams;

/* ---- library ------------------------------------------------------------ */
int acf_apr_abi_version(void);
const char* acf_apr_last_error(void);
/* "ACF_BUILD_HASH=<32 hex>": hash of the sources, headers and flags the library
 * was built from (build_native.source_hash); the loaders refuse a mismatch. */
const char* acf_apr_build_hash(void);

/* ---- context ------------------------------------------------------------ */
/* Allocates the workspace for plans of up to max_batches_per_plan batches of up
 * to max_batch_size triplets.  Synchronous.  Replaces MF(...).build_graph()
 * (APR.py:197-202) as the point where per-model device state is created. */
int acf_apr_create(acf_apr_ctx** out, int64_t num_user_rows, int64_t num_item_rows,
                   int32_t dim, int32_t max_batch_size, int32_t max_batches_per_plan);
int acf_apr_destroy(acf_apr_ctx* ctx);

/* ---- batch planning: TF's sparse-gradient de-duplication ------------------
 * Stages n_batches consecutive mini-batches (batch b = triplets
 * [b*batch_size, (b+1)*batch_size)) and builds, per batch, the unique user and
 * item rows with the ordered list of their occurrences — the structure TF builds
 * with Unique + UnsortedSegmentSum in Optimizer._apply_sparse_duplicate_indices
 * (behind APR.py:195) and that IndexedSlices->dense conversion sums
 * (APR.py:183-187).  If `check` != 0 the call synchronises the stream and
 * returns ACF_E_RANGE when any index is outside its table (TF CPU Gather raises
 * InvalidArgument there); with check == 0 bad indices are clamped to row 0. */
int acf_apr_plan(acf_apr_ctx* ctx, const int32_t* user, const int32_t* item_pos,
                 const int32_t* item_neg, int32_t batch_size, int32_t n_batches,
                 int32_t check, void* stream);

/* sess.run([model.update_P, model.update_Q], feed_dict)  (utils.py:117-118,
 * APR.py:167-191): delta rows for every row touched by planned batch `batch`.
 * Rows not touched have delta = 0 in the reference and are never read, so only
 * touched rows are materialised (in the context). */
int acf_apr_delta_update(acf_apr_ctx* ctx, const acf_apr_tables* tables,
                         const acf_apr_hparams* hp, int32_t batch, void* stream);

/* sess.run(model.optimizer, feed_dict)  (utils.py:119, APR.py:143-165,193-195):
 * clean + (if hp->adver) adversarial forward/backward, per-row gradient
 * aggregation, sparse Adagrad on the unique rows — in place on `tables`.
 * With hp->adver the delta of the last acf_apr_delta_update on the same batch
 * is used. */
int acf_apr_optimizer_step(acf_apr_ctx* ctx, const acf_apr_tables* tables,
                           const acf_apr_hparams* hp, int32_t batch, void* stream);

/* The hot loop of training_batch (utils.py:106-119, dns == 1): for planned
 * batches [first_batch, first_batch + n_batches): delta_update (if adver) then
 * optimizer_step.  graph_mode 1 replays a cached hipGraph of the whole loop
 * (captured on first use for this (tables, hparams, range)); 0 launches
 * eagerly. */
int acf_apr_train_planned(acf_apr_ctx* ctx, const acf_apr_tables* tables,
                          const acf_apr_hparams* hp, int32_t first_batch,
                          int32_t n_batches, int32_t graph_mode, void* stream);

/* training_batch over a triplet range in ONE call (utils.py:106-119 for
 * n_batches consecutive batches): acf_apr_plan(user, item_pos, item_neg,
 * batch_size, n_batches, check) followed by acf_apr_train_planned over all the
 * planned batches.  The triplet arrays are device pointers that must stay valid
 * until the stream has run the call. */
int acf_apr_train(acf_apr_ctx* ctx, const acf_apr_tables* tables, const acf_apr_hparams* hp,
                  const int32_t* user, const int32_t* item_pos, const int32_t* item_neg,
                  int32_t batch_size, int32_t n_batches, int32_t check, int32_t graph_mode,
                  void* stream);

/* Kernel timing for roofline accounting: runs planned batches
 * [first_batch, first_batch + n_batches) exactly like acf_apr_train_planned
 * (eager, same stream, same kernels, tables updated) but brackets every kernel
 * with hipExtLaunchKernelGGL start/stop events.  Writes, per kernel kind
 * k = 0 (clean pass, or the fused BPR step), 1 (adversarial pass + Adagrad),
 * 2 (write-back: k_flush / k_stream_flush), 3 (unused since r05: the
 * overlapped step k_ovl is gone), 4 (streamed step k_stream), 5 (hot-slot combine of large-batch plans), the
 * summed kernel time in ms to ms_out[k] and the launch count to
 * launches_out[k] (arrays of 6).  Synchronous.  Not part of the reference
 * surface. */
int acf_apr_time_kernels(acf_apr_ctx* ctx, const acf_apr_tables* tables,
                         const acf_apr_hparams* hp, int32_t first_batch,
                         int32_t n_batches, double* ms_out, int32_t* launches_out,
                         void* stream);

/* How step kernels map unique rows ("slots") to lanes: 0 = auto (default: one
 * wavefront per slot below 4,096 triplets per batch, where hot rows have many
 * occurrences; one lane-group of dim/4 lanes per slot at and above it, where
 * almost every row occurs once), 1 = one wavefront per slot, 2 = one lane-group
 * per slot.  Results are deterministic for a given mapping and agree across
 * mappings to fp32 summation order.  Not part of the reference surface. */
int acf_apr_set_slot_mapping(acf_apr_ctx* ctx, int32_t mode);

/* Triplet fusion in acf_apr_train_planned / acf_apr_time_kernels (1 = on, the
 * default; 0 = off).  A triplet whose user, positive and negative item each
 * occur once in its batch is stepped start to finish by one lane-group (no
 * batch-wide aggregation is needed for it); the arithmetic per row is the slot
 * kernels' own, so on and off give identical bits.  For one-lane-group-per-slot
 * plans (batches >= 4,096) the setting at acf_apr_plan time decides the plan: on
 * gives a triplet-centric plan whose steps (train_planned and the split per-batch
 * calls alike) update every row in its table; training such a plan with fusion
 * switched off returns ACF_E_STATE (plan again).  Otherwise the split per-batch
 * calls (delta_update / optimizer_step) never fuse.  Not part of the reference
 * surface. */
int acf_apr_set_fusion(acf_apr_ctx* ctx, int32_t on);

/* Which planner acf_apr_plan uses: 0 = auto (the default: the batch-local plan,
 * one workgroup per batch in two launches, for one-wavefront-per-slot plans of
 * batches up to 1,024 triplets on tables whose batch bitmaps fit 64 MB; the hash
 * plan for triplet-centric plans -- one lane-group per slot, fusion on, not
 * shard mode, batches up to 65,536; the device-wide sort plan otherwise), 1 = always the
 * device-wide sort plan.  Every planner gives the step identical bits (the hash
 * plan numbers slots and CSR ranges in another order, and keeps the occurrence
 * order inside each range).  Not part of the reference surface (A/B and the
 * planner-equivalence tests). */
int acf_apr_set_plan_mode(acf_apr_ctx* ctx, int32_t mode);

/* The planner the last acf_apr_plan used: 0 device-wide sort plan, 1 batch-local
 * plan, 2 one-workgroup shard plan, 3 hash plan; -1 before any plan.  Not part
 * of the reference surface (tests and bench). */
int acf_apr_plan_kind(const acf_apr_ctx* ctx);

/* Streamed APR steps in acf_apr_train_planned (1 = on, the default; 0 = off;
 * the setting is per context).  For plans with one wavefront
 * per slot and dim <= 256, ONE launch runs the whole batch range: every row a
 * batch updates becomes a tagged version that later batches read (bounded spin
 * until it exists), and one write-back kernel moves the last versions to the
 * tables.  Arithmetic and order of every sum are unchanged, so on and off give
 * identical bits.  Uses 3 x max_batches x 3 x max_batch_size x dim x 8 bytes of
 * device memory, allocated at first use (off when that fails, or when the
 * device cannot keep the launch resident).  Not part of the reference surface. */
int acf_apr_set_stream(acf_apr_ctx* ctx, int32_t on);

/* Failure safety of the streamed step (k_stream).  k_stream needs every one of
 * its waves resident; when a hand-off wait gives up (another process or a
 * concurrent persistent kernel on the device), its flush writes nothing, so the
 * tables are as before the call.  failsafe = 1 (default): every streamed call
 * stays asynchronous and is queued for verification; its launch reports its
 * outcome to host-mapped memory.  A failed call sets the group's gate, so every
 * later streamed call of the group applies nothing either; the queue is settled
 * by acf_apr_resolve and, implicitly, by every entry point that needs settled
 * tables (the setters, acf_apr_step_errors, acf_apr_stream_recoveries,
 * acf_apr_copy_losses, the two-phase and shard calls, a non-streamed
 * train_planned) or that re-plans a context with a queued call (acf_apr_plan):
 * the failed call and every later queued one are replayed, in order, on the
 * two-kernel schedule (exact: same result as acf_apr_set_stream 0).
 * failsafe = 0 (and timed or graph-captured calls): a give-up is reported by
 * acf_apr_step_errors (bit 0, sticky until read) and that call's rows are not
 * applied; later calls are applied normally.  Such an unverified call settles
 * the group's queue before it launches (except inside a capture), so it never
 * runs behind the gate of an earlier failed verified call.
 * acf_apr_set_spin_limit: version polls before a give-up (default 65,536; 0
 * gives up at the first unready poll -- tests force the replay with it).
 * acf_apr_stream_recoveries: streamed calls replayed so far. */
int acf_apr_set_failsafe(acf_apr_ctx* ctx, int32_t on);
int acf_apr_set_spin_limit(acf_apr_ctx* ctx, int32_t polls);
/* s_sleep between two polls of a row version in k_stream, as a code: 0-3 are
 * s_sleep 0-3, 4 / 5 / 6 are s_sleep 8 / 16 / 32 (default 2).  Timing only: the
 * results do not depend on it.  A non-default code runs the general instance of
 * the streamed kernel (k_stream_any). */
int acf_apr_set_poll_sleep(acf_apr_ctx* ctx, int32_t code);
int acf_apr_stream_recoveries(acf_apr_ctx* ctx, int64_t* out);
/* Settle every queued verified streamed call of the context's group (blocks
 * until they have all reported; replays failed ones, see above). */
int acf_apr_resolve(acf_apr_ctx* ctx);
/* acf_apr_resolve for every group of the process with a queued call: what a
 * reader of the tables outside the group calls first (evaluation, forward,
 * checkpoints; the Python layer does so in ops.settle_tables). */
int acf_apr_resolve_all(void);
/* ctx joins peer's verification group: contexts that train the same tables on
 * one stream (a PlanPipeline's contexts) must share one, so that a failed call
 * of either gates the later calls of both.  Settles both groups first. */
int acf_apr_share_failsafe(acf_apr_ctx* ctx, acf_apr_ctx* peer);
/* A non-blocking stream of the current device's lowest priority, for plans
 * that run beside a streamed call (acf_apr_plan of the next chunk on it while
 * k_stream trains this one on the caller's stream): where both have workgroups
 * to place, the step's go first.  The caller orders the two streams with
 * events and destroys the stream when its work has been waited for. */
int acf_plan_stream_create(void** out);
int acf_plan_stream_destroy(void* stream);

/* ---- shard mode: users and items row-sharded over the ranks of one node ----
 * SURVEY §8(e) (no reference counterpart: the reference trains on one CPU
 * process; this splits one training_batch, utils.py:113-119, across ranks so
 * the result is the single-process one up to fp32 summation order).  Row r of
 * P lives on rank r % G, row r of Q on rank r % G; each rank plans the
 * triplets of ITS users for one global batch on (its user shard, the item rows
 * it fetched, in working-set order), and the batch-global item sums of
 * APR.py:183-195 are completed by the item owners between the passes. */

/* Shard mode on/off for the context (forces one lane-group per slot, no triplet
 * fusion; a one-batch plan per step).  reg_batch: the global batch size the
 * reg * mean(w^2) terms divide by (0 = the planned batch size). */
int acf_apr_set_shard_mode(acf_apr_ctx* ctx, int32_t on, int32_t reg_batch);

/* (r06) Which batch of the plan the next shard pass / item map calls step: a
 * triplet-centric shard plan (batches over 1,024 triplets) may hold a chunk of
 * steps planned at once (distributed.ShardedAPR); slot-kernel shard plans are
 * one batch (0).  Reset to 0 by acf_apr_set_shard_mode. */
int acf_apr_set_shard_batch(acf_apr_ctx* ctx, int32_t batch);

/* pass 0: clean sums (users complete: delta; items: partial sums in the item
 * slots' rows; BPR also updates the users); pass 1 (APR): adversarial sums
 * (users: Adagrad + write-back to the user shard; items: partial sums).  The
 * item rows of `tables` are the fetched working set (never written). */
int acf_apr_shard_pass(acf_apr_ctx* ctx, const acf_apr_tables* tables, const acf_apr_hparams* hp,
                       int32_t pass, void* stream);

/* The item slots of the current one-batch plan, in working-set order:
 * dir 0 copies their partial sums to buf [n_items, dim]; dir 1 copies buf into
 * their delta rows (the owners' deltas, before pass 1). */
int acf_apr_shard_items(acf_apr_ctx* ctx, int32_t dir, float* buf, int64_t n_items, void* stream);

/* acf_apr_shard_pass, and the item slots' partial sums of the pass also written to
 * row map[w] of buf for working-set entry w < n_items (what acf_apr_shard_items_mapped
 * dir 0 does after the pass), by the pass's own combine launch (export workgroups):
 * the split step hands its exchange rows to the pass and needs no copy launch. */
int acf_apr_shard_pass_export(acf_apr_ctx* ctx, const acf_apr_tables* tables, const acf_apr_hparams* hp,
                              int32_t pass, float* buf, const int64_t* map, int64_t n_items, void* stream);

/* As acf_apr_shard_items, with working-set entry w at row map[w] of buf (int64
 * row indices): the split step moves the item partial sums and deltas straight
 * between the slots and its fixed-layout exchange rows (distributed.py "Static
 * step layout"), with no gather or scatter pass of its own. */
int acf_apr_shard_items_mapped(acf_apr_ctx* ctx, int32_t dir, float* buf, const int64_t* map, int64_t n_items,
                               void* stream);

/* Owner side, per owned row s of the step: the partial rows recv[pos[p]] for p
 * in [seg[s], seg[s+1]) (requester order) are summed in that order.
 * reduce_delta (APR.py:183-191): G0[s] = the sum; reply[pos[p]] = eps *
 * l2_normalize(sum) for every p of the row (hp->zero_delta: 0).
 * reduce_apply (APR.py:193-195): G = G0[s] + reg_adv * sum (APR; BPR: the sum),
 * then Adagrad on Q[rows[s]] / accQ[rows[s]]; count[s] = the row's occurrences
 * in the global batch (needed only when hp->reg != 0, with reg_batch). */
int acf_shard_reduce_delta(const float* recv, const int32_t* seg, const int32_t* pos, int32_t n_rows,
                           int32_t dim, const acf_apr_hparams* hp, float* G0, float* reply, void* stream);
int acf_shard_reduce_apply(float* Q, float* accQ, const float* recv, const int32_t* seg, const int32_t* pos,
                           int32_t n_rows, int32_t dim, const acf_apr_hparams* hp, const float* G0,
                           const int32_t* rows, const int32_t* count, int32_t reg_batch, void* stream);

/* Reads into *out and clears the step error word: bit 0 = an overlapped step
 * gave up waiting for a row (results of that call are not trustworthy).
 * Synchronous on `stream`.  Not part of the reference surface. */
int acf_apr_step_errors(acf_apr_ctx* ctx, int32_t* out, void* stream);

/* Per-triplet clean / adversarial losses computed by the last step of each
 * planned batch (softplus(-clip(x)) terms of APR.py:150,162), for the staged
 * triplets [0, n_batches*batch_size).  Either pointer may be NULL. */
int acf_apr_copy_losses(acf_apr_ctx* ctx, float* loss_clean, float* loss_adv,
                        void* stream);

/* Writes the delta rows of the last acf_apr_delta_update into dense tables
 * delta_P [num_user_rows, dim] / delta_Q [num_item_rows, dim]; untouched rows
 * are left as the caller initialised them (zero in the reference). */
int acf_apr_delta_scatter(acf_apr_ctx* ctx, float* delta_P, float* delta_Q,
                          void* stream);

/* ---- forward only: training_loss_acc (utils.py:159-175) ------------------
 * Per batch b of n_batches: batch_loss[b] = sum softplus(-clip(x+ - x-)) and
 * batch_correct[b] = #(x+ - x- > 0); optional per-triplet scores out_pos /
 * out_neg (model.output / model.output_neg).  Any output may be NULL. */
int acf_bpr_forward(const float* P, const float* Q, int64_t num_user_rows,
                    int64_t num_item_rows, int32_t dim, const int32_t* user,
                    const int32_t* item_pos, const int32_t* item_neg,
                    int32_t batch_size, int32_t n_batches, float clip_lo,
                    float clip_hi, float* batch_loss, int32_t* batch_correct,
                    float* out_pos, float* out_neg, void* stream);

/* ---- evaluation: _eval_by_user (utils.py:244-254) ------------------------
 * position[u] = #{candidate c : score(u,c) >= score(u,test_item[u])} with
 * score = P[u] . Q[c].
 * _all:  candidates = [0, num_candidates) minus the sorted, unique exclusion
 *        list excl_items[excl_off[k] .. excl_off[k+1]) of user k (the caller
 *        passes trainList[u] union {test item}, restricted to the range:
 *        utils.py:211-215).
 * _list: candidates = cand_items[cand_off[k] .. cand_off[k+1]) verbatim, with
 *        repeats ("sample" mode, utils.py:201-209). */
int acf_eval_positions_all(const float* P, const float* Q, int64_t num_user_rows,
                           int64_t num_item_rows, int32_t dim, const int32_t* users,
                           const int32_t* test_items, int32_t n_users,
                           int32_t num_candidates, const int64_t* excl_off,
                           const int32_t* excl_items, int32_t* positions,
                           void* stream);
int acf_eval_positions_list(const float* P, const float* Q, int64_t num_user_rows,
                            int64_t num_item_rows, int32_t dim, const int32_t* users,
                            const int32_t* test_items, int32_t n_users,
                            const int64_t* cand_off, const int32_t* cand_items,
                            int32_t* positions, void* stream);

/* acf_eval_positions_all with the sweep chosen per call: kernel 0 = auto (what
 * acf_eval_positions_all runs), 1 = the MFMA sweep (one kernel:
 * v_mfma_f32_16x16x4_f32 tiles, exact rescoring of candidates within the f32
 * error band of the test score, exclusions as a per-tile bitmap), 2 = the VALU
 * sweep.  Positions are identical for every kernel; no process-wide state. */
int acf_eval_positions_all_kernel(const float* P, const float* Q, int64_t num_user_rows,
                                  int64_t num_item_rows, int32_t dim, const int32_t* users,
                                  const int32_t* test_items, int32_t n_users,
                                  int32_t num_candidates, const int64_t* excl_off,
                                  const int32_t* excl_items, int32_t* positions, int32_t kernel,
                                  void* stream);

/* ---- recommendation lists: the K best items per user ----------------------
 * (no reference counterpart: the reference only ranks a held-out item.)
 * For user k (row users[k] of P; any order, repeats allowed) the candidates are
 * [0, num_candidates) minus the SET of excl_items[excl_off[k] .. excl_off[k+1]):
 * a list may be unsorted, repeat items and hold entries outside the range (-1
 * included), which are ignored.  score(u,c) is the sequential round-then-add
 * dot product the evaluation uses, bit for bit; the order is score descending by
 * float comparison, ties to the ascending item id.  out_items / out_scores
 * [n_users, k] receive the first k candidates in that order and their scores;
 * a user with fewer than k candidates gets -1 / -inf in the tail.  Exact and
 * deterministic: identical bits run to run and for every kernel (0 = auto,
 * 1 = the MFMA sweep filtering for an exact rescoring, 2 = the VALU sweep).
 * 1 <= k <= 128.  No [n_users, num_candidates] array is formed: the caller
 * provides `workspace` (device memory, 8-byte aligned) of at least the size
 * acf_recommend_topk_workspace reports for the same (n_users, num_candidates,
 * k, kernel) -- a host-only query; a smaller one is ACF_E_INVALID.  User
 * indices must lie in [0, num_user_rows) (not checked here).  Tables are
 * assumed finite: with a NaN score the order is unspecified. */
int acf_recommend_topk_workspace(int32_t n_users, int32_t num_candidates, int32_t k, int32_t kernel,
                                 size_t* bytes);
int acf_recommend_topk(const float* P, const float* Q, int64_t num_user_rows, int64_t num_item_rows,
                       int32_t dim, const int32_t* users, int32_t n_users, int32_t num_candidates,
                       const int64_t* excl_off, const int32_t* excl_items, int32_t k,
                       int32_t* out_items, float* out_scores, void* workspace, size_t workspace_bytes,
                       int32_t kernel, void* stream);

/* ---- nearest-neighbour lists: similar items, similar users -----------------
 * (no reference counterpart.)  Query r is row queries[r] of the query table X
 * [num_query_rows, dim] (any order, repeats allowed; X may be T itself); its
 * candidates are the rows [0, num_candidates) of T [num_rows, dim] minus the SET
 * of excl_items[excl_off[r] .. excl_off[r+1]) -- unsorted, repeated and
 * out-of-range entries (-1 included) are ignored; excl_off = excl_items = NULL
 * excludes nothing -- and, with exclude_self != 0, minus the candidate whose id
 * equals queries[r] (the query itself when X == T; for another X just that id).
 * Self-exclusion is decided inside the kernel: no per-query list is built.
 * With a = X[queries[r]], b = T[c] and s = the evaluation's sequential
 * round-then-add dot product of a and b (acf_recommend_topk's score):
 *   metric 0 (dot):       score = s.  With X == T, exclude_self = 0 and no
 *     lists the output equals acf_recommend_topk(T, T, ...) bit for bit.
 *   metric 1 (cosine):    na = sqrtf(s(a, a)), nb = sqrtf(s(b, b)), den = na *
 *     nb; score = den > 0 ? (s / den) + 0.0f : +0.0f.  A zero row scores +0.0
 *     against everything.
 *   metric 2 (Euclidean): score = 0.0f - D2, D2 = the sum over k ascending from
 *     +0.0 of round((a[k] - b[k])^2), acf_eval_positions_worst's chain: a larger
 *     score is a nearer row, identical rows give +0.0.
 * All of it fp32, every operation rounded on its own, the square roots and the
 * division correctly rounded.  No score is ever -0.0, which the 64-bit
 * (score, id) key of the selection relies on: s never is (the chain starts at
 * +0.0); a quotient that underflows on the negative side is -0.0 and the
 * "+ 0.0f" makes it +0.0 while changing no other value; D2 >= +0.0, so
 * 0.0f - D2 is +0.0 exactly for D2 = +0.0, the only case in which that
 * subtraction yields a zero.
 * The order is score descending by float comparison, ties to the ascending id;
 * out_items / out_scores [n_queries, k] receive the first k candidates in that
 * order, -1 / -inf past the last candidate.  1 <= k <= 128.  A query's list
 * depends only on that query's inputs.  Exact and deterministic: identical bits
 * run to run, no float atomics; no [n_queries, num_candidates] array and no
 * normalised copy of T is formed.  `workspace`: device memory, 8-byte aligned:
 * a 16-byte head, the strips' partial lists (n_queries * S * k * 8 bytes, as
 * for acf_recommend_topk's VALU sweep) and, used by metric 1 only,
 * num_candidates floats of candidate norms computed once per call.
 * acf_neighbors_topk_workspace reports all three together -- a host-only query
 * that touches no device and has no metric argument; metrics 0 and 2 accept a
 * workspace without the norms.  A smaller workspace, a metric outside 0..2 and
 * k outside [1, 128] are ACF_E_INVALID before any launch.  0 <= num_candidates
 * <= num_rows; n_queries = 0 does nothing.  A query outside [0, num_query_rows)
 * is read as row 0 (and is id 0 for exclude_self); with check != 0 the call
 * then synchronises once, after its launches, and returns ACF_E_RANGE
 * (check == 0: no error, no sync).  Tables are assumed finite: with a NaN
 * score the order is unspecified. */
int acf_neighbors_topk_workspace(int32_t n_queries, int32_t num_candidates, int32_t k, size_t* bytes);
int acf_neighbors_topk(const float* T, int64_t num_rows, int32_t dim, const float* X, int64_t num_query_rows,
                       const int32_t* queries, int32_t n_queries, int32_t num_candidates, int32_t metric,
                       int32_t exclude_self, const int64_t* excl_off, const int32_t* excl_items, int32_t k,
                       int32_t* out_items, float* out_scores, void* workspace, size_t workspace_bytes,
                       int32_t check, void* stream);

/* ---- evaluation against several held-out items per user --------------------
 * (no reference counterpart: the reference holds out one item per user.)
 * Entry r (row users[r] of P; any order, repeats allowed) has the test list
 * test_items[test_off[r] .. test_off[r+1]) (test_off: int64 [n_users + 1],
 * non-decreasing within [0, n_tests]; offsets outside are clamped) and the
 * candidates C_r = [0, num_candidates) minus the SET of
 * excl_items[excl_off[r] .. excl_off[r+1]) -- unsorted, repeated and
 * out-of-range entries (-1 included) are fine, as for acf_recommend_topk;
 * excl_off = excl_items = NULL excludes nothing.  For every x of r's list with
 * t = test_items[x]:
 *   positions[x] = #{ c in C_r, c != t : score(u,c) >= score(u,t) }
 * with the evaluation's sequential round-then-add dot product, so ties are
 * decided on equal bits exactly as by acf_eval_positions_all.  The other test
 * items of the list stay candidates unless the caller excluded them; t itself
 * never counts, excluded or not; a repeated test item gets the same position
 * each time; an empty list writes nothing.  A position depends on (u, t, C_r,
 * P, Q) only: not on the list's other items, not on the other entries.
 * The candidates are swept once per (entry, chunk of 256 test items, strip of
 * the candidate range), whatever the length of a list.  Exact integers,
 * identical bits run to run; no [n_users, num_candidates] array is formed.
 * `workspace`: device memory, 4-byte aligned, at least
 * acf_eval_positions_multi_workspace(n_users, n_tests, num_candidates) bytes --
 * a host-only query that touches no device; a smaller one is ACF_E_INVALID.
 * 1 <= num_candidates <= num_item_rows; 0 <= n_tests < 2^31.
 * A user outside [0, num_user_rows) or a test item outside [0, num_item_rows)
 * is read as row 0; with check != 0 the call then synchronises once, after its
 * launches, and returns ACF_E_RANGE (check == 0: no error, no sync). */
int acf_eval_positions_multi_workspace(int32_t n_users, int64_t n_tests, int32_t num_candidates,
                                       size_t* bytes);
int acf_eval_positions_multi(const float* P, const float* Q, int64_t num_user_rows, int64_t num_item_rows,
                             int32_t dim, const int32_t* users, const int64_t* test_off,
                             const int32_t* test_items, int32_t n_users, int64_t n_tests,
                             int32_t num_candidates, const int64_t* excl_off, const int32_t* excl_items,
                             int32_t* positions, void* workspace, size_t workspace_bytes, int32_t check,
                             void* stream);

/* Ranking metrics of such positions, reduced on the device in fp64.  User u's
 * m = test_off[u+1] - test_off[u] positions sorted ascending are r_0 <= ... <=
 * r_{m-1}; item x's j is the number of the user's entries with a smaller
 * position, or an equal position and a smaller index (exact for any m).
 * n_neg[u] >= 1 (device int32): the user's candidates that are not test items.
 * cutoffs: a HOST array of n_cutoffs <= 8 values K in [1, 1024].  Per user and
 * cutoff, per_user [n_users][n_cutoffs][5] (device fp64) =
 *   hit       [r_0 < K]
 *   recall    #{j : r_j < K} / m
 *   precision #{j : r_j < K} / K
 *   ndcg      sum_{r_j < K} 1/log2(r_j + 2)  /  sum_{i < min(m,K)} 1/log2(i + 2)
 *   map       sum_{r_j < K} (j + 1)/(r_j + 1)  /  min(m, K)
 * and per_user_free [n_users][2] = mrr 1/(r_0 + 1), auc (1/m) sum_j (1 - (r_j -
 * j)/n_neg); a user with m = 0 gets zeros.  mean_cut [n_cutoffs][5] and
 * mean_free [2]: the means over the users with m > 0 (zeros when there is
 * none); n_scored (device int64): their number.  Pure functions of the integer
 * positions; they assume that every test item is a candidate and that a list
 * holds no item twice (then r_j - j is the number of non-test candidates ahead
 * of the item).  Every sum is taken in a fixed order (no float atomics): equal
 * inputs give equal bits.  Asynchronous on `stream`. */
int acf_eval_rank_metrics(const int32_t* positions, const int64_t* test_off, int32_t n_users,
                          const int32_t* n_neg, const int32_t* cutoffs, int32_t n_cutoffs,
                          double* per_user, double* per_user_free, double* mean_cut, double* mean_free,
                          int64_t* n_scored, void* stream);

/* ---- list-level robustness: how far two sets of top-K lists differ, and what
 * lists do to the items (no reference counterpart).
 * A list array is device int32 [n][k], row-major, 1 <= k <= 128, in the form
 * acf_recommend_topk writes: ids >= 0 first, then -1.  A negative entry is
 * "none" wherever it stands and matches nothing.  A row that holds an id twice
 * gives unspecified values for that row (every loop stays in bounds and ends).
 * cutoffs: a HOST array of 1 <= n_cutoffs <= 8 values K with 1 <= K <= k.
 * Everything is asynchronous on `stream`; NULL pointers, k outside [1, 128], a
 * bad cutoff, p outside (0, 1) and a short or misaligned workspace are
 * ACF_E_INVALID before any launch.
 *
 * acf_list_compare: per row r and cutoff K, with la, lb the numbers of valid ids
 * in the whole rows A[r], B[r], D = min(K, max(la, lb)) and X_d (d = 1..D) the
 * number of ids that occur in both A[r][0..d) and B[r][0..d), per_user
 * [n][n_cutoffs][3] (device fp64) =
 *   overlap  X_D (an exact integer)
 *   jaccard  X_D / (min(la, D) + min(lb, D) - X_D)
 *   rbo      (X_D / D) p^D + ((1 - p) / p) sum_{d=1..D} (X_d / d) p^d
 * the last the extrapolated rank-biased overlap, 0 < p < 1, summed over d
 * ascending in fp64 by one thread, p^d by repeated multiplication, every
 * operation rounded on its own.  The X_d are integers (a histogram of the depth
 * max(i, j) at which a shared id is in both prefixes, prefix-summed), so
 * overlap and jaccard have exactly one right answer.  jaccard at K = 1 is "the
 * top item is unchanged".  A row with D = 0 (both lists empty) writes zeros and
 * is not scored.  mean [n_cutoffs][3]: the means over the scored rows, summed
 * in a fixed order with no float atomics (zeros when no row is scored);
 * n_scored: device int64 [n_cutoffs].  Equal inputs give equal bits.  n = 0
 * writes the zero means only.
 *
 * acf_list_exposure: counts (device int32 [n_cutoffs][num_items]) is zeroed by
 * the call, then counts[c][i] = #{(r, x) : x < K_c, lists[r][x] = i}; entries
 * outside [0, num_items) are ignored.  n * k < 2^31.  Integer atomics only, equal
 * ids combined inside a wave first: exact whatever the order.
 *
 * acf_exposure_metrics: with c_i = counts[c][i], N = num_items and T = sum c_i,
 * out [n_cutoffs][6] (device fp64) =
 *   total     T
 *   coverage  #{c_i > 0} / N
 *   gini      G / (N T), G = sum_{j=1..N} (2j - N - 1) c_(j) over the counts
 *             sorted ascending
 *   entropy   - sum_{c_i > 0} (c_i / T) log2(c_i / T)
 *   arp       (sum c_i pop_i) / T     (pop NULL: 0)
 *   aplt      (sum_{tail_i != 0} c_i) / T   (tail NULL: 0)
 * pop: device int32 [num_items] or NULL, each item's number of training
 * interactions; tail: device uint8 [num_items] or NULL, nonzero for a long-tail
 * item.  T, the covered items, G and both numerators are exact int64 (the
 * caller guarantees N T < 2^63), each converted to fp64 once, so coverage,
 * gini, arp and aplt are one fp64 division of two integers; the entropy is
 * summed in fp64 in an order fixed by N alone.  T = 0 gives a row of zeros.
 * `workspace`: device memory, 8-byte aligned, at least
 * acf_exposure_metrics_workspace(num_items, n_cutoffs) bytes (the sorted counts
 * and the partial sums) -- a host-only query that touches no device;
 * ACF_E_INVALID on a NULL out pointer, num_items < 1 or n_cutoffs outside
 * [1, 8].  The radix sort's own temporary storage comes from the stream's
 * allocator. */
int acf_list_compare(const int32_t* A, const int32_t* B, int32_t n, int32_t k, const int32_t* cutoffs,
                     int32_t n_cutoffs, double p, double* per_user, double* mean, int64_t* n_scored,
                     void* stream);
int acf_list_exposure(const int32_t* lists, int32_t n, int32_t k, int32_t num_items, const int32_t* cutoffs,
                      int32_t n_cutoffs, int32_t* counts, void* stream);
int acf_exposure_metrics_workspace(int32_t num_items, int32_t n_cutoffs, size_t* bytes);
int acf_exposure_metrics(const int32_t* counts, int32_t num_items, int32_t n_cutoffs, const int32_t* pop,
                         const uint8_t* tail, double* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- diversity: intra-list similarity and MMR re-ranking (no reference
 * counterpart).  T: device fp32 [num_rows][dim], dim as
 * the ranking calls take it.  sim(a, b) of two rows is acf_neighbors_topk's
 * score under `metric` (0 dot, 1 cosine, 2 minus the squared Euclidean
 * distance), from the same device functions: fp32, every operation rounded on
 * its own, s = the sequential round-then-add dot product; cosine is den > 0 ?
 * s / den + 0.0f : +0.0f with den = sqrtf(s_aa) * sqrtf(s_bb); sim is symmetric
 * bit for bit and never -0.0.  An id >= num_rows anywhere in `lists` / `cand` is
 * read as row 0; with check != 0 the call then synchronises once, after its
 * launches, and returns ACF_E_RANGE (check == 0: no error, no sync).  A negative
 * id is "none" wherever it stands.  dim, metric, m, k, k_out, the cutoffs or lam
 * out of range and NULL pointers are ACF_E_INVALID before any launch; n = 0
 * returns at once and writes nothing.  Both calls are asynchronous on `stream`
 * (the error word and the flags come from the stream's allocator), use no float
 * atomics, and give every row a result that depends on that row alone: equal
 * inputs give equal bits.  Tables are assumed finite.
 *
 * acf_list_similarity: lists device int32 [n][k], 1 <= k <= 128; cutoffs: a HOST
 * array of 1 <= n_cutoffs <= 8 values K in [1, k].  For row r, position b holding
 * a valid id has c_b = sum over the valid positions a < b, a ascending from
 * +0.0, of (double)sim(T[id_a], T[id_b]); repeated ids are separate entries.  With
 * L the number of valid positions among the first K and S_K the sum of their
 * c_b, b ascending from +0.0, ils[r][K] = S_K / (double)(L (L - 1) / 2) (device
 * fp64 [n][n_cutoffs]), and 0.0 where L < 2.  means [n_cutoffs]: per cutoff the
 * mean over the rows with L >= 2 (0.0 when there is none): thread t of 256 adds
 * rows t, t + 256, ... ascending, a fixed halving tree adds the 256 sums, one
 * division by the number of rows.
 *
 * acf_rerank_mmr: cand device int32 [n][m], rel device fp32 [n][m], 1 <= m <=
 * 128, 1 <= k_out <= m, 0 <= lam <= 1.  Position c is valid iff cand >= 0 and rel
 * is finite.  a_c = lam * rel_c; oml = 1.0f - lam (host, once).  Step 0 picks the
 * valid position with the largest a_c; step j >= 1 the unpicked valid position
 * with the largest a_c - oml * pen_c (two products and a subtraction, each
 * rounded), where pen_c = sim(T[cand_c], T[cand_s]) for the first pick s and
 * fmaxf(pen_c, that) for every later one (no sim is -0.0, so no pen is).  Equal
 * values (-0 and +0 are equal) go to the lower position.  Step j writes items[r][j] = cand as given, rel_out =
 * its rel, obj = the value it was picked at; once the valid positions run out the
 * tail is -1 / -inf / -inf. */
int acf_list_similarity(const float* T, int64_t num_rows, int32_t dim, const int32_t* lists, int32_t n, int32_t k,
                        const int32_t* cutoffs, int32_t n_cutoffs, int32_t metric, double* ils, double* means,
                        int32_t check, void* stream);
int acf_rerank_mmr(const float* T, int64_t num_rows, int32_t dim, const int32_t* cand, const float* rel, int32_t n,
                   int32_t m, int32_t k_out, float lam, int32_t metric, int32_t* items, float* rel_out, float* obj,
                   int32_t check, void* stream);

/* ---- certified ranking robustness: worst-case positions under an eps attack --
 * (no reference counterpart.)  Entry r (row users[r] of P; any order, repeats
 * allowed) has the test item t = test_items[r] and the candidates C_r =
 * [0, num_candidates) minus the SET of excl_items[excl_off[r] .. excl_off[r+1])
 * -- unsorted, repeated and out-of-range entries (-1 included) are fine;
 * excl_off = excl_items = NULL excludes nothing; t itself never counts,
 * excluded or not, exactly as for acf_eval_positions_multi.  With s_x the
 * evaluation's sequential round-then-add dot product of P[users[r]] and Q[x]
 * and m_c = s_t - s_c (one rounded fp32 subtraction),
 *   worst[e * n_users + r] = #{ c in C_r, c != t : m_c <= thr_e(c) }
 *   side 0 (user): the attacker adds any delta with |delta|_2 <= eps_e to the
 *     user row.  thr_e(c) = eps_e * D_c, D_c = sqrtf(D2), D2 = the sum over k
 *     ascending from +0.0 of round((Q[t][k] - Q[c][k])^2): identical rows give 0.
 *   side 1 (item): the attacker adds to EVERY item row its own delta with
 *     |delta|_2 <= eps_e.  thr_e = (2 eps_e) * Np, Np = sqrtf(N2), N2 = the same
 *     chain over P[users[r]][k]^2.
 * All of it fp32, every operation rounded on its own, the square roots
 * correctly rounded.  Candidate c can be brought to score >= t within the
 * budget iff its inequality holds, and one perturbation has to satisfy the
 * inequality of every candidate it lifts, so no perturbation within the budget
 * puts more than worst candidates at or above t: worst < K certifies t in the
 * top K, and a metric that does not increase with the position, taken at
 * worst, is a lower bound under every such attack.  eps = 0 gives
 * acf_eval_positions_multi's positions; both thresholds grow with eps, so worst
 * does not decrease in eps.  A count depends on (u, t, C_r, P, Q, eps_e) only.
 * eps: a HOST array of 1 <= n_eps <= 8 finite values >= 0; the candidates are
 * swept once whatever n_eps.  Exact integers, identical bits run to run; no
 * [n_users, num_candidates] array is formed.  `worst`: device int32
 * [n_eps][n_users].  `workspace`: device memory, 4-byte aligned, at least
 * acf_eval_positions_worst_workspace(n_users, num_candidates, n_eps) bytes -- a
 * host-only query that touches no device; a smaller one is ACF_E_INVALID, as
 * are n_eps outside [1, 8], a negative or non-finite eps and a side other than
 * 0 or 1, all before any launch.  1 <= num_candidates <= num_item_rows;
 * n_users = 0 does nothing.  A user outside [0, num_user_rows) or a test item
 * outside [0, num_item_rows) is read as row 0; with check != 0 the call then
 * synchronises once, after its launches, and returns ACF_E_RANGE (check == 0:
 * no error, no sync).  Tables are assumed finite. */
int acf_eval_positions_worst_workspace(int32_t n_users, int32_t num_candidates, int32_t n_eps, size_t* bytes);
int acf_eval_positions_worst(const float* P, const float* Q, int64_t num_user_rows, int64_t num_item_rows,
                             int32_t dim, const int32_t* users, const int32_t* test_items, int32_t n_users,
                             int32_t num_candidates, const int64_t* excl_off, const int32_t* excl_items,
                             const float* eps, int32_t n_eps, int32_t side, int32_t* worst, void* workspace,
                             size_t workspace_bytes, int32_t check, void* stream);

/* ---- certified radius: the largest eps each entry's top-K hit survives --------
 * (no reference counterpart.)  Entries, candidates C_r, exclusions and the test
 * item are acf_eval_positions_worst's, and so are the fp32 values m_c, D_c and
 * Np, bit for bit.  For candidate c, eps_c is the smallest finite fp32 eps >= 0
 * at which acf_eval_positions_worst's predicate holds as that kernel evaluates
 * it,
 *   side 0 (user): m_c <= fl(eps * D_c)
 *   side 1 (item): m_c <= fl(fl(2 eps) * Np)
 * and +inf when no finite eps satisfies it (m_c > 0 with D_c or Np equal to 0).
 * Both products do not decrease in eps, so the minimum exists and is exact (a
 * quotient fl(m / D) would be off by a few ulps either way); m_c <= 0 gives 0.
 * Per entry r the call returns the k smallest (eps_c, c) over c in C_r, c != t:
 *   eps_out[r * k + j] ascending, ties to the lower item id, items_out[r * k + j]
 * their items, padded with +inf / -1 when the entry has fewer than k candidates.
 * eps_out[r * k + j] is the certified radius at j + 1: for every finite eps >= 0
 *   worst_eps[r] < j + 1  <=>  eps < eps_out[r * k + j]
 * with acf_eval_positions_worst's integers, so no perturbation within a smaller
 * budget pushes t out of the top j + 1, and the number of zeros in the row is
 * min(k, acf_eval_positions_multi's position of t).  items_out are the
 * candidates that break the certificate first.  One sweep of the candidates
 * whatever k; exact, identical bits run to run; no [n_users, num_candidates]
 * array is formed.  eps_out: device float [n_users][k]; items_out: device int32
 * [n_users][k].  `workspace`: device memory, 8-byte aligned, at least
 * acf_eval_radius_workspace(n_users, num_candidates, k) bytes -- a host-only
 * query that touches no device; a smaller or misaligned one is ACF_E_INVALID, as
 * are k outside [1, 128], a side other than 0 or 1, num_candidates outside [1,
 * num_item_rows] and a NULL argument (excl_off = excl_items = NULL excludes
 * nothing), all before any launch.  n_users = 0 does nothing.  A user outside
 * [0, num_user_rows) or a test item outside [0, num_item_rows) is read as row
 * 0; with check != 0 the call then synchronises once, after its launches, and
 * returns ACF_E_RANGE (check == 0: no error, no sync).  Tables are assumed
 * finite. */
int acf_eval_radius_workspace(int32_t n_users, int32_t num_candidates, int32_t k, size_t* bytes);
int acf_eval_radius(const float* P, const float* Q, int64_t num_user_rows, int64_t num_item_rows, int32_t dim,
                    const int32_t* users, const int32_t* test_items, int32_t n_users, int32_t num_candidates,
                    const int64_t* excl_off, const int32_t* excl_items, int32_t k, int32_t side, float* eps_out,
                    int32_t* items_out, void* workspace, size_t workspace_bytes, int32_t check, void* stream);

/* ---- robustness evaluation: a whole-stream adversarial direction ------------
 * utils.py:145-154 (adv_update): ONE delta over all n triplets as one batch, as
 * dense tables.  acf_adv_direction fills EVERY row of the unit-direction tables
 * nP [num_user_rows, dim] and nQ [num_item_rows, dim]; acf_adv_apply turns a
 * direction into delta = N * eps and W + delta, so one direction serves every
 * eps.  No context; P, Q and the accumulators are never written; everything runs
 * on `stream`; the only scratch is `workspace` (device memory, 16-byte aligned,
 * at least acf_adv_direction_workspace(n, ...) bytes -- a host-only query; a
 * smaller one is ACF_E_INVALID).  0 <= n < 2^29, no multiple-of-anything rule.
 *  adv_mode 0 ("grad", APR.py:180-191): g = d/d(P,Q) sum_t softplus(-clip(x+_t -
 *    x-_t)), the clean loss only; scores are the evaluation's sequential dot
 *    product, the clip mask and softplus those of the step.  A row is
 *    g_row * rsqrt(max(|g_row|^2, 1e-12)); a row no triplet touches is +0.0; n = 0
 *    gives all-zero tables.  A row's terms are added in a fixed order: the pos
 *    branch's terms in triplet order, then the neg branch's (the reference's
 *    IndexedSlices concat order); rows of more than 256 terms as partial sums of
 *    256 consecutive terms added in order.  Two calls on the same inputs give the
 *    same bits; no float atomics.
 *  adv_mode 1 ("random", APR.py:170-177): every row of both tables is the
 *    l2-normalised truncated-normal draw the step's random mode makes for
 *    (seed, call, t, table, row); the triplets are not read (may be NULL).
 * check != 0: the call synchronises after its first kernel and returns
 * ACF_E_RANGE when an index is outside its table, before anything is built on
 * it (check == 0: such an index is read as row 0, no error).
 * acf_adv_apply: delta_out = N * eps, sum_out = W + delta_out, two separately
 * rounded fp32 operations (TF: l2_normalize(...) * eps, then embedding + delta);
 * either output may be NULL (W may be NULL when sum_out is). */
int acf_adv_direction_workspace(int64_t n, int64_t num_user_rows, int64_t num_item_rows, int32_t dim,
                                size_t* bytes);
int acf_adv_direction(const float* P, const float* Q, int64_t num_user_rows, int64_t num_item_rows,
                      int32_t dim, const int32_t* user, const int32_t* item_pos, const int32_t* item_neg,
                      int64_t n, float clip_lo, float clip_hi, int32_t adv_mode, uint64_t seed, uint32_t call,
                      int32_t t, float* nP, float* nQ, void* workspace, size_t workspace_bytes, int32_t check,
                      void* stream);
int acf_adv_apply(const float* W, const float* N, int64_t rows, int32_t dim, float eps, float* delta_out,
                  float* sum_out, void* stream);

/* ---- robustness evaluation: a kept plan, the planned direction, an iterated attack
 * (no reference counterpart).  As above: no context, P and Q
 * never written, everything on `stream`, no float atomics, every size from a
 * host-only query, buffers 16-byte aligned, a short one is ACF_E_INVALID.
 * acf_adv_plan: everything of acf_adv_direction's grad mode that depends on the
 *   triplets alone -- the 4n term values sorted stably by row, the row offsets and
 *   the range-error word -- written to the caller's `plan` (device memory of
 *   plan_bytes from acf_adv_plan_workspace, which also gives the call's scratch
 *   `workspace` size).  The tables are not read, so one plan serves every (P, Q)
 *   of num_user_rows x num_item_rows; it is valid for exactly the (user, item_pos,
 *   item_neg, n, num_user_rows, num_item_rows) it was built from.  check as in
 *   acf_adv_direction (one sync after the first kernel).
 * acf_adv_direction_planned: nP, nQ of acf_adv_direction's grad mode, the same
 *   bits, from a plan and the same triplets: coefficients, term records, chunk
 *   sums, combine; no sort.  workspace: acf_adv_direction_workspace(n, ...) bytes.
 *   loss_out (device, may be NULL): the stream's clean loss sum_t softplus(-clip(x_t))
 *   at (P, Q), each fp32 term widened to fp64 and added in a fixed order (a tree over
 *   the 256 triplets of a block, then blocks b, b + 256, ... per lane and the same
 *   tree): the same bits every run.  Never synchronises.
 * acf_adv_pgd: `iters` projected gradient steps.  delta_0 = (dP0, dQ0) (NULL:
 *   zeros; taken as given, not projected); for k = 0..iters-1: (nP, nQ) = the
 *   planned direction at (P + dP_k, Q + dQ_k), and on every moving side, per row,
 *   v = delta_k + alpha * n (two rounded operations), s = |v|_2 in fp32 (per-lane
 *   sums of rounded squares over the row's float4 chunks lane, lane + LPR, ..., then
 *   the row-group's butterfly: xor 1, 2, 4, 8, 16, 32), delta_{k+1} = v if s <= eps
 *   else v * (eps / s) (one division per row), P + delta_{k+1} one rounded add.
 *   side: ACF_ADV_SIDE_BOTH, _USER (dQ stays dQ0) or _ITEM (dP stays dP0); both
 *   tables always enter the gradient.  dP, dQ: the final delta tables (may alias
 *   dP0, dQ0); loss (device, fp64 [iters + 1]): loss[k] the clean loss at iterate k,
 *   loss[iters] from one more coefficient pass.  plan: NULL (the call plans once in
 *   its workspace) or an acf_adv_plan of the same triplets; with check != 0 the
 *   call synchronises once and returns ACF_E_RANGE when the plan's error word is
 *   set.  n = 0: every moving row is projected once, loss is all zero.
 *   ACF_E_INVALID before any launch: iters outside [1, ACF_ADV_PGD_MAX_ITERS], eps
 *   or alpha negative or not finite, an unknown side, a short workspace or plan. */
#define ACF_ADV_PGD_MAX_ITERS 1024
#define ACF_ADV_SIDE_BOTH 0
#define ACF_ADV_SIDE_USER 1
#define ACF_ADV_SIDE_ITEM 2
int acf_adv_plan_workspace(int64_t n, int64_t num_user_rows, int64_t num_item_rows, size_t* plan_bytes,
                           size_t* bytes);
int acf_adv_plan(const int32_t* user, const int32_t* item_pos, const int32_t* item_neg, int64_t n,
                 int64_t num_user_rows, int64_t num_item_rows, void* plan, size_t plan_bytes, void* workspace,
                 size_t workspace_bytes, int32_t check, void* stream);
int acf_adv_direction_planned(const float* P, const float* Q, int64_t num_user_rows, int64_t num_item_rows,
                              int32_t dim, const int32_t* user, const int32_t* item_pos, const int32_t* item_neg,
                              int64_t n, float clip_lo, float clip_hi, const void* plan, size_t plan_bytes,
                              float* nP, float* nQ, double* loss_out, void* workspace, size_t workspace_bytes,
                              void* stream);
int acf_adv_pgd_workspace(int64_t n, int64_t num_user_rows, int64_t num_item_rows, int32_t dim, size_t* bytes);
int acf_adv_pgd(const float* P, const float* Q, int64_t num_user_rows, int64_t num_item_rows, int32_t dim,
                const int32_t* user, const int32_t* item_pos, const int32_t* item_neg, int64_t n, float clip_lo,
                float clip_hi, const void* plan, size_t plan_bytes, float eps, float alpha, int32_t iters,
                int32_t side, const float* dP0, const float* dQ0, float* dP, float* dQ, double* loss,
                void* workspace, size_t workspace_bytes, int32_t check, void* stream);

/* ---- fold-in: new users against a frozen item table --------------------------
 * (no reference counterpart: the reference can only retrain.)  User r of the CSR
 * user_off int64 [n + 1] / item_pos [T] gets a row fitted to its list while Q
 * stays fixed.  For epoch e = 0..epochs-1 and every consecutive slice of at most
 * `batch` positions of [user_off[r], user_off[r+1]) (the last one may be short;
 * the same order every epoch) the user takes ONE training_batch iteration
 * (APR.py:143-195) on the one-row user table [p_r] and Q with the batch
 * {(0, item_pos[k], item_neg[e*T + k])}; only p_r and its Adagrad accumulator are
 * kept.  With hp->adver the delta is the step's own: delta_p from the slice's
 * summed clean gradient of p_r, delta_q per item row of the slice from its clean
 * gradient summed over all the row's occurrences in the slice (pos branch, then
 * neg branch, triplet order), both l2-normalised with the 1e-12 floor; reg acts
 * on p_r as in the step (2*reg/(B_slice*dim), twice when adversarial).
 * hp->adv_mode != 0 or hp->zero_delta != 0 is ACF_E_INVALID.
 *   init, acc_init [n, dim]: starting rows / accumulators (NULL: zeros / 0.1);
 *   P_new, acc_new [n, dim]: the fitted rows and accumulators (pass them back as
 *     init / acc_init to continue when a list grows);
 *   loss [epochs, n] (may be NULL): the clean loss summed over the user's slices
 *     of that epoch, each slice before its own update.
 * A user with an empty list keeps its inits and has loss 0; epochs = 0 copies the
 * inits.  A user's outputs depend on that user's inputs only and are the same
 * bits in every call (no float atomics, fixed summation orders).  Q is never
 * written; no workspace.  1 <= batch <= ACF_FOLD_MAX_BATCH.  user_off must be
 * non-decreasing within [0, T] (offsets outside are clamped).
 * check != 0: the call first synchronises and returns ACF_E_RANGE when an item is
 * outside [0, num_item_rows), before anything is written (check == 0: such an
 * item is read as row 0). */
#define ACF_FOLD_MAX_BATCH 512
int acf_fold_in_users(const float* Q, int64_t num_item_rows, int32_t dim, const int64_t* user_off,
                      int64_t n_users, const int32_t* item_pos, const int32_t* item_neg, int64_t T,
                      int32_t epochs, int32_t batch, const acf_apr_hparams* hp, const float* init,
                      const float* acc_init, float* P_new, float* acc_new, float* loss, int32_t check,
                      void* stream);

/* ---- fold-in: new items against frozen user and item tables -------------------
 * (no reference counterpart.)  New item r of the CSR item_off int64 [n + 1] /
 * user_pos [T] gets a row fitted to the users who interacted with it while P and
 * Q stay fixed.  For epoch e = 0..epochs-1 and every consecutive slice of at most
 * `batch` positions of [item_off[r], item_off[r+1]) (the last one may be short;
 * the same order every epoch) the item takes ONE training_batch iteration
 * (APR.py:143-195) on the tables P and [Q ; q_r] -- q_r appended as row
 * num_item_rows -- with the batch {(user_pos[k], num_item_rows, item_neg[e*T + k])};
 * only q_r and its Adagrad accumulator are kept.  A negative lies in
 * [0, num_item_rows), so it can never equal the new item.  With hp->adver the
 * delta is the step's own: delta_q from the slice's summed clean gradient of q_r;
 * per user row of the slice from its clean gradient summed over all the row's
 * occurrences in the slice (pos branch g * q_r, then neg branch -g * q_j, triplet
 * order); per negative row likewise (-g * p_u, triplet order); all l2-normalised
 * with the 1e-12 floor.  reg acts on q_r as in the step on the extended tables
 * (2*reg/(B_slice*dim) per occurrence, twice when adversarial).
 * hp->adv_mode != 0 or hp->zero_delta != 0 is ACF_E_INVALID.
 *   init, acc_init [n, dim]: starting rows / accumulators (NULL: zeros / 0.1);
 *   Q_new, acc_new [n, dim]: the fitted rows and accumulators (pass them back as
 *     init / acc_init to continue when a list grows);
 *   loss [epochs, n] (may be NULL): the clean loss summed over the item's slices
 *     of that epoch, each slice before its own update.
 * An item with an empty list keeps its inits and has loss 0; epochs = 0 copies the
 * inits.  An item's outputs depend on that item's inputs only and are the same
 * bits in every call (no float atomics, fixed summation orders).  P and Q are
 * never written; no workspace.  1 <= batch <= ACF_FOLD_MAX_BATCH.
 * num_user_rows <= 2^31, num_item_rows < 2^31.  item_off must be non-decreasing
 * within [0, T] (offsets outside are clamped).
 * check != 0: the call first synchronises and returns ACF_E_RANGE when a user is
 * outside [0, num_user_rows) or a negative outside [0, num_item_rows), before
 * anything is written (check == 0: such an index is read as row 0). */
int acf_fold_in_items(const float* P, int64_t num_user_rows, const float* Q, int64_t num_item_rows, int32_t dim,
                      const int64_t* item_off, int64_t n_items, const int32_t* user_pos, const int32_t* item_neg,
                      int64_t T, int32_t epochs, int32_t batch, const acf_apr_hparams* hp,
                      const float* init, const float* acc_init, float* Q_new, float* acc_new, float* loss,
                      int32_t check, void* stream);

/* ---- grid training: M models over one triplet stream in one call --------------
 * (the reference sweeps eps, reg_adv and d as one job per point; DESIGN.md
 * section 4m.)  training_batch (utils.py:106-119, dns == 1) for n_batches
 * consecutive batches of the shared triplets, for n_models members at once.
 * Member m owns slice m of P, accP [M][num_user_rows][dim] and Q, accQ
 * [M][num_item_rows][dim] (contiguous, member-major: a slice is an ordinary dense
 * table for every other entry point) and trains under hp[m] (a HOST array of M):
 * lr, eps, reg, reg_adv, adver, clip_lo, clip_hi.  Members with adver = 0 (BPR:
 * no delta and no adversarial term at all) and adver = 1 may share a grid; reg acts
 * per occurrence, twice when adversarial, as in the step.  adv_mode != 0 (the
 * random delta is keyed on a context's call counter) and zero_delta != 0 are
 * ACF_E_INVALID.  dim: a multiple of 4 in [4, 256]; 1 <= n_models <=
 * ACF_GRID_MAX_MODELS; 1 <= batch_size <= ACF_GRID_MAX_BATCH; num_user_rows +
 * num_item_rows <= 2^31.  No context: the plan and all scratch live in `workspace`
 * (device memory, 16-byte aligned, at least acf_apr_grid_workspace(...) bytes -- a
 * host-only query).  Asynchronous on `stream`; the call never synchronises unless
 * check != 0.
 *   Plan: built once per call from the triplets alone and read by all members: per
 *   batch the unique user and item rows and per row its terms in a fixed order, the
 *   pos branch's terms in triplet order, then the neg branch's (acf_adv_direction's
 *   order); a row of more than 256 terms is summed as partial sums of 256
 *   consecutive terms, added in order.
 *   Schedule: per batch three launches with (member, unique row) as the grid: the
 *   clean gradient and delta, the adversarial sum, Adagrad.  No float atomics.
 *   loss_clean, loss_adv [M][n_batches * batch_size] (may be NULL): the per-triplet
 *   losses of every member, each batch before its own update; loss_adv of a member
 *   with adver = 0 is not written.
 * Guarantees.  A member's outputs depend on that member's tables, its hp and the
 * triplets only: they are the same bits whatever n_models is and whichever position
 * the member has.  Two calls on equal inputs give equal bits.  One call of n batches
 * equals n calls of one batch.  The results are NOT bit-identical to acf_apr_train,
 * whose summation order depends on its team geometry; they agree with it at the
 * oracle's tolerance.
 * Errors.  ACF_E_INVALID before any launch: a NULL pointer, n_models, dim,
 * batch_size or n_batches out of range, a short or misaligned workspace, an
 * unsupported hp field.  check != 0: the call synchronises once after the plan
 * kernel and returns ACF_E_RANGE when an index is outside its table, before any
 * table is written (check == 0: such an index is read as row 0).  n_batches = 0
 * does nothing. */
#define ACF_GRID_MAX_MODELS 64
#define ACF_GRID_MAX_BATCH 1024
int acf_apr_grid_workspace(int32_t n_models, int32_t batch_size, int32_t n_batches, int64_t num_user_rows,
                           int64_t num_item_rows, int32_t dim, size_t* bytes);
int acf_apr_grid_train(float* P, float* Q, float* accP, float* accQ, int32_t n_models, int64_t num_user_rows,
                       int64_t num_item_rows, int32_t dim, const acf_apr_hparams* hp, const int32_t* user,
                       const int32_t* item_pos, const int32_t* item_neg, int32_t batch_size, int32_t n_batches,
                       float* loss_clean, float* loss_adv, void* workspace, size_t workspace_bytes, int32_t check,
                       void* stream);

/* ---- grid training against a K-step inner attack ------------------------------
 * acf_apr_grid_train with, per member, a projected-gradient attack of adv_iters[m]
 * steps of size adv_step[m] in place of the one normalised gradient step (Madry-style
 * adversarial training inside APR's per-row L2 ball).  Per
 * member and batch, with K = adv_iters[m], alpha = adv_step[m], eps = hp[m].eps:
 *   delta_0 = 0 on every unique row of the batch; for k = 1 .. K:
 *     g_k = the batch's BPR-loss gradient of the row with the triplets' rows taken at
 *           (P + delta_{k-1}, Q + delta_{k-1}), summed in the plan's order as above;
 *     n_k = g_k * rsqrt(max(g_k . g_k, 1e-12));  v = delta_{k-1} + alpha * n_k (the
 *     product rounded, then the sum);  s = sqrt(v . v);  delta_k = v when s <= eps,
 *     else v * (eps / s)  (acf_adv_pgd's step).
 *   The step's gradient is acf_apr_grid_train's with delta = delta_K: the clean
 *   gradient at the unperturbed tables, the reg term, reg_adv times the gradient at
 *   delta_K; loss_adv is the per-triplet loss at delta_K.
 * A member with K = 1 is acf_apr_grid_train's member, the same bits (delta = eps *
 * l2norm(g_1); its adv_step is not read).  A member with adver = 0 has no delta; its
 * two fields are range-checked and otherwise ignored.  Both tables' deltas always
 * move.  adv_iters, adv_step: HOST arrays of n_models; 1 <= adv_iters[m] <=
 * ACF_GRID_MAX_ADV_ITERS, adv_step[m] finite and >= 0, else ACF_E_INVALID before any
 * launch, as is a NULL array.  Schedule: per batch the clean launch, max(K) - 1 inner
 * launches (a member whose K is reached does nothing in the later ones), the
 * adversarial launch, Adagrad.  workspace: acf_apr_grid_pgd_workspace(...) bytes,
 * acf_apr_grid_workspace's plus a second delta buffer of n_models * 3 * batch_size *
 * dim floats.  Everything else, the guarantees included (a member's bits do not
 * depend on n_models, its position or the other members' K), is acf_apr_grid_train's. */
#define ACF_GRID_MAX_ADV_ITERS 32
int acf_apr_grid_pgd_workspace(int32_t n_models, int32_t batch_size, int32_t n_batches, int64_t num_user_rows,
                               int64_t num_item_rows, int32_t dim, size_t* bytes);
int acf_apr_grid_train_pgd(float* P, float* Q, float* accP, float* accQ, int32_t n_models, int64_t num_user_rows,
                           int64_t num_item_rows, int32_t dim, const acf_apr_hparams* hp, const int32_t* adv_iters,
                           const float* adv_step, const int32_t* user, const int32_t* item_pos,
                           const int32_t* item_neg, int32_t batch_size, int32_t n_batches, float* loss_clean,
                           float* loss_adv, void* workspace, size_t workspace_bytes, int32_t check, void* stream);

/* ---- sampler: shuffle/_get_train_batch (APR.py:39-81) --------------------
 * Shuffles the n_pos positive pairs with a counter-based permutation of
 * `seed`, keeps floor(n_pos / batch_size) * batch_size of them (drop-last,
 * APR.py:52), and draws one negative per triplet uniformly from
 * [0, num_items), redrawn while it is in the user's list
 * list_items[list_off[u] .. list_off[u+1]) (sorted ascending; the
 * OriginalDataset.trainList of APR.py:77).  Writes out_user/out_pos/out_neg of
 * length n_out = floor(n_pos/batch_size)*batch_size.  Users with a full list
 * (no admissible negative) get -1 after max_tries draws; with check != 0 the
 * call synchronises and returns ACF_E_RANGE in that case. */
int acf_sample_epoch(const int32_t* pos_user, const int32_t* pos_item, int64_t n_pos,
                     int32_t batch_size, int32_t num_items, int32_t num_lists,
                     const int64_t* list_off, const int32_t* list_items,
                     uint64_t seed, int32_t max_tries, int32_t check,
                     int32_t* out_user, int32_t* out_pos, int32_t* out_neg,
                     void* stream);

/* acf_sample_epoch with the negatives proposed from an alias table instead of
 * uniformly (SURVEY §8(f)1, config 5's on-GPU alias sampler): column k of the
 * table (prob, alias: DEVICE arrays of num_items) keeps k with probability
 * prob[k], else yields alias[k]; the proposal is then accepted or redrawn by
 * the same trainList rule (APR.py:76-78).  A table of equal weights is the
 * reference's uniform sampler. */
int acf_sample_epoch_alias(const int32_t* pos_user, const int32_t* pos_item, int64_t n_pos,
                           int32_t batch_size, int32_t num_items, int32_t num_lists,
                           const int64_t* list_off, const int32_t* list_items,
                           const float* prob, const int32_t* alias, uint64_t seed,
                           int32_t max_tries, int32_t check, int32_t* out_user,
                           int32_t* out_pos, int32_t* out_neg, void* stream);

/* Builds an alias table (Vose) for sampling k with probability w[k] / sum(w).
 * HOST arrays: w [n] (>= 0, finite, not all 0) in; prob [n], alias [n] out.
 * Synchronous, deterministic. */
int acf_alias_build(const float* w, int64_t n, float* prob, int32_t* alias);

/* dns > 1 negative selection (utils.py:121-133): per triplet, the candidate of
 * cand[e*dns .. e*dns+dns) with the largest clean score P[user[e]].Q[c] (first
 * maximum wins, np.argmax). */
int acf_dns_select(const float* P, const float* Q, int64_t num_user_rows,
                   int64_t num_item_rows, int32_t dim, const int32_t* user,
                   const int32_t* cand, int64_t n, int32_t dns, int32_t* out_neg,
                   void* stream);

/* ---- the step decomposed into TF's ops (csrc/acf_ops.hip) ----------------
 * The fused step above is the training path; these expose its pieces one
 * kernel each, with TF's data flow, for callers that compose the step (the
 * PyTorch custom ops acf::gather_bpr_fwd_bwd, row_segment_sum, l2norm_perturb,
 * sparse_adagrad_apply) and for op-level tests.  All asynchronous on `stream`. */

/* The inference gathers + BPR loss of APR.py:121-150 and the gradient of the
 * loss w.r.t. the gathered rows, as TF's IndexedSlices (APR.py:183): for each of
 * n triplets, loss[b] = softplus(-clip(x_b)), x[b] = p.q_i - p.q_j, and
 *   P slices: p_idx = [u ; u],  p_val = [g*q_i ; -g*q_j]   ([2n], [2n, dim])
 *   Q slices: q_idx = [i ; j],  q_val = [g*p ; -g*p]
 * with g = d loss / d x (zero outside the clip range): pos-branch lookups
 * first, then neg-branch, each product rounded as TF's Mul. */
int acf_gather_bpr_fwd_bwd(const float* P, const float* Q, int64_t num_user_rows,
                           int64_t num_item_rows, int32_t dim, const int32_t* user,
                           const int32_t* item_pos, const int32_t* item_neg, int64_t n,
                           float clip_lo, float clip_hi, float* loss, float* x,
                           int32_t* p_idx, float* p_val, int32_t* q_idx, float* q_val,
                           void* stream);

/* IndexedSlices -> unique rows (unsorted_segment_sum behind APR.py:183-187 and
 * the optimizer's dedup, APR.py:195): the m (index, value-row) pairs become
 * *out_k <= m unique indices in ascending order (out_uniq), each with the
 * sequential sum of its value rows in input order (out_sum [m, dim], first
 * *out_k rows used) and their count.  Indices must lie in [0, num_rows).
 * out_k is a DEVICE int64.  workspace: acf_row_segment_sum_workspace(m). */
int acf_row_segment_sum_workspace(int64_t m, size_t* bytes);
int acf_row_segment_sum(const int32_t* idx, const float* vals, int64_t m, int32_t dim,
                        int64_t num_rows, void* workspace, size_t workspace_bytes,
                        int32_t* out_uniq, float* out_sum, int32_t* out_count,
                        int64_t* out_k, void* stream);

/* delta = eps * l2_normalize(g, 1) = eps * g * rsqrt(max(sum g^2, 1e-12)) for k
 * rows (APR.py:186-191). */
int acf_l2norm_perturb(const float* g, int64_t k, int32_t dim, float eps, float* out,
                       void* stream);

/* TF SparseApplyAdagrad on k UNIQUE rows idx of W / acc ([rows, dim]) with
 * gradient rows g [k, dim]: acc += g^2; W -= lr * g * rsqrt(acc) (APR.py:195). */
int acf_sparse_adagrad_apply(float* W, float* acc, int64_t rows, int32_t dim,
                             const int32_t* idx, const float* g, int64_t k, float lr,
                             void* stream);

#ifdef __cplusplus
}
#endif

#endif /* ACF_APR_H */
