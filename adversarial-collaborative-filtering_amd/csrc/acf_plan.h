// acf_plan.h — what the plan (acf_plan.hip) writes and the step (acf_apr.hip) reads, private to
// libacf_apr.so: the occurrence records and their bit layout, the hot lists, the training context
// whose buffers hold them, and the few host functions that cross between the two units.  Neither
// unit sees a kernel or a device function of the other.  After hip_runtime.h, acf_apr.h, acf_host.h.
#pragma once

#include <algorithm>
#include <cstring>
#include <deque>
#include <map>
#include <vector>

// For every unique row of batch t: where its current value lives when batch t
// starts ("src").  src = row (>= 0) when no earlier batch of the plan touches
// the row; otherwise src = ~((dt << kb) | k): the row was last updated dt >= 1
// batches earlier, in that batch's local slot k (kb = slot bits of the plan).
//  - the two-kernel step reads dt = 1 rows from W scratch of batch t-1 (the
//    flush to the table happens inside batch t's first kernel) and every other
//    row from the table (pend1);
//  - the streamed step (k_stream) reads any dt from that batch's row version.
// Plans with one lane-group per slot (packed) encode dt = 1 only (binary
// search of batch t-1); one-wave-per-slot plans encode every dt (k_prev_next).
// user local slot = g - ubs[t]; item local slot = nU(t) + g - ibs[t].
// info[g] = {row, src, occurrence count | NEXT (batch t+1 touches the row too),
//            CSR offset of the first occurrence}.
#define ACF_INFO_NEXT (1 << 30)

__device__ __forceinline__ int32_t src_dt(int32_t src, int kb) {
  return src < 0 ? (int32_t)((uint32_t)(~src) >> kb) : 0;
}
__device__ __forceinline__ int32_t src_slot(int32_t src, int kb) { return (~src) & ((1 << kb) - 1); }
__device__ __forceinline__ int32_t make_src(int32_t dt, int32_t k, int kb) { return ~((dt << kb) | k); }

// src names W scratch of batch t-1 (not an older batch, not the table)
__device__ __forceinline__ bool pend1(int32_t src, int kb) { return src_dt(src, kb) == 1; }

// Occurrence record: everything one lane-group needs to process one occurrence
// of a unique row, so that a step kernel reaches the partner rows after ONE
// dependent load.  Records are written in CSR order (all occurrences) and the
// first R of each slot are also inlined at [batch][slot][r] so the kernel finds
// them by address arithmetic alone.  `gen` tags the plan that wrote a record:
// inlined records of an older plan read as absent.
struct __align__(16) OccRec {
  int32_t own_row;  // the unique row this slot updates
  int32_t own_src;  // where its value lives at batch start (see k_prev_src)
  int32_t meta;     // occurrence count | ITEM_BIT for item slots
  int32_t ovf;      // CSR index of the slot's first occurrence
  int32_t e_role;   // user slot: triplet e; item slot: 2e + role (0 pos, 1 neg)
  int32_t pa_row;   // user slot: item i;  item slot: user u
  int32_t pb_row;   // user slot: item j;  item slot: the other item of the triplet
  int32_t pa_src;
  int32_t pb_src;
  int32_t pa_slot;  // local slot of pa in batch t (for its delta) | SOLO_BIT if pa occurs once
  int32_t pb_slot;
  int32_t gen;
};
// A partner row that occurs once in the batch ("solo"): its batch-summed clean
// gradient is this occurrence's own term, so a reader can form its delta itself
// (k_stream, solo_delta) instead of waiting for the partner's wave to publish it.
#define ACF_SOLO_BIT (1 << 30)
#define ACF_SLOT_MASK (ACF_SOLO_BIT - 1)
#define ACF_ITEM_BIT (1 << 28)
#define ACF_SINGLE_BIT (1 << 29)   // the slot's only occurrence is a fused triplet
#define ACF_INPLACE_BIT (1 << 30)  // the fused triplet writes this row to the table itself
#define ACF_COUNT_MASK ((1 << 28) - 1)

// Hot slots of packed (one lane-group per slot) plans.  A large batch of
// Zipf-popular items holds a few rows with thousands of occurrences (10M x 5M,
// B = 65,536: the top item ~4,000), and one lane-group would sum them one pass
// after another.  A non-fused slot with more than ACF_HOT_MIN occurrences is
// therefore split into pieces of consecutive occurrences (at least
// ACF_HOT_PIECE each, at most ACF_HOT_MAXP pieces); one wave sums a piece into
// hot_part, and k_hot_combine adds a slot's pieces in piece order (fixed order:
// deterministic bits).  Each plan appends a batch's hot slots and their pieces
// with atomics; the order of the lists changes nothing but which wave does what.
#ifndef ACF_HOT_MIN
#define ACF_HOT_MIN 8
#endif
#ifndef ACF_HOT_PIECE
#define ACF_HOT_PIECE 16
#endif
#define ACF_HOT_MAXP 256

__host__ __device__ __forceinline__ int32_t hot_pieces(int32_t count) {
  const int32_t np = (count + ACF_HOT_PIECE - 1) / ACF_HOT_PIECE;
  return np < ACF_HOT_MAXP ? np : ACF_HOT_MAXP;
}

// Per-batch capacity of the hot lists: slots with > ACF_HOT_MIN of a batch's
// 3B occurrences, and sum(ceil(count / ACF_HOT_PIECE)) <= 3B / ACF_HOT_PIECE + hot slots.
__host__ __forceinline__ int32_t hot_stride_for(int32_t B) { return 3 * B / (ACF_HOT_MIN + 1) + 1; }
__host__ __forceinline__ int32_t piece_stride_for(int32_t B) { return 3 * B / ACF_HOT_PIECE + hot_stride_for(B); }

struct HotLists {
  int4* list;       // [nb][hot_stride]   {slot, pieces, piece base, count}
  int4* piece;      // [nb][piece_stride] {slot, piece, pieces, piece base}
  int32_t* cnt;     // [nb] hot slots of the batch
  int32_t* pcnt;    // [nb] pieces of the batch
  int32_t* arrive;  // [nb][piece_stride] at a hot slot's piece base: its pieces stored so far
                    // (triplet-centric combine: the slot's combine waits for all of them)
  int2* paux;       // [nb][piece_stride] beside each piece: {slot count, local CSR base | item << 31}
  int32_t hot_stride, piece_stride;
};

// ---------------------------------------------------------------------------
// Diagnostic build only (-DACF_DIAG, libacf_apr_diag.so): per-wave
// s_memrealtime stamps (100 MHz) to locate latency inside the step kernels.
// The product library compiles every STAMP() to nothing.
// The stamp words are per translation unit (no relocatable device code): each
// unit that stamps has a setter, and acf_diag_set_stamps calls them all.
// ---------------------------------------------------------------------------
#ifdef ACF_DIAG
static __device__ uint64_t* g_stamps = nullptr;
static __device__ int g_stamp_launch = 0;
static __device__ int g_stamp_cap = 0;
#define STAMP(launch, wave, i)                                                       \
  do {                                                                               \
    uint64_t t_;                                                                     \
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory"); \
    if (g_stamps && (threadIdx.x & 63) == 0 && (wave) < g_stamp_cap)                 \
      g_stamps[((int64_t)(launch) * g_stamp_cap + (wave)) * 8 + (i)] = t_;          \
  } while (0)
#define CLOCKSTAMP(launch, wave, i)                                                  \
  do {                                                                               \
    uint64_t t_;                                                                     \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");     \
    if (g_stamps && (threadIdx.x & 63) == 0 && (wave) < g_stamp_cap)                 \
      g_stamps[((int64_t)(launch) * g_stamp_cap + (wave)) * 8 + (i)] = t_;          \
  } while (0)
#else
#define CLOCKSTAMP(launch, wave, i) \
  do {                              \
  } while (0)
#define STAMP(launch, wave, i) \
  do {                         \
  } while (0)
#endif

// ---------------------------------------------------------------------------
// host side: the training context
// ---------------------------------------------------------------------------
#define ACF_PACKED_MIN_BATCH 4096  // auto slot mapping: packed from this batch size
#define ACF_SPIN_LIMIT (1 << 16)  // default version polls before a k_stream wait gives up
#define ACF_POLL_SLEEP 2  // default s_sleep between version polls: what the default k_stream instance has folded in

struct GraphKey {
  const void* ptrs[4];
  acf_apr_hparams hp;
  int32_t first, n, B, d, mapping, fusion, stream;  // stream: the context's k_stream switch
  bool operator<(const GraphKey& o) const { return memcmp(this, &o, sizeof(GraphKey)) < 0; }
};

// (r04) Verified streamed calls are checked lazily, without a host sync per
// call.  Each one is queued on its group's FIFO (the contexts that train the same
// tables on one stream: a PlanPipeline's two contexts share one group); its
// launch reports COMMIT / FAIL in the context's host-mapped status ring.  A
// failed call applied nothing and set the group's gate, so every later streamed
// launch of the group ran nothing either (and applied nothing).  acf_apr_resolve
// (and every entry point that needs settled tables or re-plans a context with a
// queued call) walks the FIFO: committed calls leave it; at the first failed one
// the gate is cleared and that call and every later queued call are replayed,
// in order, on the two-kernel schedule, which waits on nothing -- exact, as
// k_stream is bit-identical to it.  A context keeps its plan while it has a
// queued call (acf_apr_plan resolves the context's calls first).
struct acf_apr_ctx;
struct Pending {
  acf_apr_ctx* c;
  uint32_t seq;
  int32_t first, n;
  acf_apr_tables tb;
  acf_apr_hparams hp;
  hipStream_t s;
};
struct FailGroup {
  int32_t* gate = nullptr;  // device word, see StepArgs.gate
  std::deque<Pending> q;
  int refs = 0;
};

struct acf_apr_ctx {
  int64_t U1 = 0, I1 = 0;
  int32_t d = 0, maxB = 0, maxNB = 0, lpr = 0, nv = 0, R = 0;
  int64_t maxE = 0;
  // plan
  uint64_t *key_in = nullptr, *key_out = nullptr;  // [E user keys | 2E item keys]
  int32_t *flag = nullptr, *inc = nullptr;
  int32_t *uuniq = nullptr, *uoff = nullptr, *ubs = nullptr;
  int32_t* tsl = nullptr;                    // [E][4] slots of each triplet's rows
  int32_t* tpos = nullptr;                   // [E][4] CSR positions of its occurrences
  int4 *uinfo = nullptr, *iinfo = nullptr;   // per unique row, see k_slot_info
  int32_t *iuniq = nullptr, *ioff = nullptr, *ibs = nullptr;
  OccRec* trec = nullptr;
  OccRec *urec = nullptr, *irec = nullptr, *inl = nullptr;
  int32_t *err = nullptr, *gen_dev = nullptr;
  void* tmp = nullptr;
  size_t tmp_bytes = 0;
  // per-batch scratch
  float *g0 = nullptr, *delta = nullptr, *wnew[2] = {nullptr, nullptr};
  float *loss_clean = nullptr, *loss_adv = nullptr;
  // state
  int32_t B = 0, nb = 0, gen = 0;
  int32_t last_delta_batch = -1;
  int32_t mapping = 0;  // slot mapping, see get_kernels
  int32_t plan_R = 1;   // inline records per slot in the current plan (<= R)
  int32_t lists = 0;    // the plan built slot / write-back lists (packed mode)
  int32_t touch_next = 1;  // phase 2 reads the next batch's records (a constant: nothing sets it)
  int32_t *slot_list = nullptr, *flush_list = nullptr, *slot_cnt = nullptr, *flush_cnt = nullptr;
  HotLists hot = {};            // hot slots of list plans (k_records)
  int32_t shard = 0;            // shard mode (acf_apr_set_shard_mode): item rows are partial sums
  int32_t tri = 0;              // the plan is triplet-centric (packed, not shard: k_tri_*)
  float* contrib = nullptr;     // [4 maxB, d] per-occurrence contributions of shared rows (k_tri_*)
  unsigned long long* ready = nullptr;  // [3 maxB] k_tri_cadv's per-slot tags (zeroed: never a tag)
  int32_t reg_batch = 0;        // batch size of the reg mean (0: the planned batch size)
  int32_t shard_t = 0;          // the batch shard passes use (acf_apr_set_shard_batch)
  float* hot_part = nullptr;    // their piece sums
  int32_t fusion = 1;   // fused triplets in train_planned / time_kernels
  const float* xdelta = nullptr;    // triplet-centric shard passes: the owners' item deltas (acf_apr_shard_items_mapped)
  const int64_t* xdmap = nullptr;
  int32_t plan_kind2 = 0;  // the plan encodes sources at every distance (k_prev_next)
  int32_t plan_kb = 1;     // slot bits of the plan's src encoding
  int32_t* nextt = nullptr;  // [maxNB][S] next batch touching each slot's row (k_prev_next)
  // streamed step (k_stream): row versions of every batch of a launch
  int32_t stream = 1;        // ACF_STREAM=0 disables
  int32_t stream_depth = 2;  // max waves per position (batches in flight); a constant: nothing sets it
  int32_t poll_sleep = ACF_POLL_SLEEP;  // s_sleep between version polls (0-3; 4/5/6 = 8/16/32; acf_apr_set_poll_sleep)
  int32_t spin_limit = ACF_SPIN_LIMIT;  // k_stream version polls before a give-up (acf_apr_set_spin_limit)
  // a replay of a call of this context may still be reading the plan's records:
  // replay_ev was recorded behind it on its stream, and the next plan waits on it
  // (acf_apr_plan; the event, not the stream's handle, is what is kept)
  hipEvent_t replay_ev = nullptr;
  bool replay_dirty = false;
  int32_t failsafe = 1;      // verify every streamed call, replay a failed one (acf_apr_set_failsafe)
  unsigned long long* status = nullptr;      // host-mapped ring of 8: (seq << 2) | failed, per streamed launch
  unsigned long long* status_dev = nullptr;  // its device address
  int64_t recoveries = 0;    // streamed calls replayed on the two-kernel schedule
  uint32_t seq = 0;          // streamed launches so far (StepArgs.seq)
  uint32_t last_tail_seq = 0;  // seq of the last launch with a tail (StepArgs.decide_prev)
  unsigned long long* tail_diag = nullptr;  // diagnostic builds, ACF_TAIL_DIAG=1: tail stamps (acf_apr_diag_tail)
  unsigned long long* decide = nullptr;  // [0] decide word, [16, 16 + 288) the tail's arrival counters
  uint32_t tail_launches = 0;            // launches with a tail so far (StepArgs.tail_par)
  FailGroup* grp = nullptr;  // contexts whose streamed calls are verified together (PlanPipeline)
  int2* final_list = nullptr;  // the batch plan's final slots (k_stream's tail write-back)
  int32_t* final_cnt = nullptr;
  int32_t final_ok = 0;        // the current plan wrote final_list
  int32_t stream_ok = -1;    // -1 unknown, 0 unavailable (allocation / occupancy), 1 ready
  int64_t stream_max_waves = 0;
  unsigned long long *ver_w = nullptr, *ver_a = nullptr, *ver_d = nullptr;
  uint32_t* epoch = nullptr;
  int32_t *task_list = nullptr, *task_cnt = nullptr;  // streamed-step task lists of the plan
  int32_t task_lists = 0, task_stride = 0;
  // batch-local plan (k_bplan_sort / k_bplan_build)
  int32_t plan_mode = 0;     // 0 auto (batch-local plan where it applies), 1 always the sort plan
  // hash plan of triplet-centric steps (k_hplan_*); acf_apr_set_plan_mode(ctx, 1) keeps the sort plan (A/B)
  int32_t plan_kind = -1;    // acf_apr_plan_kind
  int32_t hplan_ok = -1;     // -1 unknown, 0 unavailable, 1 buffers allocated
  int2* hplan_occ = nullptr;   // [3 maxE] occurrence -> {slot or -1, CSR position}
  int32_t* hplan_pcnt = nullptr;  // [2][maxNB << pb][tiles] partition counts, their scan
  int4* hplan_claims = nullptr;   // [3 maxE / 2] shared keys, partition-local numbering
  int32_t* hplan_ptot = nullptr;  // [2][maxNB << pb][6] partition totals, their scan
  void* hplan_tmp = nullptr;   // rocPRIM temporary storage when c->tmp is too small
  size_t hplan_tmp_bytes = 0;
  int32_t* hplan_cnt = nullptr;  // [3][maxNB] shared slots, user / item CSR positions
  int32_t* hplan_haux = nullptr;  // [maxNB][hot_stride] CSR base | item of each hot-list entry
  int32_t* hplan_perm = nullptr;  // [maxE] triplet -> its place (fused first, r06)
  int32_t* hplan_tcnt = nullptr;  // [maxNB] fused triplets per batch
  unsigned long long* hplan_ttc = nullptr;  // [maxNB * tiles + 1] triplet classes per tile of 256, then its scan
  int32_t bplan_ok = -1;     // -1 unknown, 0 unavailable, 1 buffers allocated
  unsigned long long* bmask[2] = {nullptr, nullptr};
  size_t bmask_words = 0;
  int32_t bmask_dirty[2] = {0, 0};
  uint16_t* slot_of = nullptr;
  uint32_t* bkey = nullptr;
  int32_t *bstart = nullptr, *bocc = nullptr, *berr = nullptr;
  int2* bn = nullptr;
  hipStream_t cap_stream = nullptr;
  std::map<GraphKey, hipGraphExec_t> graphs;
  std::vector<void*> allocs;
};

// one lane-group per slot: large batches (auto), mapping 2, and always in shard mode
static inline int is_packed(const acf_apr_ctx* c, int32_t B) {
  return c->shard || c->mapping == 2 || (c->mapping == 0 && B >= ACF_PACKED_MIN_BATCH);
}

static inline uint32_t bits_for(uint64_t v) {  // bits to represent values in [0, v)
  uint32_t b = 0;
  while (b < 64 && (v > (1ull << b))) ++b;
  return b == 0 ? 1 : b;
}

template <typename T>
static int dalloc(acf_apr_ctx* c, T** p, size_t n) {
  void* q = nullptr;
  if (hipMalloc(&q, n * sizeof(T) + 16) != hipSuccess) {
    (void)hipGetLastError();
    return acf_set_error(ACF_E_NOMEM, "hipMalloc of %zu bytes failed", n * sizeof(T));
  }
  c->allocs.push_back(q);
  *p = static_cast<T*>(q);
  return ACF_OK;
}

static inline void free_alloc(acf_apr_ctx* c, void* p) {
  auto it = std::find(c->allocs.begin(), c->allocs.end(), p);
  if (it != c->allocs.end()) {
    (void)hipFree(p);
    c->allocs.erase(it);
  }
}

// ---- host functions that cross the seam (defined in acf_apr.hip, hidden like acf_set_error) ----
// Settle the queued streamed calls of c's group: acf_apr_plan and acf_apr_set_plan_mode settle a
// context's calls before its plan (or how it is built) changes.
__attribute__((visibility("hidden"))) int resolve(acf_apr_ctx* c, int mode);
#ifdef ACF_DIAG
// acf_diag_set_stamps (acf_apr.hip) sets the plan unit's stamp words through this.
__attribute__((visibility("hidden"))) int plan_set_stamps(uint64_t* buf, int32_t cap);
#endif
