"""Torch-tensor front end of the C-ABI.

PyTorch provides device memory and the current HIP stream; every computation runs
in ``libacf_apr.so``.  Arguments are validated here the way TF validated feeds
(dtype/shape/device errors raise ``TypeError``/``ValueError`` before any launch);
index ranges are validated on device by the plan / sampler (``NativeIndexError``).
"""
from __future__ import annotations

import ctypes
import math
import weakref
from dataclasses import dataclass

import torch

from . import _native
from ._native import HParams, Tables, call

CLIP_LO = -80.0   # APR.py:148
CLIP_HI = 1e8


class _Null:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NULL = _Null()


def _on(device: torch.device):
    """torch.cuda.device(device) unless it is already current (a few us saved per call)."""
    return _NULL if torch.cuda.current_device() == device.index else torch.cuda.device(device)


def _stream_ptr(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


_RAW = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _raw_stream(device: torch.device) -> int:
    """The current stream of `device` as an integer handle (torch's raw accessor:
    no Stream object per call)."""
    return _RAW(device.index) if _RAW is not None else _stream_ptr(device)


def _require(t: torch.Tensor, name: str, dtype: torch.dtype, device: torch.device | None = None,
             ndim: int | None = None) -> int:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if t.device.type != "cuda":
        raise ValueError(f"{name} must live on a HIP device (got {t.device}); there is no CPU path")
    if device is not None and t.device != device:
        raise ValueError(f"{name} is on {t.device}, expected {device}")
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"{name} must be {ndim}-D, got shape {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t.data_ptr()


def _idx(t, name, device) -> torch.Tensor:
    """Accept [N] or [N,1] int tensors/arrays (the placeholders are [None,1])."""
    if (isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.dim() == 1 and t.device == device
            and t.is_contiguous()):
        return t
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t)
    t = t.reshape(-1)
    if t.dtype != torch.int32:
        t = t.to(torch.int32)
    return t.to(device, non_blocking=True).contiguous()


class StepWaitError(RuntimeError):
    """A streamed step gave up waiting for a row (ACF_SPIN_LIMIT
    polls): the tables of that call hold stale rows and must not be trusted."""

    def __init__(self, bits: int):
        self.bits = int(bits)
        super().__init__(f"step error word {bits:#x}: a step kernel gave up waiting for a row version; "
                         "the tables of this call are not trustworthy")


@dataclass
class StepHParams:
    """Hyper-parameters of one MF graph (APR.py:86-97)."""
    lr: float = 0.05
    eps: float = 0.5
    reg: float = 0.0
    reg_adv: float = 1.0
    adver: int = 0
    adv: str = "grad"        # "grad" | "random" (APR.py:170-191)
    seed: int = 0
    zero_delta: int = 0
    clip_lo: float = CLIP_LO
    clip_hi: float = CLIP_HI
    # the K-step inner attack of grid_train (Python side only: not fields of the C struct);
    # adv_step None is 2.5 * eps / adv_iters.  Every other trainer refuses adv_iters > 1.
    adv_iters: int = 1
    adv_step: float | None = None

    def require_one_step(self, who: str = "this trainer") -> None:
        """ValueError unless adv_iters is 1: only grid_train trains against a K-step attack,
        and no other trainer may train one-step silently."""
        if self.adv_iters != 1:
            raise ValueError(f"{who} trains against the one-step delta only: adv_iters = {self.adv_iters!r} "
                             "needs ops.grid_train (MFGrid, --adv_iters)")

    def to_c(self) -> HParams:
        self.require_one_step()
        return self._struct()

    def _struct(self) -> HParams:
        key = (self.lr, self.eps, self.reg, self.reg_adv, self.adver, self.adv, self.seed, self.zero_delta,
               self.clip_lo, self.clip_hi)
        c = self.__dict__.get("_c")
        if c is not None and c[0] == key:
            return c[1]
        if self.adv not in ("grad", "random"):
            raise ValueError(f"adv must be 'grad' or 'random', got {self.adv!r}")
        h = HParams(self.lr, self.eps, self.reg, self.reg_adv, self.clip_lo, self.clip_hi,
                    int(bool(self.adver)), 0 if self.adv == "grad" else 1,
                    int(self.seed) & 0xFFFFFFFFFFFFFFFF, int(bool(self.zero_delta)), 0)
        self.__dict__["_c"] = (key, h)
        return h


class APRContext:
    """Owns an ``acf_apr_ctx``: plan workspace, per-batch scratch, graph cache."""

    def __init__(self, num_user_rows: int, num_item_rows: int, dim: int, max_batch_size: int,
                 max_batches: int, device: torch.device):
        self.device = torch.device(device)
        self.U1, self.I1, self.d = int(num_user_rows), int(num_item_rows), int(dim)
        self.max_batch_size, self.max_batches = int(max_batch_size), int(max_batches)
        self._ptr = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            call("acf_apr_create", ctypes.byref(self._ptr), self.U1, self.I1, self.d,
                 self.max_batch_size, self.max_batches)
        self.batch_size = 0
        self.n_batches = 0
        self._staged = None
        self._tb_key, self._tb = None, None

    def __del__(self):
        try:
            if self._ptr:
                _native.load().acf_apr_destroy(self._ptr)
                self._ptr = ctypes.c_void_p()
        except Exception:
            pass

    def fits(self, batch_size: int, n_batches: int) -> bool:
        return batch_size <= self.max_batch_size and n_batches <= self.max_batches

    def plan(self, user, item_pos, item_neg, batch_size: int, check: bool = True) -> int:
        """Stage triplets and build the dedup plan; returns the number of batches."""
        u = _idx(user, "user", self.device)
        i = _idx(item_pos, "item_pos", self.device)
        j = _idx(item_neg, "item_neg", self.device)
        if not (u.numel() == i.numel() == j.numel()):
            raise ValueError(f"triplet lengths differ: {u.numel()}, {i.numel()}, {j.numel()}")
        if batch_size <= 0 or u.numel() % batch_size:
            raise ValueError(f"{u.numel()} triplets is not a multiple of batch_size {batch_size}")
        nb = u.numel() // batch_size
        if not self.fits(batch_size, nb):
            raise ValueError(f"plan of {nb} x {batch_size} exceeds context capacity "
                             f"{self.max_batches} x {self.max_batch_size}")
        with torch.cuda.device(self.device):
            call("acf_apr_plan", self._ptr, u.data_ptr(), i.data_ptr(), j.data_ptr(), batch_size, nb,
                 int(check), _stream_ptr(self.device))
        self._staged = (u, i, j)  # keep alive until the stream has consumed them
        self.batch_size, self.n_batches = batch_size, nb
        return nb

    def _tables(self, P, Q, accP, accQ) -> Tables:
        # the same storage, shape, strides and dtype as the last validated call (the
        # device cannot differ at the same address)
        key = (P.data_ptr(), Q.data_ptr(), accP.data_ptr(), accQ.data_ptr(), P.shape, Q.shape, accP.shape,
               accQ.shape, P.stride(), Q.stride(), accP.stride(), accQ.stride(), P.dtype, Q.dtype, accP.dtype,
               accQ.dtype)
        if self._tb_key == key:
            return self._tb
        for t, n, rows in ((P, "embedding_P", self.U1), (Q, "embedding_Q", self.I1),
                           (accP, "accumulator_P", self.U1), (accQ, "accumulator_Q", self.I1)):
            _require(t, n, torch.float32, self.device, 2)
            if tuple(t.shape) != (rows, self.d):
                raise ValueError(f"{n} has shape {tuple(t.shape)}, expected {(rows, self.d)}")
        self._tb = Tables(P.data_ptr(), Q.data_ptr(), accP.data_ptr(), accQ.data_ptr())
        self._tb_key = key
        return self._tb

    def train_range(self, tables, hp: StepHParams, user: torch.Tensor, item_pos: torch.Tensor,
                    item_neg: torch.Tensor, batch_size: int, first_batch: int, n_batches: int,
                    graph: bool = True, check: bool = False, _checked: bool = False) -> None:
        """plan + train_planned of batches [first_batch, first_batch + n_batches) of
        device int32 triplet streams, in ONE C call (acf_apr_train); the range is
        addressed in place (no slicing).  (_checked: the caller, PlanPipeline.run,
        has validated the three streams and the range.)"""
        B, nb = int(batch_size), int(n_batches)
        if not _checked:
            for t, n in ((user, "user"), (item_pos, "item_pos"), (item_neg, "item_neg")):
                if t.dtype != torch.int32 or t.device != self.device or not t.is_contiguous() or t.dim() != 1:
                    raise ValueError(f"{n} must be a contiguous 1-D int32 tensor on {self.device}")
                if (first_batch + nb) * B > t.numel() or first_batch < 0:
                    raise ValueError(f"batches [{first_batch}, {first_batch + nb}) outside {n}")
        if not self.fits(B, nb):
            raise ValueError(f"plan of {nb} x {B} exceeds context capacity {self.max_batches} x "
                             f"{self.max_batch_size}")
        tb, h = self._tables(*tables), hp.to_c()
        off = first_batch * B * 4
        with _on(self.device):
            call("acf_apr_train", self._ptr, ctypes.byref(tb), ctypes.byref(h), user.data_ptr() + off,
                 item_pos.data_ptr() + off, item_neg.data_ptr() + off, B, nb, int(check), int(bool(graph)),
                 torch.cuda.current_stream(self.device).cuda_stream)
        self._staged = (user, item_pos, item_neg)
        self.batch_size, self.n_batches = B, nb

    def delta_update(self, tables, hp: StepHParams, batch: int) -> None:
        tb, h = self._tables(*tables), hp.to_c()
        with torch.cuda.device(self.device):
            call("acf_apr_delta_update", self._ptr, ctypes.byref(tb), ctypes.byref(h), batch,
                 _stream_ptr(self.device))

    def optimizer_step(self, tables, hp: StepHParams, batch: int) -> None:
        tb, h = self._tables(*tables), hp.to_c()
        with torch.cuda.device(self.device):
            call("acf_apr_optimizer_step", self._ptr, ctypes.byref(tb), ctypes.byref(h), batch,
                 _stream_ptr(self.device))

    def train_planned(self, tables, hp: StepHParams, first: int = 0, n: int | None = None,
                      graph: bool = True) -> None:
        n = self.n_batches - first if n is None else n
        tb, h = self._tables(*tables), hp.to_c()
        with torch.cuda.device(self.device):
            call("acf_apr_train_planned", self._ptr, ctypes.byref(tb), ctypes.byref(h), first, n,
                 int(bool(graph)), _stream_ptr(self.device))

    def set_slot_mapping(self, mode: str | int) -> None:
        """'auto' | 'wave' (one wavefront per unique row) | 'group' (one lane-group per row)."""
        m = {"auto": 0, "wave": 1, "group": 2}.get(mode, mode)
        call("acf_apr_set_slot_mapping", self._ptr, int(m))

    def set_plan_mode(self, mode: str | int) -> None:
        """'auto' (batch-local plan where it applies: one-wave-per-slot plans of
        batches <= 1,024) | 'sort' (always the device-wide sort plan).  Both
        write identical plans; 'sort' is for A/B and the equivalence test."""
        m = {"auto": 0, "sort": 1}.get(mode, mode)
        call("acf_apr_set_plan_mode", self._ptr, int(m))
        self.plan_mode = int(m)

    PLAN_KINDS = {-1: None, 0: "sort", 1: "batch", 2: "shard", 3: "hash"}

    def plan_kind(self) -> str | None:
        """The planner the last plan() used: 'sort' (device-wide radix sort),
        'batch' (batch-local, B <= 1,024), 'shard' (one-workgroup shard plan) or
        'hash' (triplet-centric plans); None before any plan."""
        return self.PLAN_KINDS[_native.load().acf_apr_plan_kind(self._ptr)]

    def set_fusion(self, on: bool) -> None:
        """Fuse triplets whose three rows occur once in their batch (default on;
        identical results either way).  Applies to train_planned / time_kernels;
        for large batches (one lane-group per slot) set it before plan(): a plan
        made with fusion on is triplet-centric and updates every row in place, and
        training it with fusion off raises."""
        call("acf_apr_set_fusion", self._ptr, int(bool(on)))
        self.fusion = bool(on)

    def time_kernels(self, tables, hp: StepHParams, first: int = 0, n: int | None = None):
        """Per-kernel-kind device time (ms) and launch counts over planned batches,
        measured with start/stop events attached to each launch of the sequence
        train_planned runs (tables are trained exactly as by it).  Kinds: clean
        (phase 1, or the fused BPR step), adv (phase 2 + Adagrad), flush
        (end-of-call write-back), stream (the whole range in one launch,
        k_stream), hot (the hot-slot combine of large-batch plans)."""
        n = self.n_batches - first if n is None else n
        tb, h = self._tables(*tables), hp.to_c()
        ms = (ctypes.c_double * 6)()
        cnt = (ctypes.c_int32 * 6)()
        with torch.cuda.device(self.device):
            call("acf_apr_time_kernels", self._ptr, ctypes.byref(tb), ctypes.byref(h), first, n, ms, cnt,
                 _stream_ptr(self.device))
        # (slot 3 was the overlapped step k_ovl, removed in r05)
        return {k: (ms[x], cnt[x]) for x, k in enumerate(("clean", "adv", "flush", None, "stream", "hot")) if k}

    def set_stream(self, on: bool) -> None:
        """Streamed APR steps (default on; identical results either way): one
        launch runs the whole batch range through tagged row versions."""
        call("acf_apr_set_stream", self._ptr, int(bool(on)))

    def set_failsafe(self, on: bool) -> None:
        """Verified streamed steps (default on): a streamed call stays asynchronous
        and is queued; if a hand-off wait gave up (k_stream needs all its waves
        resident), the call applied nothing and gated the later streamed calls of
        its group, and the next settling point (resolve(), step_errors(),
        stream_recoveries(), losses(), a re-plan of this context, ...) replays
        them in order on the two-kernel schedule -- exact.  Off: a give-up is
        reported by step_errors() and that call is not applied."""
        call("acf_apr_set_failsafe", self._ptr, int(bool(on)))

    def resolve(self) -> None:
        """Settle the queued streamed calls of this context's group (blocking)."""
        call("acf_apr_resolve", self._ptr)

    def share_failsafe(self, peer: "APRContext") -> None:
        """Verify this context's streamed calls together with peer's (contexts
        training the same tables on one stream)."""
        call("acf_apr_share_failsafe", self._ptr, peer._ptr)

    def set_spin_limit(self, polls: int) -> None:
        """Version polls before a k_stream wait gives up (default 65,536; tests use
        0 to force the replay)."""
        call("acf_apr_set_spin_limit", self._ptr, int(polls))

    def set_poll_sleep(self, code: int) -> None:
        """s_sleep between two version polls of k_stream, as a code (0-3: s_sleep 0-3;
        4 / 5 / 6: s_sleep 8 / 16 / 32; default 2).  Timing only; a non-default code
        runs the streamed kernel's general instance."""
        call("acf_apr_set_poll_sleep", self._ptr, int(code))

    def stream_recoveries(self) -> int:
        """Streamed calls replayed on the two-kernel schedule so far."""
        out = ctypes.c_int64(0)
        call("acf_apr_stream_recoveries", self._ptr, ctypes.byref(out))
        return int(out.value)

    # -- shard mode (distributed.ShardedAPR; include/acf_apr.h "shard mode") --------
    def set_shard_mode(self, on: bool, reg_batch: int = 0) -> None:
        """Item rows are this rank's partial sums (one lane-group per slot, no
        fusion, one-batch plans); reg_batch = the global batch of the reg mean."""
        call("acf_apr_set_shard_mode", self._ptr, int(bool(on)), int(reg_batch))
        self.batch_size = self.n_batches = 0

    def set_shard_batch(self, t: int) -> None:
        """The plan's batch the next shard passes step (a triplet-centric shard
        plan may hold a chunk of steps; 0 otherwise)."""
        call("acf_apr_set_shard_batch", self._ptr, int(t))

    def shard_pass(self, tables, hp: StepHParams, pass_: int) -> None:
        """pass 0: clean sums (users: delta; items: partial sums); pass 1 (APR):
        adversarial sums, user Adagrad + write-back."""
        tb, h = self._tables(*tables), hp.to_c()
        with torch.cuda.device(self.device):
            call("acf_apr_shard_pass", self._ptr, ctypes.byref(tb), ctypes.byref(h), int(pass_),
                 _stream_ptr(self.device))

    def shard_pass_export(self, tables, hp: StepHParams, pass_: int, buf: torch.Tensor, rows: torch.Tensor) -> None:
        """shard_pass, with working-set entry w's partial item sum also written to
        buf[rows[w]] by the pass's own launches (the split step's exchange rows)."""
        tb, h = self._tables(*tables), hp.to_c()
        _require(buf, "buf", torch.float32, self.device, 2)
        _require(rows, "rows", torch.int64, self.device, 1)
        with torch.cuda.device(self.device):
            call("acf_apr_shard_pass_export", self._ptr, ctypes.byref(tb), ctypes.byref(h), int(pass_),
                 buf.data_ptr(), rows.data_ptr(), rows.numel(), _stream_ptr(self.device))

    def shard_items_out(self, out: torch.Tensor) -> None:
        """The item slots' partial sums (working-set order) -> out [n_items, d]."""
        _require(out, "out", torch.float32, self.device, 2)
        with torch.cuda.device(self.device):
            call("acf_apr_shard_items", self._ptr, 0, out.data_ptr(), out.shape[0], _stream_ptr(self.device))

    def shard_items_delta(self, delta: torch.Tensor) -> None:
        """The owners' deltas [n_items, d] (working-set order) -> the item slots."""
        _require(delta, "delta", torch.float32, self.device, 2)
        with torch.cuda.device(self.device):
            call("acf_apr_shard_items", self._ptr, 1, delta.data_ptr(), delta.shape[0], _stream_ptr(self.device))

    def shard_items_mapped(self, dir_: int, buf: torch.Tensor, rows: torch.Tensor) -> None:
        """Working-set entry w <-> row rows[w] of buf, for w < rows.numel(): dir 0
        writes the item slots' partial sums there, dir 1 takes the owners'
        deltas from there (the split step's exchange rows)."""
        _require(buf, "buf", torch.float32, self.device, 2)
        _require(rows, "rows", torch.int64, self.device, 1)
        with torch.cuda.device(self.device):
            call("acf_apr_shard_items_mapped", self._ptr, int(dir_), buf.data_ptr(), rows.data_ptr(), rows.numel(),
                 _stream_ptr(self.device))

    def step_errors(self) -> int:
        """Read and clear the step error words (bit 0: an overlapped step gave up
        waiting for a row, or an unverified streamed call gave up -- set_failsafe)."""
        out = ctypes.c_int32(0)
        with torch.cuda.device(self.device):
            call("acf_apr_step_errors", self._ptr, ctypes.byref(out), _stream_ptr(self.device))
        return int(out.value)

    def losses(self):
        """Per-triplet (clean, adversarial) softplus terms of the last steps."""
        n = self.batch_size * self.n_batches
        lc = torch.empty(n, dtype=torch.float32, device=self.device)
        la = torch.empty(n, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            call("acf_apr_copy_losses", self._ptr, lc.data_ptr(), la.data_ptr(),
                 _stream_ptr(self.device))
        return lc, la

    def delta_tables(self):
        """Dense delta_P / delta_Q of the last delta_update (zeros elsewhere)."""
        dP = torch.zeros(self.U1, self.d, dtype=torch.float32, device=self.device)
        dQ = torch.zeros(self.I1, self.d, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            call("acf_apr_delta_scatter", self._ptr, dP.data_ptr(), dQ.data_ptr(),
                 _stream_ptr(self.device))
        return dP, dQ


class PlanPipeline:
    """training_batch's epoch loop with the dedup plan off the critical path.

    A long triplet stream is trained in chunks of ``chunk`` batches.  The plan of
    chunk c+1 (sort / dedup / records — it reads triplets only, never the tables)
    runs on a side stream while chunk c trains on the caller's stream; two
    contexts alternate so a plan never overwrites records still in use.  Chunks
    are independent calls of train_planned (each ends with its flush), so the
    result is the one of planning and training the chunks in sequence.

    overlap=False plans on the caller's stream instead.  overlap=True (the
    constructor's default) and overlap=None (the library's own choice, what
    the benchmark and the model pass) now take the same schedule: concurrent
    planning whenever the run has more than one chunk.  For large batches (B >= 4,096) that is the device-wide sort plan,
    ~40 us per batch, on a side stream of the default priority.  For smaller
    ones it is the batch-local plan (two launches per chunk)
    beside the persistent k_stream: it goes to a stream of the lowest priority
    (acf_plan_stream_create) and may start with the chunk it runs beside, so
    the step's workgroups are placed first and the plan takes the slots
    k_stream leaves free.  A run of a single chunk always plans in line: the
    events and stream hand-offs cost more than a 20-batch plan.
    ``overlapped`` tells which schedule the last run took.  The lowest-priority
    stream belongs to the pipeline: ``close()`` (or a ``with`` block) destroys it.
    """

    def __init__(self, num_user_rows: int, num_item_rows: int, dim: int, batch_size: int,
                 chunk: int, device: torch.device, overlap: bool | None = True):
        self.device = torch.device(device)
        self.overlap = None if overlap is None else bool(overlap)
        self._ov = bool(overlap)  # the current run's choice
        self.batch_size, self.chunk = int(batch_size), int(chunk)
        self.ctx = [APRContext(num_user_rows, num_item_rows, dim, batch_size, chunk, self.device)
                    for _ in range(2)]
        self.ctx[1].share_failsafe(self.ctx[0])  # one verification queue for both (acf_apr.h)
        # default priority: a high-priority plan stream halved the configs[4] rate
        # (608M -> 313M triplets/s at d = 64, tools/large_prio.py, r03)
        # (the steps on a high-priority stream instead, the plan filling what they
        # leave idle, was 1.8x slower at configs[4]: 775M -> 424M triplets/s, r04)
        # small batches plan beside the persistent k_stream: the lowest priority,
        # which a torch stream cannot have (created at the first overlapped run)
        self._low = None
        self.side = torch.cuda.Stream(self.device) if self.batch_size >= 4096 else None
        self._free = [None, None]  # event: the last training on ctx[k] has been issued before it
        self._memo = None  # the last single-chunk call, validated (_repeat)

    def set_fusion(self, on: bool) -> None:
        for c in self.ctx:
            c.set_fusion(on)

    def set_stream(self, on: bool) -> None:
        for c in self.ctx:
            c.set_stream(on)

    def step_errors(self) -> int:
        e = 0
        for c in self.ctx:
            e |= c.step_errors()
        return e

    def set_failsafe(self, on: bool) -> None:
        for c in self.ctx:
            c.set_failsafe(on)

    def set_spin_limit(self, polls: int) -> None:
        for c in self.ctx:
            c.set_spin_limit(polls)

    def stream_recoveries(self) -> int:
        return sum(c.stream_recoveries() for c in self.ctx)

    def resolve(self) -> None:
        self.ctx[0].resolve()

    def set_slot_mapping(self, mode) -> None:
        for c in self.ctx:
            c.set_slot_mapping(mode)

    def set_plan_mode(self, mode) -> None:
        for c in self.ctx:
            c.set_plan_mode(mode)

    def _remember(self, tables, hp, user, item_pos, item_neg, first_batch, n_arg, n_batches, graph) -> None:
        c = self.ctx[0]
        P, Q, aP, aQ = tables
        tb, h = c._tables(P, Q, aP, aQ), hp.to_c()
        off = first_batch * self.batch_size * 4
        args = (c._ptr, ctypes.byref(tb), ctypes.byref(h), user.data_ptr() + off, item_pos.data_ptr() + off,
                item_neg.data_ptr() + off, self.batch_size, n_batches, 0, int(bool(graph)))
        self._memo = (user, item_pos, item_neg, hp, first_batch, n_arg, graph, P, Q, aP, aQ, dict(hp.__dict__),
                      (P.data_ptr(), Q.data_ptr(), aP.data_ptr(), aQ.data_ptr(), user.data_ptr(),
                       item_pos.data_ptr(), item_neg.data_ptr()),
                      _native.load().acf_apr_train, args, c, tb, h)

    @property
    def overlapped(self) -> bool:
        """The last run planned chunk c+1 beside chunk c (False: in line)."""
        return bool(self._ov)

    def _side_stream(self):
        if self.side is None:
            h = ctypes.c_void_p()
            with torch.cuda.device(self.device):
                call("acf_plan_stream_create", ctypes.byref(h))
            self._low = h.value
            self.side = torch.cuda.ExternalStream(self._low, device=self.device)
        return self.side

    def close(self) -> None:
        """Wait for the plan stream's work and destroy it (the lowest-priority
        stream of small batches is this pipeline's own; a later overlapped run
        makes a new one).  Errors surface here; __del__ calls it as a last
        resort only."""
        low, self._low = getattr(self, "_low", None), None
        if low is None:
            return
        side, self.side = self.side, None
        side.synchronize()
        call("acf_plan_stream_destroy", low)

    def __enter__(self):
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 -- interpreter shutdown: the process frees the stream
            pass

    def _plan(self, k, u, i, j, b, n, check, go=None):
        B, c = self.batch_size, self.ctx[k % 2]
        s = slice(b * B, (b + n) * B)
        if not self._ov:
            c.plan(u[s], i[s], j[s], B, check=check)
            return None
        with torch.cuda.stream(self.side):
            if self._free[k % 2] is not None:
                self.side.wait_event(self._free[k % 2])
            if go is not None:  # not before the chunk it runs beside may start
                self.side.wait_event(go)
            c.plan(u[s], i[s], j[s], B, check=check)
            ev = torch.cuda.Event()
            ev.record(self.side)
        return ev

    def _repeat(self, tables, hp, user, item_pos, item_neg, first_batch, n_batches, graph) -> bool:
        """The exact call the last run made (same tensor objects, storage, shapes
        and hyper-parameters; one chunk): issue it straight to the C-ABI with the
        arguments validated then.  Saves the per-call validation (~10 us of host
        time in front of the first kernel of a short call)."""
        m = self._memo
        if not (m[0] is user and m[1] is item_pos and m[2] is item_neg and m[3] is hp and m[4] == first_batch
                and m[5] == n_batches and m[6] == graph):
            return False
        P, Q, aP, aQ = tables
        # the same tensor objects on the same storage (a storage swap moves data_ptr)
        # and the same hyper-parameters; the launches go to the device's current
        # stream, which selects the device
        if not (P is m[7] and Q is m[8] and aP is m[9] and aQ is m[10] and hp.__dict__ == m[11]
                and m[12] == (P.data_ptr(), Q.data_ptr(), aP.data_ptr(), aQ.data_ptr(), user.data_ptr(),
                              item_pos.data_ptr(), item_neg.data_ptr())):
            return False
        fn, args, ctx = m[13], m[14], m[15]
        rc = fn(*args, _raw_stream(self.device))
        if rc:
            _native.call_failed(rc, "acf_apr_train")
        ctx._staged = (user, item_pos, item_neg)
        return True

    def run(self, tables, hp: StepHParams, user, item_pos, item_neg, first_batch: int = 0,
            n_batches: int | None = None, graph: bool = True, check: bool = False) -> None:
        """Train batches [first_batch, first_batch + n_batches) of the stream."""
        if self._memo is not None and not check and self._repeat(tables, hp, user, item_pos, item_neg, first_batch,
                                                                 n_batches, graph):
            return
        self._memo = None
        n_arg = n_batches  # the memo compares the caller's own argument (None or a count)
        B = self.batch_size
        u, i, j = (_idx(x, n, self.device) for x, n in ((user, "user"), (item_pos, "item_pos"),
                                                       (item_neg, "item_neg")))
        total = min(u.numel(), i.numel(), j.numel()) // B
        n_batches = total - first_batch if n_batches is None else int(n_batches)
        if first_batch < 0 or n_batches <= 0 or first_batch + n_batches > total:
            raise ValueError(f"batches [{first_batch}, {first_batch + n_batches}) outside the "
                             f"{total} batches of the stream")
        main = torch.cuda.current_stream(self.device)
        chunks = [(b, min(self.chunk, first_batch + n_batches - b))
                  for b in range(first_batch, first_batch + n_batches, self.chunk)]
        self._ov = self.overlap is not False and len(chunks) > 1
        if not self._ov:  # plan + train per chunk in one C call each, on the caller's stream
            for k, (b, n) in enumerate(chunks):
                self.ctx[k % 2].train_range(tables, hp, u, i, j, B, b, n, graph=graph, check=check, _checked=True)
            self._staged = (u, i, j)
            if len(chunks) == 1 and not check and u is user and i is item_pos and j is item_neg:
                self._remember(tables, hp, user, item_pos, item_neg, first_batch, n_arg, n_batches, graph)
            return
        ready = torch.cuda.Event()
        ready.record(main)  # triplets produced on the caller's stream
        self._side_stream().wait_event(ready)
        planned = self._plan(0, u, i, j, *chunks[0], check)
        for k, (b, n) in enumerate(chunks):
            if planned is not None:
                main.wait_event(planned)
            go = None
            if self._low is not None and k + 1 < len(chunks):
                # beside k_stream: the next plan may start with this chunk, not ahead of it
                go = torch.cuda.Event()
                go.record(main)
            self.ctx[k % 2].train_planned(tables, hp, 0, n, graph=graph)
            done = torch.cuda.Event()
            done.record(main)
            self._free[k % 2] = done
            if k + 1 < len(chunks):
                planned = self._plan(k + 1, u, i, j, *chunks[k + 1], check, go)
        self._staged = (u, i, j)


def settle_tables() -> None:
    """Settle every queued (lazily verified) streamed call of the process
    (acf_apr_resolve_all): a failed one is replayed before anything reads the
    tables.  The readers outside a context's group call it first: the forward,
    evaluation, dns selection, Session fetches of the tables and checkpoints."""
    call("acf_apr_resolve_all")


def bpr_forward(P, Q, user, item_pos, item_neg, batch_size: int, clip_lo=CLIP_LO, clip_hi=CLIP_HI,
                want_scores: bool = False):
    """training_loss_acc's forward (utils.py:159-175): per-batch loss sum and #correct."""
    settle_tables()
    dev = P.device
    _require(P, "embedding_P", torch.float32, None, 2)
    _require(Q, "embedding_Q", torch.float32, dev, 2)
    if P.shape[1] != Q.shape[1]:
        raise ValueError("embedding_P and embedding_Q dims differ")
    u, i, j = (_idx(x, n, dev) for x, n in ((user, "user"), (item_pos, "item_pos"), (item_neg, "item_neg")))
    n = u.numel()
    if batch_size <= 0 or n % batch_size or i.numel() != n or j.numel() != n:
        raise ValueError("triplets must be equal-length multiples of batch_size")
    nb = n // batch_size
    _check_range(u, P.shape[0], "user")
    _check_range(i, Q.shape[0], "item")
    _check_range(j, Q.shape[0], "item")
    bl = torch.empty(nb, dtype=torch.float32, device=dev)
    bc = torch.empty(nb, dtype=torch.int32, device=dev)
    op = torch.empty(n, dtype=torch.float32, device=dev) if want_scores else None
    on = torch.empty(n, dtype=torch.float32, device=dev) if want_scores else None
    with torch.cuda.device(dev):
        call("acf_bpr_forward", P.data_ptr(), Q.data_ptr(), P.shape[0], Q.shape[0], P.shape[1],
             u.data_ptr(), i.data_ptr(), j.data_ptr(), batch_size, nb, clip_lo, clip_hi,
             bl.data_ptr(), bc.data_ptr(), op.data_ptr() if op is not None else None,
             on.data_ptr() if on is not None else None, _stream_ptr(dev))
    return bl, bc, op, on


_RANGE_OK: dict = {}  # (address, length, version, bound, device) -> weakref of the checked tensor


def _check_range(idx: torch.Tensor, rows: int, name: str) -> None:
    """IndexError unless every index lies in [0, rows).  The check reads the
    extremes back to the host (a device sync), so a tensor that passed is
    remembered by (address, length, in-place version, bound): an evaluation plan
    re-uses the same user / test tensors every epoch and pays the check once.
    The cache holds weak references only: an entry never extends a
    tensor's lifetime and leaves the cache when the tensor is freed."""
    key = (idx.data_ptr(), idx.numel(), idx._version, rows, idx.device)
    ref = _RANGE_OK.get(key)
    if ref is not None and ref() is idx:
        return
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= rows):
        raise _native.NativeIndexError(_native.ACF_E_RANGE, "range check",
                                       f"{name} index outside [0, {rows})")

    def _evict(r, k=key):
        if _RANGE_OK.get(k) is r:
            del _RANGE_OK[k]
    _RANGE_OK[key] = weakref.ref(idx, _evict)


EVAL_KERNELS = {"auto": 0, "mfma": 1, "valu": 2}


def _unique_exclusions(off: torch.Tensor, ex: torch.Tensor, n_users: int) -> torch.Tensor:
    """Each user's exclusion list as a SET (the reference's set(trainList[u]),
    utils.py:188-195): a repeated entry of a list is replaced by -1, which every
    sweep ignores (never a candidate).  The MFMA sweep applies a list as a bitmap
    (set semantics) and the VALU sweep subtracts once per entry, so without this a
    duplicate made them disagree.  Sort + compare on the device, no
    host sync; the lengths stay as given."""
    if ex.numel() < 2:
        return ex
    # each list's segment id by a search over the offsets (no assumption that
    # off[0] == 0 or off[-1] == len(ex); entries outside every list get -1 and
    # are left alone)
    pos = torch.arange(ex.numel(), device=ex.device, dtype=off.dtype)
    seg = torch.searchsorted(off[1:].contiguous(), pos, right=True)
    seg = torch.where((pos >= off[0]) & (seg < n_users), seg, torch.full_like(seg, -1))
    wide = int(2 ** 31)
    key = seg * wide + ex.long().clamp(-1, wide - 2) + 1
    skey, perm = torch.sort(key)
    dup = torch.zeros(ex.numel(), dtype=torch.bool, device=ex.device)
    dup[perm[1:]] = skey[1:] == skey[:-1]
    return torch.where(dup, torch.full_like(ex, -1), ex)


# ---- what the ranking calls below share: argument checks, exclusion lists, workspace ----
TOPK_MAX_K = 128


def _check_k(k) -> None:
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= TOPK_MAX_K:
        raise ValueError(f"k must be an int in [1, {TOPK_MAX_K}], got {k!r}")


def _kernel_id(kernel) -> int:
    if kernel not in EVAL_KERNELS:
        raise ValueError(f"kernel must be one of {sorted(EVAL_KERNELS)}, got {kernel!r}")
    return EVAL_KERNELS[kernel]


def _check_num_candidates(num_candidates) -> None:
    if isinstance(num_candidates, bool) or not isinstance(num_candidates, int) or num_candidates < 1:
        raise ValueError(f"num_candidates must be an int >= 1, got {num_candidates!r}")


def _table_types(A, B, a: str = "embedding_P", b: str = "embedding_Q") -> None:
    """TypeError unless both tables are 2-D float32 tensors, ValueError if their
    dims differ.  Looks at no device: a caller checks its host arguments between
    this and _table_pair, so that tables on the CPU are what fails last."""
    for tab, name in ((A, a), (B, b)):
        if not isinstance(tab, torch.Tensor) or tab.dtype != torch.float32 or tab.dim() != 2:
            raise TypeError(f"{name} must be a 2-D torch.float32 tensor")
    if A.shape[1] != B.shape[1]:
        raise ValueError(f"{a} and {b} dims differ")


def _table_pair(A, B, a: str = "embedding_P", b: str = "embedding_Q") -> torch.device:
    """The device of a pair of tables: both 2-D float32 and contiguous, B on A's
    HIP device, equal dims (TypeError / ValueError)."""
    _require(A, a, torch.float32, None, 2)
    _require(B, b, torch.float32, A.device, 2)
    _table_types(A, B, a, b)  # (only the dims are left to differ)
    return A.device


def _to_i32(t: torch.Tensor, dev) -> torch.Tensor:
    return t.to(device=dev, dtype=torch.int32).contiguous()


def _exclusions(excl_off, excl_items, n: int, dev, rows: str | None = None):
    """Per-row exclusion lists as (off int64 [n + 1], items int32) on `dev`, or
    (None, None) without them; an empty item array becomes a one-element
    placeholder (its pointer must not be NULL).  rows=None: a strict CSR
    (_csr_items, _csr_offsets; checked on the host before anything moves).
    rows="users" | "queries": whatever _idx takes, the offsets checked for their
    length only, the message naming `rows`."""
    if (excl_off is None) != (excl_items is None):
        raise ValueError("excl_off and excl_items go together")
    if excl_off is None:
        return None, None
    if rows is None:
        ex = _csr_items(excl_items, "excl_items")
        off = _csr_offsets(excl_off, n, ex.numel(), "excl_off").to(device=dev, dtype=torch.int64).contiguous()
        ex = _to_i32(ex, dev) if ex.numel() else None
    else:
        off = torch.as_tensor(excl_off).to(device=dev, dtype=torch.int64).contiguous()
        ex = _idx(excl_items, "excl_items", dev) if len(excl_items) else None
        if off.numel() != n + 1:
            raise ValueError(f"excl_off must have len({rows}) + 1 entries")
    return off, ex if ex is not None else torch.zeros(1, dtype=torch.int32, device=dev)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _workspace_bytes(symbol: str, *sizes) -> int:
    """A host-only acf_*_workspace query: ints in, bytes out."""
    size = ctypes.c_size_t()
    call(symbol, *(int(v) for v in sizes), ctypes.byref(size))
    return int(size.value)


def _workspace(nbytes: int, align: int, dev) -> torch.Tensor:
    """At least nbytes of uninitialised device memory in units of `align` (4 or 8) bytes."""
    return torch.empty((nbytes + align - 1) // align, dtype=torch.int64 if align == 8 else torch.int32, device=dev)


def eval_positions_all(P, Q, users, test_items, num_candidates: int, excl_off, excl_items, kernel: str = "auto",
                       unique_lists: bool = False):
    """_eval_by_user positions over all items minus the exclusion lists.  kernel:
    'auto' | 'mfma' | 'valu' (acf_eval_positions_all_kernel; same positions).
    A list may repeat an item: it is excluded once (set semantics); callers whose
    lists are already duplicate-free (EvalPlan: np.union1d) pass unique_lists=True
    to skip the device-side dedup."""
    settle_tables()
    dev = P.device
    _require(P, "embedding_P", torch.float32, None, 2)
    _require(Q, "embedding_Q", torch.float32, dev, 2)
    u, t = _idx(users, "users", dev), _idx(test_items, "test_items", dev)
    off, ex = _exclusions(excl_off, excl_items, u.numel(), dev, "users")
    kernel = _kernel_id(kernel)
    _check_range(u, P.shape[0], "user")
    _check_range(t, Q.shape[0], "test item")
    if num_candidates > Q.shape[0]:
        raise ValueError("num_candidates exceeds item rows")
    if not unique_lists and len(excl_items):
        ex = _unique_exclusions(off, ex, u.numel())
    pos = torch.empty(u.numel(), dtype=torch.int32, device=dev)
    with _on(dev):
        call("acf_eval_positions_all_kernel", P.data_ptr(), Q.data_ptr(), P.shape[0], Q.shape[0], P.shape[1],
             u.data_ptr(), t.data_ptr(), u.numel(), int(num_candidates), off.data_ptr(), ex.data_ptr(),
             pos.data_ptr(), kernel, _stream_ptr(dev))
    return pos


def recommend_topk_workspace(n_users: int, num_candidates: int, k: int, kernel: str = "auto") -> int:
    """Bytes of device workspace acf_recommend_topk needs (a host-only query)."""
    kernel = _kernel_id(kernel)
    if not 1 <= int(k) <= TOPK_MAX_K:
        raise ValueError(f"k must be in [1, {TOPK_MAX_K}], got {k}")
    return _workspace_bytes("acf_recommend_topk_workspace", n_users, num_candidates, k, kernel)


def recommend_topk(P, Q, users, k: int, num_candidates: int | None = None, excl_off=None, excl_items=None,
                   kernel: str = "auto"):
    """The k best items per user: (items int32 [n, k], scores float32 [n, k]).
    Candidates of users[j] are [0, num_candidates) (default: every row of Q) minus
    the set of excl_items[excl_off[j]:excl_off[j+1]] (unsorted, repeated and
    out-of-range entries are fine; no exclusion arguments: nothing is excluded).
    Scores are the evaluation's sequential dot product bit for bit, ordered by
    score descending, ties to the lower item id; a user with fewer than k
    candidates gets -1 / -inf in the tail.  kernel: 'auto' | 'mfma' | 'valu'
    (identical outputs).  No [n, num_candidates] score array is formed."""
    _check_k(k)
    kernel_id = _kernel_id(kernel)
    dev = _table_pair(P, Q)
    settle_tables()
    u = _idx(users, "users", dev)
    n = u.numel()
    if num_candidates is None:
        num_candidates = Q.shape[0]
    num_candidates = int(num_candidates)
    if not 0 <= num_candidates <= Q.shape[0]:
        raise ValueError("num_candidates must lie in [0, item rows]")
    off, ex = _exclusions(excl_off, excl_items, n, dev, "users")
    if off is None:  # the C side takes no NULL here: an empty list per user
        off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        ex = torch.zeros(1, dtype=torch.int32, device=dev)
    _check_range(u, P.shape[0], "user")
    items = torch.empty((n, k), dtype=torch.int32, device=dev)
    scores = torch.empty((n, k), dtype=torch.float32, device=dev)
    if n == 0:
        return items, scores
    nbytes = recommend_topk_workspace(n, num_candidates, k, kernel)
    work = _workspace(nbytes, 8, dev)
    with _on(dev):
        call("acf_recommend_topk", P.data_ptr(), Q.data_ptr(), P.shape[0], Q.shape[0], P.shape[1], u.data_ptr(),
             n, num_candidates, off.data_ptr(), ex.data_ptr(), k, items.data_ptr(), scores.data_ptr(),
             work.data_ptr(), nbytes, kernel_id, _stream_ptr(dev))
    return items, scores


NEIGHBOR_METRICS = {"dot": 0, "cosine": 1, "euclid": 2}  # NBR_DOT, NBR_COS, NBR_EUC


def neighbors_topk_workspace(n_queries: int, num_candidates: int, k: int) -> int:
    """Bytes of device workspace acf_neighbors_topk needs (a host-only query): a
    16-byte head, the strips' partial lists and the num_candidates floats of
    candidate norms the cosine metric uses."""
    _check_k(k)
    return _workspace_bytes("acf_neighbors_topk_workspace", n_queries, num_candidates, k)


def neighbors_topk(T, queries, k: int, metric: str = "cosine", X=None, num_candidates: int | None = None,
                   exclude_self: bool = True, excl_off=None, excl_items=None, check: bool = True):
    """The k nearest rows of T per query: (items int32 [n, k], scores float32
    [n, k]).  Query j is row queries[j] of X (default: T itself); its candidates
    are rows [0, num_candidates) of T (default: every row) minus the set of
    excl_items[excl_off[j]:excl_off[j+1]] (unsorted, repeated and out-of-range
    entries are fine; no exclusion arguments: nothing is excluded) and, with
    exclude_self, minus the row whose id equals queries[j].  metric: 'dot'
    (recommend_topk's score bit for bit), 'cosine' (s / (|a| |b|), +0.0 for a
    zero row) or 'euclid' (minus the squared distance: larger is nearer), in
    fp32 as include/acf_apr.h states; ordered by score descending, ties to the
    lower id, -1 / -inf past the last candidate.  Exact and bit-identical run
    to run; no [n, num_candidates] array and no normalised copy of T is formed.
    Bad shapes, k and metric raise ValueError / TypeError before any native
    call; with check, a query outside X raises NativeIndexError (one sync),
    without it such a query is read as row 0."""
    _check_k(k)
    if metric not in NEIGHBOR_METRICS:
        raise ValueError(f"metric must be one of {sorted(NEIGHBOR_METRICS)}, got {metric!r}")
    if X is None:
        X = T
    dev = _table_pair(T, X, "T", "X")
    settle_tables()
    q = _idx(queries, "queries", dev)
    n = q.numel()
    if num_candidates is None:
        num_candidates = T.shape[0]
    num_candidates = int(num_candidates)
    if not 0 <= num_candidates <= T.shape[0]:
        raise ValueError("num_candidates must lie in [0, table rows]")
    off, ex = _exclusions(excl_off, excl_items, n, dev, "queries")
    items = torch.empty((n, k), dtype=torch.int32, device=dev)
    scores = torch.empty((n, k), dtype=torch.float32, device=dev)
    if n == 0:
        return items, scores
    nbytes = neighbors_topk_workspace(n, num_candidates, k)
    work = _workspace(nbytes, 8, dev)
    with _on(dev):
        call("acf_neighbors_topk", T.data_ptr(), T.shape[0], T.shape[1], X.data_ptr(), X.shape[0], q.data_ptr(), n,
             num_candidates, NEIGHBOR_METRICS[metric], int(bool(exclude_self)), _ptr(off), _ptr(ex), k,
             items.data_ptr(), scores.data_ptr(), work.data_ptr(), nbytes, int(bool(check)), _stream_ptr(dev))
    return items, scores


RANK_MAX_CUTOFFS, RANK_MAX_K = 8, 1024          # EVX_MAX_CUT, EVX_MAX_K
RANK_CUT_METRICS = ("hit", "recall", "precision", "ndcg", "map")
RANK_FREE_METRICS = ("mrr", "auc")

_CSR_OK: dict = {}  # as _RANGE_OK, for offset tensors that passed _csr_offsets


def _csr_offsets(off, n_rows: int, n_items: int, name: str) -> torch.Tensor:
    """`off` as a tensor (where it is) after the CSR checks (ValueError): 1-D
    integers, n_rows + 1 entries, off[0] = 0, non-decreasing, off[-1] = n_items.
    A host array is checked on the host; a device tensor is checked on the device
    (one read-back, remembered like _check_range's)."""
    import numpy as np
    if not isinstance(off, torch.Tensor):
        off = np.asarray(off)
        if off.dtype.kind not in "iu":
            raise ValueError(f"{name} must be an integer array, got {off.dtype}")
        off = torch.from_numpy(np.ascontiguousarray(off, dtype=np.int64))
    if off.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{name} must be an integer array, got {off.dtype}")
    if off.dim() != 1 or off.numel() != n_rows + 1:
        raise ValueError(f"{name} must be 1-D with {n_rows + 1} entries, got shape {tuple(off.shape)}")
    key = (off.data_ptr(), off.numel(), off._version, n_items, off.device, off.dtype)
    ref = _CSR_OK.get(key)
    if not (off.is_cuda and ref is not None and ref() is off):
        bad = torch.stack([off[0] != 0, (off[1:] < off[:-1]).any(), off[-1] != n_items]).tolist()
        if bad[0]:
            raise ValueError(f"{name}[0] must be 0, got {int(off[0])}")
        if bad[1]:
            raise ValueError(f"{name} must be non-decreasing")
        if bad[2]:
            raise ValueError(f"{name}[-1] must be {n_items}, got {int(off[-1])}")
        if off.is_cuda:
            def _evict(r, k=key):
                if _CSR_OK.get(k) is r:
                    del _CSR_OK[k]
            _CSR_OK[key] = weakref.ref(off, _evict)
    return off


def _csr_items(t, name: str) -> torch.Tensor:
    """A flat int32 / int64 item array as a (host or device) tensor (ValueError)."""
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t)
    if t.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{name} must be int32 or int64, got {t.dtype}")
    if t.dim() != 1:
        raise ValueError(f"{name} must be 1-D, got shape {tuple(t.shape)}")
    return t


def eval_positions_multi_workspace(n_users: int, n_tests: int, num_candidates: int) -> int:
    """Bytes of device workspace acf_eval_positions_multi needs (a host-only query)."""
    return _workspace_bytes("acf_eval_positions_multi_workspace", n_users, n_tests, num_candidates)


def eval_positions_multi(P, Q, users, test_off, test_items, num_candidates: int, excl_off=None, excl_items=None,
                         check: bool = True):
    """Positions of SEVERAL held-out items per entry, one candidate sweep per
    entry whatever the length of its list (acf_eval_positions_multi): int32
    [len(test_items)].  Entry r is row users[r] of P with the test list
    test_items[test_off[r]:test_off[r+1]] (CSR) and the candidates
    [0, num_candidates) minus the SET of excl_items[excl_off[r]:excl_off[r+1]]
    (unsorted, repeated and out-of-range entries are fine; no exclusion
    arguments: nothing is excluded).  positions[x] = the number of candidates
    other than test_items[x] that score >= it, by the evaluation's sequential dot
    product: the same integers as eval_positions_all on the entry repeated once
    per item with that item added to its exclusions.  The other test items stay
    candidates unless excluded.  Bad shapes and dtypes raise ValueError /
    TypeError before any native call; with check, a user or test item outside
    its table raises NativeIndexError (one sync)."""
    ti = _csr_items(test_items, "test_items")
    us = _csr_items(users, "users")
    n, T = us.numel(), ti.numel()
    _check_num_candidates(num_candidates)
    _table_types(P, Q)
    if num_candidates > Q.shape[0]:
        raise ValueError("num_candidates exceeds item rows")
    toff = _csr_offsets(test_off, n, T, "test_off")
    eoff, ex = _exclusions(excl_off, excl_items, n, P.device)
    dev = _table_pair(P, Q)
    toff = toff.to(device=dev, dtype=torch.int64).contiguous()
    settle_tables()
    u, t = _to_i32(us, dev), _to_i32(ti, dev)
    pos = torch.empty(T, dtype=torch.int32, device=dev)
    if n == 0 or T == 0:
        return pos
    nbytes = eval_positions_multi_workspace(n, T, num_candidates)
    work = _workspace(nbytes, 4, dev)
    with _on(dev):
        call("acf_eval_positions_multi", P.data_ptr(), Q.data_ptr(), P.shape[0], Q.shape[0], P.shape[1],
             u.data_ptr(), toff.data_ptr(), t.data_ptr(), n, T, num_candidates, _ptr(eoff), _ptr(ex),
             pos.data_ptr(), work.data_ptr(), nbytes, int(bool(check)), _stream_ptr(dev))
    return pos


@dataclass
class RankMetrics:
    """What rank_metrics returns (device tensors, fp64 unless noted): per_user
    [n, n_cut, 5] in RANK_CUT_METRICS order, per_user_free [n, 2] in
    RANK_FREE_METRICS order, their means over the users with a non-empty list
    mean_cut [n_cut, 5] / mean_free [2], and n_scored (int64 [1]), their number."""
    cutoffs: tuple
    per_user: torch.Tensor
    per_user_free: torch.Tensor
    mean_cut: torch.Tensor
    mean_free: torch.Tensor
    n_scored: torch.Tensor


def _cutoffs(cutoffs) -> tuple:
    try:
        ks = tuple(cutoffs)
    except TypeError:
        raise ValueError(f"cutoffs must be a sequence of ints, got {cutoffs!r}") from None
    if len(ks) > RANK_MAX_CUTOFFS:
        raise ValueError(f"at most {RANK_MAX_CUTOFFS} cutoffs, got {len(ks)}")
    for k in ks:
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= RANK_MAX_K:
            raise ValueError(f"a cutoff must be an int in [1, {RANK_MAX_K}], got {k!r}")
    return ks


def rank_metrics(positions, test_off, n_neg, cutoffs) -> RankMetrics:
    """Ranking metrics of eval_positions_multi's positions, reduced on the device
    in fp64 (acf_eval_rank_metrics; definitions in include/acf_apr.h and
    evaluate.metrics_from_positions_multi, the host yardstick).  positions int32
    [T] and n_neg int32 [n] (>= 1: the user's candidates that are not test items)
    are device tensors, test_off the lists' CSR offsets [n + 1], cutoffs up to 8
    ints in [1, 1024].  Deterministic: equal inputs give equal bits."""
    ks = _cutoffs(cutoffs)
    _require(positions, "positions", torch.int32, None, 1)
    dev = positions.device
    _require(n_neg, "n_neg", torch.int32, dev, 1)
    n, T = n_neg.numel(), positions.numel()
    toff = _csr_offsets(test_off, n, T, "test_off").to(device=dev, dtype=torch.int64).contiguous()
    nc = len(ks)
    out = RankMetrics(ks, torch.empty((n, nc, 5), dtype=torch.float64, device=dev),
                      torch.empty((n, 2), dtype=torch.float64, device=dev),
                      torch.empty((nc, 5), dtype=torch.float64, device=dev),
                      torch.empty(2, dtype=torch.float64, device=dev),
                      torch.empty(1, dtype=torch.int64, device=dev))
    cuts = (ctypes.c_int32 * max(nc, 1))(*ks)
    if T == 0:  # every list is empty: nothing is read, but the pointer must not be NULL
        positions = torch.zeros(1, dtype=torch.int32, device=dev)
    with _on(dev):
        call("acf_eval_rank_metrics", positions.data_ptr(), toff.data_ptr(), n, n_neg.data_ptr(), cuts, nc,
             out.per_user.data_ptr(), out.per_user_free.data_ptr(), out.mean_cut.data_ptr(),
             out.mean_free.data_ptr(), out.n_scored.data_ptr(), _stream_ptr(dev))
    return out


# ---- list-level robustness: list overlap and item exposure ----
LIST_METRICS = ("overlap", "jaccard", "rbo")                                   # LST_NM
EXPOSURE_METRICS = ("total", "coverage", "gini", "entropy", "arp", "aplt")     # LSM_NM


@dataclass
class ListCompare:
    """What list_compare returns (device tensors): per_user fp64 [n, n_cut, 3] in
    LIST_METRICS order, mean fp64 [n_cut, 3] over the scored rows (those where a
    list holds at least one id) and n_scored int64 [n_cut], their number."""
    cutoffs: tuple
    per_user: torch.Tensor
    mean: torch.Tensor
    n_scored: torch.Tensor


def _id_lists(t, name: str) -> None:
    """TypeError / ValueError unless t is a contiguous 2-D int32 tensor [n, k],
    1 <= k <= TOPK_MAX_K; the device is the caller's to check, after its host
    arguments."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
        raise TypeError(f"{name} must be a torch.int32 tensor")
    if t.dim() != 2:
        raise ValueError(f"{name} must be 2-D [n, k], got shape {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if not 1 <= t.shape[1] <= TOPK_MAX_K:
        raise ValueError(f"{name}: k must lie in [1, {TOPK_MAX_K}], got {t.shape[1]}")


def _list_cutoffs(cutoffs, k: int):
    """The cutoffs of a [n, k] list array as a tuple and a C array: 1 to 8 ints in [1, k]."""
    ks = _cutoffs(cutoffs)
    if not ks:
        raise ValueError("cutoffs must hold at least one value")
    for c in ks:
        if c > k:
            raise ValueError(f"a cutoff must lie in [1, k = {k}], got {c}")
    return ks, (ctypes.c_int32 * len(ks))(*ks)


def _hip(t, name: str, dev=None):
    if t.device.type != "cuda":
        raise ValueError(f"{name} must live on a HIP device (got {t.device}); there is no CPU path")
    if dev is not None and t.device != dev:
        raise ValueError(f"{name} is on {t.device}, expected {dev}")
    return t.device


def list_compare(A, B, cutoffs, p: float = 0.9) -> ListCompare:
    """How far the lists B differ from the lists A, row by row (acf_list_compare;
    definitions in include/acf_apr.h, tests/lists_ref.py is the numpy yardstick).
    A, B: device int32 [n, k] as recommend_topk writes them (-1: none), k <= 128;
    cutoffs: 1 to 8 ints in [1, k]; p: the rank-biased overlap's persistence in
    (0, 1).  Per row and cutoff: overlap (an integer), jaccard, extrapolated rbo.
    Exact integers and fp64 in a fixed order: equal inputs give equal bits."""
    _id_lists(A, "A")
    _id_lists(B, "B")
    if A.shape != B.shape:
        raise ValueError(f"A and B must have one shape, got {tuple(A.shape)} and {tuple(B.shape)}")
    n, k = A.shape
    ks, cuts = _list_cutoffs(cutoffs, k)
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 < float(p) < 1.0:
        raise ValueError(f"p must lie in (0, 1), got {p!r}")
    dev = _hip(A, "A")
    _hip(B, "B", dev)
    nc = len(ks)
    out = ListCompare(ks, torch.zeros((n, nc, 3), dtype=torch.float64, device=dev),
                      torch.zeros((nc, 3), dtype=torch.float64, device=dev),
                      torch.zeros(nc, dtype=torch.int64, device=dev))
    if n == 0:
        return out
    with _on(dev):
        call("acf_list_compare", A.data_ptr(), B.data_ptr(), n, k, cuts, nc, float(p), out.per_user.data_ptr(),
             out.mean.data_ptr(), out.n_scored.data_ptr(), _stream_ptr(dev))
    return out


def _check_num_items(num_items) -> None:
    if isinstance(num_items, bool) or not isinstance(num_items, int) or not 1 <= num_items < 1 << 31:
        raise ValueError(f"num_items must be an int in [1, 2^31), got {num_items!r}")


def list_exposure(lists, num_items: int, cutoffs) -> torch.Tensor:
    """How often the lists recommend each item: counts int32 [n_cut, num_items],
    counts[c, i] = the number of rows that hold item i among their first
    cutoffs[c] entries (acf_list_exposure).  lists: device int32 [n, k]; entries
    outside [0, num_items) are ignored.  Integer atomics only: exact."""
    _id_lists(lists, "lists")
    n, k = lists.shape
    ks, cuts = _list_cutoffs(cutoffs, k)
    _check_num_items(num_items)
    if n * k >= 1 << 31:
        raise ValueError("n * k must stay below 2^31")
    if num_items * n * k >= 1 << 63:
        raise ValueError("num_items * n * k must stay below 2^63 (the Gini numerator is an int64)")
    dev = _hip(lists, "lists")
    counts = torch.zeros((len(ks), num_items), dtype=torch.int32, device=dev)
    if n == 0:
        return counts
    with _on(dev):
        call("acf_list_exposure", lists.data_ptr(), n, k, num_items, cuts, len(ks), counts.data_ptr(),
             _stream_ptr(dev))
    return counts


def exposure_metrics_workspace(num_items: int, n_cutoffs: int) -> int:
    """Bytes of device workspace acf_exposure_metrics needs (a host-only query)."""
    _check_num_items(num_items)
    if isinstance(n_cutoffs, bool) or not isinstance(n_cutoffs, int) or not 1 <= n_cutoffs <= RANK_MAX_CUTOFFS:
        raise ValueError(f"n_cutoffs must be an int in [1, {RANK_MAX_CUTOFFS}], got {n_cutoffs!r}")
    return _workspace_bytes("acf_exposure_metrics_workspace", num_items, n_cutoffs)


def exposure_metrics(counts, pop=None, tail=None) -> torch.Tensor:
    """Exposure metrics of list_exposure's counts: fp64 [n_cut, 6] in
    EXPOSURE_METRICS order (acf_exposure_metrics: total, catalogue coverage, Gini
    index, entropy in bits, average popularity of what is recommended, long-tail
    share).  pop: device int32 [num_items], each item's training interactions;
    tail: device uint8 (or bool) [num_items], nonzero for a long-tail item; None:
    that column is 0.  All but the entropy are one fp64 division of exact
    integers; the entropy is summed in a fixed order."""
    if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32:
        raise TypeError("counts must be a torch.int32 tensor")
    if counts.dim() != 2 or not counts.is_contiguous():
        raise ValueError(f"counts must be a contiguous 2-D [n_cut, num_items] tensor, got shape {tuple(counts.shape)}")
    nc, N = counts.shape
    if not 1 <= nc <= RANK_MAX_CUTOFFS or N < 1:
        raise ValueError(f"counts must be [1..{RANK_MAX_CUTOFFS}, >= 1], got shape {tuple(counts.shape)}")
    for t, name, dtypes in ((pop, "pop", (torch.int32,)), (tail, "tail", (torch.uint8, torch.bool))):
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.dtype not in dtypes:
            raise TypeError(f"{name} must be a torch.{str(dtypes[0]).split('.')[-1]} tensor")
        if t.dim() != 1 or t.numel() != N or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous 1-D tensor of num_items = {N} entries, got shape "
                             f"{tuple(t.shape)}")
    dev = _hip(counts, "counts")
    for t, name in ((pop, "pop"), (tail, "tail")):
        if t is not None:
            _hip(t, name, dev)
    out = torch.empty((nc, 6), dtype=torch.float64, device=dev)
    nbytes = exposure_metrics_workspace(N, nc)
    work = _workspace(nbytes, 8, dev)
    with _on(dev):
        call("acf_exposure_metrics", counts.data_ptr(), N, nc, _ptr(pop), _ptr(tail), out.data_ptr(),
             work.data_ptr(), nbytes, _stream_ptr(dev))
    return out


# ---- diversity: intra-list similarity and MMR re-ranking ----
def _metric_id(metric) -> int:
    if metric not in NEIGHBOR_METRICS:
        raise ValueError(f"metric must be one of {sorted(NEIGHBOR_METRICS)}, got {metric!r}")
    return NEIGHBOR_METRICS[metric]


def _sim_table(T) -> None:
    """TypeError / ValueError unless T is a contiguous 2-D float32 tensor with at
    least one row and a dim the ranking calls take; its device is checked last."""
    if not isinstance(T, torch.Tensor) or T.dtype != torch.float32 or T.dim() != 2:
        raise TypeError("T must be a 2-D torch.float32 tensor")
    if not T.is_contiguous():
        raise ValueError("T must be contiguous")
    rows, d = T.shape
    if rows < 1 or not 4 <= d <= 1024 or d % 4:
        raise ValueError(f"T must be [>= 1, dim] with dim a multiple of 4 in [4, 1024], got shape {tuple(T.shape)}")


def list_similarity(T, lists, cutoffs, metric: str = "cosine", check: bool = True):
    """Intra-list similarity of the lists under table T (acf_list_similarity;
    tests/diverse_ref.py is the numpy yardstick): (ils fp64 [n, n_cut], means fp64
    [n_cut]) device tensors.  lists: device int32 [n, k], k <= 128, a negative
    entry is "none"; cutoffs: 1 to 8 ints in [1, k]; metric as neighbors_topk's.
    ils[r, c] is the mean similarity over the pairs of valid entries among the
    first cutoffs[c] of row r, the pairs added in fp64 in a fixed order and divided
    once; a row with fewer than 2 valid entries there gets 0.0 and is left out of
    means[c].  Equal inputs give equal bits.  An id >= the table's rows is read as
    row 0; with check the call then raises NativeIndexError (one sync, after its
    launches).  Bad types, shapes, cutoffs and metric raise before any launch."""
    _sim_table(T)
    _id_lists(lists, "lists")
    n, k = lists.shape
    ks, cuts = _list_cutoffs(cutoffs, k)
    mid = _metric_id(metric)
    dev = _hip(T, "T")
    _hip(lists, "lists", dev)
    ils = torch.zeros((n, len(ks)), dtype=torch.float64, device=dev)
    means = torch.zeros(len(ks), dtype=torch.float64, device=dev)
    if n == 0:
        return ils, means
    settle_tables()
    with _on(dev):
        call("acf_list_similarity", T.data_ptr(), T.shape[0], T.shape[1], lists.data_ptr(), n, k, cuts, len(ks), mid,
             ils.data_ptr(), means.data_ptr(), int(bool(check)), _stream_ptr(dev))
    return ils, means


def rerank_mmr(T, cand, rel, k: int, lam: float, metric: str = "cosine", check: bool = True):
    """Greedy maximal-marginal-relevance re-ranking of candidate pools
    (acf_rerank_mmr): (items int32 [n, k], rel float32 [n, k], obj float32 [n, k])
    device tensors.  cand: device int32 [n, m], m <= 128; rel: device float32
    [n, m], the pool's relevances; an entry counts if its id is >= 0 and its
    relevance finite.  The first pick maximises lam * rel; every later one lam *
    rel - (1 - lam) * max over the picks so far of sim(entry, pick), sim being
    neighbors_topk's `metric` between rows of T; ties go to the lower pool position.
    obj is the value each pick was made at; -1 / -inf / -inf once a pool runs out.
    lam = 1 keeps the order of relevance, lam = 0 looks at similarity alone.  Every
    operation is fp32 and rounded on its own: equal inputs give equal bits.  An id
    >= the table's rows is read as row 0; with check the call then raises
    NativeIndexError (one sync, after its launches).  Bad types, shapes, k, lam and
    metric raise before any launch."""
    _sim_table(T)
    _id_lists(cand, "cand")
    if not isinstance(rel, torch.Tensor) or rel.dtype != torch.float32:
        raise TypeError("rel must be a torch.float32 tensor")
    if rel.shape != cand.shape or not rel.is_contiguous():
        raise ValueError(f"rel must be contiguous with cand's shape {tuple(cand.shape)}, got {tuple(rel.shape)}")
    n, m = cand.shape
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= m:
        raise ValueError(f"k must be an int in [1, m = {m}], got {k!r}")
    if isinstance(lam, bool) or not isinstance(lam, (int, float)) or not 0.0 <= float(lam) <= 1.0:
        raise ValueError(f"lam must lie in [0, 1], got {lam!r}")
    mid = _metric_id(metric)
    dev = _hip(T, "T")
    _hip(cand, "cand", dev)
    _hip(rel, "rel", dev)
    items = torch.empty((n, k), dtype=torch.int32, device=dev)
    rel_out = torch.empty((n, k), dtype=torch.float32, device=dev)
    obj = torch.empty((n, k), dtype=torch.float32, device=dev)
    if n == 0:
        return items, rel_out, obj
    settle_tables()
    with _on(dev):
        call("acf_rerank_mmr", T.data_ptr(), T.shape[0], T.shape[1], cand.data_ptr(), rel.data_ptr(), n, m, k,
             float(lam), mid, items.data_ptr(), rel_out.data_ptr(), obj.data_ptr(), int(bool(check)), _stream_ptr(dev))
    return items, rel_out, obj


WORST_MAX_EPS = 8                       # EVW_MAX_EPS
WORST_SIDES = {"user": 0, "item": 1}


def _worst_eps(eps) -> tuple:
    """eps as a tuple of 1..WORST_MAX_EPS finite floats >= 0 (ValueError)."""
    try:
        es = tuple(float(e) for e in eps)
    except TypeError:
        raise ValueError(f"eps must be a sequence of numbers, got {eps!r}") from None
    if not 1 <= len(es) <= WORST_MAX_EPS:
        raise ValueError(f"1 to {WORST_MAX_EPS} eps per call, got {len(es)}")
    for e in es:
        if not (math.isfinite(e) and e >= 0.0):
            raise ValueError(f"eps must be finite and >= 0, got {e!r}")
    return es


def _cert_entries(P, Q, users, test_items, num_candidates, excl_off, excl_items, side):
    """The arguments eval_positions_worst and eval_radius share, checked and on the
    tables' device: (side code, users, test items, n, excl offsets, excl items, device)."""
    if side not in WORST_SIDES:
        raise ValueError(f"side must be one of {sorted(WORST_SIDES)}, got {side!r}")
    ti = _csr_items(test_items, "test_items")
    us = _csr_items(users, "users")
    n = us.numel()
    if ti.numel() != n:
        raise ValueError(f"test_items must have one entry per user: {ti.numel()} for {n}")
    _check_num_candidates(num_candidates)
    _table_types(P, Q)
    if num_candidates > Q.shape[0]:
        raise ValueError("num_candidates exceeds item rows")
    eoff, ex = _exclusions(excl_off, excl_items, n, P.device)
    dev = _table_pair(P, Q)
    settle_tables()
    return WORST_SIDES[side], _to_i32(us, dev), _to_i32(ti, dev), n, eoff, ex, dev


def eval_positions_worst_workspace(n_users: int, num_candidates: int, n_eps: int) -> int:
    """Bytes of device workspace acf_eval_positions_worst needs (a host-only query)."""
    return _workspace_bytes("acf_eval_positions_worst_workspace", n_users, num_candidates, n_eps)


def eval_positions_worst(P, Q, users, test_items, num_candidates: int, excl_off=None, excl_items=None,
                         eps=(0.0,), side: str = "user", check: bool = True):
    """Certified worst-case positions under an attack of budget eps
    (acf_eval_positions_worst): int32 [len(eps), n].  Entry r is row users[r] of
    P with the test item t = test_items[r] and the candidates [0, num_candidates)
    minus the SET of excl_items[excl_off[r]:excl_off[r+1]] (unsorted, repeated
    and out-of-range entries are fine; no exclusion arguments: nothing is
    excluded; t itself never counts).  side="user": any delta with |delta|_2 <=
    eps is added to the user row; side="item": every item row gets its own such
    delta.  worst[e, r] = the number of candidates that SOME admissible
    perturbation brings to score >= t (m_c <= eps |q_t - q_c|, or m_c <= 2 eps
    |p|, in fp32 as include/acf_apr.h states); no single perturbation lifts
    more, so worst < K certifies t in the top K.  eps = 0 gives
    eval_positions_multi's positions; rows do not decrease in eps.  Up to 8 eps
    per call share one sweep of the candidates.  Bad shapes, dtypes, eps and
    side raise ValueError / TypeError before any native call; with check, a
    user or test item outside its table raises NativeIndexError (one sync)."""
    es = _worst_eps(eps)
    sd, u, t, n, eoff, ex, dev = _cert_entries(P, Q, users, test_items, num_candidates, excl_off, excl_items, side)
    worst = torch.empty((len(es), n), dtype=torch.int32, device=dev)
    if n == 0:
        return worst
    nbytes = eval_positions_worst_workspace(n, num_candidates, len(es))
    work = _workspace(nbytes, 4, dev)
    ceps = (ctypes.c_float * len(es))(*es)
    with _on(dev):
        call("acf_eval_positions_worst", P.data_ptr(), Q.data_ptr(), P.shape[0], Q.shape[0], P.shape[1],
             u.data_ptr(), t.data_ptr(), n, num_candidates, _ptr(eoff), _ptr(ex), ceps, len(es), sd,
             worst.data_ptr(), work.data_ptr(), nbytes, int(bool(check)), _stream_ptr(dev))
    return worst


def eval_radius_workspace(n_users: int, num_candidates: int, k: int) -> int:
    """Bytes of device workspace acf_eval_radius needs (a host-only query)."""
    return _workspace_bytes("acf_eval_radius_workspace", n_users, num_candidates, k)


def eval_radius(P, Q, users, test_items, num_candidates: int, excl_off=None, excl_items=None, k: int = 10,
                side: str = "user", check: bool = True, workspace=None):
    """Certified radius (acf_eval_radius): (eps float32 [n, k], items int32 [n,
    k]).  Entries, candidates, exclusions and sides are eval_positions_worst's.
    Every candidate c has a smallest fp32 eps_c >= 0 at which that call's
    predicate counts it (0 when it already scores >= t, +inf when no finite
    budget lifts it); eps[r] are the k smallest of entry r ascending, ties to
    the lower item id, items[r] their candidates, +inf / -1 past the entry's
    candidates.  eps[r, j] is the certified radius at j + 1: for every finite e
    >= 0, eval_positions_worst(..., eps=(e,))[0, r] < j + 1 iff e < eps[r, j],
    exactly, so no perturbation within a smaller budget pushes t out of the top
    j + 1.  One sweep of the candidates whatever k (1..128); identical bits run
    to run.  workspace: None (allocated per call) or an int64 tensor on the
    tables' device of at least eval_radius_workspace(n, num_candidates, k)
    bytes, kept by a caller that repeats the call.  Bad shapes, dtypes, k, side
    and a short workspace raise ValueError / TypeError before any native call;
    with check, a user or test item outside its table raises NativeIndexError
    (one sync), without it such an index is read as row 0."""
    _check_k(k)
    sd, u, t, n, eoff, ex, dev = _cert_entries(P, Q, users, test_items, num_candidates, excl_off, excl_items, side)
    eps = torch.empty((n, k), dtype=torch.float32, device=dev)
    items = torch.empty((n, k), dtype=torch.int32, device=dev)
    if n == 0:
        return eps, items
    nbytes = eval_radius_workspace(n, num_candidates, k)
    if workspace is None:
        work = _workspace(nbytes, 8, dev)
    else:
        _require(workspace, "workspace", torch.int64, dev, 1)
        work = workspace
        if work.numel() * 8 < nbytes:
            raise ValueError(f"workspace too small: {work.numel() * 8} < {nbytes} bytes")
    with _on(dev):
        call("acf_eval_radius", P.data_ptr(), Q.data_ptr(), P.shape[0], Q.shape[0], P.shape[1], u.data_ptr(),
             t.data_ptr(), n, num_candidates, _ptr(eoff), _ptr(ex), k, sd, eps.data_ptr(), items.data_ptr(),
             work.data_ptr(), nbytes, int(bool(check)), _stream_ptr(dev))
    return eps, items


ADV_MODES = {"grad": 0, "random": 1}
ADV_MAX_TRIPLETS = (1 << 29) - 1


def adv_direction_workspace(n: int, num_user_rows: int, num_item_rows: int, dim: int) -> int:
    """Bytes of device workspace acf_adv_direction needs for n triplets (a host-only query)."""
    if not 0 <= int(n) <= ADV_MAX_TRIPLETS:
        raise ValueError(f"n must lie in [0, {ADV_MAX_TRIPLETS}], got {n}")
    return _workspace_bytes("acf_adv_direction_workspace", n, num_user_rows, num_item_rows, dim)


class AdvPlan:
    """What adv_plan returns: the part of the gradient direction that depends on
    the triplets alone (sorted term values, row offsets, range-error word) in a
    device buffer it owns, with the index tensors it was built from."""

    def __init__(self, user, item_pos, item_neg, num_user_rows: int, num_item_rows: int, buf, nbytes: int):
        self.user, self.item_pos, self.item_neg = user, item_pos, item_neg
        self.n = int(user.numel())
        self.num_user_rows, self.num_item_rows = int(num_user_rows), int(num_item_rows)
        self.buf, self.nbytes = buf, int(nbytes)

    @property
    def device(self):
        return self.buf.device

    def fits(self, P, Q) -> None:
        """ValueError unless the plan was built for tables of P's and Q's rows on their device."""
        if (P.shape[0], Q.shape[0]) != (self.num_user_rows, self.num_item_rows):
            raise ValueError(f"plan was built for {self.num_user_rows} x {self.num_item_rows} table rows, "
                             f"got {P.shape[0]} x {Q.shape[0]}")
        if P.device != self.device:
            raise ValueError(f"plan is on {self.device}, the tables on {P.device}")


def _triplet_lengths(user, item_pos, item_neg) -> int:
    n = len(user)
    if len(item_pos) != n or len(item_neg) != n:
        raise ValueError("user, item_pos and item_neg must have equal lengths")
    if n > ADV_MAX_TRIPLETS:
        raise ValueError(f"at most {ADV_MAX_TRIPLETS} triplets, got {n}")
    return n


def adv_plan(user, item_pos, item_neg, num_user_rows: int, num_item_rows: int, device=None, check: bool = True):
    """Plan the whole-stream gradient direction once (acf_adv_plan): the stable
    sort of the 4n terms by row and the row offsets, which depend on the triplets
    alone.  The AdvPlan serves adv_direction(plan=...) and adv_pgd(plan=...) for
    every table pair of these row counts.  device: default the index tensors'
    HIP device.  check: an index outside its table raises NativeIndexError."""
    n = _triplet_lengths(user, item_pos, item_neg)
    U1, I1 = int(num_user_rows), int(num_item_rows)
    if U1 <= 0 or I1 <= 0:
        raise ValueError("num_user_rows and num_item_rows must be positive")
    if device is None:
        if not isinstance(user, torch.Tensor) or user.device.type != "cuda":
            raise ValueError("adv_plan needs a HIP device: pass device= or device index tensors; there is no CPU path")
        device = user.device
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"adv_plan needs a HIP device (got {dev}); there is no CPU path")
    u, i, j = (_idx(x, nm, dev) for x, nm in ((user, "user"), (item_pos, "item_pos"), (item_neg, "item_neg")))
    if not (u.numel() == i.numel() == j.numel() == n):
        raise ValueError("user, item_pos and item_neg must have equal lengths")
    pb, wb = ctypes.c_size_t(), ctypes.c_size_t()
    _native.call("acf_adv_plan_workspace", n, U1, I1, ctypes.byref(pb), ctypes.byref(wb))
    buf = _workspace(pb.value, 8, dev)
    work = _workspace(wb.value, 8, dev) if wb.value else None
    with _on(dev):
        _native.call("acf_adv_plan", u.data_ptr() if n else None, i.data_ptr() if n else None,
                     j.data_ptr() if n else None, n, U1, I1, buf.data_ptr(), pb.value, _ptr(work), wb.value,
                     int(bool(check)), _stream_ptr(dev))
    return AdvPlan(u, i, j, U1, I1, buf, pb.value)


def _plan_type(plan) -> None:
    if not isinstance(plan, AdvPlan):
        raise TypeError(f"plan must be an AdvPlan (ops.adv_plan), got {type(plan).__name__}")


def _plan_matches(plan, P, Q, n: int) -> None:
    plan.fits(P, Q)
    if plan.n != n:
        raise ValueError(f"plan was built for {plan.n} triplets, got {n}")


def adv_direction(P, Q, user, item_pos, item_neg, adv: str = "grad", seed: int = 0, call: int = 1, t: int = 0,
                  clip_lo=CLIP_LO, clip_hi=CLIP_HI, check: bool = True, plan=None):
    """The adversarial direction of the WHOLE triplet stream as one batch
    (utils.py:145-154): dense unit-direction tables (nP [rows of P, d], nQ [rows of
    Q, d]); delta = direction * eps is adv_apply's job, so one direction serves
    every eps.  adv="grad" (APR.py:180-191): the l2-normalised gradient of the
    clean loss of all triplets; rows no triplet touches are exact zeros; the
    order in which a row's terms are added is a fixed function of the input
    order, so equal inputs give equal bits.  adv="random" (APR.py:170-177): every
    row is the step's l2-normalised truncated-normal draw for (seed, call, t,
    table, row); the triplets are not read.  P and Q are never written.
    check: an index outside its table raises NativeIndexError.
    plan: an AdvPlan of these triplets (adv_plan): grad mode skips the sort and
    takes acf_adv_direction_planned, the same bits; the indices are the plan's
    own (range-checked when it was built)."""
    if adv not in ADV_MODES:
        raise ValueError(f"adv must be one of {sorted(ADV_MODES)}, got {adv!r}")
    if plan is not None and adv == "grad":
        _plan_type(plan)
        n = _triplet_lengths(user, item_pos, item_neg)
        _table_pair(P, Q)
        _plan_matches(plan, P, Q, n)
        return _adv_direction_planned(P, Q, plan, clip_lo, clip_hi)[:2]
    n = len(user)
    if len(item_pos) != n or len(item_neg) != n:
        raise ValueError("user, item_pos and item_neg must have equal lengths")
    if n > ADV_MAX_TRIPLETS:
        raise ValueError(f"at most {ADV_MAX_TRIPLETS} triplets, got {n}")
    dev = _table_pair(P, Q)
    u, i, j = (_idx(x, nm, dev) for x, nm in ((user, "user"), (item_pos, "item_pos"), (item_neg, "item_neg")))
    if not (u.numel() == i.numel() == j.numel() == n):
        raise ValueError("user, item_pos and item_neg must have equal lengths")
    settle_tables()
    U1, I1, d = P.shape[0], Q.shape[0], P.shape[1]
    nP = torch.empty((U1, d), dtype=torch.float32, device=dev)
    nQ = torch.empty((I1, d), dtype=torch.float32, device=dev)
    grad = adv == "grad"
    nbytes = adv_direction_workspace(n, U1, I1, d) if grad and n else 0
    work = _workspace(nbytes, 8, dev) if nbytes else None  # (the allocator aligns far above the 16 bytes asked for)
    with _on(dev):
        _native.call("acf_adv_direction", P.data_ptr(), Q.data_ptr(), U1, I1, d, u.data_ptr() if n else None,
                     i.data_ptr() if n else None, j.data_ptr() if n else None, n, clip_lo, clip_hi, ADV_MODES[adv],
                     int(seed) & 0xFFFFFFFFFFFFFFFF, int(call) & 0xFFFFFFFF, int(t),
                     nP.data_ptr(), nQ.data_ptr(), _ptr(work), nbytes, int(bool(check)), _stream_ptr(dev))
    return nP, nQ


def _adv_direction_planned(P, Q, plan: AdvPlan, clip_lo=CLIP_LO, clip_hi=CLIP_HI, want_loss: bool = False):
    """(nP, nQ, loss float64 [1] or None) of acf_adv_direction_planned; arguments already checked."""
    dev = P.device
    settle_tables()
    U1, I1, d, n = P.shape[0], Q.shape[0], P.shape[1], plan.n
    nP = torch.empty((U1, d), dtype=torch.float32, device=dev)
    nQ = torch.empty((I1, d), dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float64, device=dev) if want_loss else None
    nbytes = adv_direction_workspace(n, U1, I1, d) if n else 0
    work = _workspace(nbytes, 8, dev) if nbytes else None
    with _on(dev):
        _native.call("acf_adv_direction_planned", P.data_ptr(), Q.data_ptr(), U1, I1, d,
                     plan.user.data_ptr() if n else None, plan.item_pos.data_ptr() if n else None,
                     plan.item_neg.data_ptr() if n else None, n, clip_lo, clip_hi, plan.buf.data_ptr(), plan.nbytes,
                     nP.data_ptr(), nQ.data_ptr(), _ptr(loss), _ptr(work), nbytes, _stream_ptr(dev))
    return nP, nQ, loss


PGD_SIDES = {"both": 0, "user": 1, "item": 2}  # ACF_ADV_SIDE_*
PGD_MAX_ITERS = 1024                           # ACF_ADV_PGD_MAX_ITERS


def pgd_arguments(eps, iters, alpha, side):
    """(eps, iters, alpha, side id) of adv_pgd after its checks (ValueError / TypeError);
    alpha None is 2.5 * eps / iters."""
    if isinstance(iters, bool) or not isinstance(iters, int):
        raise TypeError(f"iters must be an int, got {type(iters).__name__}")
    if not 1 <= iters <= PGD_MAX_ITERS:
        raise ValueError(f"iters must lie in [1, {PGD_MAX_ITERS}], got {iters}")
    eps = float(eps)
    if not (math.isfinite(eps) and eps >= 0):
        raise ValueError(f"eps must be finite and >= 0, got {eps}")
    alpha = 2.5 * eps / iters if alpha is None else float(alpha)
    if not (math.isfinite(alpha) and alpha >= 0):
        raise ValueError(f"alpha must be finite and >= 0, got {alpha}")
    if side not in PGD_SIDES:
        raise ValueError(f"side must be one of {sorted(PGD_SIDES)}, got {side!r}")
    return eps, iters, alpha, PGD_SIDES[side]


def adv_pgd_workspace(n: int, num_user_rows: int, num_item_rows: int, dim: int) -> int:
    """Bytes of device workspace acf_adv_pgd needs for n triplets (a host-only query)."""
    if not 0 <= int(n) <= ADV_MAX_TRIPLETS:
        raise ValueError(f"n must lie in [0, {ADV_MAX_TRIPLETS}], got {n}")
    return _workspace_bytes("acf_adv_pgd_workspace", n, num_user_rows, num_item_rows, dim)


def adv_pgd(P, Q, user, item_pos, item_neg, eps: float, iters: int = 10, alpha=None, side: str = "both", start=None,
            plan=None, check: bool = True, seed: int = 0, clip_lo=CLIP_LO, clip_hi=CLIP_HI):
    """An iterated gradient attack on the clean loss of the WHOLE triplet stream
    (acf_adv_pgd): (delta_P, delta_Q, losses).  From delta_0 = start, `iters` times:
    the l2-normalised per-row gradient direction n at (P + delta_P, Q + delta_Q)
    (adv_direction's, planned once), then on every moving side per row
    delta <- project(delta + alpha * n) onto the L2 ball of radius eps.
    alpha=None: 2.5 * eps / iters.  side: "both", or "user" / "item" to move only
    that table's delta (both tables always enter the gradient; the other delta
    stays at its start).  start: None (zeros), "random" (eps x adv_direction's
    random draw for (seed, call 1, t 0)) or (delta_P0, delta_Q0), taken as given.
    losses: float64 [iters + 1] on the device, losses[k] the stream's summed clean
    loss at iterate k.  plan: an AdvPlan of these triplets (adv_plan), else the
    call plans once.  Equal inputs give equal bits; P and Q are never written.
    Bad arguments raise ValueError / TypeError before any native call; check: an
    index outside its table raises NativeIndexError."""
    eps, iters, alpha, sd = pgd_arguments(eps, iters, alpha, side)
    n = _triplet_lengths(user, item_pos, item_neg)
    if plan is not None:
        _plan_type(plan)
    if isinstance(start, str):
        if start != "random":
            raise ValueError(f"start must be None, 'random' or (delta_P0, delta_Q0), got {start!r}")
    elif start is not None:
        if not isinstance(start, (tuple, list)) or len(start) != 2:
            raise TypeError("start must be None, 'random' or a (delta_P0, delta_Q0) pair")
        for t, w, nm in ((start[0], P, "delta_P0"), (start[1], Q, "delta_Q0")):
            if isinstance(t, torch.Tensor) and isinstance(w, torch.Tensor) and t.shape != w.shape:
                raise ValueError(f"{nm} {tuple(t.shape)} must have its table's shape {tuple(w.shape)}")
    dev = _table_pair(P, Q)
    if plan is not None:
        _plan_matches(plan, P, Q, n)
        u, i, j = plan.user, plan.item_pos, plan.item_neg
    else:
        u, i, j = (_idx(x, nm, dev) for x, nm in ((user, "user"), (item_pos, "item_pos"), (item_neg, "item_neg")))
        if not (u.numel() == i.numel() == j.numel() == n):
            raise ValueError("user, item_pos and item_neg must have equal lengths")
    if isinstance(start, (tuple, list)):
        _require(start[0], "delta_P0", torch.float32, dev, 2)
        _require(start[1], "delta_Q0", torch.float32, dev, 2)
    settle_tables()
    U1, I1, d = P.shape[0], Q.shape[0], P.shape[1]
    if isinstance(start, str):  # "random"
        rP, rQ = adv_direction(P, Q, u[:0], i[:0], j[:0], adv="random", seed=seed, call=1, t=0)
        start = (adv_apply(P, rP, eps, want_delta=True)[1], adv_apply(Q, rQ, eps, want_delta=True)[1])
    dP = torch.empty((U1, d), dtype=torch.float32, device=dev)
    dQ = torch.empty((I1, d), dtype=torch.float32, device=dev)
    losses = torch.empty(iters + 1, dtype=torch.float64, device=dev)
    nbytes = adv_pgd_workspace(n, U1, I1, d)
    work = _workspace(nbytes, 8, dev)
    with _on(dev):
        _native.call("acf_adv_pgd", P.data_ptr(), Q.data_ptr(), U1, I1, d, u.data_ptr() if n else None,
                     i.data_ptr() if n else None, j.data_ptr() if n else None, n, clip_lo, clip_hi,
                     plan.buf.data_ptr() if plan is not None else None, plan.nbytes if plan is not None else 0,
                     eps, alpha, iters, sd, start[0].data_ptr() if start is not None else None,
                     start[1].data_ptr() if start is not None else None, dP.data_ptr(), dQ.data_ptr(),
                     losses.data_ptr(), work.data_ptr(), nbytes, int(bool(check)), _stream_ptr(dev))
    return dP, dQ, losses


def adv_apply(W, N, eps: float, want_delta: bool = False):
    """sum = W + delta with delta = N * eps, two separately rounded fp32 operations
    (TF: l2_normalize(...) * eps, then embedding + delta): the perturbed table, or
    (sum, delta) with want_delta."""
    _require(W, "W", torch.float32, None, 2)
    _require(N, "N", torch.float32, W.device, 2)
    if W.shape != N.shape:
        raise ValueError(f"W {tuple(W.shape)} and N {tuple(N.shape)} differ in shape")
    dev = W.device
    out = torch.empty_like(W)
    delta = torch.empty_like(W) if want_delta else None
    with _on(dev):
        _native.call("acf_adv_apply", W.data_ptr(), N.data_ptr(), W.shape[0], W.shape[1], float(eps),
                     _ptr(delta), out.data_ptr(), _stream_ptr(dev))
    return (out, delta) if want_delta else out


FOLD_MAX_BATCH = 512  # ACF_FOLD_MAX_BATCH


def _fold_csr(off, n_entries: int, off_name: str, list_name: str):
    """The CSR offsets `off` as a host int64 array after the CSR checks (ValueError)."""
    import numpy as np
    off = off.detach().cpu().numpy() if isinstance(off, torch.Tensor) else np.asarray(off)
    if off.ndim != 1 or off.size < 1:
        raise ValueError(f"{off_name} must be 1-D with n + 1 entries, got shape {off.shape}")
    if off.dtype.kind not in "iu":
        raise ValueError(f"{off_name} must be an integer array, got {off.dtype}")
    off = off.astype(np.int64)
    if off[0] != 0:
        raise ValueError(f"{off_name}[0] must be 0, got {off[0]}")
    if (np.diff(off) < 0).any():
        raise ValueError(f"{off_name} must be non-decreasing")
    if off[-1] != n_entries:
        raise ValueError(f"{off_name}[-1] must be len({list_name}) = {n_entries}, got {off[-1]}")
    return off


def _fold_items(t, name: str, device, shape) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t)
    if t.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{name} must be int32 or int64, got {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    return t.to(device=device, dtype=torch.int32).contiguous()


def _fold_table(t, name: str, device, shape=None) -> int:
    try:
        ptr = _require(t, name, torch.float32, device, 2)
    except TypeError as e:
        raise ValueError(str(e)) from None
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    return ptr


def _fold_in(entry: str, tables, off_name: str, off_in, list_name: str, first, item_neg, hp, epochs, batch, init,
             acc_init, check):
    """fold_in_users / fold_in_items behind their argument names: the checks, in
    one order, and the call.  tables: [(tensor, name)], the frozen tables in the
    entry point's order; the CSR (off_in, first) indexes rows of the first."""
    if not isinstance(hp, StepHParams):
        raise ValueError(f"hp must be a StepHParams, got {type(hp).__name__}")
    if hp.adv != "grad" or hp.zero_delta:
        raise ValueError("fold-in takes only the gradient delta: adv='grad' and zero_delta=0 "
                         f"(got adv={hp.adv!r}, zero_delta={hp.zero_delta})")
    if isinstance(batch, bool) or not isinstance(batch, int) or not 1 <= batch <= FOLD_MAX_BATCH:
        raise ValueError(f"batch must be an int in [1, {FOLD_MAX_BATCH}], got {batch!r}")
    if isinstance(epochs, bool) or not isinstance(epochs, int) or epochs < 0:
        raise ValueError(f"epochs must be an int >= 0, got {epochs!r}")
    T = len(first)
    off = _fold_csr(off_in, T, off_name, list_name)
    n = off.size - 1
    if tuple(getattr(item_neg, "shape", ())) != (epochs, T):
        raise ValueError(f"item_neg must have shape (epochs, len({list_name})) = {(epochs, T)}, "
                         f"got {tuple(getattr(item_neg, 'shape', ()))}")
    (t0, name0), rest = tables[0], tables[1:]
    _fold_table(t0, name0, None)
    dev, d = t0.device, t0.shape[1]
    for t, name in rest:
        _fold_table(t, name, dev)
        if t.shape[1] != d:
            raise ValueError(f"{name0} and {name} differ in dim: {d} and {t.shape[1]}")
    if d < 4 or d > 1024 or d % 4:
        raise ValueError(f"dim must be a multiple of 4 in [4, 1024], got {d}")
    rows = _fold_items(first, list_name, dev, (T,))
    ineg = _fold_items(item_neg, "item_neg", dev, (epochs, T))
    if init is not None:
        _fold_table(init, "init", dev, (n, d))
    if acc_init is not None:
        _fold_table(acc_init, "acc_init", dev, (n, d))
    offd = (off_in if isinstance(off_in, torch.Tensor) and off_in.dtype == torch.int64
            and off_in.device == dev and off_in.is_contiguous()
            else torch.as_tensor(off).to(dev))
    settle_tables()
    W_new = torch.empty((n, d), dtype=torch.float32, device=dev)
    acc_new = torch.empty((n, d), dtype=torch.float32, device=dev)
    loss = torch.empty((epochs, n), dtype=torch.float32, device=dev)
    if n == 0:
        return W_new, acc_new, loss
    c = hp.to_c()
    with _on(dev):
        call(entry, *[x for t, _ in tables for x in (t.data_ptr(), t.shape[0])], d, offd.data_ptr(), n,
             rows.data_ptr() if T else None, ineg.data_ptr() if T and epochs else None, T, epochs, batch,
             ctypes.byref(c), init.data_ptr() if init is not None else None,
             acc_init.data_ptr() if acc_init is not None else None, W_new.data_ptr(), acc_new.data_ptr(),
             loss.data_ptr() if epochs else None, int(bool(check)), _stream_ptr(dev))
    return W_new, acc_new, loss


def fold_in_users(Q, user_off, item_pos, item_neg, hp: StepHParams, epochs: int, batch: int = FOLD_MAX_BATCH,
                  init=None, acc_init=None, check: bool = True):
    """Rows for n NEW users fitted against the frozen item table Q, on the GPU
    (acf_fold_in_users): (P_new [n, d], acc_new [n, d], loss [epochs, n]).
    User r owns item_pos[user_off[r]:user_off[r+1]] (CSR; user_off int64 [n + 1],
    item_pos int32 [T]); item_neg [epochs, T] holds one negative per positive per
    epoch.  For every epoch, every consecutive slice of at most `batch` positions
    of a user's list is one training_batch iteration (APR.py:143-195) on the
    one-row user table [p_r] and Q: with hp.adver the step's own gradient delta
    (of p_r and of every item row of the slice), reg as in the step; only p_r and
    its Adagrad accumulator are kept, Q is never written.  init / acc_init [n, d]
    (default zeros / 0.1): pass a previous (P_new, acc_new) to continue a fit.
    loss[e, r]: the user's clean loss of epoch e, each slice before its update.
    A user's outputs depend on that user's inputs only, bit for bit, and equal
    inputs give equal bits.  Bad arguments raise ValueError before any native
    call; with check, an item outside Q raises NativeIndexError."""
    return _fold_in("acf_fold_in_users", [(Q, "embedding_Q")], "user_off", user_off, "item_pos", item_pos, item_neg,
                    hp, epochs, batch, init, acc_init, check)


def fold_in_items(P, Q, item_off, user_pos, item_neg, hp: StepHParams, epochs: int, batch: int = FOLD_MAX_BATCH,
                  init=None, acc_init=None, check: bool = True):
    """Rows for n NEW items fitted against the frozen tables P and Q, on the GPU
    (acf_fold_in_items): (Q_new [n, d], acc_new [n, d], loss [epochs, n]).
    New item r owns user_pos[item_off[r]:item_off[r+1]] (CSR; item_off int64
    [n + 1], user_pos int32 [T]: the users who interacted with it); item_neg
    [epochs, T] holds one negative item (a row of Q) per position per epoch.  For
    every epoch, every consecutive slice of at most `batch` positions of an item's
    list is one training_batch iteration (APR.py:143-195) on P and [Q ; q_r] with
    the new item as the positive of every triplet: with hp.adver the step's own
    gradient delta (of q_r, of every user row and of every negative row of the
    slice), reg as in the step; only q_r and its Adagrad accumulator are kept, P
    and Q are never written.  init / acc_init [n, d] (default zeros / 0.1): pass a
    previous (Q_new, acc_new) to continue a fit.  loss[e, r]: the item's clean
    loss of epoch e, each slice before its update.  An item's outputs depend on
    that item's inputs only, bit for bit, and equal inputs give equal bits.  Bad
    arguments raise ValueError before any native call; with check, a user outside
    P or a negative outside Q raises NativeIndexError."""
    return _fold_in("acf_fold_in_items", [(P, "embedding_P"), (Q, "embedding_Q")], "item_off", item_off, "user_pos",
                    user_pos, item_neg, hp, epochs, batch, init, acc_init, check)


GRID_MAX_MODELS = 64    # ACF_GRID_MAX_MODELS
GRID_MAX_BATCH = 1024   # ACF_GRID_MAX_BATCH
GRID_MAX_DIM = 256
GRID_MAX_ADV_ITERS = 32  # ACF_GRID_MAX_ADV_ITERS


def grid_workspace(n_models: int, batch_size: int, n_batches: int, num_user_rows: int, num_item_rows: int,
                   dim: int) -> int:
    """Bytes of workspace grid_train needs (acf_apr_grid_workspace; host only)."""
    return _workspace_bytes("acf_apr_grid_workspace", n_models, batch_size, n_batches, num_user_rows, num_item_rows,
                            dim)


def grid_pgd_workspace(n_models: int, batch_size: int, n_batches: int, num_user_rows: int, num_item_rows: int,
                       dim: int) -> int:
    """Bytes of workspace grid_train needs when a member has adv_iters > 1
    (acf_apr_grid_pgd_workspace; host only): grid_workspace plus the second delta buffer."""
    return _workspace_bytes("acf_apr_grid_pgd_workspace", n_models, batch_size, n_batches, num_user_rows,
                            num_item_rows, dim)


def grid_pgd_arguments(h: StepHParams, m: int = 0):
    """(adv_iters, adv_step) of grid member m after their checks (ValueError / TypeError);
    adv_step None is 2.5 * eps / adv_iters (pgd_arguments' default)."""
    K = h.adv_iters
    if isinstance(K, bool) or not isinstance(K, int):
        raise TypeError(f"hparams[{m}]: adv_iters must be an int, got {type(K).__name__}")
    if not 1 <= K <= GRID_MAX_ADV_ITERS:
        raise ValueError(f"hparams[{m}]: adv_iters must lie in [1, {GRID_MAX_ADV_ITERS}], got {K}")
    alpha = 2.5 * float(h.eps) / K if h.adv_step is None else float(h.adv_step)
    if not (math.isfinite(alpha) and alpha >= 0):
        if h.adv_step is not None or K > 1:
            raise ValueError(f"hparams[{m}]: adv_step must be finite and >= 0, got {alpha!r}")
        alpha = 0.0  # a one-step member never reads it
    return K, alpha


def grid_train(P, Q, accP, accQ, hparams, user, item_pos, item_neg, batch_size: int, *, losses: bool = False,
               check: bool = True):
    """training_batch for M models over ONE triplet stream in one call
    (acf_apr_grid_train), in place.  P, accP [M, user rows, d] and Q, accQ
    [M, item rows, d] are member-major, so P[m] is an ordinary dense table;
    hparams is a sequence of M StepHParams (lr, eps, reg, reg_adv, adver, clip_lo,
    clip_hi per member; adv="random" and zero_delta are not grid modes); the
    triplets (int32, a multiple of batch_size long) are shared by all members.
    d is a multiple of 4 in [4, 256], 1 <= M <= 64, 1 <= batch_size <= 1024.
    A member's result depends on its own tables and hparams and the triplets only,
    bit for bit, whatever M and its position are; equal inputs give equal bits.
    losses: return (loss_clean, loss_adv) [M, n] float32, the per-triplet losses of
    each batch before its update (loss_adv rows of members with adver = 0 stay 0);
    otherwise None.  A member with adv_iters = K > 1 trains against a K-step
    projected-gradient attack of step adv_step (None: 2.5 * eps / K) inside the
    eps ball instead of the one normalised gradient step; such a grid goes through
    acf_apr_grid_train_pgd, a grid of one-step members through acf_apr_grid_train
    as before, and a K = 1 member gives the same bits either way.  Bad arguments raise ValueError / TypeError before any native
    call; with check, an index outside its table raises NativeIndexError before
    any table is written."""
    hps = list(hparams)
    M = len(hps)
    if not 1 <= M <= GRID_MAX_MODELS:
        raise ValueError(f"a grid has 1 to {GRID_MAX_MODELS} members, got {M}")
    for m, h in enumerate(hps):
        if not isinstance(h, StepHParams):
            raise TypeError(f"hparams[{m}] must be a StepHParams, got {type(h).__name__}")
        if h.adv != "grad" or h.zero_delta:
            raise ValueError(f"hparams[{m}]: adv='random' and zero_delta are not grid modes")
    pgd = [grid_pgd_arguments(h, m) for m, h in enumerate(hps)]
    for t, n in ((P, "embedding_P"), (Q, "embedding_Q"), (accP, "accumulator_P"), (accQ, "accumulator_Q")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{n} must be a torch.Tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{n} must be torch.float32, got {t.dtype}")
        if t.dim() != 3 or t.shape[0] != M:
            raise ValueError(f"{n} must be [M = {M}, rows, d], got shape {tuple(t.shape)}")
    if accP.shape != P.shape or accQ.shape != Q.shape:
        raise ValueError(f"accumulator shapes {tuple(accP.shape)} / {tuple(accQ.shape)} differ from the tables' "
                         f"{tuple(P.shape)} / {tuple(Q.shape)}")
    d = P.shape[2]
    if Q.shape[2] != d:
        raise ValueError("embedding_P and embedding_Q dims differ")
    if d % 4 or not 4 <= d <= GRID_MAX_DIM:
        raise ValueError(f"grid dim must be a multiple of 4 in [4, {GRID_MAX_DIM}], got {d}")
    B = int(batch_size)
    if not 1 <= B <= GRID_MAX_BATCH:
        raise ValueError(f"batch_size must lie in [1, {GRID_MAX_BATCH}], got {batch_size}")
    n = len(user)
    if len(item_pos) != n or len(item_neg) != n:
        raise ValueError("user, item_pos and item_neg must have equal lengths")
    if n % B:
        raise ValueError(f"{n} triplets is not a multiple of batch_size {B}")
    dev = P.device
    for t, nm in ((P, "embedding_P"), (Q, "embedding_Q"), (accP, "accumulator_P"), (accQ, "accumulator_Q")):
        _require(t, nm, torch.float32, dev, 3)
    u, i, j = (_idx(x, nm, dev) for x, nm in ((user, "user"), (item_pos, "item_pos"), (item_neg, "item_neg")))
    settle_tables()
    nb = n // B
    U1, I1 = P.shape[1], Q.shape[1]
    lc = torch.zeros((M, n), dtype=torch.float32, device=dev) if losses else None
    la = torch.zeros((M, n), dtype=torch.float32, device=dev) if losses else None
    chp = (HParams * M)(*[h._struct() for h in hps])
    if all(K == 1 for K, _ in pgd):
        entry, extra = "acf_apr_grid_train", ()
        nbytes = grid_workspace(M, B, nb, U1, I1, d)
    else:
        entry = "acf_apr_grid_train_pgd"
        extra = ((ctypes.c_int32 * M)(*[K for K, _ in pgd]), (ctypes.c_float * M)(*[a for _, a in pgd]))
        nbytes = grid_pgd_workspace(M, B, nb, U1, I1, d)
    work = _workspace(nbytes, 8, dev)
    with _on(dev):
        call(entry, P.data_ptr(), Q.data_ptr(), accP.data_ptr(), accQ.data_ptr(), M, U1, I1, d, chp, *extra,
             u.data_ptr() if n else None, i.data_ptr() if n else None, j.data_ptr() if n else None, B, nb,
             _ptr(lc), _ptr(la), work.data_ptr(), nbytes, int(bool(check)), _stream_ptr(dev))
    return (lc, la) if losses else None


def eval_positions_list(P, Q, users, test_items, cand_off, cand_items):
    """_eval_by_user positions over explicit candidate lists ("sample" mode)."""
    settle_tables()
    dev = P.device
    _require(P, "embedding_P", torch.float32, None, 2)
    _require(Q, "embedding_Q", torch.float32, dev, 2)
    u, t = _idx(users, "users", dev), _idx(test_items, "test_items", dev)
    off = torch.as_tensor(cand_off).to(device=dev, dtype=torch.int64).contiguous()
    c = _idx(cand_items, "cand_items", dev) if len(cand_items) else torch.zeros(1, dtype=torch.int32, device=dev)
    _check_range(u, P.shape[0], "user")
    _check_range(t, Q.shape[0], "item")
    _check_range(c, Q.shape[0], "item")
    pos = torch.empty(u.numel(), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        call("acf_eval_positions_list", P.data_ptr(), Q.data_ptr(), P.shape[0], Q.shape[0], P.shape[1],
             u.data_ptr(), t.data_ptr(), u.numel(), off.data_ptr(), c.data_ptr(), pos.data_ptr(),
             _stream_ptr(dev))
    return pos


def alias_table(weights):
    """(prob, alias) float32 / int32 numpy arrays of Vose's alias table for
    sampling k with probability weights[k] / sum(weights) (acf_alias_build)."""
    import numpy as np
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.float32).reshape(-1))
    prob = np.empty(w.size, np.float32)
    alias = np.empty(w.size, np.int32)
    call("acf_alias_build", w.ctypes.data, w.size, prob.ctypes.data, alias.ctypes.data)
    return prob, alias


def sample_epoch(pos_user, pos_item, batch_size: int, num_items: int, list_off, list_items,
                 seed: int, max_tries: int = 1 << 20, check: bool = True, alias=None):
    """Device-side shuffle + negative sampling for one epoch (APR.py:39-81).
    alias: None (uniform proposals, APR.py:76) or a (prob, alias) pair of device
    tensors from alias_table (acf_sample_epoch_alias)."""
    dev = pos_user.device
    pu = _idx(pos_user, "pos_user", dev)
    pi = _idx(pos_item, "pos_item", dev)
    off = torch.as_tensor(list_off).to(device=dev, dtype=torch.int64).contiguous()
    li = _idx(list_items, "list_items", dev) if len(list_items) else torch.zeros(1, dtype=torch.int32, device=dev)
    n_out = (pu.numel() // batch_size) * batch_size
    ou = torch.empty(n_out, dtype=torch.int32, device=dev)
    op = torch.empty(n_out, dtype=torch.int32, device=dev)
    on = torch.empty(n_out, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        if alias is None:
            call("acf_sample_epoch", pu.data_ptr(), pi.data_ptr(), pu.numel(), batch_size, int(num_items),
                 off.numel() - 1, off.data_ptr(), li.data_ptr(), int(seed) & 0xFFFFFFFFFFFFFFFF,
                 int(max_tries), int(check), ou.data_ptr(), op.data_ptr(), on.data_ptr(), _stream_ptr(dev))
        else:
            prob, al = alias
            _require(prob, "alias prob", torch.float32, dev, 1)
            _require(al, "alias", torch.int32, dev, 1)
            if prob.numel() != num_items or al.numel() != num_items:
                raise ValueError(f"alias table has {prob.numel()} columns, expected num_items = {num_items}")
            call("acf_sample_epoch_alias", pu.data_ptr(), pi.data_ptr(), pu.numel(), batch_size, int(num_items),
                 off.numel() - 1, off.data_ptr(), li.data_ptr(), prob.data_ptr(), al.data_ptr(),
                 int(seed) & 0xFFFFFFFFFFFFFFFF, int(max_tries), int(check), ou.data_ptr(), op.data_ptr(),
                 on.data_ptr(), _stream_ptr(dev))
    return ou, op, on


def dns_select(P, Q, user, cand, dns: int):
    """utils.py:121-133: argmax-score negative among dns candidates per triplet."""
    settle_tables()
    dev = P.device
    _require(P, "embedding_P", torch.float32, None, 2)
    _require(Q, "embedding_Q", torch.float32, dev, 2)
    u = _idx(user, "user", dev)
    c = _idx(cand, "cand", dev)
    if c.numel() != u.numel() * dns:
        raise ValueError("cand must hold dns candidates per triplet")
    _check_range(u, P.shape[0], "user")
    _check_range(c, Q.shape[0], "item")
    out = torch.empty(u.numel(), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        call("acf_dns_select", P.data_ptr(), Q.data_ptr(), P.shape[0], Q.shape[0], P.shape[1],
             u.data_ptr(), c.data_ptr(), u.numel(), int(dns), out.data_ptr(), _stream_ptr(dev))
    return out


def shard_reduce_delta(recv, seg, pos, hp: StepHParams, G0, reply) -> None:
    """Owner side of the APR delta (APR.py:183-191): per owned row s, the partial
    clean sums recv[pos[seg[s]:seg[s+1]]] in order -> G0[s]; eps * l2_normalize
    of it -> reply[pos[...]] (include/acf_apr.h acf_shard_reduce_delta)."""
    n = seg.numel() - 1
    if n <= 0:
        return
    dev = recv.device
    for t, nm, dt in ((recv, "recv", torch.float32), (G0, "G0", torch.float32), (reply, "reply", torch.float32),
                      (seg, "seg", torch.int32), (pos, "pos", torch.int32)):
        _require(t, nm, dt, dev)
    h = hp.to_c()
    with torch.cuda.device(dev):
        call("acf_shard_reduce_delta", recv.data_ptr(), seg.data_ptr(), pos.data_ptr(), n, recv.shape[1],
             ctypes.byref(h), G0.data_ptr(), reply.data_ptr(), _stream_ptr(dev))


def shard_reduce_apply(Q, accQ, recv, seg, pos, hp: StepHParams, G0, rows, count=None, reg_batch: int = 0) -> None:
    """Owner side of the item Adagrad (APR.py:193-195): per owned row s,
    G0[s] + reg_adv * sum of its partial adversarial rows (BPR: the sum of its
    partial clean rows), then sparse Adagrad on Q[rows[s]], accQ[rows[s]]."""
    n = seg.numel() - 1
    if n <= 0:
        return
    dev = recv.device
    for t, nm, dt in ((Q, "Q", torch.float32), (accQ, "accQ", torch.float32), (recv, "recv", torch.float32),
                      (seg, "seg", torch.int32), (pos, "pos", torch.int32), (rows, "rows", torch.int32)):
        _require(t, nm, dt, dev)
    h = hp.to_c()
    with torch.cuda.device(dev):
        call("acf_shard_reduce_apply", Q.data_ptr(), accQ.data_ptr(), recv.data_ptr(), seg.data_ptr(),
             pos.data_ptr(), n, Q.shape[1], ctypes.byref(h), 0 if G0 is None else G0.data_ptr(),
             rows.data_ptr(), 0 if count is None else count.data_ptr(), int(reg_batch), _stream_ptr(dev))
