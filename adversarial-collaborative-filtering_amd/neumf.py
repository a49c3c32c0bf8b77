"""NeuMF and adversarial NeuMF on the GPU (libacf_neumf.so, include/acf_neumf.h).

``NeuMF(uNum, iNum, mf_dim)`` is the reference's Keras model (NeuMF.py:10-52)
behind the Recommender API run.py drives (run.py:142-146,242-248):
``get_train_instances`` (MF.py:42-56: one positive + one rejected negative per
training pair), ``train(x_train, y_train, batch_size)`` (MF.py:30-33: Keras
``fit(shuffle=True)``, mean binary cross-entropy, Adam, last partial batch kept,
returns the epoch's mean loss), ``rank(users, items)`` (MF.py:38-40: sigmoid
scores, shape [n, 1]) and ``save``.

``AdversarialNeuMF(uNum, iNum, mf_dim, weight, pop_percent)`` keeps the reference
signature (NeuMF.py:58-59).  The reference's discriminator version does not run
(NeuMF.py:131), so the adversary here is APR's: FGSM perturbations of the touched
rows of the four embedding tables (eps * g/|g| of the clean gradient), with the
adversarial loss weighted by ``weight`` (the role of its ``loss_weights``,
NeuMF.py:110).  ``pop_percent`` is accepted and unused.  oracle/neumf_oracle.py
states the arithmetic.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _native
from .ops import _idx, _require, _stream_ptr

NAMES = ("MF_U", "MF_I", "MLP_U", "MLP_I", "W1", "b1", "W2", "b2", "Wo", "bo")
RANK_MAX_K = 128  # TOPK_MAX_K of acf_topk_select.h


def rank_all_workspace(n_users: int, num_candidates: int, k: int) -> int:
    """Bytes of device workspace acf_neumf_rank_all needs (a host-only query)."""
    size = ctypes.c_size_t()
    _native.call_neumf("acf_neumf_rank_all_workspace", int(n_users), int(num_candidates), int(k),
                       ctypes.byref(size))
    return int(size.value)


def _int_vec(x, name: str):
    """A 1-D integer index argument (tensor or array-like; [N] or [N, 1]), checked on
    the host: TypeError for a non-integer dtype."""
    if isinstance(x, torch.Tensor):
        if x.dtype.is_floating_point or x.dtype.is_complex or x.dtype == torch.bool:
            raise TypeError(f"{name} must hold integers, got {x.dtype}")
        if x.dim() > 2 or (x.dim() == 2 and x.shape[1] != 1):
            raise ValueError(f"{name} must be [N] or [N, 1], got shape {tuple(x.shape)}")
        return x.reshape(-1)
    a = np.asarray(x)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"{name} must hold integers, got {a.dtype}")
    if a.ndim > 2 or (a.ndim == 2 and a.shape[1] != 1):
        raise ValueError(f"{name} must be [N] or [N, 1], got shape {a.shape}")
    return torch.as_tensor(a.reshape(-1).astype(np.int64, copy=False))


def _shapes(U1, I1, d):
    return {"MF_U": (U1, d), "MF_I": (I1, d), "MLP_U": (U1, d), "MLP_I": (I1, d),
            "W1": (2 * d, 2 * d), "b1": (2 * d,), "W2": (2 * d, d), "b2": (d,),
            "Wo": (2 * d, 1), "bo": (1,)}


class NeuMFState:
    """Flat fp32 parameter / gradient / Adam-moment buffers in the C-ABI layout,
    with per-tensor views (Keras names and shapes)."""

    def __init__(self, num_user_rows: int, num_item_rows: int, dim: int, device):
        self.U1, self.I1, self.d = int(num_user_rows), int(num_item_rows), int(dim)
        self.device = torch.device(device)
        lib = _native.load_neumf()
        n = lib.acf_neumf_param_count(self.U1, self.I1, self.d)
        if n < 0:
            raise ValueError(lib.acf_neumf_last_error().decode())
        off = (ctypes.c_int64 * 10)()
        _native.call_neumf("acf_neumf_param_offsets", self.U1, self.I1, self.d, off)
        self.offsets = list(off)
        f = dict(dtype=torch.float32, device=self.device)
        self.params = torch.zeros(n, **f)
        self.grad = torch.zeros(n, **f)
        self.m = torch.zeros(n, **f)
        self.v = torch.zeros(n, **f)
        self.t = 0  # Adam iterations done

    def view(self, name: str, buf: torch.Tensor | None = None) -> torch.Tensor:
        buf = self.params if buf is None else buf
        k = NAMES.index(name)
        shape = _shapes(self.U1, self.I1, self.d)[name]
        n = int(np.prod(shape))
        return buf[self.offsets[k]: self.offsets[k] + n].view(*shape)

    def load(self, arrays: dict) -> None:
        for n in NAMES:
            self.view(n).copy_(torch.as_tensor(np.asarray(arrays[n], dtype=np.float32)))

    def numpy(self) -> dict:
        return {n: self.view(n).cpu().numpy() for n in NAMES}

    def keras_init(self, seed=None) -> None:
        """Embedding RandomUniform(-0.05, 0.05); Dense glorot-uniform kernels, zero bias."""
        rng = np.random.default_rng(seed)
        arr = {}
        for n, s in _shapes(self.U1, self.I1, self.d).items():
            if n in ("MF_U", "MF_I", "MLP_U", "MLP_I"):
                arr[n] = rng.uniform(-0.05, 0.05, s)
            elif n.startswith("W"):
                lim = np.sqrt(6.0 / (s[0] + s[1]))
                arr[n] = rng.uniform(-lim, lim, s)
            else:
                arr[n] = np.zeros(s)
        self.load(arr)


class NeuMFContext:
    """Owns an ``acf_neumf_ctx`` (per-batch scratch for up to max_batch instances)."""

    def __init__(self, state: NeuMFState, max_batch: int):
        self.state, self.max_batch = state, int(max_batch)
        self._ptr = ctypes.c_void_p()
        with torch.cuda.device(state.device):
            _native.call_neumf("acf_neumf_create", ctypes.byref(self._ptr), state.U1, state.I1, state.d,
                               self.max_batch)

    def __del__(self):
        try:
            if self._ptr:
                _native.load_neumf().acf_neumf_destroy(self._ptr)
                self._ptr = ctypes.c_void_p()
        except Exception:
            pass

    def set_rows_in_line(self, on: bool) -> None:
        """Batches of <= 1,024 instances: rows summed inside the instance kernels
        (default) or by the separate row-sum kernel (bit-identical; tests / A/B)."""
        _native.call_neumf("acf_neumf_set_rows_in_line", self._ptr, int(bool(on)))

    def set_spin_limit(self, polls: int) -> None:
        """Polls a rows-in-line wait makes before it gives up (0: at once; tests)."""
        _native.call_neumf("acf_neumf_set_spin_limit", self._ptr, int(polls))

    def set_failsafe(self, on: bool) -> None:
        """On (default): a give-up is replayed exactly on the row-sum path;
        off: it raises RuntimeError."""
        _native.call_neumf("acf_neumf_set_failsafe", self._ptr, int(bool(on)))

    def recoveries(self) -> int:
        """Calls replayed after a rows-in-line give-up."""
        out = ctypes.c_int64()
        _native.call_neumf("acf_neumf_recoveries", self._ptr, ctypes.byref(out))
        return int(out.value)

    @staticmethod
    def hparams(lr=0.001, beta1=0.9, beta2=0.999, adam_eps=1e-7, adver=0, eps=0.5, reg_adv=1.0):
        return _native.NeuMFHParams(lr, beta1, beta2, adam_eps, eps, reg_adv, int(bool(adver)), 0)

    def grad(self, user, item, label, hp, loss_out: torch.Tensor | None = None, check=True) -> None:
        """Add the batch's loss gradient to state.grad (see acf_neumf_grad)."""
        s = self.state
        u, i = _idx(user, "user", s.device), _idx(item, "item", s.device)
        y = torch.as_tensor(label, dtype=torch.float32).reshape(-1).to(s.device).contiguous()
        if not (u.numel() == i.numel() == y.numel()):
            raise ValueError("user, item and label lengths differ")
        if not 0 < u.numel() <= self.max_batch:
            raise ValueError(f"batch of {u.numel()} outside (0, {self.max_batch}]")
        lp = 0 if loss_out is None else _require(loss_out, "loss_out", torch.float32, s.device)
        with torch.cuda.device(s.device):
            _native.call_neumf("acf_neumf_grad", self._ptr, s.params.data_ptr(), s.grad.data_ptr(),
                               u.data_ptr(), i.data_ptr(), y.data_ptr(), u.numel(), ctypes.byref(hp),
                               lp, int(bool(check)), _stream_ptr(s.device))
        self._keep = (u, i, y)

    def adam(self, hp) -> None:
        s = self.state
        s.t += 1
        with torch.cuda.device(s.device):
            _native.call_neumf("acf_neumf_adam", self._ptr, s.params.data_ptr(), s.grad.data_ptr(),
                               s.m.data_ptr(), s.v.data_ptr(), s.t, ctypes.byref(hp), _stream_ptr(s.device))

    def train(self, user, item, label, batch_size: int, hp) -> torch.Tensor:
        """One epoch over already-shuffled instances (acf_neumf_train); returns the
        per-batch [clean, adversarial] mean losses as a device tensor."""
        s = self.state
        u, i = _idx(user, "user", s.device), _idx(item, "item", s.device)
        y = torch.as_tensor(label, dtype=torch.float32).reshape(-1).to(s.device).contiguous()
        n = u.numel()
        if not (n == i.numel() == y.numel()):
            raise ValueError("user, item and label lengths differ")
        if not 0 < batch_size <= self.max_batch:
            raise ValueError(f"batch_size {batch_size} outside (0, {self.max_batch}]")
        nb = (n + batch_size - 1) // batch_size
        losses = torch.zeros(nb, 2, dtype=torch.float32, device=s.device)
        with torch.cuda.device(s.device):
            _native.call_neumf("acf_neumf_train", self._ptr, s.params.data_ptr(), s.grad.data_ptr(),
                               s.m.data_ptr(), s.v.data_ptr(), u.data_ptr(), i.data_ptr(), y.data_ptr(), n,
                               batch_size, s.t + 1, ctypes.byref(hp), losses.data_ptr(),
                               _stream_ptr(s.device))
        s.t += nb
        return losses

    def predict(self, user, item) -> torch.Tensor:
        s = self.state
        u, i = _idx(user, "user", s.device), _idx(item, "item", s.device)
        if u.numel() != i.numel():
            raise ValueError("user and item lengths differ")
        out = torch.empty(u.numel(), dtype=torch.float32, device=s.device)
        if u.numel():
            with torch.cuda.device(s.device):
                _native.call_neumf("acf_neumf_predict", self._ptr, s.params.data_ptr(), u.data_ptr(),
                                   i.data_ptr(), u.numel(), out.data_ptr(), _stream_ptr(s.device))
        return out

    def rank_all(self, users, k: int = 0, num_candidates: int | None = None, excl_off=None, excl_items=None,
                 test_items=None):
        """All-items ranking without a pair list or a score array (acf_neumf_rank_all):
        -> (positions int32 [n] | None, items int32 [n, k] | None, scores float32
        [n, k] | None) on the device.  Candidates of users[j]: [0, num_candidates)
        (default: every item row) minus the set excl_items[excl_off[j]:excl_off[j+1]]
        (unsorted, repeated and out-of-range entries are fine).  Scores are
        ``predict``'s bit for bit; lists are ordered by score descending, ties to
        the lower id, -1 / -inf past a user's candidates.  With test_items,
        positions[j] = #(candidates scoring >= the test item); put the test item
        into the exclusion list.  Everything is validated before any launch."""
        s = self.state
        if not isinstance(k, (int, np.integer)) or isinstance(k, bool) or not 0 <= k <= RANK_MAX_K:
            raise ValueError(f"k must be an int in [0, {RANK_MAX_K}], got {k!r}")
        k = int(k)
        u = _int_vec(users, "users")
        n = u.numel()
        nc = s.I1 if num_candidates is None else int(num_candidates)
        if not 1 <= nc <= s.I1:
            raise ValueError(f"num_candidates must lie in [1, {s.I1}] (item rows), got {nc}")
        if (excl_off is None) != (excl_items is None):
            raise ValueError("excl_off and excl_items go together")
        off = ex = None
        if excl_off is not None:
            off, ex = _int_vec(excl_off, "excl_off"), _int_vec(excl_items, "excl_items")
            if off.numel() != n + 1:
                raise ValueError(f"excl_off must have len(users) + 1 = {n + 1} entries, got {off.numel()}")
            o = off.cpu()
            if int(o[0]) < 0 or int(o[-1]) > ex.numel() or bool((o[1:] < o[:-1]).any()):
                raise ValueError("excl_off must be non-decreasing within [0, len(excl_items)]")
        t = None
        if test_items is not None:
            t = _int_vec(test_items, "test_items")
            if t.numel() != n:
                raise ValueError(f"test_items must have len(users) = {n} entries, got {t.numel()}")
        if k == 0 and t is None:
            raise ValueError("nothing to compute: k == 0 and no test_items")
        dev = s.device
        u = _idx(u, "users", dev)
        if off is not None:
            off = off.to(device=dev, dtype=torch.int64).contiguous()
            ex = _idx(ex, "excl_items", dev) if ex.numel() else torch.zeros(1, dtype=torch.int32, device=dev)
        pos = items = scores = None
        if t is not None:
            t = _idx(t, "test_items", dev)
            pos = torch.empty(n, dtype=torch.int32, device=dev)
        if k:
            items = torch.empty((n, k), dtype=torch.int32, device=dev)
            scores = torch.empty((n, k), dtype=torch.float32, device=dev)
        if n == 0:
            return pos, items, scores
        nbytes = rank_all_workspace(n, nc, k)
        work = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            _native.call_neumf("acf_neumf_rank_all", self._ptr, s.params.data_ptr(), u.data_ptr(), n, nc,
                               0 if off is None else off.data_ptr(), 0 if ex is None else ex.data_ptr(),
                               0 if t is None else t.data_ptr(), 0 if pos is None else pos.data_ptr(), k,
                               0 if items is None else items.data_ptr(),
                               0 if scores is None else scores.data_ptr(), work.data_ptr(), nbytes,
                               _stream_ptr(dev))
        return pos, items, scores


def _train_pairs(train):
    """(users, items) int64 of the train matrix (dok: key order; else coo order)."""
    if hasattr(train, "keys"):
        pairs = np.array(list(train.keys()), dtype=np.int64).reshape(-1, 2)
        return pairs[:, 0], pairs[:, 1]
    coo = train.tocoo()
    return np.asarray(coo.row, np.int64), np.asarray(coo.col, np.int64)


class _TrainLists:
    """The train matrix as what evaluate.train_exclusions reads: sorted_lists() ->
    (offsets [rows + 1], items), each user's unique train items ascending."""

    def __init__(self, train, num_rows: int, num_items: int):
        u, i = _train_pairs(train)
        keys = np.unique(u * int(num_items) + i)
        self.off = np.zeros(int(num_rows) + 1, dtype=np.int64)
        np.cumsum(np.bincount(keys // int(num_items), minlength=int(num_rows))[:int(num_rows)], out=self.off[1:])
        self.items = (keys % int(num_items)).astype(np.int32)

    def sorted_lists(self):
        return self.off, self.items


def _append_columns(off, items, extra):
    """The exclusion CSR with extra[j] (int [n, m]) appended to list j."""
    n, m = extra.shape
    lens = np.diff(off)
    noff = off + m * np.arange(n + 1, dtype=np.int64)
    out = np.empty(int(noff[-1]), dtype=np.int32)
    out[np.arange(off[-1], dtype=np.int64) + m * np.repeat(np.arange(n, dtype=np.int64), lens)] = items
    for j in range(m):
        out[noff[1:] - m + j] = extra[:, j]
    return noff, out


def mf_train_instances(train, iNum, rng):
    """MF.py:42-56: per training pair (u, i), in the train matrix's key order, a
    positive (label 1) and a negative j ~ U[1, iNum) redrawn while (u, j) is a
    training pair (label 0).  The reference redraws until the negative is valid;
    a user whose pairs cover all of [1, iNum) has none, and is refused here
    (the reference would loop forever)."""
    u, i = _train_pairs(train)
    keys = np.unique(u * iNum + i)
    per_user = np.bincount((keys // iNum)[(keys % iNum) >= 1], minlength=int(u.max(initial=0)) + 1)
    if len(u) and (per_user[u] >= iNum - 1).any():
        raise ValueError("get_train_instances: a user has every item of [1, iNum) as a training pair")
    j = rng.randint(1, iNum, size=len(u)).astype(np.int64)
    bad = np.isin(u * iNum + j, keys)
    while bad.any():
        j[bad] = rng.randint(1, iNum, size=int(bad.sum()))
        bad = np.isin(u * iNum + j, keys)
    users = np.stack([u, u], 1).reshape(-1)
    items = np.stack([i, j], 1).reshape(-1)
    labels = np.tile(np.array([1, 0], dtype=np.int64), len(u))
    return [users, items], labels


class NeuMF:
    """NeuMF.py:10-55 on the GPU, with the run.py Recommender surface."""

    adver = 0

    def __init__(self, uNum, iNum, mf_dim=10, lr=0.001, seed=None, device=None):
        if not torch.cuda.is_available():
            raise RuntimeError("NeuMF needs a HIP device: there is no CPU path")
        self.uNum, self.iNum, self.dim = int(uNum) + 1, int(iNum) + 1, int(mf_dim)  # NeuMF.py:12-13
        self.device = torch.device(device if device is not None else "cuda")
        self.state = NeuMFState(self.uNum, self.iNum, self.dim, self.device)
        self.state.keras_init(seed)
        self.lr = float(lr)
        self.eps, self.reg_adv = 0.5, 1.0
        self._rng = np.random.RandomState(seed)
        self._ctx = None

    # -- helpers -----------------------------------------------------------------
    def _context(self, batch_size: int) -> NeuMFContext:
        if self._ctx is None or self._ctx.max_batch < batch_size:
            self._ctx = NeuMFContext(self.state, max(batch_size, 1024))
        return self._ctx

    def hparams(self):
        return NeuMFContext.hparams(lr=self.lr, adver=self.adver, eps=self.eps, reg_adv=self.reg_adv)

    # -- Recommender API -----------------------------------------------------------
    def get_params(self):
        return ""

    def get_train_instances(self, train):
        """MF.py:42-56 (see mf_train_instances)."""
        return mf_train_instances(train, self.iNum, self._rng)

    def train(self, x_train, y_train, batch_size):
        """Keras fit for one epoch (MF.py:30-33): shuffled, batches of batch_size
        including the last partial one, one Adam step each; returns the mean loss
        (batch losses weighted by batch size, as Keras' History reports)."""
        users = np.asarray(x_train[0]).reshape(-1)
        items = np.asarray(x_train[1]).reshape(-1)
        y = np.asarray(y_train, dtype=np.float32).reshape(-1)
        n = len(y)
        if n == 0:
            return float("nan")
        perm = self._rng.permutation(n)
        dev = self.device
        U = torch.as_tensor(users[perm], dtype=torch.int32).to(dev)
        I = torch.as_tensor(items[perm], dtype=torch.int32).to(dev)
        Y = torch.as_tensor(y[perm]).to(dev)
        ctx = self._context(batch_size)
        nb = (n + batch_size - 1) // batch_size
        losses = ctx.train(U, I, Y, batch_size, self.hparams())
        weights = torch.full((nb,), float(batch_size))
        weights[-1] = n - (nb - 1) * batch_size
        lc = losses[:, 0].cpu()
        la = losses[:, 1].cpu()
        total = lc + (self.reg_adv * la if self.adver else 0.0)
        return float((total * weights).sum() / weights.sum())

    def rank(self, users, items):
        """MF.py:38-40 (model.predict): scores of shape [n, 1]."""
        ctx = self._context(1)
        out = ctx.predict(np.asarray(users).reshape(-1), np.asarray(items).reshape(-1))
        return out.cpu().numpy().reshape(-1, 1)

    def _exclusions(self, users, train, test_items=None):
        """Exclusion CSR of `users`: item 0 (run.py's masking id), the test item if
        given, and with `train` the user's train items (evaluate.train_exclusions)."""
        from .evaluate import train_exclusions
        users = np.asarray(users, dtype=np.int64).reshape(-1)
        if train is None:
            off, items = np.zeros(len(users) + 1, np.int64), np.zeros(0, np.int32)
        else:
            if getattr(self, "_lists_of", None) is not train:  # one CSR per train matrix, not per epoch
                self._lists, self._lists_of = _TrainLists(train, self.uNum, self.iNum), train
            off, items = train_exclusions(self._lists, users)
        extra = [np.zeros(len(users), np.int32)]
        if test_items is not None:
            extra.append(np.asarray(test_items, dtype=np.int32).reshape(-1))
        return _append_columns(off, items, np.stack(extra, 1))

    def recommend(self, users, k, train=None):
        """The k best items of every user in `users` under ``rank``'s scores, on the
        GPU with no pair list (NeuMFContext.rank_all): numpy (items int32 [n, k],
        scores float32 [n, k]), -1 / -inf past a user's candidates.  With `train`
        (what get_train_instances takes) each user's train items and item 0 (the
        masking id) are excluded; without it nothing is.  Candidates are the ids
        below the constructor's iNum (the table has one more row, NeuMF.py:12-13)."""
        users = np.asarray(users, dtype=np.int64).reshape(-1)
        off = ex = None
        if train is not None:
            off, ex = self._exclusions(users, train)
        _, items, scores = self._context(1).rank_all(users, int(k), self.iNum - 1, off, ex)
        return items.cpu().numpy(), scores.cpu().numpy()

    def similar_items(self, items, k=10, metric="cosine"):
        raise NotImplementedError("NeuMF has two item tables (the GMF and the MLP embeddings) that only the "
                                  "network combines, so there is no single similarity between two items.")

    def _no_item_similarity(self, *args, **kwargs):
        raise NotImplementedError("NeuMF has two item tables (the GMF and the MLP embeddings) that only the "
                                  "network combines, so there is no single similarity between two items to "
                                  "diversify or to measure a list by.")

    recommend_diverse = diversity = diversity_tradeoff = _no_item_similarity

    def similar_users(self, users, k=10, metric="cosine", rows=None):
        raise NotImplementedError("NeuMF has two user tables (the GMF and the MLP embeddings) that only the "
                                  "network combines, so there is no single similarity between two users.")

    def positions_all(self, users, test_items, train):
        """Per user the number of candidates scoring >= the user's test item, the
        candidates being every item except 0, the user's train items and the test
        item: the rank run.py's --eval all protocol gives it.  int32 numpy [n]."""
        users = np.asarray(users, dtype=np.int64).reshape(-1)
        tests = np.asarray(test_items, dtype=np.int64).reshape(-1)
        if len(tests) != len(users):
            raise ValueError("users and test_items lengths differ")
        off, ex = self._exclusions(users, train, tests)
        pos, _, _ = self._context(1).rank_all(users, 0, self.iNum - 1, off, ex, tests)
        return pos.cpu().numpy()

    def save(self, path):
        np.savez(path if path.endswith(".npz") else path + ".npz", **self.state.numpy())

    def load_pre_train(self, pre):
        with np.load(pre if pre.endswith(".npz") else pre + ".npz", allow_pickle=False) as z:
            self.state.load({n: z[n] for n in NAMES})


class AdversarialNeuMF(NeuMF):
    """NeuMF + FGSM adversary on the four embedding tables (see module docstring)."""

    adver = 1

    def __init__(self, uNum, iNum, mf_dim, weight=1.0, pop_percent=0.2, eps=0.5, lr=0.001, seed=None,
                 device=None):
        super().__init__(uNum, iNum, mf_dim, lr=lr, seed=seed, device=device)
        self.weight, self.pop_percent = float(weight), float(pop_percent)
        self.eps, self.reg_adv = float(eps), float(weight)

    def get_params(self):
        return "_w%.3f_e%.2f" % (self.weight, self.eps)
