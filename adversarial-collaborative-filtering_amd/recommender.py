"""``Recommender`` plugin interface (``Recommender.py:3-27``) and the ``APR`` class
``run.py`` dispatches to (``run.py:157-161,231-244``: ``APR(uNum, iNum, dim,
adver)``, ``get_params``, ``build_graph(path, opath, data, runName[, restore])``,
``get_train_instances``, ``train``, ``rank``, ``save``, ``load_pre_train``).

The reference imports ``from APR import APR`` but ``APR.py`` defines no such class
(``run.py:6``); this is the class that call site expects, implemented on the GPU
APR path.
"""
from __future__ import annotations

import ctypes
from abc import ABC, abstractmethod
from types import SimpleNamespace

import numpy as np
import torch

from . import _native, ops
from .model import MF
from .sampler import EpochTriplets


class Recommender(ABC):
    """Recommender.py:3-27."""

    @abstractmethod
    def get_params(self):
        pass

    @abstractmethod
    def load_pre_train(self, pre):
        pass

    @abstractmethod
    def save(self, path):
        pass

    @abstractmethod
    def train(self, x_train, y_train, batch_size):
        pass

    @abstractmethod
    def rank(self, users, items):
        pass

    @abstractmethod
    def get_train_instances(self, train):
        pass

    # -- nearest neighbours (not in the reference; MF-shaped recommenders) --------
    def neighbor_tables(self):
        """What evaluate.similar_items / similar_users take: an object with
        embedding_P, embedding_Q, num_users and num_items.  A recommender with one
        user table and one item table in the same space overrides this."""
        raise NotImplementedError(f"{type(self).__name__} has no single user / item table to compare rows of")

    def similar_items(self, items, k=10, metric="cosine"):
        """evaluate.similar_items on the recommender's item table: the k items
        nearest to each of `items` ('cosine', 'dot' or 'euclid'), never the item
        itself: (ids [n, k] int32, scores [n, k] float32) numpy arrays."""
        from .evaluate import similar_items
        return similar_items(self.neighbor_tables(), items, k=k, metric=metric)

    def similar_users(self, users, k=10, metric="cosine", rows=None):
        """evaluate.similar_users on the recommender's user table; with rows (a
        FoldIn or a [m, d] tensor) the queries are those rows instead."""
        from .evaluate import similar_users
        return similar_users(self.neighbor_tables(), users, k=k, metric=metric, rows=rows)


def _npz(path):
    return path if path.endswith(".npz") else path + ".npz"


class FlatMF(Recommender):
    """What keras_bpr.BPR and fast_adversarial_mf.FastAdversarialMF share: a dot-product
    model of libacf_neumf.so whose parameters, gradient and Adam moments are four flat
    float32 tensors in one layout that starts with [uEmb | iEmb], a native context
    sized by the largest batch seen, and u . i scoring.  ``_prefix`` names the
    engine's entry points (``<prefix>create / destroy / predict``)."""
    _prefix = ""

    def _init_flat(self, uNum, iNum, dim, init, adam, seed, device):
        """init: the parameter buffer's initial values (numpy float32); adam: (lr, beta1, beta2, eps)."""
        self.uNum, self.iNum, self.dim = int(uNum), int(iNum), int(dim)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.hp = _native.NeuMFHParams(*adam, 0.0, 0.0, 0, 0)
        self.params = torch.as_tensor(init).to(self.device)
        self.grad, self.m, self.v = (torch.zeros_like(self.params) for _ in range(3))
        self.t = 0  # Adam iterations done
        self._rng = np.random.RandomState(seed)
        self._ctx, self._ctx_batch = ctypes.c_void_p(), 0

    def __del__(self):
        try:
            if self._ctx:
                getattr(_native.load_neumf(), self._prefix + "destroy")(self._ctx)
        except Exception:
            pass

    # -- Keras layer views -------------------------------------------------------
    @property
    def uEmb(self) -> torch.Tensor:
        return self.params[: self.uNum * self.dim].view(self.uNum, self.dim)

    @property
    def iEmb(self) -> torch.Tensor:
        return self.params[self.uNum * self.dim: (self.uNum + self.iNum) * self.dim].view(self.iNum, self.dim)

    def neighbor_tables(self):
        """uEmb / iEmb as evaluate.similar_items / similar_users take them (no padding rows)."""
        return SimpleNamespace(embedding_P=self.uEmb, embedding_Q=self.iEmb, num_users=self.uNum,
                               num_items=self.iNum)

    def _context(self, batch):
        if batch > self._ctx_batch:
            if self._ctx:
                getattr(_native.load_neumf(), self._prefix + "destroy")(self._ctx)
                self._ctx = ctypes.c_void_p()
            with torch.cuda.device(self.device):
                _native.call_neumf(self._prefix + "create", ctypes.byref(self._ctx), self.uNum, self.iNum, self.dim,
                                   int(batch))
            self._ctx_batch = int(batch)
        return self._ctx

    def rank(self, users, items):
        u = ops._idx(users, "users", self.device)
        it = ops._idx(items, "items", self.device)
        out = torch.empty(u.numel(), dtype=torch.float32, device=self.device)
        ctx = self._context(max(self._ctx_batch, 1))
        with torch.cuda.device(self.device):
            _native.call_neumf(self._prefix + "predict", ctx, self.params.data_ptr(), u.data_ptr(), it.data_ptr(),
                               u.numel(), out.data_ptr(), ops._stream_ptr(self.device))
        return out.cpu().numpy().reshape(-1, 1)


class APR(Recommender):
    """BPR-MF (adver=False) or APR (adver=True) behind the Recommender API."""

    def __init__(self, uNum, iNum, dim, adver=False, lr=0.05, eps=0.5, reg=0.0, reg_adv=1.0,
                 adv="grad", seed=None, device=None):
        self.uNum, self.iNum, self.dim, self.adver = int(uNum), int(iNum), int(dim), bool(adver)
        args = SimpleNamespace(embed_size=self.dim, lr=lr, reg=reg, dns=1, adv=adv, eps=eps,
                               adver=int(self.adver), reg_adv=reg_adv, epochs=0, seed=seed)
        # uNum/iNum are max id + 1 in run.py (run.py:114): tables sized like APR.py (+1)
        self.model = MF(self.uNum, self.iNum, args)
        self._device = device
        self._rng = np.random.RandomState(seed)

    def get_params(self):
        return "_e%.2f_l%.2f" % (self.model.eps, self.model.reg_adv) if self.adver else ""

    def build_graph(self, path="", opath="", data="", runName="", restore=False, previous=None):
        """Create the tables.  With restore=True the embeddings of `previous` (the BPR
        phase's ranker) are carried over and the Adagrad slots start fresh, like the
        phase switch of run_adv_ori.py:106-114."""
        self.model.build_graph(device=self._device)
        if restore and previous is not None:
            self.model.load_embeddings(previous.model.embedding_P.cpu(), previous.model.embedding_Q.cpu())
        self.path, self.opath, self.data, self.runName = path, opath, data, runName
        return self

    def _ensure(self):
        if not self.model.built:
            self.build_graph()

    def load_pre_train(self, pre):
        self._ensure()
        with np.load(_npz(pre), allow_pickle=False) as z:
            self.model.load_embeddings(z["embedding_P"], z["embedding_Q"])

    def save(self, path):
        self._ensure()
        ops.settle_tables()
        np.savez(_npz(path), embedding_P=self.model.embedding_P.cpu().numpy(),
                 embedding_Q=self.model.embedding_Q.cpu().numpy())

    def get_train_instances(self, train):
        """Shuffled positives of a dok/CSR train matrix with one uniform negative
        each, rejected while (u, j) is a training pair (APR.py:64-81 rule)."""
        coo = train.tocoo() if hasattr(train, "tocoo") else train
        u = np.asarray(coo.row, dtype=np.int64)
        i = np.asarray(coo.col, dtype=np.int64)
        keys = np.unique(u * self.iNum + i)
        idx = self._rng.permutation(len(u))
        u, i = u[idx], i[idx]
        j = self._rng.randint(self.iNum, size=len(u)).astype(np.int64)
        for _ in range(10000):
            bad = np.isin(u * self.iNum + j, keys, assume_unique=False)
            if not bad.any():
                break
            j[bad] = self._rng.randint(self.iNum, size=int(bad.sum()))
        x = [u.astype(np.int32), i.astype(np.int32), j.astype(np.int32)]
        return x, np.ones(len(u), dtype=np.float32)

    def train(self, x_train, y_train, batch_size):
        """One pass over x_train in batches of batch_size (the trailing partial batch
        is dropped, as in APR.py:52); returns the mean clean loss per triplet."""
        from .train import training_batch, training_loss_acc
        self._ensure()
        m = self.model
        n = (len(x_train[0]) // batch_size) * batch_size
        if n == 0:
            return float("nan")
        T = lambda a: torch.as_tensor(np.asarray(a[:n]), dtype=torch.int32, device=m.device)  # noqa
        ep = EpochTriplets(T(x_train[0]), T(x_train[1]), T(x_train[2]), batch_size)
        training_batch(m, None, ep, adver=self.adver)
        loss, _ = training_loss_acc(m, None, ep)
        return loss / batch_size

    def rank(self, users, items):
        self._ensure()
        return self.model.scores(np.asarray(users).reshape(-1), np.asarray(items).reshape(-1))

    def neighbor_tables(self):
        """The model: tables of uNum + 1 / iNum + 1 rows, the last one padding."""
        self._ensure()
        return self.model

    def recommend(self, users, k, train=None):
        """The k best items of each user among [0, iNum): (items [n, k] int32,
        scores [n, k] float32) numpy arrays, best first, -1 / -inf past a user's
        candidates.  train: the dok/CSR matrix of get_train_instances; its pairs
        are never recommended."""
        self._ensure()
        m = self.model
        users = np.asarray(users, dtype=np.int64).reshape(-1)
        off = ex = None
        if train is not None:
            csr = train.tocsr()
            lens = np.where(users < csr.shape[0], np.diff(csr.indptr)[np.minimum(users, csr.shape[0] - 1)], 0)
            off = np.zeros(len(users) + 1, dtype=np.int64)
            np.cumsum(lens, out=off[1:])
            start = np.repeat(csr.indptr[np.minimum(users, csr.shape[0] - 1)].astype(np.int64), lens)
            within = np.arange(off[-1], dtype=np.int64) - np.repeat(off[:-1], lens)
            ex = csr.indices[start + within].astype(np.int32)
        items, scores = ops.recommend_topk(m.embedding_P, m.embedding_Q, users.astype(np.int32), int(k), self.iNum,
                                           off, ex)
        return items.cpu().numpy(), scores.cpu().numpy()

    @staticmethod
    def _new_lists(train):
        """Item lists of new users: a dok/CSR matrix (row r = new user r), or
        lists / a dict as evaluate.fold_lists takes them."""
        if hasattr(train, "tocsr"):
            csr = train.tocsr()
            return [csr.indices[csr.indptr[r]:csr.indptr[r + 1]] for r in range(csr.shape[0])]
        return train

    def fold_in(self, train, **fold_args):
        """evaluate.fold_in for the new users of `train` (a matrix like
        get_train_instances takes, one row per new user, or item lists)."""
        self._ensure()
        fold_args.setdefault("num_items", self.iNum)
        return self.model.fold_in(self._new_lists(train), **fold_args)

    def recommend_new(self, train, k, **fold_args):
        """evaluate.recommend_new for the new users of `train`: (items [n, k],
        scores [n, k]) numpy arrays among [0, iNum), their own items excluded."""
        self._ensure()
        fold_args.setdefault("num_items", self.iNum)
        return self.model.recommend_new(self._new_lists(train), k, **fold_args)

    @staticmethod
    def _new_item_lists(train):
        """User lists of new items: a dok/CSC matrix (column c = new item c, rows
        = the existing users), or lists / a dict as evaluate.fold_lists takes them."""
        if hasattr(train, "tocsc"):
            csc = train.tocsc()
            return [csc.indices[csc.indptr[c]:csc.indptr[c + 1]] for c in range(csc.shape[1])]
        return train

    def fold_in_items(self, train, **fold_args):
        """evaluate.fold_in_items for the new items of `train` (a matrix with one
        COLUMN per new item and the existing users as rows, or user lists)."""
        self._ensure()
        return self.model.fold_in_items(self._new_item_lists(train), **fold_args)

    def audience_new(self, train, k, **fold_args):
        """evaluate.audience_new for the new items of `train`: (users [n, k],
        scores [n, k]) numpy arrays among [0, uNum), their own users excluded."""
        self._ensure()
        return self.model.audience_new(self._new_item_lists(train), k, **fold_args)

    def evaluate_multi(self, plan, cutoffs=(10, 50, 100), raw=False):
        """evaluate.evaluate_multi against the test lists of `plan`
        (evaluate.init_eval_multi): a dict of recall / ndcg / map / ... @K, mrr, auc."""
        self._ensure()
        return self.model.evaluate_multi(plan, cutoffs=cutoffs, raw=raw)

    def adv_update(self, x_train, adv=None):
        """train.adv_update on the triplets of get_train_instances: the model's
        delta_P / delta_Q over all of them as one batch."""
        self._ensure()
        return self.model.adv_update((([x_train[0]], [x_train[1]], [x_train[2]])), adv=adv)

    def robustness(self, dataset, plan, x_train, eps_list, modes=("grad", "random"), seed=0, iters=10, step=None,
                   side="both"):
        """evaluate.robustness on the triplets of get_train_instances: rows
        (mode, eps, hr@K, ndcg@K, auc); iters, step and side are the "pgd" mode's."""
        self._ensure()
        return self.model.robustness(dataset, plan, ([x_train[0]], [x_train[1]], [x_train[2]]), eps_list,
                                     modes=modes, seed=seed, iters=iters, step=step, side=side)

    def exposure(self, dataset, users=None, k=100, cutoffs=(10, 100), exclude_train=True):
        """evaluate.exposure: rows (cutoff, total, coverage, gini, entropy, arp,
        aplt) of the model's own top-k lists."""
        self._ensure()
        return self.model.exposure(dataset, users=users, k=k, cutoffs=cutoffs, exclude_train=exclude_train)

    def recommend_diverse(self, dataset=None, users=None, k=10, pool=128, lam=0.7, metric="cosine",
                          rel_norm="minmax", exclude_train=True):
        """evaluate.recommend_diverse: the model's `pool` best items per user
        re-ranked to k by maximal marginal relevance: (items [n, k], scores [n, k])."""
        self._ensure()
        return self.model.recommend_diverse(dataset, users=users, k=k, pool=pool, lam=lam, metric=metric,
                                            rel_norm=rel_norm, exclude_train=exclude_train)

    def diversity(self, dataset, users=None, k=100, cutoffs=(10, 100), metric="cosine"):
        """evaluate.diversity: rows (cutoff, ils) of the model's own top-k lists."""
        self._ensure()
        return self.model.diversity(dataset, users=users, k=k, cutoffs=cutoffs, metric=metric)

    def diversity_tradeoff(self, dataset, lams=(1.0, 0.7, 0.5), k=10, pool=128, cutoffs=(10,), metric="cosine"):
        """evaluate.diversity_tradeoff: rows (lam, cutoff, hr, ndcg, ils, total,
        coverage, gini, entropy, arp, aplt) of the MMR re-ranked lists."""
        self._ensure()
        return self.model.diversity_tradeoff(dataset, lams=lams, k=k, pool=pool, cutoffs=cutoffs, metric=metric)

    def list_robustness(self, dataset, x_train, eps_list, k=100, cutoffs=(1, 10, 100), modes=("grad", "random"),
                        p=0.9, seed=0, iters=10, step=None, side="both", users=None):
        """evaluate.list_robustness on the triplets of get_train_instances: rows
        (mode, eps, cutoff, jaccard, rbo, overlap, coverage, gini, entropy, arp, aplt)."""
        self._ensure()
        return self.model.list_robustness(dataset, ([x_train[0]], [x_train[1]], [x_train[2]]), eps_list, k=k,
                                          cutoffs=cutoffs, modes=modes, p=p, seed=seed, iters=iters, step=step,
                                          side=side, users=users)

    def certified(self, plan, eps_list, side="user", cutoffs=None):
        """evaluate.certified against an all-items plan: rows (side, eps, K, hr_lb,
        ndcg_lb, auc_lb), lower bounds under every attack of that budget."""
        self._ensure()
        return self.model.certified(plan, eps_list, side=side, cutoffs=cutoffs)

    def certified_radius(self, plan, k=None, side="user"):
        """evaluate.certified_radius against an all-items plan: (eps [n, k], items
        [n, k]), per user the largest eps up to which the held-out item provably
        stays in the top 1..k and the items that break the certificate first."""
        self._ensure()
        return self.model.certified_radius(plan, k=k, side=side)
