"""``torch.ops.acf.*``: the APR hot path as PyTorch custom ops.

``lib/libacf_torch.so`` (csrc/acf_torch.cpp) registers ``TORCH_LIBRARY(acf, m)``
over the C-ABI of ``libacf_apr.so`` (include/acf_apr.h), with the operator set
SURVEY.md §8(b) proposes:

- ``bpr_apr_step(P, Q, accP, accQ, u, i, j, lr, eps, reg, reg_adv, adver, clip_lo, clip_hi)
  -> (loss_clean, loss_adv, n_correct)``: one training_batch iteration
  (utils.py:114-119, APR.py:143-195), tables updated in place;
- ``apr_train(..., batch_size, ...) -> (loss_clean[n], loss_adv[n])``: n/batch_size
  consecutive batches (the streamed step);
- decomposed, one TF op each: ``gather_bpr_fwd_bwd`` (APR.py:121-150,183),
  ``row_segment_sum`` (IndexedSlices dedup, APR.py:183-187,195), ``l2norm_perturb``
  (APR.py:186-191), ``sparse_adagrad_apply`` (APR.py:193-195);
- evaluation: ``score_rank`` / ``score_rank_all`` (_eval_by_user, utils.py:211-254);
- ``recommend_topk(P, Q, users, k, num_candidates, excl_off, excl_items) -> (items, scores)``:
  the k best items per user (exact; ``ops.recommend_topk``);
- ``adv_direction(P, Q, user, item_pos, item_neg, adv, seed, call, t, clip_lo, clip_hi) -> (nP, nQ)``
  and ``adv_apply(W, N, eps) -> (sum, delta)``: the whole-stream adversarial direction and
  the perturbed table (``ops.adv_direction`` / ``ops.adv_apply``);
- ``adv_pgd(P, Q, user, item_pos, item_neg, eps, iters, alpha, side, delta_P0, delta_Q0, clip_lo, clip_hi)
  -> (delta_P, delta_Q, losses)``: the iterated projected gradient attack (``ops.adv_pgd``, the same bits;
  the op plans inside the call and always range-checks);
- ``fold_in_users(Q, user_off, item_pos, item_neg, epochs, batch, init, acc_init, lr, eps, reg, reg_adv,
  adver, clip_lo, clip_hi) -> (P_new, acc_new, loss)``: rows for new users against a frozen
  item table (``ops.fold_in_users``, the same bits).  The op always synchronises with the host:
  it copies ``user_off`` back to validate the CSR, and it always runs the native range check
  of the items (``check=1``: a small stream-ordered allocation, one kernel and a stream
  synchronise before the fold-in launch).  Use ``ops.fold_in_users(..., check=False)`` with a
  host ``user_off`` for a call that stays asynchronous;
- ``fold_in_items(P, Q, item_off, user_pos, item_neg, epochs, batch, init, acc_init, lr, eps, reg,
  reg_adv, adver, clip_lo, clip_hi) -> (Q_new, acc_new, loss)``: rows for new items against frozen
  user and item tables (``ops.fold_in_items``, the same bits); it synchronises with the host as
  ``fold_in_users`` does (CSR read back, native range check of users and negatives);
- ``eval_positions_multi(P, Q, users, test_off, test_items, num_candidates, excl_off, excl_items)
  -> positions`` and ``rank_metrics(positions, test_off, n_neg, cutoffs) -> (per_user,
  per_user_free, mean_cut, mean_free, n_scored)``: evaluation against several held-out items
  per user (``ops.eval_positions_multi`` / ``ops.rank_metrics``, the same values).  Both copy
  their CSR offsets back to validate them, and the positions op checks users and test items
  before any gather; empty ``excl_off`` and ``excl_items`` exclude nothing;
- ``eval_positions_worst(P, Q, users, test_items, num_candidates, excl_off, excl_items, eps, side)
  -> worst [n_eps, n]``: certified worst-case positions under an eps attack on the user or the
  item rows (``ops.eval_positions_worst``, the same values); users and test items are checked
  before any gather; empty ``excl_off`` and ``excl_items`` exclude nothing;
- ``eval_radius(P, Q, users, test_items, num_candidates, excl_off, excl_items, k, side)
  -> (eps [n, k], items [n, k])``: the certified radius, per entry the k smallest eps at which a
  candidate breaks the certificate and those candidates (``ops.eval_radius``, the same values);
  ``eps[r, j]`` is the largest budget up to which the test item provably stays in the top j + 1.
  Checks as ``eval_positions_worst``;
- ``release_contexts() -> int``: frees the cached step contexts (plan workspace and
  the streamed step's version buffers) that ``apr_train`` / ``bpr_apr_step`` keep per
  (device, table shape, batch shape).

There is no CPU kernel: calling an op on CPU tensors raises (no fallback).
"""
from __future__ import annotations

import os
import threading

import torch

from . import build_native

LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libacf_torch.so")
OPS = ("bpr_apr_step", "apr_train", "gather_bpr_fwd_bwd", "row_segment_sum", "l2norm_perturb",
       "sparse_adagrad_apply", "score_rank", "score_rank_all", "recommend_topk", "adv_direction", "adv_apply",
       "adv_pgd",
       "fold_in_users", "fold_in_items", "eval_positions_multi", "rank_metrics", "eval_positions_worst", "eval_radius",
       "release_contexts")
_lock = threading.Lock()
_loaded = False


def load():
    """Load the op library (once) and return the ``torch.ops.acf`` namespace."""
    global _loaded
    with _lock:
        if not _loaded:
            if not os.path.exists(LIB):
                raise ImportError(f"{LIB} not found: build it with __graft_entry__.build() "
                                  "(build_native.build_torch_ops); there is no CPU fallback")
            build_native.verify("torch", LIB)  # built from these sources (ImportError otherwise)
            torch.ops.load_library(LIB)
            _loaded = True
    return torch.ops.acf
