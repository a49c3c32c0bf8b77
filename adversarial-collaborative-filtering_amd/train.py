"""Epoch driver and logging: ``training``, ``training_batch``,
``training_loss_acc``, ``output_evaluate``, ``write2file``, ``prediction2file``
(``APR.py:206-292``, ``utils.py:18-32,81-175``).

Log lines, file names and checkpoint layout follow the reference so existing
tooling reading ``out/<opath>/<runName>.out|.hr|.ndcg`` keeps working.
Checkpoints are ``.npz`` files holding the tensors ``embedding_P`` /
``embedding_Q`` under the reference's ``Pretrain/<ds>/{MF_BPR,APR}/embed_<d>/<ts>/``
directories, with a TF-style ``checkpoint`` index file (TF checkpoint V2 cannot be
written without TensorFlow).
"""
from __future__ import annotations

import logging
import os
import re
from time import time

import numpy as np
import torch

from . import ops
from .evaluate import evaluate, init_eval_model, perturbed_tables, triplet_arrays
from .sampler import DeviceSampler, EpochTriplets, sampling, shuffle


def write2file(path, name, output):
    """utils.py:18-24."""
    print(output, flush=True)
    if not os.path.exists(path):
        os.makedirs(path)
    with open(path + name, "a") as f:
        f.write("%s\n" % output)


def prediction2file(path, name, pred):
    """utils.py:26-32."""
    if not os.path.exists(path):
        os.makedirs(path)
    with open(path + name, "w") as f:
        for item in pred:
            f.write("%f\n" % item)


# ---------------------------------------------------------------------------
def _as_epoch(model, batches) -> EpochTriplets:
    if isinstance(batches, EpochTriplets):
        return batches
    user_input, item_input_pos, _user_dns, item_dns = batches
    B = int(np.asarray(user_input[0]).shape[0])
    dev = model.device
    u = torch.as_tensor(np.concatenate([np.asarray(x).reshape(-1) for x in user_input]),
                        dtype=torch.int32).to(dev)
    i = torch.as_tensor(np.concatenate([np.asarray(x).reshape(-1) for x in item_input_pos]),
                        dtype=torch.int32).to(dev)
    j = torch.as_tensor(np.concatenate([np.asarray(x).reshape(-1) for x in item_dns]),
                        dtype=torch.int32).to(dev)
    return EpochTriplets(u, i, j, B)


def training_batch(model, sess, batches, adver=False, graph=True):
    """utils.py:106-140.  dns == 1: the epoch is planned in chunks (plan_chunk),
    each trained by the streamed step (APR) or replayed as one hipGraph
    (delta_update + optimizer_step per batch, in batch order).  The step error
    word is read once per epoch: a step that gave up waiting for a row version
    raises StepWaitError instead of leaving silently stale rows.
    dns > 1: per batch, the highest-scoring of dns negatives under the current
    weights, then the optimizer step (the reference never runs update_P/update_Q
    on this branch, so the adversarial terms see delta = 0)."""
    if model.dns == 1:
        ep = _as_epoch(model, batches)
        B, nb = ep.batch_size, ep.n_batches
        hp = model.hparams(adver=int(bool(adver)))
        pipe = model.pipeline(B, min(nb, plan_chunk(B)))
        pipe.run(model.launch_tables, hp, ep.user, ep.item_pos, ep.item_neg, graph=graph, check=True)
        errs = pipe.step_errors()  # one stream sync per epoch
        if errs:
            raise ops.StepWaitError(errs)
        return ep
    user_input, item_input_pos, user_dns_list, item_dns_list = batches
    hp = model.hparams(adver=int(bool(adver)))
    hp.zero_delta = 1
    negs = []
    for k in range(len(user_input)):
        u = ops._idx(user_dns_list[k], "user", model.device)
        cand = ops._idx(item_dns_list[k], "cand", model.device)
        uu = ops._idx(user_input[k], "user", model.device)
        sel = ops.dns_select(model.embedding_P, model.embedding_Q, u[::model.dns].contiguous(), cand,
                             model.dns)
        ctx = model.context(uu.numel(), 1)
        ctx.plan(uu, item_input_pos[k], sel, uu.numel())
        if hp.adver:
            ctx.delta_update(model.launch_tables, hp, 0)
        ctx.optimizer_step(model.launch_tables, hp, 0)
        negs.append(sel.cpu().numpy().reshape(-1, 1))
    return user_input, item_input_pos, negs


def plan_chunk(batch_size: int) -> int:
    """Batches per plan / hipGraph; the next chunk is planned during this one.
    Small batches: 512 (the chunk's inline records stay in the Infinity Cache);
    large batches: 2M triplets (the plan's fixed sort cost amortised)."""
    return 512 if batch_size < 4096 else max(1, (1 << 21) // batch_size)


def training_loss_acc(model, sess, train_batches, output_adv=0):
    """utils.py:159-175: mean per-batch summed clean loss and mean pairwise accuracy.
    output_adv=1: loss_adv, output_adv and output_neg_adv (utils.py:169-170), the
    same forward on (P + delta_P, Q + delta_Q), where delta_P / delta_Q are what
    the last adv_update put there (zeros before any; see adv_update)."""
    if isinstance(train_batches, EpochTriplets):
        u, i, j, B = train_batches.user, train_batches.item_pos, train_batches.item_neg, train_batches.batch_size
    else:
        ep = _as_epoch(model, (train_batches[0], train_batches[1], None, train_batches[2]))
        u, i, j, B = ep.user, ep.item_pos, ep.item_neg, ep.batch_size
    nb = u.numel() // B
    if nb == 0:
        return 0.0, 0.0
    P, Q = perturbed_tables(model) if output_adv else (model.embedding_P, model.embedding_Q)
    bl, bc, _, _ = ops.bpr_forward(P, Q, u, i, j, B)
    bl = bl.double().cpu().numpy()
    bc = bc.cpu().numpy().astype(np.float64)
    return float(bl.sum() / nb), float((bc / B).sum() / nb)


def adv_update(model, sess, train_batches, adv=None):
    """utils.py:145-154: one sess.run([update_P, update_Q]) over the whole epoch's
    triplets as ONE batch.  train_batches: what training_batch returns (an
    EpochTriplets or its three lists).  Sets model.delta_P / model.delta_Q (dense
    device tables, zeros from build_graph on) to direction * model.eps and
    returns them; adv defaults to model.adv ("random": a fresh draw per call).
    The tables and accumulators are not written.
    One deviation from the reference: training here never materialises delta, so
    after training delta_P / delta_Q hold what the last adv_update put there, not
    the last mini-batch's delta as in TF."""
    u, i, j = triplet_arrays(train_batches)
    mode = model.adv if adv is None else adv
    model._adv_calls = getattr(model, "_adv_calls", 0) + 1
    nP, nQ = ops.adv_direction(model.embedding_P, model.embedding_Q, u, i, j, adv=mode,
                               seed=int(model.seed or 0), call=model._adv_calls, t=0)
    model.delta_P = ops.adv_apply(model.embedding_P, nP, model.eps, want_delta=True)[1]
    model.delta_Q = ops.adv_apply(model.embedding_Q, nQ, model.eps, want_delta=True)[1]
    return model.delta_P, model.delta_Q


def output_evaluate(model, sess, dataset, train_batches, eval_feed_dicts, epoch_count, batch_time,
                    train_time, prev_acc, runName, args, output_adv=0):
    """utils.py:81-101."""
    loss_begin = time()
    train_loss, post_acc = training_loss_acc(model, sess, train_batches, output_adv)
    _ = time() - loss_begin
    eval_begin = time()
    result, raw_result = evaluate(model, sess, dataset, eval_feed_dicts, output_adv, args)
    eval_time = time() - eval_begin
    nP = float(torch.linalg.vector_norm(model.embedding_P.double()))
    nQ = float(torch.linalg.vector_norm(model.embedding_Q.double()))
    hr, ndcg, auc = np.swapaxes(result, 0, 1)[-1]
    res = ("Epoch %d [%.1fs + %.1fs]: HR = %.4f, NDCG = %.4f ACC = %.4f ACC_adv = %.4f [%.1fs], "
           "|P|=%.2f, |Q|=%.2f" % (epoch_count, batch_time, train_time, hr, ndcg, prev_acc, post_acc,
                                   eval_time, nP, nQ))
    write2file(args.path + "out/" + args.opath, runName + ".out", res)
    return post_acc, ndcg, result, raw_result


# ---------------------------------------------------------------------------
# checkpoints (APR.py:209-232, 289-292)
def ckpt_dirs(args, time_stamp):
    if args.adver:
        save = "Pretrain/%s/APR/embed_%d/%s/" % (args.dataset, args.embed_size, time_stamp)
        restore = "Pretrain/%s/MF_BPR/embed_%d/%s/" % (args.dataset, args.embed_size, time_stamp)
    else:
        save = "Pretrain/%s/MF_BPR/embed_%d/%s/" % (args.dataset, args.embed_size, time_stamp)
        restore = 0 if args.restore is None else "Pretrain/%s/MF_BPR/embed_%d/%s/" % (
            args.dataset, args.embed_size, args.restore)
    return save, restore


def save_checkpoint(model, directory, step):
    os.makedirs(directory, exist_ok=True)
    ops.settle_tables()
    name = "weights-%d" % step
    np.savez(os.path.join(directory, name + ".npz"),
             embedding_P=model.embedding_P.cpu().numpy(), embedding_Q=model.embedding_Q.cpu().numpy())
    with open(os.path.join(directory, "checkpoint"), "w") as f:
        f.write('model_checkpoint_path: "%s"\nall_model_checkpoint_paths: "%s"\n' % (name, name))
    return os.path.join(directory, name)


def latest_checkpoint(directory):
    idx = os.path.join(directory, "checkpoint")
    if not os.path.exists(idx):
        return None
    with open(idx) as f:
        m = re.search(r'model_checkpoint_path:\s*"([^"]+)"', f.read())
    if not m:
        return None
    path = os.path.join(directory, m.group(1))
    return path if os.path.exists(path + ".npz") else None


def restore_checkpoint(model, path):
    with np.load(path + ".npz", allow_pickle=False) as z:
        P, Q = z["embedding_P"], z["embedding_Q"]
    if P.shape != tuple(model.embedding_P.shape) or Q.shape != tuple(model.embedding_Q.shape):
        raise ValueError(f"checkpoint shapes {P.shape}/{Q.shape} do not match the model")
    model.load_embeddings(P, Q)


# ---------------------------------------------------------------------------
def training(model, dataset, args, runName, epoch_start, epoch_end, time_stamp, sampler=None):
    """APR.py:206-292 on the GPU path.  Differences kept deliberately small: the
    triplet stream comes from the device sampler (seeded; the reference's forked
    sampler is not reproducible), and an epoch that is not evaluated does not
    reuse a stale NDCG (the reference raises NameError there)."""
    from .model import Session
    if not model.built:
        model.build_graph()
    sess = Session(model)
    ckpt_save_path, ckpt_restore_path = ckpt_dirs(args, time_stamp)
    os.makedirs(ckpt_save_path, exist_ok=True)
    if ckpt_restore_path:
        os.makedirs(ckpt_restore_path, exist_ok=True)
    if args.restore is not None or epoch_start:
        ck = latest_checkpoint(ckpt_restore_path) if ckpt_restore_path else None
        if ck:
            restore_checkpoint(model, ck)
            print("restored")
    else:
        logging.info("Initialized from scratch")
    eval_feed_dicts = init_eval_model(dataset, args)
    use_host = getattr(args, "sampler", "device") == "host"
    samples = sampling(dataset) if use_host else None
    if sampler is None and not use_host:
        sampler = DeviceSampler(dataset, args.batch_size, model.device, seed=getattr(args, "seed", 0) or 0)
    graph = not getattr(args, "no_graph", False)
    max_ndcg = 0
    best_res = {}
    epoch_count = epoch_start
    for epoch_count in range(epoch_start, epoch_end + 1):
        batch_begin = time()
        if use_host:
            batches = _as_epoch(model, shuffle(samples, args.batch_size, dataset, model))
        else:
            batches = sampler.epoch(epoch_count)
        torch.cuda.synchronize(model.device)
        batch_time = time() - batch_begin
        _, prev_acc = training_loss_acc(model, sess, batches, output_adv=0)
        train_begin = time()
        train_batches = training_batch(model, sess, batches, args.adver, graph=graph)
        torch.cuda.synchronize(model.device)
        train_time = time() - train_begin
        model.last_train_batches = train_batches  # the CLI's --robust_eps evaluates on them
        if epoch_count % args.verbose == 0:
            _, ndcg, cur_res, raw_result = output_evaluate(
                model, sess, dataset, train_batches, eval_feed_dicts, epoch_count, batch_time,
                train_time, prev_acc, runName, args, output_adv=0)
            if max_ndcg < ndcg:
                max_ndcg = ndcg
                best_res["result"] = cur_res
                best_res["epoch"] = epoch_count
                prediction2file(args.path + "out/" + args.opath, runName + ".hr", raw_result[:, 0, -1])
                prediction2file(args.path + "out/" + args.opath, runName + ".ndcg", raw_result[:, 1, -1])
        if model.epochs == epoch_count and best_res:
            write2file(args.path + "out/" + args.opath, runName + ".out",
                       "Epoch %d is the best epoch" % best_res["epoch"])
            for idx, (hr_k, ndcg_k, auc_k) in enumerate(np.swapaxes(best_res["result"], 0, 1)):
                write2file(args.path + "out/" + args.opath, runName + ".out",
                           "K = %d: HR = %.4f, NDCG = %.4f AUC = %.4f" % (idx + 1, hr_k, ndcg_k, auc_k))
        if args.ckpt > 0 and epoch_count % args.ckpt == 0:
            save_checkpoint(model, ckpt_save_path, epoch_count)
    save_checkpoint(model, ckpt_save_path, epoch_count)
    return best_res


# ---------------------------------------------------------------------------
# a grid of models over one triplet stream
def grid_run_names(grid_model, args, time_stamp):
    """The run name of every member: the name cli.main gives a single apr run at
    that member's (eps, reg_adv); a grid that also varies lr or the seed appends
    _lr<lr> / _s<seed>, which no single-model name has.  A member trained against a
    K-step attack (adv_iters = K > 1) gets _k<K> right after the single-run name;
    one-step members' names are unchanged."""
    from .cli import apr_run_name
    lrs = {a.lr for a in grid_model.member_args}
    seeds = {getattr(a, "seed", None) for a in grid_model.member_args}
    names = []
    for a in grid_model.member_args:
        name = apr_run_name(args.dataset, args.model, args.embed_size, a.eps, a.reg_adv, time_stamp)
        if _adv_iters(a) > 1:
            name += "_k%d" % _adv_iters(a)
        if len(lrs) > 1:
            name += "_lr%f" % a.lr
        if len(seeds) > 1:
            name += "_s%d" % int(a.seed or 0)
        names.append(name)
    if len(set(names)) != len(names):
        names = ["%s_g%d" % (n, m) for m, n in enumerate(names)]  # members equal in all four: tell them apart
    return names


def _adv_iters(a):
    return int(getattr(a, "adv_iters", 1) or 1)


def write_grid_table(path, name, grid_model, best):
    """<runName>.grid: one line per member, "member<TAB>eps<TAB>reg_adv<TAB>lr<TAB>reg<TAB>adver<TAB>seed<TAB>
    best_epoch<TAB>hr10<TAB>ndcg10" (floats by repr; best_epoch -1 and nan metrics: never evaluated).  A grid
    with a member of adv_iters > 1 appends "<TAB>adv_iters<TAB>adv_step" to every line (adv_step: the step
    size trained with, ops.grid_pgd_arguments); a grid of one-step members writes the ten columns alone."""
    from .ops import StepHParams, grid_pgd_arguments
    os.makedirs(path, exist_ok=True)
    pgd = any(_adv_iters(a) > 1 for a in grid_model.member_args)
    with open(os.path.join(path, name), "w") as f:
        for m, a in enumerate(grid_model.member_args):
            b = best[m]
            line = "%d\t%r\t%r\t%r\t%r\t%d\t%d\t%d\t%r\t%r" % (
                m, float(a.eps), float(a.reg_adv), float(a.lr), float(a.reg), int(bool(a.adver)),
                int(getattr(a, "seed", 0) or 0), b.get("epoch", -1), float(b.get("hr10", float("nan"))),
                float(b.get("ndcg10", float("nan"))))
            if pgd:
                K, alpha = grid_pgd_arguments(StepHParams(eps=a.eps, adv_iters=_adv_iters(a),
                                                          adv_step=getattr(a, "adv_step", None)), m)
                line += "\t%d\t%r" % (K, float(alpha))
            f.write(line + "\n")


def read_grid_table(file):
    """The rows [(member, eps, reg_adv, lr, reg, adver, seed, best_epoch, hr10, ndcg10)] write_grid_table wrote;
    rows of a file with the two trailing columns end in (..., adv_iters, adv_step)."""
    rows = []
    with open(file) as f:
        for n, line in enumerate(f):
            p = line.rstrip("\n").split("\t")
            if len(p) not in (10, 12):
                raise ValueError(f"{file}: line {n} has {len(p)} fields, expected 10 or 12")
            row = (int(p[0]), float(p[1]), float(p[2]), float(p[3]), float(p[4]), int(p[5]), int(p[6]),
                   int(p[7]), float(p[8]), float(p[9]))
            rows.append(row + (int(p[10]), float(p[11])) if len(p) == 12 else row)
    return rows


def training_grid(grid_model, dataset, args, runName, epoch_start, epoch_end, time_stamp, sampler=None,
                  single=False):
    """`training` for an MFGrid: every epoch draws ONE sampled triplet stream and
    trains all members on it in one ops.grid_train call.  The members therefore
    see common negatives (common random numbers): a difference between two
    members of a grid is a difference of their hyper-parameters or seeds, not
    sampling noise, but M members are not M independent replications of the
    sampler.  Every args.verbose epochs each member is evaluated through the
    existing evaluation (output_evaluate on grid_model.member(m)) and logs to its
    own <name>.out / .hr / .ndcg in the reference's formats, under the name a
    single run at its (eps, reg_adv) gets (grid_run_names); the best epoch is
    tracked per member, and <runName>.grid holds one line per member
    (write_grid_table).  Returns the per-member best results.
    single: a grid of one standing in for a plain run (training_single_pgd): the
    member logs under runName itself and is checkpointed as `training` does, every
    args.ckpt epochs and at the end, and no .grid table is written."""
    M = len(grid_model)
    if single and M != 1:
        raise ValueError(f"single=True is a grid of one, got {M} members")
    names = [runName] if single else grid_run_names(grid_model, args, time_stamp)
    out = args.path + "out/" + args.opath
    eval_feed_dicts = init_eval_model(dataset, args)
    if sampler is None:
        sampler = DeviceSampler(dataset, args.batch_size, grid_model.device, seed=getattr(args, "seed", 0) or 0)
    members = [grid_model.member(m) for m in range(M)]
    best = [{} for _ in range(M)]
    max_ndcg = [0.0] * M
    k10 = min(10, eval_feed_dicts.K) - 1
    epoch_count = epoch_start
    for epoch_count in range(epoch_start, epoch_end + 1):
        batch_begin = time()
        ep = sampler.epoch(epoch_count)
        torch.cuda.synchronize(grid_model.device)
        batch_time = time() - batch_begin
        evaluated = epoch_count % args.verbose == 0
        prev_acc = [training_loss_acc(mf, None, ep, output_adv=0)[1] for mf in members] if evaluated else None
        train_begin = time()
        grid_model.train_epoch(ep.user, ep.item_pos, ep.item_neg, ep.batch_size)
        torch.cuda.synchronize(grid_model.device)
        train_time = time() - train_begin
        for mf in members:
            mf.last_train_batches = ep
        if evaluated:
            for m, mf in enumerate(members):
                _, ndcg, cur_res, raw_result = output_evaluate(
                    mf, None, dataset, ep, eval_feed_dicts, epoch_count, batch_time, train_time, prev_acc[m],
                    names[m], args, output_adv=0)
                if max_ndcg[m] < ndcg:
                    max_ndcg[m] = ndcg
                    hr_k, ndcg_k, _ = cur_res
                    best[m] = {"result": cur_res, "epoch": epoch_count, "hr10": hr_k[k10], "ndcg10": ndcg_k[k10]}
                    prediction2file(out, names[m] + ".hr", raw_result[:, 0, -1])
                    prediction2file(out, names[m] + ".ndcg", raw_result[:, 1, -1])
        if args.epochs == epoch_count:
            for m in range(M):
                if not best[m]:
                    continue
                write2file(out, names[m] + ".out", "Epoch %d is the best epoch" % best[m]["epoch"])
                for idx, (hr_k, ndcg_k, auc_k) in enumerate(np.swapaxes(best[m]["result"], 0, 1)):
                    write2file(out, names[m] + ".out",
                               "K = %d: HR = %.4f, NDCG = %.4f AUC = %.4f" % (idx + 1, hr_k, ndcg_k, auc_k))
        if single and args.ckpt > 0 and epoch_count % args.ckpt == 0:
            save_checkpoint(members[0], ckpt_dirs(args, time_stamp)[0], epoch_count)
    if single:
        save_checkpoint(members[0], ckpt_dirs(args, time_stamp)[0], epoch_count)
        return best
    write_grid_table(out, runName + ".grid", grid_model, best)
    if getattr(args, "ckpt", 0) > 0:
        for m, mf in enumerate(members):
            save_checkpoint(mf, ckpt_dirs(args, "%s_g%d" % (time_stamp, m))[0], epoch_count)
    return best


def training_single_pgd(bpr_model, dataset, args, runName, time_stamp):
    """The APR phase of a plain apr run trained against a K-step attack (args.adv_iters
    > 1): only the grid trainer has that attack, so the run is a grid of one.  The member
    branches from the BPR model (args.adv_epoch > 0) or starts from the seed's init, as the
    members of a --grid_* run do, trains epochs adv_epoch .. epochs and evaluates,
    logs and checkpoints under runName as `training` would.  Returns the member, an MF."""
    from .model import MFGrid
    if args.adv_epoch > 0:
        gm = MFGrid.from_model(bpr_model, [{}], args)
    else:
        gm = MFGrid(dataset.num_users, dataset.num_items, args, [{}], device=bpr_model.device)
    write2file(args.path + "out/" + args.opath, runName + ".out", "Initialize APR")
    training_grid(gm, dataset, args, runName, epoch_start=args.adv_epoch, epoch_end=args.epochs,
                  time_stamp=time_stamp, single=True)
    return gm.member(0)
