"""Command-line drivers with the flag surface of ``run_adv_ori.py:17-64`` (the
script that produced the published logs) and ``run_adv.py:15-54`` (the one named
in the task), restricted to the models on the APR path (``bpr``, ``apr``).

    python run_adv_ori.py --dataset Video --model apr --epochs 2000 --adv_epoch 1000 \
        --verbose 20 --eval_mode all --embed_size 64
"""
from __future__ import annotations

import argparse
import logging
import os
import sys
from time import localtime, strftime

# (flag, type, default-for-run_adv_ori, default-for-run_adv, help)
_FLAGS = [
    ("--path", str, "", "", "Input data path."),
    ("--opath", str, "aaa/", "aaa/", "Output path."),
    ("--dataset", str, "fsq11-sort", "ml-1m", "Dataset file prefix under <path>data/, or "
                                              "ml-1m-synthetic / pinterest-20-synthetic."),
    ("--model", str, "pop", "apr", "bpr or apr."),
    ("--verbose", int, 1, 1, "Evaluate per X epochs."),
    ("--batch_size", int, 512, 512, "batch_size"),
    ("--epochs", int, 10, 2, "Number of epochs."),
    ("--adv_epoch", int, 0, 1, "Add APR in epoch X (0: pure APR; > epochs: pure BPR)."),
    ("--embed_size", int, 64, 64, "Embedding size."),
    ("--dns", int, 1, 1, "Number of negative samples per positive (dns)."),
    ("--reg", float, 0.0, 0.0, "Regularization for user and item embeddings."),
    ("--lr", float, 0.05, 0.05, "Learning rate."),
    ("--reg_adv", float, 1.0, 1.0, "Regularization for adversarial loss."),
    ("--restore", str, None, None, "Restore time_stamp for weights in Pretrain/."),
    ("--ckpt", int, 10, 1, "Save the model per X epochs."),
    ("--task", str, "", "", "Task name for launching experiments."),
    ("--adv", str, "grad", "grad", "Adversarial perturbation: grad or random."),
    ("--eps", float, 0.5, 0.5, "Epsilon for adversarial weights."),
]
_ORI_ONLY = [
    ("--eps_dense", float, 0.5, "Accepted for compatibility (SASRec only)."),
    ("--eps_conv", float, 0.5, "Accepted for compatibility (SASRec only)."),
    ("--eps_pos", float, 0.5, "Accepted for compatibility (SASRec only)."),
    ("--eval_mode", str, "sample", "Eval mode: sample or all."),
]


def parse_args(argv=None, flavor="ori"):
    p = argparse.ArgumentParser(description="Run AMF (MI355X APR path).")
    for flag, typ, d_ori, d_adv, hlp in _FLAGS:
        nargs = "?" if flag in ("--path", "--opath", "--dataset", "--task", "--adv") else None
        kw = dict(type=typ, default=d_ori if flavor == "ori" else d_adv, help=hlp)
        if nargs:
            kw["nargs"] = nargs
        p.add_argument(flag, **kw)
    if flavor == "ori":
        for flag, typ, d, hlp in _ORI_ONLY:
            p.add_argument(flag, type=typ, default=d, help=hlp)
    else:
        p.set_defaults(eval_mode="all")  # run_adv.py evaluates all items (evaluation_adv.py:440)
    # MI355X-build extras
    p.add_argument("--seed", type=int, default=0, help="Seed of init and device sampler.")
    p.add_argument("--sampler", choices=["device", "host"], default="device")
    p.add_argument("--no_graph", action="store_true", help="Launch eagerly instead of hipGraph replay.")
    p.add_argument("--topk", type=int, default=0,
                   help="After training, write each user's K best items (train items excluded) to "
                        "<out>/<runName>.topk (0: off).")
    p.add_argument("--robust_eps", type=parse_eps_list, default=[],
                   help="After training, evaluate under perturbed tables at these eps (comma separated, e.g. "
                        "\"0.5,1,2\"), gradient and random directions over the last epoch's triplets, and write "
                        "<out>/<runName>.robust (empty: off).")
    p.add_argument("--robust_iters", type=parse_robust_iters, default=0,
                   help="With --robust_eps: also an iterated gradient attack of this many projected steps per eps "
                        "(1 to 1024), written as 'pgd' rows after the others (0: off).")
    p.add_argument("--robust_step", type=parse_robust_step, default=None,
                   help="Step size of --robust_iters (default: 2.5 * eps / iters).")
    p.add_argument("--robust_lists", type=parse_radius_cutoffs, default=[],
                   help="With --robust_eps: also how far each attack moves the users' top-K lists, at these K "
                        "(comma separated, e.g. \"1,10,100\"; 1 to 8 integers in [1, 128]; the lists are as long "
                        "as the largest): Jaccard, rank-biased overlap and overlap against the clean lists, and "
                        "coverage, Gini, entropy, average popularity and long-tail share of what is recommended, "
                        "to <out>/<runName>.lists (empty: off).")
    p.add_argument("--certify_eps", type=parse_eps_list, default=[],
                   help="After training, certify the ranking at these eps (comma separated, e.g. \"0.1,0.5,1\"): "
                        "lower bounds of HR@K, NDCG@K and AUC (all-items evaluation) under EVERY perturbation of "
                        "at most eps per embedding row in L2; writes <out>/<runName>.certified (empty: off).")
    p.add_argument("--certify_side", choices=["user", "item", "both"], default="user",
                   help="Which rows --certify_eps and --certify_radius let the attacker move: the user rows, the "
                        "item rows, or both as two separate passes (not a joint attack).")
    p.add_argument("--certify_radius", type=parse_radius_cutoffs, default=[],
                   help="After training, write the distribution over users of the certified radius at these K "
                        "(comma separated, e.g. \"1,10,50\"; 1 to 8 integers in [1, 128]): the largest eps up to "
                        "which the held-out item provably stays in the top K (all-items evaluation, one sweep at "
                        "K = the largest), to <out>/<runName>.radius (empty: off).  Uses --certify_side.")
    p.add_argument("--fold_in", type=str, default=None, metavar="FILE",
                   help="After training, fold in the new users of FILE (rating TSV: uid<TAB>item<TAB>...; its "
                        "uids are keys of new users, not rows of the user table) and write their --topk best "
                        "items to <out>/<runName>.foldin.topk (rows in ascending uid order) and the uids to "
                        "<out>/<runName>.foldin.users.  Needs --topk.")
    p.add_argument("--fold_in_items", type=str, default=None, metavar="FILE",
                   help="After training, fold in the new items of FILE (rating TSV: uid<TAB>item<TAB>...; its "
                        "items are keys of new items, not rows of the item table; its uids are rows of the user "
                        "table) and write the --topk best existing users of each to <out>/<runName>.folditems.topk "
                        "(rows in ascending item key order, the item's own users excluded) and the keys to "
                        "<out>/<runName>.folditems.items.  Needs --topk.")
    p.add_argument("--test_multi", type=str, default=None, metavar="FILE",
                   help="After training, evaluate against SEVERAL held-out items per user: the rows of FILE "
                        "(rating TSV: uid<TAB>item<TAB>...) are the users' test lists; writes "
                        "<out>/<runName>.multi, one line name<TAB>value per metric (hit, recall, precision, "
                        "ndcg, map at every --cutoffs K, then mrr, auc, n_users).")
    p.add_argument("--cutoffs", type=parse_cutoffs, default=[10, 50, 100],
                   help="The K of --test_multi's metrics: up to 8 integers in [1, 1024], comma separated.")
    p.add_argument("--similar", type=str, default=None, metavar="FILE",
                   help="After training, write the --topk items most like each item of FILE (one item id per line) "
                        "to <out>/<runName>.similar: line n is for the n-th id of FILE, in --topk's format; an item "
                        "is never its own neighbour.  Needs --topk.")
    p.add_argument("--similar_metric", choices=["dot", "cosine", "euclid"], default="cosine",
                   help="The similarity of --similar: cosine, the dot product, or euclid (nearest by L2 distance).")
    p.add_argument("--diverse_lambda", type=parse_lambda_list, default=[],
                   help="After training, re-rank each user's --diverse_pool best items to --topk by maximal marginal "
                        "relevance at these lambda in [0, 1] (comma separated, e.g. \"1,0.7,0.5\"; 1 keeps the "
                        "plain top-K) and write, per lambda, HR and NDCG of the held-out item, the intra-list "
                        "similarity and the exposure metrics of the lists to <out>/<runName>.diverse (empty: off).  "
                        "Needs --topk.")
    p.add_argument("--diverse_pool", type=int, default=128,
                   help="The size of the candidate pool of --diverse_lambda: --topk <= N <= 128.")
    p.add_argument("--diverse_metric", choices=["dot", "cosine", "euclid"], default="cosine",
                   help="The item similarity of --diverse_lambda.")
    p.add_argument("--grid_eps", type=parse_eps_list, default=[],
                   help="With --model apr: train the APR phase as a grid, one member per value of eps (comma "
                        "separated, e.g. \"0.1,0.5,1\"), all members over one triplet stream in one call per epoch. "
                        "The BPR phase runs once; every member branches from it.  The grid is the product of the "
                        "--grid_* lists; each member logs under the run name a single run at its (eps, reg_adv) "
                        "gets, and <out>/<runName>.grid lists the members (empty: off).")
    p.add_argument("--grid_reg_adv", type=parse_eps_list, default=[],
                   help="Grid axis: values of reg_adv (comma separated).")
    p.add_argument("--grid_lr", type=parse_grid_lr, default=[], help="Grid axis: values of lr (comma separated).")
    p.add_argument("--grid_seeds", type=parse_grid_seeds, default=0,
                   help="Grid axis: N members per point, seeds 0..N-1 (they differ where the APR phase starts from "
                        "scratch, --adv_epoch 0; 0: off).")
    p.add_argument("--grid_adv_iters", type=parse_grid_adv_iters, default=[],
                   help="Grid axis (the outermost): steps K of the inner attack each member is trained against (comma "
                        "separated, e.g. \"1,3,5\", each in [1, 32]).  K = 1 is APR's one normalised gradient step; "
                        "K > 1 is a projected-gradient attack of K steps inside the eps ball, and that member logs "
                        "under its run name plus _k<K>.")
    p.add_argument("--adv_iters", type=parse_adv_iters, default=1,
                   help="With --model apr: train the APR phase against a K-step projected-gradient attack inside "
                        "the eps ball (1 to 32) instead of one normalised gradient step; the run is named "
                        "<runName>_k<K>.  With --grid_*: the K of every member (unless --grid_adv_iters is given).  "
                        "Check the result with --robust_eps ... --robust_iters.")
    p.add_argument("--adv_step", type=parse_robust_step, default=None,
                   help="Step size of --adv_iters / --grid_adv_iters (default: 2.5 * eps / K).")
    args = p.parse_args(argv)
    if args.model != "apr" and (args.adv_iters > 1 or args.grid_adv_iters):
        p.error("--adv_iters / --grid_adv_iters train the APR phase: they need --model apr")
    if args.adv_step is not None and args.adv_iters == 1 and not args.grid_adv_iters:
        p.error("--adv_step needs --adv_iters K > 1 or --grid_adv_iters")
    if (args.adv_iters > 1 or args.grid_adv_iters) and (args.adv != "grad" or args.dns != 1):
        p.error("--adv_iters / --grid_adv_iters need --adv grad and --dns 1")
    if grid_of(args) is not None:
        extras = [f for f in ("topk", "fold_in", "fold_in_items", "test_multi", "similar", "robust_eps",
                              "robust_lists", "certify_eps", "certify_radius", "diverse_lambda") if getattr(args, f)]
        if extras:
            p.error("--grid_* trains several models; --%s works on one (run it on a member's checkpoint)" % extras[0])
        if len(grid_of(args)) > 64:
            p.error("a grid has at most 64 members, the product of the --grid_* lists has %d" % len(grid_of(args)))
    if args.fold_in is not None and args.topk <= 0:
        p.error("--fold_in needs --topk K (K > 0)")
    if args.fold_in_items is not None and args.topk <= 0:
        p.error("--fold_in_items needs --topk K (K > 0)")
    if args.similar is not None and args.topk <= 0:
        p.error("--similar needs --topk K (K > 0)")
    if args.diverse_lambda and not 1 <= args.topk <= args.diverse_pool <= 128:
        p.error("--diverse_lambda needs 1 <= --topk <= --diverse_pool <= 128")
    return args


def parse_eps_list(text):
    """"0.5,1,2" -> [0.5, 1.0, 2.0]; empty -> [] (off); a negative or non-numeric value is an error."""
    out = []
    for tok in str(text).split(","):
        tok = tok.strip()
        if not tok:
            continue
        try:
            v = float(tok)
        except ValueError:
            raise argparse.ArgumentTypeError(f"not a number: {tok!r}")
        if not v >= 0 or v == float("inf"):
            raise argparse.ArgumentTypeError(f"eps must be finite and >= 0, got {tok!r}")
        out.append(v)
    return out


def parse_grid_lr(text):
    """--grid_lr: "0.01,0.05" -> [0.01, 0.05]; every value finite and > 0."""
    out = parse_eps_list(text)
    for v in out:
        if not v > 0:
            raise argparse.ArgumentTypeError(f"a learning rate must be > 0, got {v!r}")
    return out


def parse_grid_seeds(text):
    """--grid_seeds: an integer in [0, 64] (0: off)."""
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not an integer: {text!r}")
    if not 0 <= v <= 64:
        raise argparse.ArgumentTypeError(f"grid_seeds must lie in [0, 64], got {text!r}")
    return v


def parse_lambda_list(text):
    """--diverse_lambda: "1,0.7,0.5" -> [1.0, 0.7, 0.5]; every value in [0, 1]."""
    out = parse_eps_list(text)
    for v in out:
        if not v <= 1:
            raise argparse.ArgumentTypeError(f"a lambda must lie in [0, 1], got {v!r}")
    return out


def parse_adv_iters(text):
    """--adv_iters: an integer in [1, 32] (ops.GRID_MAX_ADV_ITERS)."""
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not an integer: {text!r}")
    if not 1 <= v <= 32:
        raise argparse.ArgumentTypeError(f"adv_iters must lie in [1, 32], got {text!r}")
    return v


def parse_grid_adv_iters(text):
    """--grid_adv_iters: "1,3,5" -> [1, 3, 5]; every value in [1, 32]."""
    return [parse_adv_iters(tok.strip()) for tok in str(text).split(",") if tok.strip()]


def grid_of(args):
    """The grid dicts of the --grid_* flags (model.MFGrid.product order: adv_iters
    slowest when given, then eps, reg_adv, lr, the seed fastest), or None when no
    --grid_* flag is given."""
    axes = dict(eps=args.grid_eps or None, reg_adv=args.grid_reg_adv or None, lr=args.grid_lr or None,
                seeds=args.grid_seeds or None)
    iters = getattr(args, "grid_adv_iters", None) or None
    if iters is not None:
        axes.update(adv_iters=iters, adv_step=getattr(args, "adv_step", None))
    if all(v is None for v in axes.values()):
        return None
    from .model import MFGrid
    return MFGrid.product(**axes)


def single_adv_iters(args):
    """K of a plain apr run trained through a one-member grid (--adv_iters K > 1 without a
    --grid_* flag), else 0."""
    K = getattr(args, "adv_iters", 1)
    return K if K > 1 and grid_of(args) is None else 0


def apr_run_name(dataset, model, embed_size, eps, reg_adv, time_stamp):
    """The run name of an apr run (run_adv_ori.py:91)."""
    return "%s_%s_d%d_e%f_l%f_%s" % (dataset, model, embed_size, eps, reg_adv, time_stamp)


def parse_robust_iters(text):
    """--robust_iters: an integer in [0, 1024] (0: off)."""
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not an integer: {text!r}")
    if not 0 <= v <= 1024:
        raise argparse.ArgumentTypeError(f"robust_iters must lie in [0, 1024], got {text!r}")
    return v


def parse_robust_step(text):
    """--robust_step: a finite step size >= 0."""
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a number: {text!r}")
    if not v >= 0 or v == float("inf"):
        raise argparse.ArgumentTypeError(f"robust_step must be finite and >= 0, got {text!r}")
    return v


def parse_cutoffs(text):
    """"10,50,100" -> [10, 50, 100]: 1 to 8 integers in [1, 1024]."""
    out = []
    for tok in str(text).split(","):
        tok = tok.strip()
        if not tok:
            continue
        try:
            v = int(tok)
        except ValueError:
            raise argparse.ArgumentTypeError(f"not an integer: {tok!r}")
        if not 1 <= v <= 1024:
            raise argparse.ArgumentTypeError(f"a cutoff must lie in [1, 1024], got {tok!r}")
        out.append(v)
    if not 1 <= len(out) <= 8:
        raise argparse.ArgumentTypeError(f"1 to 8 cutoffs, got {len(out)}")
    return out


def write_multi(path, name, metrics, cutoffs):
    """One line "name<TAB>value" per metric of evaluate.evaluate_multi, in
    evaluate.metric_names order (floats by repr: the reader gets the same values back)."""
    from .evaluate import metric_names
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, name), "w") as f:
        for key in metric_names(cutoffs):
            v = metrics[key]
            f.write("%s\t%s\n" % (key, "%d" % v if key == "n_users" else repr(float(v))))


def read_multi(file):
    """The dict write_multi wrote (insertion order = file order; n_users an int)."""
    out = {}
    with open(file) as f:
        for n, line in enumerate(f):
            parts = line.rstrip("\n").split("\t")
            if len(parts) != 2:
                raise ValueError(f"{file}: line {n} has {len(parts)} fields, expected 2")
            out[parts[0]] = int(parts[1]) if parts[0] == "n_users" else float(parts[1])
    return out


def parse_radius_cutoffs(text):
    """"1,10,50" -> [1, 10, 50]: 1 to 8 integers in [1, 128] (ops.TOPK_MAX_K)."""
    out = parse_cutoffs(text)
    for v in out:
        if v > 128:
            raise argparse.ArgumentTypeError(f"a radius cutoff must lie in [1, 128], got {v}")
    return out


def write_robust(path, name, rows):
    """One line "mode<TAB>eps<TAB>hr<TAB>ndcg<TAB>auc" per row of evaluate.robustness
    (floats by repr: the reader gets the same values back)."""
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, name), "w") as f:
        for mode, eps, hr, ndcg, auc in rows:
            f.write("%s\t%r\t%r\t%r\t%r\n" % (mode, float(eps), float(hr), float(ndcg), float(auc)))


def read_robust(file):
    """The rows [(mode, eps, hr, ndcg, auc)] write_robust wrote."""
    rows = []
    with open(file) as f:
        for n, line in enumerate(f):
            parts = line.rstrip("\n").split("\t")
            if len(parts) != 5:
                raise ValueError(f"{file}: line {n} has {len(parts)} fields, expected 5")
            rows.append((parts[0], *[float(x) for x in parts[1:]]))
    return rows


def write_certified(path, name, rows):
    """One line "side<TAB>eps<TAB>K<TAB>hr_lb<TAB>ndcg_lb<TAB>auc_lb" per row of
    evaluate.certified (floats by repr: the reader gets the same values back)."""
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, name), "w") as f:
        for side, eps, K, hr, ndcg, auc in rows:
            f.write("%s\t%r\t%d\t%r\t%r\t%r\n" % (side, float(eps), int(K), float(hr), float(ndcg), float(auc)))


def read_certified(file):
    """The rows [(side, eps, K, hr_lb, ndcg_lb, auc_lb)] write_certified wrote."""
    rows = []
    with open(file) as f:
        for n, line in enumerate(f):
            parts = line.rstrip("\n").split("\t")
            if len(parts) != 6:
                raise ValueError(f"{file}: line {n} has {len(parts)} fields, expected 6")
            rows.append((parts[0], float(parts[1]), int(parts[2]), *[float(x) for x in parts[3:]]))
    return rows


def write_lists(path, name, rows):
    """One line "mode<TAB>eps<TAB>K<TAB>jaccard<TAB>rbo<TAB>overlap<TAB>coverage<TAB>gini<TAB>entropy<TAB>arp
    <TAB>aplt" per row of evaluate.list_robustness (floats by repr: the reader gets the same values back)."""
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, name), "w") as f:
        for mode, eps, K, *vals in rows:
            if len(vals) != 8:
                raise ValueError(f"a lists row has 8 metrics, got {len(vals)}")
            f.write("%s\t%r\t%d\t%s\n" % (mode, float(eps), int(K), "\t".join(repr(float(v)) for v in vals)))


def read_lists(file):
    """The rows [(mode, eps, K, jaccard, rbo, overlap, coverage, gini, entropy, arp, aplt)] write_lists wrote."""
    rows = []
    with open(file) as f:
        for n, line in enumerate(f):
            parts = line.rstrip("\n").split("\t")
            if len(parts) != 11:
                raise ValueError(f"{file}: line {n} has {len(parts)} fields, expected 11")
            rows.append((parts[0], float(parts[1]), int(parts[2]), *[float(x) for x in parts[3:]]))
    return rows


def write_diverse(path, name, rows):
    """One line "lam<TAB>K<TAB>hr<TAB>ndcg<TAB>ils<TAB>total<TAB>coverage<TAB>gini<TAB>entropy<TAB>arp<TAB>aplt"
    per row of evaluate.diversity_tradeoff (floats by repr: the reader gets the same values back)."""
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, name), "w") as f:
        for lam, K, *vals in rows:
            if len(vals) != 9:
                raise ValueError(f"a diverse row has 9 metrics, got {len(vals)}")
            f.write("%r\t%d\t%s\n" % (float(lam), int(K), "\t".join(repr(float(v)) for v in vals)))


def read_diverse(file):
    """The rows [(lam, K, hr, ndcg, ils, total, coverage, gini, entropy, arp, aplt)] write_diverse wrote."""
    rows = []
    with open(file) as f:
        for n, line in enumerate(f):
            parts = line.rstrip("\n").split("\t")
            if len(parts) != 11:
                raise ValueError(f"{file}: line {n} has {len(parts)} fields, expected 11")
            rows.append((float(parts[0]), int(parts[1]), *[float(x) for x in parts[2:]]))
    return rows


def write_radius(path, name, rows):
    """One line "side<TAB>K<TAB>missed<TAB>unbounded<TAB>q10<TAB>q25<TAB>q50<TAB>q75<TAB>q90" per
    (side, *row of evaluate.radius_summary) (floats by repr: the reader gets the same
    values back; a quantile of no finite radius is nan)."""
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, name), "w") as f:
        for side, K, missed, unbounded, *qs in rows:
            if len(qs) != 5:
                raise ValueError(f"a radius row has 5 quantiles, got {len(qs)}")
            f.write("%s\t%d\t%s\n" % (side, int(K), "\t".join(repr(float(v)) for v in (missed, unbounded, *qs))))


def read_radius(file):
    """The rows [(side, K, missed, unbounded, q10, q25, q50, q75, q90)] write_radius wrote."""
    rows = []
    with open(file) as f:
        for n, line in enumerate(f):
            parts = line.rstrip("\n").split("\t")
            if len(parts) != 9:
                raise ValueError(f"{file}: line {n} has {len(parts)} fields, expected 9")
            rows.append((parts[0], int(parts[1]), *[float(x) for x in parts[2:]]))
    return rows


def read_fold_file(file):
    """{uid: [items]} of a rating file in the reference's TSV format
    ("uid<TAB>item[<TAB>rating[<TAB>time]]", ids possibly written as floats);
    items in file order, repeats kept (fold_lists de-duplicates)."""
    lists = {}
    with open(file) as f:
        for n, line in enumerate(f):
            line = line.strip()
            if not line:
                continue
            parts = line.split("\t")
            if len(parts) < 2:
                raise ValueError(f"{file}: line {n} has {len(parts)} field(s), expected uid<TAB>item")
            try:
                uid, item = float(parts[0]), float(parts[1])
            except ValueError:
                raise ValueError(f"{file}: line {n}: uid and item must be numbers") from None
            if uid != int(uid) or item != int(item) or uid < 0 or item < 0:
                raise ValueError(f"{file}: line {n}: uid and item must be integers >= 0")
            lists.setdefault(int(uid), []).append(int(item))
    return lists


def read_fold_items_file(file):
    """{item key: [uids]} of the same rating file read by its item column: the
    users of every new item, in file order, repeats kept."""
    lists = {}
    for uid, items in read_fold_file(file).items():
        for item in items:
            lists.setdefault(item, []).append(uid)
    return lists


def read_id_file(file):
    """The ids of a file with one integer >= 0 per line (blank lines skipped)."""
    ids = []
    with open(file) as f:
        for n, line in enumerate(f):
            line = line.strip()
            if not line:
                continue
            try:
                v = int(line)
            except ValueError:
                raise ValueError(f"{file}: line {n}: not an integer: {line!r}") from None
            if v < 0:
                raise ValueError(f"{file}: line {n}: an id must be >= 0, got {v}")
            ids.append(v)
    return ids


def write_fold_users(path, name, keys):
    """One uid per line, in the row order of the .foldin.topk file."""
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, name), "w") as f:
        for k in keys:
            f.write("%d\n" % int(k))


def write_topk(path, name, items):
    """One line per user 0..n-1 of an [n, K] item array: "user<TAB>item1,item2,...",
    best first; the -1 padding of a user with fewer than K candidates is left out."""
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, name), "w") as f:
        for u, row in enumerate(items):
            f.write("%d\t%s\n" % (u, ",".join(str(int(i)) for i in row if i >= 0)))


def read_topk(file, k=None):
    """The int32 [n, K] array write_topk wrote (short lines padded with -1; K: the
    longest line unless given)."""
    import numpy as np
    rows = []
    with open(file) as f:
        for n, line in enumerate(f):
            user, _, items = line.rstrip("\n").partition("\t")
            if int(user) != n:
                raise ValueError(f"{file}: line {n} is for user {user}")
            rows.append([int(i) for i in items.split(",") if i])
    k = max([len(r) for r in rows], default=0) if k is None else k
    out = np.full((len(rows), k), -1, dtype=np.int32)
    for n, r in enumerate(rows):
        out[n, :len(r)] = r[:k]
    return out


def init_logging(args, time_stamp):
    """utils.py:270-277."""
    path = "Log/%s_%s/" % (strftime("%Y-%m-%d_%H", localtime()), args.task)
    os.makedirs(path, exist_ok=True)
    logging.basicConfig(filename=path + "%s_log_embed_size%d_%s" % (args.dataset, args.embed_size, time_stamp),
                        level=logging.INFO)
    logging.info(args)
    print(args)


def main(argv=None, flavor="ori"):
    from .data import get_dataset
    from .model import MF
    from .train import training, write2file

    time_stamp = strftime("%Y_%m_%d_%H_%M_%S", localtime())
    args = parse_args(argv, flavor)
    init_logging(args, time_stamp)
    dataset = get_dataset(args.dataset, args.path, seed=2019)
    out = args.path + "out/" + args.opath
    if args.model == "bpr":
        runName = "%s_%s_d%d_%s" % (args.dataset, args.model, args.embed_size, time_stamp)
        write2file(out, runName + ".out", runName)
        args.adver = 0
        m = MF(dataset.num_users, dataset.num_items, args).build_graph()
        write2file(out, runName + ".out", "Initialize MF_BPR")
        training(m, dataset, args, runName, epoch_start=0, epoch_end=args.epochs, time_stamp=time_stamp)
    elif args.model == "apr":
        runName = "%s_%s_d%d_e%f_l%f_%s" % (args.dataset, args.model, args.embed_size, args.eps,
                                             args.reg_adv, time_stamp)
        if single_adv_iters(args):  # trained through a one-member grid, named as that member is
            runName += "_k%d" % args.adv_iters
        write2file(out, runName + ".out", runName)
        args.adver = 0
        m = MF(dataset.num_users, dataset.num_items, args).build_graph()
        write2file(out, runName + ".out", "Initialize BPR")
        training(m, dataset, args, runName, epoch_start=0, epoch_end=args.adv_epoch - 1,
                 time_stamp=time_stamp)
        args.adver = 1
        grid = grid_of(args)
        if grid is not None:  # the APR phase as a grid: every member branches from the one BPR model
            from .model import MFGrid
            from .train import training_grid
            if args.adv_epoch > 0:
                gm = MFGrid.from_model(m, grid, args)
            else:  # no BPR phase: every member starts from its own seed's init
                gm = MFGrid(dataset.num_users, dataset.num_items, args, grid, device=m.device)
            write2file(out, runName + ".out", "Initialize APR grid of %d" % len(gm))
            training_grid(gm, dataset, args, runName, epoch_start=args.adv_epoch, epoch_end=args.epochs,
                          time_stamp=time_stamp)
            return 0
        if single_adv_iters(args):  # the K-step attack lives in the grid trainer: a grid of one
            from .train import training_single_pgd
            amf = training_single_pgd(m, dataset, args, runName, time_stamp)
        else:
            amf = MF(dataset.num_users, dataset.num_items, args).build_graph(device=m.device)
            write2file(out, runName + ".out", "Initialize APR")
            training(amf, dataset, args, runName, epoch_start=args.adv_epoch, epoch_end=args.epochs,
                     time_stamp=time_stamp)
    else:
        print("model %r is not on the APR path of this build (bpr, apr)" % args.model, file=sys.stderr)
        return 2
    if args.topk > 0:
        from .evaluate import recommend
        final = amf if args.model == "apr" else m
        items, _ = recommend(final, dataset, k=args.topk)
        write_topk(out, runName + ".topk", items)
    if args.fold_in is not None:
        from .evaluate import recommend_new
        final = amf if args.model == "apr" else m
        lists = read_fold_file(args.fold_in)
        items, _ = recommend_new(final, lists, args.topk, seed=args.seed, batch=min(args.batch_size, 512))
        write_topk(out, runName + ".foldin.topk", items)
        write_fold_users(out, runName + ".foldin.users", sorted(lists))
    if args.fold_in_items is not None:
        from .evaluate import audience_new
        final = amf if args.model == "apr" else m
        lists = read_fold_items_file(args.fold_in_items)
        users, _ = audience_new(final, lists, args.topk, seed=args.seed, batch=min(args.batch_size, 512),
                                dataset=dataset)
        write_topk(out, runName + ".folditems.topk", users)
        write_fold_users(out, runName + ".folditems.items", sorted(lists))
    if args.similar is not None:
        from .evaluate import similar_items
        final = amf if args.model == "apr" else m
        items, _ = similar_items(final, read_id_file(args.similar), k=args.topk, metric=args.similar_metric)
        write_topk(out, runName + ".similar", items)  # line n: the n-th id of FILE
    if args.diverse_lambda:
        from .evaluate import diversity_tradeoff
        final = amf if args.model == "apr" else m
        rows = diversity_tradeoff(final, dataset, lams=args.diverse_lambda, k=args.topk, pool=args.diverse_pool,
                                  cutoffs=[args.topk], metric=args.diverse_metric)
        write_diverse(out, runName + ".diverse", rows)
    if args.test_multi is not None:
        from .data import load_test_lists
        from .evaluate import evaluate_multi, init_eval_multi
        final = amf if args.model == "apr" else m
        plan = init_eval_multi(dataset, load_test_lists(args.test_multi))
        write_multi(out, runName + ".multi", evaluate_multi(final, plan, args.cutoffs), args.cutoffs)
    if args.robust_eps:
        from .evaluate import init_eval_model, robustness
        final = amf if args.model == "apr" else m
        trip = getattr(final, "last_train_batches", None)
        if trip is None:
            print("--robust_eps: no epoch was trained, nothing to evaluate on", file=sys.stderr)
        else:
            modes = ("grad", "random", "pgd") if args.robust_iters > 0 else ("grad", "random")
            rows = robustness(final, dataset, init_eval_model(dataset, args), trip, args.robust_eps, modes=modes,
                              seed=args.seed, iters=args.robust_iters or 10, step=args.robust_step)
            write_robust(out, runName + ".robust", rows)
            if args.robust_lists:
                from .evaluate import list_robustness
                rows = list_robustness(final, dataset, trip, args.robust_eps, k=max(args.robust_lists),
                                       cutoffs=args.robust_lists, modes=modes, seed=args.seed,
                                       iters=args.robust_iters or 10, step=args.robust_step)
                write_lists(out, runName + ".lists", rows)
    elif args.robust_lists:
        print("--robust_lists: needs --robust_eps, nothing to evaluate", file=sys.stderr)
    if args.certify_eps:
        from .evaluate import certified, init_eval_model
        final = amf if args.model == "apr" else m
        plan = init_eval_model(dataset, argparse.Namespace(eval_mode="all"))  # certified positions rank all items
        sides = ("user", "item") if args.certify_side == "both" else (args.certify_side,)
        rows = [row for side in sides for row in certified(final, plan, args.certify_eps, side=side)]
        write_certified(out, runName + ".certified", rows)
    if args.certify_radius:
        from .evaluate import certified_radius, init_eval_model, radius_summary
        final = amf if args.model == "apr" else m
        plan = init_eval_model(dataset, argparse.Namespace(eval_mode="all"))  # the radius ranks all items
        sides = ("user", "item") if args.certify_side == "both" else (args.certify_side,)
        rows = []
        for side in sides:  # one sweep per side at K = the largest cutoff serves every smaller one
            eps, _ = certified_radius(final, plan, k=max(args.certify_radius), side=side)
            rows += [(side, *row) for row in radius_summary(eps.cpu().numpy(), args.certify_radius)]
        write_radius(out, runName + ".radius", rows)
    return 0
