"""Bit-compare two builds of libacf_apr.so on the certified evaluations, which
share one margin sweep (k_cert_sweep): ops.eval_positions_worst with 1, 4 and 8
eps and ops.eval_radius with k = 1, 10 and 128, on both sides, each with
exclusion lists and with none, at test sizes (sigma = 0.1 tables, the test
items' rows moved so that they rank near the top and the radii are not all 0):

  d          4, 8, 64, 100, 512, 516, 1024 x 1, 7, 8, 9, 13 entries, 300 candidates
             (d = 512 is the last size with a tile of 8 entries, 516 the first with 4)
  num_cand   1, 255, 256, 257, 2049, 2053 at d = 8 and d = 516, 9 entries: the edges
             of the 256-candidate window and of the 2,048-candidate bitmap
  strips     70,000 candidates, 3 entries, d = 8: several strips
  denormal   tables scaled by 1e-20 at d = 4: evr_min_eps ends in its bisection

One JSON line per case: sha256 of every output.  ACF_ALT_LIB=path loads that
build in place of the package's (tools/alt_lib.py).  Run it once per
build, then
  python3 tools/bitcmp_certified.py --compare a.jsonl b.jsonl out.json
writes the per-case equality."""
import hashlib
import importlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def compare(a, b, out):
    ra, rb = ([json.loads(x) for x in open(p) if x.startswith("{")] for p in (a, b))
    cases = []
    for x, y in zip(ra, rb):
        keys = [k for k in x if k != "lib"]
        cases.append({"case": x["case"], "equal": all(x[k] == y.get(k) for k in keys),
                      "differs": [k for k in keys if x[k] != y.get(k)]})
    res = {"parent": ra[0]["lib"], "change": rb[0]["lib"], "n_cases": [len(ra), len(rb)],
           "digests_per_case": len(ra[0]) - 2,
           "all_equal": len(ra) == len(rb) and all(c["equal"] for c in cases), "cases": cases}
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps({"all_equal": res["all_equal"], "cases": len(cases)}))
    return 0 if res["all_equal"] else 1


if len(sys.argv) > 1 and sys.argv[1] == "--compare":
    sys.exit(compare(*sys.argv[2:5]))

import torch  # noqa: E402

import bench  # noqa: E402
from tools.alt_lib import use_alt_lib  # noqa: E402

ops = importlib.import_module(bench.PKG + ".ops")
alt = use_alt_lib(bench.PKG)
dev = torch.device("cuda", 0)
EPS = {1: (0.05,), 4: (0.0, 0.02, 0.05, 0.1), 8: (0.0, 0.005, 0.01, 0.025, 0.05, 0.1, 0.2, 0.4)}
KS = (1, 10, 128)


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()


def case(name, d, n, num_cand, scale=1.0):
    rng = np.random.default_rng([d, n, num_cand])
    U1, I1 = n + 3, num_cand + 3
    P = 0.1 * rng.standard_normal((U1, d))
    Q = 0.1 * rng.standard_normal((I1, d))
    users = rng.permutation(U1)[:n].astype(np.int32)
    tests = rng.integers(0, num_cand, n).astype(np.int32)
    tests[0] = num_cand - 1
    for r, (u, t) in enumerate(zip(users, tests)):  # t scores like the (r mod 7)-th best candidate
        s = Q[:num_cand] @ P[u]
        Q[t] += (np.sort(s)[::-1][min(r % 7, num_cand - 1)] - s[t]) * P[u] / (P[u] @ P[u])
    lists = [np.concatenate([rng.integers(0, num_cand, 12), [-1, num_cand, num_cand - 1]]) for _ in users]
    if n > 2:  # an item row outside the range, nothing inside excluded: every candidate counts for entry 2
        tests[2], lists[2] = num_cand + 1, np.array([-1, num_cand + 1])
    off = np.zeros(n + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    tP = torch.tensor((scale * P).astype(np.float32), device=dev)
    tQ = torch.tensor((scale * Q).astype(np.float32), device=dev)
    out = {}
    for side in ("user", "item"):
        for tag, excl in (("excl", (off, np.concatenate(lists).astype(np.int32))), ("none", (None, None))):
            for ne, eps in EPS.items():
                out[f"worst_{side}_{tag}_{ne}"] = sha(ops.eval_positions_worst(
                    tP, tQ, users, tests, num_cand, *excl, eps=tuple(scale * e for e in eps), side=side))
            for k in KS:
                out[f"radius_{side}_{tag}_{k}"] = sha(*ops.eval_radius(tP, tQ, users, tests, num_cand, *excl, k=k,
                                                                       side=side))
    print(json.dumps({"case": name, "lib": alt or "package", **out}), flush=True)


for d in (4, 8, 64, 100, 512, 516, 1024):
    for n in (1, 7, 8, 9, 13):
        case(f"d{d}_n{n}", d, n, 300)
for d in (8, 516):
    for num_cand in (1, 255, 256, 257, 2049, 2053):
        case(f"cand{num_cand}_d{d}", d, 9, num_cand)
case("strips_70000", 8, 3, 70000)
case("denormal_d4", 4, 3, 1500, scale=1e-20)
