"""Record the workspace byte counts of a built libacf_apr.so over the strip grid."""
import ctypes
import json
import sys

lib = ctypes.CDLL(sys.argv[1])
lib.acf_recommend_topk_workspace.argtypes = [ctypes.c_int32] * 4 + [ctypes.POINTER(ctypes.c_size_t)]
lib.acf_eval_positions_multi_workspace.argtypes = [ctypes.c_int32, ctypes.c_int64, ctypes.c_int32,
                                                   ctypes.POINTER(ctypes.c_size_t)]
USERS = [0, 1, 8, 9, 64, 65, 6040, 55187]
CANDS = [1, 127, 128, 129, 3706, 70000, 5_000_000]
topk, multi = {}, {}
for n in USERS:
    for c in CANDS:
        for k in (1, 100, 128):
            for kernel in (0, 1, 2):
                b = ctypes.c_size_t(0)
                assert lib.acf_recommend_topk_workspace(n, c, k, kernel, ctypes.byref(b)) == 0
                topk[f"{n},{c},{k},{kernel}"] = b.value
        for t in (1, 10 * n):
            b = ctypes.c_size_t(0)
            assert lib.acf_eval_positions_multi_workspace(n, t, c, ctypes.byref(b)) == 0
            multi[f"{n},{t},{c}"] = b.value
doc = {"comment": "workspace bytes returned at commit 49ce069; keys: topk 'n_users,num_cand,k,kernel', "
                  "multi 'n_users,n_tests,num_cand'", "topk": topk, "multi": multi}
with open(sys.argv[2], "w") as f:
    json.dump(doc, f, indent=0, sort_keys=False)
    f.write("\n")
print(len(topk), len(multi))
