"""Bit-compare two builds of libacf_neumf.so on its three engines, small tables
(300 x 200 rows).  Per d (default 4 12 32 64 132 256, every lane-group width of
the Keras BPR / FastAdversarialMF kernels): a Keras BPR epoch of three batches, the
last one partial; acf_amf_train over three batches; one acf_amf_grad; both
predicts on 50 pairs.  Then adversarial NeuMF, d = 8 and 64, three grad + adam
steps and a fourth gradient at batch 64 (rows in line) and 1,100 (row-sum path),
and a predict.  One JSON
line per case with the sha256 of params, grad, m, v, losses and scores.
ACF_ALT_LIB=path loads that build in place of the package's (as
tools/bitcmp_lib.py).  Run it once per build and compare the digests.
usage: python3 tools/bitcmp_neumf.py [d ...]"""
import ctypes
import hashlib
import importlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402

nat = importlib.import_module(bench.PKG + "._native")
alt = os.environ.get("ACF_ALT_LIB")
if alt:
    lib = ctypes.CDLL(alt)
    for fname, (res, args) in nat.NEUMF_SIGNATURES.items():
        fn = getattr(lib, fname)
        fn.restype, fn.argtypes = res, args
    nat._neumf = lib
KB = importlib.import_module(bench.PKG + ".keras_bpr")
FM = importlib.import_module(bench.PKG + ".fast_adversarial_mf")
NM = importlib.import_module(bench.PKG + ".neumf")
dev = torch.device("cuda", 0)
U1, I1, B, n = 300, 200, 64, 160


def digests(**tensors):
    return {k: hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest() for k, t in tensors.items()}


def report(case, d, **tensors):
    print(json.dumps({"case": case, "d": d, "lib": alt or "package", **digests(**tensors)}), flush=True)


def T(a):
    return torch.as_tensor(a).to(dev).contiguous()


for d in [int(x) for x in sys.argv[1:]] or [4, 12, 32, 64, 132, 256]:
    rng = np.random.default_rng(d)
    u = rng.integers(0, U1, n).astype(np.int32)
    i = ((rng.zipf(1.3, n) - 1) % I1).astype(np.int32)  # hot items: many occurrences per batch
    j = rng.integers(0, I1, n).astype(np.int32)
    r = KB.BPR(U1, I1, d, seed=3, device=dev)
    r._rng = np.random.RandomState(5)
    loss = r.train([u, i, j], np.ones(n), B)
    report("kbpr", d, params=r.params, grad=r.grad, m=r.m, v=r.v, losses=torch.tensor([loss], dtype=torch.float64),
           scores=torch.as_tensor(r.rank(u[:50], i[:50])))

    a = FM.FastAdversarialMF(U1, I1, d, seed=2, device=dev)
    ua = rng.integers(0, U1, n).astype(np.int32)
    ua[::5] = u[::5]  # rows gathered by both the MSE and the discriminator
    ia = rng.integers(0, I1, n).astype(np.int32)
    y, tu, ti = (rng.integers(0, 2, n).astype(np.float32) for _ in range(3))
    inst = [T(x) for x in (u, i, y, ua, ia, tu, ti, 1 - tu, 1 - ti)]
    losses = torch.empty(n, 3, device=dev)
    nat.call_neumf("acf_amf_train", a._context(B), a.params.data_ptr(), a.grad.data_ptr(), a.m.data_ptr(),
                   a.v.data_ptr(), *[t.data_ptr() for t in inst], n, B, 1, ctypes.byref(a.hp), losses.data_ptr(),
                   torch.cuda.current_stream().cuda_stream)
    gl = a.grad_batch(*[t[:37].contiguous() for t in inst])
    report("amf", d, params=a.params, grad=a.grad, m=a.m, v=a.v, losses=torch.cat([losses, gl]),
           scores=torch.as_tensor(a.rank(u[:50], i[:50])))

for d in (8, 64):
    for batch in (64, 1100):  # FR_MAXB = 1,024 lies between
        rng = np.random.default_rng(1000 * d + batch)
        st = NM.NeuMFState(U1, I1, d, dev)
        st.keras_init(seed=7)
        ctx = NM.NeuMFContext(st, batch)
        hp = ctx.hparams(adver=1)
        loss = torch.zeros(4, 2, device=dev)
        for k in range(4):  # the fourth gradient stays in grad
            u = rng.integers(0, U1, batch).astype(np.int32)
            i = ((rng.zipf(1.3, batch) - 1) % I1).astype(np.int32)
            ctx.grad(u, i, rng.integers(0, 2, batch).astype(np.float32), hp, loss_out=loss[k])
            if k < 3:
                ctx.adam(hp)
        torch.cuda.synchronize()
        print(json.dumps({"case": "neumf", "d": d, "batch": batch, "lib": alt or "package",
                          "recoveries": ctx.recoveries(),
                          **digests(params=st.params, grad=st.grad, m=st.m, v=st.v, losses=loss,
                                    scores=ctx.predict(u[:50], i[:50]))}), flush=True)
