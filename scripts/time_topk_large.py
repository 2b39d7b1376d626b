"""Latency of the any-k exact top-k (anirec_cosine_topk_large / anirec_predict_topk_large_act), each shape timed
interleaved with the existing kernels' k = 128 call of the same shape (anirec_cosine_topk / anirec_predict_topk_act;
k = 10 for the batched predict) in one process.
Workspaces are allocated once outside the timed loop; times are wall clock over `reps` calls after a warm-up.
Prints one JSON line per shape; `--out FILE` also writes them as a JSON list."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from anime_recommendations_amd import _lib, ops

HEAD = dict(w=4.0, b=0.0, gamma=1.1, beta=0.2, mov_mean=0.1, mov_var=0.3)


def _cosine_call(lib, Wh, q, k, large=True):
    n, nq = Wh.shape[0], q.numel()
    nb = lib.anirec_topk_large_workspace_bytes(n, nq, k) if large else lib.anirec_topk_workspace_bytes(n, nq)
    ws = torch.empty(int(nb), dtype=torch.uint8, device=Wh.device)
    oi = torch.empty(nq, k, dtype=torch.int32, device=Wh.device)
    os_ = torch.empty(nq, k, dtype=torch.float32, device=Wh.device)
    fn = lib.anirec_cosine_topk_large if large else lib.anirec_cosine_topk
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return lambda: _lib.check(fn(_lib.ptr(Wh), n, _lib.ptr(q), nq, None, 1, k, _lib.ptr(oi), _lib.ptr(os_),
                                 _lib.ptr(ws), ws.numel(), s), "cosine")


def _predict_call(lib, U, A, users, k, large=True):
    n_a, nq = A.shape[0], users.numel()
    nb = (lib.anirec_predict_topk_large_workspace_bytes(n_a, nq, k) if large
          else lib.anirec_predict_workspace_bytes(n_a, nq, 1))
    ws = torch.empty(int(nb), dtype=torch.uint8, device=U.device)
    oi = torch.empty(nq, k, dtype=torch.int32, device=U.device)
    op = torch.empty(nq, k, dtype=torch.float32, device=U.device)
    fn = lib.anirec_predict_topk_large_act if large else lib.anirec_predict_topk_act
    h = ops._head_struct(HEAD)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return lambda: _lib.check(fn(_lib.ptr(U), _lib.ptr(A), n_a, _lib.ptr(users), nq, C.byref(h), 0, None, k,
                                 _lib.ptr(oi), _lib.ptr(op), _lib.ptr(ws), ws.numel(), s), "predict")


def _interleaved(f_new, f_ref, reps, warm):
    for _ in range(warm):
        f_new()
        f_ref()
    torch.cuda.synchronize()
    t_new = t_ref = 0.0
    for _ in range(reps):
        t0 = time.perf_counter()
        f_new()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        f_ref()
        torch.cuda.synchronize()
        t_ref += time.perf_counter() - t1
        t_new += t1 - t0
    return t_new / reps * 1e3, t_ref / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-batched", action="store_true")
    a = ap.parse_args()
    lib = _lib.load()
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    rows = []

    def report(shape, k, ms, ms_ref, reps, ref_k=128):
        r = dict(shape=shape, k=k, ms=round(ms, 4), ref_k=ref_k, ms_ref=round(ms_ref, 4), ratio=round(ms / ms_ref, 3),
                 reps=reps)
        rows.append(r)
        print(json.dumps(r), flush=True)

    Wh = ops.rownorm(torch.randn(350_000, 128, generator=g, device="cuda"))
    q = torch.tensor([12345], dtype=torch.int32, device="cuda")
    ref = _cosine_call(lib, Wh, q, 128, large=False)
    for k in (128, 1000, 10_000, 50_000, 350_000):
        report("cosine 1 x 350000", k, *_interleaved(_cosine_call(lib, Wh, q, k), ref, a.reps, a.warmup), a.reps)
    del Wh
    U = torch.randn(100_000, 128, generator=g, device="cuda")
    A = torch.randn(17_560, 128, generator=g, device="cuda")
    one = torch.tensor([777], dtype=torch.int32, device="cuda")
    report("predict 1 x 17560", 17_560, *_interleaved(_predict_call(lib, U, A, one, 17_560),
                                                      _predict_call(lib, U, A, one, 128, False), a.reps, a.warmup), a.reps)
    if not a.skip_batched:
        users = torch.arange(100_000, dtype=torch.int32, device="cuda")
        r = max(2, a.reps // 5)
        report("predict 100000 x 17560", 1000, *_interleaved(_predict_call(lib, U, A, users, 1000),
                                                             _predict_call(lib, U, A, users, 10, False), r, 1), r, ref_k=10)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
