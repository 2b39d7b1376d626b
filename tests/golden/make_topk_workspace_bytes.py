"""Writes topk_workspace_bytes.json: the four workspace size functions of the exact top-k over a grid of shapes, as the
library at ANIREC_LIB_PATH (or the in-tree build) returns them.  Host code only: no GPU is needed.

The committed file was written from the build of the commit before the select / batch-driver merge; the CPU test
tests/test_width_cpu.py::test_topk_workspace_sizes_keep_their_recorded_values holds every later build to it.

    python tests/golden/make_topk_workspace_bytes.py
"""
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from anime_recommendations_amd import _lib  # noqa: E402

N = (1, 300, 4095, 4096, 17_560, 350_000)
NQ = (1, 5, 1023, 1024, 4096, 100_000)      # n = 350 000 with nq >= 4096: the 4 GiB halving of a batch fires
DIM = (32, 128, 256)


def ks(n):
    return sorted({1, 128, 129, 20_480, 20_481, n})


def main():
    lib = _lib.load()
    out = {"anirec_topk_workspace_bytes": [], "anirec_topk_large_workspace_bytes": [],
           "anirec_predict_workspace_bytes_w": [], "anirec_predict_topk_large_workspace_bytes_w": []}

    def rec(name, *args):
        out[name].append([list(args), int(getattr(lib, name)(*args))])

    for n, nq in itertools.product(N, NQ):
        rec("anirec_topk_workspace_bytes", n, nq)
        for k in ks(n):
            rec("anirec_topk_large_workspace_bytes", n, nq, k)
        for dim in DIM:
            for topk in (0, 1):
                rec("anirec_predict_workspace_bytes_w", n, nq, topk, dim)
            for k in ks(n):
                rec("anirec_predict_topk_large_workspace_bytes_w", n, nq, k, dim)
    # the invalid arguments: every one of them gives 0
    for n, nq in ((0, 5), (-1, 5), (300, 0), (300, -1)):
        rec("anirec_topk_workspace_bytes", n, nq)
        rec("anirec_topk_large_workspace_bytes", n, nq, 10)
        rec("anirec_predict_workspace_bytes_w", n, nq, 1, 128)
        rec("anirec_predict_topk_large_workspace_bytes_w", n, nq, 10, 128)
    for k in (0, -1):
        rec("anirec_topk_large_workspace_bytes", 300, 5, k)
        rec("anirec_predict_topk_large_workspace_bytes_w", 300, 5, k, 128)
    for dim in (0, 48, 100, 512, -128):
        rec("anirec_predict_workspace_bytes_w", 300, 5, 1, dim)
        rec("anirec_predict_topk_large_workspace_bytes_w", 300, 5, 10, dim)
    with open(os.path.join(HERE, "topk_workspace_bytes.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print({k: len(v) for k, v in out.items()})


if __name__ == "__main__":
    main()
