#!/usr/bin/env python3
"""Whitelist serving: N-byte masks vs the candidate-list kernel
(docs/KERNELS.md "Candidate-list top-K").

Workload: N items of rank 64, K=20, every query ranks its own random
whitelist of L items. For each (L, B):

  (a) per_query_mask  B sequential topk_score(B=1, item_mask=ones with
                      L zeros) calls, mask construction included — what
                      predict() did for a whiteList query, and
                      batch_predict once per such query
  (b) cand_list       ONE topk_score(B, cand_indptr=, cand_indices=) call

Each figure is the median of --repeats device-synchronized runs after
--warmup runs of the same shape; the two paths alternate in one process.
(a) is timed with a single synchronize at the end of its B calls, which
favours it. --max-mask-calls caps the B of (a): above it (a) runs that
many queries and the figure is scaled to B (marked "scaled" in the row).
--rehearse runs tiny shapes on the CPU to check the harness only.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--lists", type=int, nargs="+", default=[100, 10_000])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--max-mask-calls", type=int, default=1024)
    ap.add_argument("--seg-len", type=int, default=None)
    ap.add_argument("--wave-max", type=int, default=None)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch
    from predictionio_amd.ops import topk as topk_ops

    if args.rehearse:
        dev = torch.device("cpu")
        args.items, args.lists, args.batches = 5000, [10, 100], [1, 4]
        args.warmup, args.repeats = 1, 2
    else:
        if not torch.cuda.is_available():
            sys.exit("whitelist_serve_bench needs a GPU (or --rehearse)")
        dev = torch.device("cuda", 0)
        from predictionio_amd.ops import hip_ext
        hip_ext()  # the native extension must be there

    N, f, K = args.items, args.rank, args.k
    g = torch.Generator().manual_seed(5)
    rng = np.random.default_rng(5)
    Y = torch.randn((N, f), generator=g).to(dev)
    tiers = {}
    if args.seg_len is not None:
        tiers["seg_len"] = args.seg_len
    if args.wave_max is not None:
        tiers["wave_max"] = args.wave_max

    def sync():
        if dev.type == "cuda":
            torch.cuda.synchronize()

    def once(fn):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return time.perf_counter() - t0

    results = []
    for L in args.lists:
        for B in args.batches:
            Xq = torch.randn((B, f), generator=g).to(dev)
            lists = [np.sort(rng.choice(N, L, replace=False)).astype(np.int32)
                     for _ in range(B)]
            ip = torch.arange(B + 1, dtype=torch.int64, device=dev) * L
            ci = torch.from_numpy(np.concatenate(lists)).to(dev)
            ids = ci.long().view(B, L)
            Ba = min(B, args.max_mask_calls)

            def per_query_mask():
                out = []
                for b in range(Ba):
                    m = torch.ones(N, dtype=torch.uint8, device=dev)
                    m[ids[b]] = 0
                    out.append(topk_ops.topk_score(Xq[b:b + 1], Y, K,
                                                   item_mask=m))
                return out

            def cand_list():
                if tiers and dev.type == "cuda":
                    return topk_ops._topk_score_cands(Xq, Y, K, ip, ci,
                                                      **tiers)
                return topk_ops.topk_score(Xq, Y, K, cand_indptr=ip,
                                           cand_indices=ci)

            # the two paths must agree before their times mean much
            cv, cidx = cand_list()
            ref = per_query_mask()
            for b in range(min(Ba, 16)):
                assert torch.allclose(cv[b], ref[b][0][0], atol=1e-4,
                                      rtol=1e-4), f"query {b} differs"
                assert torch.equal(cidx[b].sort().values,
                                   ref[b][1][0].sort().values), f"query {b}"
            for _ in range(args.warmup):
                per_query_mask()
                cand_list()
            ta, tb = [], []
            for _ in range(args.repeats):      # alternate the two paths
                ta.append(once(per_query_mask) * (B / Ba))
                tb.append(once(cand_list))
            row = {"N": N, "rank": f, "K": K, "list": L, "B": B,
                   "per_query_mask_ms": round(statistics.median(ta) * 1e3, 3),
                   "per_query_mask_min_max_ms": [round(min(ta) * 1e3, 3),
                                                 round(max(ta) * 1e3, 3)],
                   "cand_list_ms": round(statistics.median(tb) * 1e3, 3),
                   "cand_list_min_max_ms": [round(min(tb) * 1e3, 3),
                                            round(max(tb) * 1e3, 3)],
                   "scaled": Ba < B, **tiers}
            row["speedup"] = round(row["per_query_mask_ms"]
                                   / row["cand_list_ms"], 2)
            print(json.dumps(row), flush=True)
            results.append(row)

    if args.rehearse:
        print("rehearsal on the CPU: harness check only, not a measurement")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)),
                    exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"device": str(dev), "results": results}, fh,
                      indent=1)


if __name__ == "__main__":
    main()
