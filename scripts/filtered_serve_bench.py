#!/usr/bin/env python3
"""Category-filtered serving: per-query masks vs the fused per-query
category filter (docs/KERNELS.md "Per-query category filters").

Workload: N items of rank 64, K=20, 31 categories with ~2 per item, every
query filters on ONE category (~6% selectivity). For each batch size B:

  (a) per_query_mask  B sequential topk_score(B=1, item_mask=
                      CategoryMasks.banned_outside([c])) calls, mask
                      construction included — what batch_predict did for
                      the filter-carrying templates before the fused filter
  (b) fused_cats      ONE topk_score(B, item_cats=, query_cats=) call
  (c) unfiltered      the same batch without any filter: the floor that
                      shows what the filter itself costs

Each figure is the median of --repeats device-synchronized runs after
--warmup runs of the same shape. (a) is timed with a single synchronize
at the end of the B calls, which favours it (the template path also
copies every result to the host). --rehearse runs tiny shapes on the CPU
to check the harness only; it prints no timings worth quoting.
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
    ap.add_argument("--cats", type=int, default=31)
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch
    from predictionio_amd.ops import topk as topk_ops
    from predictionio_amd.templates.common import CategoryMasks

    if args.rehearse:
        dev = torch.device("cpu")
        args.items, args.batches = 5000, [4, 16]
        args.warmup, args.repeats = 1, 2
    else:
        if not torch.cuda.is_available():
            sys.exit("filtered_serve_bench needs a GPU (or --rehearse)")
        dev = torch.device("cuda", 0)
        from predictionio_amd.ops import hip_ext
        hip_ext()  # the native extension must be there

    N, f, K, ncat = args.items, args.rank, args.k, args.cats
    assert ncat <= 31, "one 32-bit word: ANY bit + 31 categories"
    g = torch.Generator().manual_seed(5)
    rng = np.random.default_rng(5)
    Y = torch.randn((N, f), generator=g).to(dev)
    # ~2 categories per item (two draws, may coincide); bit 0 = ANY
    c1 = rng.integers(0, ncat, N)
    c2 = rng.integers(0, ncat, N)
    words = (np.uint32(1) | (np.uint32(1) << (c1 + 1).astype(np.uint32))
             | (np.uint32(1) << (c2 + 1).astype(np.uint32)))
    item_cats = torch.from_numpy(
        words.astype(np.uint32).view(np.int32).reshape(N, 1)).to(dev)
    member = {}
    for c in range(ncat):
        member[f"c{c}"] = torch.from_numpy(
            ((c1 == c) | (c2 == c)).astype(np.uint8)).to(dev)
    masks = CategoryMasks(member, N, dev)

    def sync():
        if dev.type == "cuda":
            torch.cuda.synchronize()

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        sync()
        ts = []
        for _ in range(args.repeats):
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts), min(ts), max(ts)

    results = []
    for B in args.batches:
        Xq = torch.randn((B, f), generator=g).to(dev)
        qcat = rng.integers(0, ncat, B)
        query_cats = torch.from_numpy(
            (np.uint32(1) << (qcat + 1).astype(np.uint32))
            .astype(np.uint32).view(np.int32).reshape(B, 1)).to(dev)

        def per_query_mask():
            out = []
            for b in range(B):
                m = masks.banned_outside([f"c{qcat[b]}"])
                out.append(topk_ops.topk_score(Xq[b:b + 1], Y, K,
                                               item_mask=m))
            return out

        def fused_cats():
            return topk_ops.topk_score(Xq, Y, K, item_cats=item_cats,
                                       query_cats=query_cats)

        def unfiltered():
            return topk_ops.topk_score(Xq, Y, K)

        # the two filtered paths must agree before their times mean much
        fv, fi = fused_cats()
        ref = per_query_mask()
        for b in range(min(B, 16)):
            assert torch.allclose(fv[b], ref[b][0][0], atol=1e-4,
                                  rtol=1e-4), f"query {b} differs"
            assert torch.equal(fi[b].sort().values,
                               ref[b][1][0].sort().values), f"query {b}"
        sel = float(np.mean([(member[f"c{c}"].sum().item()) / N
                             for c in set(qcat.tolist())]))

        row = {"B": B, "N": N, "rank": f, "K": K,
               "selectivity": round(sel, 4)}
        for name, fn in (("per_query_mask", per_query_mask),
                         ("fused_cats", fused_cats),
                         ("unfiltered", unfiltered)):
            med, lo, hi = timed(fn)
            row[name + "_ms"] = round(med * 1e3, 3)
            row[name + "_min_max_ms"] = [round(lo * 1e3, 3),
                                         round(hi * 1e3, 3)]
            row[name + "_qps"] = round(B / med, 1)
        row["speedup_fused_vs_per_query"] = round(
            row["per_query_mask_ms"] / row["fused_cats_ms"], 2)
        row["fused_over_unfiltered"] = round(
            row["fused_cats_ms"] / row["unfiltered_ms"], 3)
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
