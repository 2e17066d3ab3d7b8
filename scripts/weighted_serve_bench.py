#!/usr/bin/env python3
"""Weighted serving: what per-item score weights cost inside the fused
top-K (docs/KERNELS.md "Per-item score weights").

Workload: N items of rank 64, K=20, one [N] weight vector drawn from
{0.25, 0.5, 1, 2, 8} with a few zero and negative entries. For each batch
size B:

  (a) weighted     ONE topk_score(B, item_weights=) call
  (b) unweighted   the same call without weights: the floor that shows
                   what the weights themselves cost

Each figure is the median of --repeats device-synchronized runs after
--warmup runs of the same shape. --unweighted-only skips (a), so the
script also runs against a build that predates item_weights (the
unweighted path before / after comparison). --rehearse runs tiny shapes
on the CPU to check the harness only; it prints no timings worth quoting.
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
    ap.add_argument("--batches", type=int, nargs="+",
                    default=[1, 64, 1024, 4096])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--mode", default=None, help="topk_score mode")
    ap.add_argument("--unweighted-only", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()

    import torch
    from predictionio_amd.ops import topk as topk_ops

    if args.rehearse:
        dev = torch.device("cpu")
        args.items, args.batches = 5000, [4, 16]
        args.warmup, args.repeats = 1, 2
    else:
        if not torch.cuda.is_available():
            sys.exit("weighted_serve_bench needs a GPU (or --rehearse)")
        dev = torch.device("cuda", 0)
        from predictionio_amd.ops import hip_ext
        hip_ext()  # the native extension must be there

    N, f, K = args.items, args.rank, args.k
    g = torch.Generator().manual_seed(5)
    Y = torch.randn((N, f), generator=g).to(dev)
    wset = torch.tensor([0.25, 0.5, 1.0, 1.0, 1.0, 2.0, 8.0, 0.0, -1.0])
    weights = wset[torch.randint(0, len(wset), (N,), generator=g)].to(dev)

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

        def weighted():
            return topk_ops.topk_score(Xq, Y, K, mode=args.mode,
                                       item_weights=weights)

        def unweighted():
            return topk_ops.topk_score(Xq, Y, K, mode=args.mode)

        paths = [("unweighted", unweighted)]
        if not args.unweighted_only:
            # the weighted call must be right before its time means much
            wv, wi = weighted()
            rv, ri = topk_ops.topk_score_ref(
                Xq[:8].cpu(), Y.cpu(), K, item_weights=weights.cpu())
            assert torch.allclose(wv[:8].cpu(), rv, atol=1e-3, rtol=1e-4)
            paths.insert(0, ("weighted", weighted))

        row = {"B": B, "N": N, "rank": f, "K": K, "mode": args.mode}
        for name, fn in paths:
            med, lo, hi = timed(fn)
            row[name + "_ms"] = round(med * 1e3, 3)
            row[name + "_min_max_ms"] = [round(lo * 1e3, 3),
                                         round(hi * 1e3, 3)]
            row[name + "_qps"] = round(B / med, 1)
        if not args.unweighted_only:
            row["weighted_over_unweighted"] = round(
                row["weighted_ms"] / row["unweighted_ms"], 3)
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
