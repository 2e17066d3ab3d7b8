#!/usr/bin/env python3
"""Serving at large K: the union path against the list kernel, the
materialized fallback and the gather + einsum re-score (docs/KERNELS.md
"Top-K above 64: the union path").

Workload: N random items of rank --rank, no filters. For each batch size B:

  list_K     topk_score(K) through the default list kernel, K <= 64
  union_K    topk_score(K, mode="union"): plan (L, S), flagged count, and
             the time as a ratio to list_20 of the same session
  fallback_K _topk_torch_gpu(K) — only with --fallback, and only where the
             B x N fp32 score matrix fits --fallback-bytes
  rescore_K  with --rescore: topk_rescore against Y[idx] + einsum on a
             random [B, 2K] shortlist

Each figure is the median of --repeats device-synchronized runs after
--warmup runs of the same shape. --rehearse runs tiny shapes on the CPU to
check the harness only (the union path needs the GPU, so it times the
reference there); it prints no timings worth quoting.
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
    ap.add_argument("--items", type=int, default=10_000_000)
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--batches", type=int, nargs="+",
                    default=[64, 1024, 4096])
    ap.add_argument("--union-k", type=int, nargs="*",
                    default=[20, 40, 64, 100, 256, 1024])
    ap.add_argument("--list-k", type=int, nargs="*", default=[20, 40, 64])
    ap.add_argument("--fallback", type=int, nargs="*", default=[],
                    metavar="K", help="also time the materialized fallback")
    ap.add_argument("--fallback-bytes", type=int, default=8 << 30)
    ap.add_argument("--rescore", type=int, nargs="*", default=[],
                    metavar="K", help="also time topk_rescore vs einsum")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()

    import torch
    from predictionio_amd.ops import topk as topk_ops

    if args.rehearse:
        dev = torch.device("cpu")
        args.items, args.batches = 5000, [4, 16]
        args.warmup, args.repeats = 1, 2
        args.rescore = []
    else:
        if not torch.cuda.is_available():
            sys.exit("large_k_serve_bench needs a GPU (or --rehearse)")
        dev = torch.device("cuda", 0)
        from predictionio_amd.ops import hip_ext
        ext = hip_ext()  # the native extension must be there

    N, f = args.items, args.rank
    g = torch.Generator().manual_seed(5)
    Y = torch.randn((N, f), generator=g).to(dev)

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

    def put(row, name, t, B):
        med, lo, hi = t
        row[name + "_ms"] = round(med * 1e3, 3)
        row[name + "_min_max_ms"] = [round(lo * 1e3, 3), round(hi * 1e3, 3)]
        row[name + "_qps"] = round(B / med, 1)

    results = []
    for B in args.batches:
        Xq = torch.randn((B, f), generator=g).to(dev)
        row = {"B": B, "N": N, "rank": f}
        for K in args.list_k:
            put(row, f"list_{K}",
                timed(lambda: topk_ops.topk_score(Xq, Y, K)), B)
        base = row.get("list_20_ms")
        for K in args.union_k:
            if args.rehearse:
                put(row, f"union_{K}",
                    timed(lambda: topk_ops.topk_score_ref(Xq, Y, K)), B)
                continue
            pf = topk_ops._mfma_rank(f)
            plan = topk_ops._union_plan(B, N, pf, K, 0)
            if plan is None:
                row[f"union_{K}_plan"] = None
                continue
            before = topk_ops.union_stats()["flagged"]
            put(row, f"union_{K}",
                timed(lambda: topk_ops.topk_score(Xq, Y, K, mode="union")),
                B)
            runs = args.warmup + args.repeats
            row[f"union_{K}_plan"] = list(plan)
            row[f"union_{K}_flagged_per_call"] = (
                topk_ops.union_stats()["flagged"] - before) / runs
            if base:
                row[f"union_{K}_over_list_20"] = round(
                    row[f"union_{K}_ms"] / base, 2)
        for K in args.fallback:
            if B * N * 4 > args.fallback_bytes:
                row[f"fallback_{K}_ms"] = None
                continue
            put(row, f"fallback_{K}",
                timed(lambda: topk_ops._topk_torch_gpu(
                    Xq, Y, K, None, None, None)), B)
        for K in args.rescore:
            C = 2 * K
            idx = torch.randint(0, N, (B, C), generator=g,
                                dtype=torch.int32).to(dev)
            idx64 = idx.long()
            put(row, f"rescore_{K}_kernel",
                timed(lambda: ext.topk_rescore(Xq, Y, idx)), B)
            put(row, f"rescore_{K}_einsum",
                timed(lambda: torch.einsum("bf,bcf->bc", Xq, Y[idx64])), B)
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
