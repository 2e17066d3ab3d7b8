#!/usr/bin/env python3
"""Held-out ranking evaluation: the fused kernels vs the blocked torch
route (docs/KERNELS.md "Held-out ranks").

Workload: N items of rank f, B users with `--seen` training items and
`--heldout` held-out items each, gaussian factors. For each B:

  (a) kernel  ONE heldout_ranks call (csrc/rank_count.hip), validation,
              slot building and the final integer arithmetic included
  (b) torch   ONE heldout_ranks_ref call on the same device (fp32 GEMM in
              blocks of --block-elems scores, masks, compares)

(a) and (b) are the median of --repeats device-synchronized runs after
--warmup runs of the same shape, alternating in one process. The two
routes sum in different orders, so on float data a few ranks may differ by
a near-tie: the share of pairs that differ and the largest difference are
reported, not asserted (the tests hold the kernels to exact counts).

The stream kernel alone is also timed with device events; its share of
the fp32-MFMA peak is the MFMA work it issues (2 f flops per slot and
item, padding slots and tail rows included) over 64 flop / clk / SIMD x 4
SIMDs x CUs x --clock-mhz (2400, the MI355X peak engine clock).
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
    ap.add_argument("--seen", type=int, default=20)
    ap.add_argument("--heldout", type=int, default=2)
    ap.add_argument("--batches", type=int, nargs="+", default=[1024, 16384])
    ap.add_argument("--block-elems", type=int, default=1 << 28)
    ap.add_argument("--clock-mhz", type=float, default=2400.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()

    import torch
    from predictionio_amd.ops import ranking

    if args.rehearse:
        dev = torch.device("cpu")
        args.items, args.batches = 3000, [4, 16]
        args.warmup, args.repeats = 1, 2
    else:
        if not torch.cuda.is_available():
            sys.exit("heldout_eval_bench needs a GPU (or --rehearse)")
        dev = torch.device("cuda", 0)
        from predictionio_amd.ops import hip_ext
        ext = hip_ext()  # the native extension must be there

    N, f, ns, nt = args.items, args.rank, args.seen, args.heldout
    g = torch.Generator().manual_seed(11)
    Y = torch.randn((N, f), generator=g).to(dev)

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
    for B in args.batches:
        X = torch.randn((B, f), generator=g).to(dev)
        # sorted draws plus 0..m-1: strictly ascending ids below N; the
        # first nt of a shuffled row are held out, the rest seen
        m = ns + nt
        ids = torch.randint(0, N - m, (B, m), generator=g).sort(1).values
        ids = ids + torch.arange(m)
        pick = torch.rand((B, m), generator=g).argsort(1)
        test = ids.gather(1, pick[:, :nt]).sort(1).values
        seen = ids.gather(1, pick[:, nt:]).sort(1).values
        tp = (torch.arange(B + 1, dtype=torch.int64) * nt).to(dev)
        sp = (torch.arange(B + 1, dtype=torch.int64) * ns).to(dev)
        ti = test.reshape(-1).to(torch.int32).to(dev)
        si = seen.reshape(-1).to(torch.int32).to(dev)

        def kernel():
            return ranking.heldout_ranks(X, Y, tp, ti, sp, si)

        def torch_route():
            return ranking.heldout_ranks_ref(X, Y, tp, ti, sp, si,
                                             block_elems=args.block_elems)

        a, b = kernel(), torch_route()
        diff = (a[0] - b[0]).abs()
        assert torch.equal(a[2], b[2])
        for _ in range(args.warmup):
            kernel()
            torch_route()
        ta, tb = [], []
        for _ in range(args.repeats):      # alternate the two routes
            ta.append(once(kernel))
            tb.append(once(torch_route))
        row = {"N": N, "f": f, "seen": ns, "heldout": nt, "B": B,
               "kernel_ms": round(statistics.median(ta) * 1e3, 3),
               "kernel_min_max_ms": [round(min(ta) * 1e3, 3),
                                     round(max(ta) * 1e3, 3)],
               "torch_ms": round(statistics.median(tb) * 1e3, 3),
               "torch_min_max_ms": [round(min(tb) * 1e3, 3),
                                    round(max(tb) * 1e3, 3)],
               "gt_differs_share": round(float((diff > 0).double().mean()), 6),
               "gt_max_diff": int(diff.max())}
        row["speedup"] = round(row["torch_ms"] / row["kernel_ms"], 2)
        mpr = [ranking.ranking_metrics(*r, tp)["mpr"] for r in (a, b)]
        row["mpr_kernel_torch"] = [round(v, 9) for v in mpr]

        if dev.type == "cuda":
            # the stream kernel alone, at the wrapper's own launch shape
            from predictionio_amd.ops.als import pad_rank
            pf = pad_rank(f)
            Xp, Yp, _ = ranking._pad_factors(X, Y)
            group = ext.rank_count_group()
            su, st, _ = ranking._build_slots(tp, ti, ext.rank_count_tmax(),
                                             group)
            n_sl = ranking.default_slices(su.numel() // group, N, pf,
                                          ext.rank_stream_lds_bytes(pf))
            tscore, _ = ext.rank_list(Xp, Yp, su, st, sp, si)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ts = []
            for _ in range(args.warmup + args.repeats):
                ev[0].record()
                ext.rank_stream(Xp, Yp, su, tscore, n_sl, True)
                ev[1].record()
                torch.cuda.synchronize()
                ts.append(ev[0].elapsed_time(ev[1]))
            t_ms = statistics.median(ts[args.warmup:])
            n_cu = torch.cuda.get_device_properties(0).multi_processor_count
            peak = 64 * 4 * n_cu * args.clock_mhz * 1e6
            flops = 2.0 * pf * su.numel() * (-(-N // 64) * 64)
            row.update(stream_ms=round(t_ms, 3), n_slices=n_sl,
                       slots=su.numel(),
                       stream_tflops=round(flops / t_ms / 1e9, 2),
                       mfma_peak_tflops=round(peak / 1e12, 1),
                       mfma_share=round(flops / (t_ms * 1e-3) / peak, 3))
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
