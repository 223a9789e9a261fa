#!/usr/bin/env python3
"""
select_bench.py — device time of cstripe_scan_select next to its natural
yardstick: cstripe_scan_agg with a single COUNT_STAR on the SAME staged scan
reads exactly the predicate columns the select mask pass reads.

Generates the bench's lineitem (default 100 M rows, sharded), stages once
with the Q6 predicates, warms both paths, then alternates
agg([COUNT_STAR]) and select(device=True) of l_extendedprice, l_discount
plus row numbers. All figures are hipEvent times on the scan's stream as
the library reports them; the median over the repetitions is reported with
the min/max spread. Prints one JSON line.

  python tools/select_bench.py [--rows N] [--compression lz4|zstd] [--reps K]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def spread(xs):
    return {"median": round(statistics.median(xs), 4),
            "min": round(min(xs), 4), "max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--compression", default="lz4", choices=["lz4", "zstd"])
    ap.add_argument("--shards", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=0,
                    help="timed repetitions (0 = auto: at least 20 and at "
                         "least 2 s of device time)")
    args = ap.parse_args()

    import torch
    torch.cuda.is_available()       # torch's HIP view first (see bench.py)
    import citus_amd as ca
    assert ca.gpu_available(), "select_bench needs a visible MI355X"

    comp = {"lz4": ca.COMP_LZ4, "zstd": ca.COMP_ZSTD}[args.compression]
    default_cache = ("/dev/shm/cstripe_bench" if os.path.isdir("/dev/shm")
                     else "/tmp/cstripe_bench")
    cache = os.environ.get("CSTRIPE_BENCH_DIR", default_cache)
    os.makedirs(cache, exist_ok=True)
    shard = os.path.join(cache, f"li_{args.rows}_{args.compression}_s0_m0_c1"
                                f"_n{args.shards}_r0")
    t0 = time.time()
    if not os.path.exists(os.path.join(shard, f"shard{args.shards - 1:02d}.cs")):
        threads = int(os.environ.get("OMP_NUM_THREADS", "0")) or \
            min(32, os.cpu_count() or 8)
        ca.gen_lineitem_shards(shard, args.rows, args.shards, base_seed=42,
                               compression=comp, threads=max(2, threads))
    gen_s = time.time() - t0

    C = ca.LINEITEM_COLS
    preds = [(5, ca.PRED_GE, 8766), (5, ca.PRED_LT, 9131),
             (3, ca.PRED_GE, 5), (3, ca.PRED_LE, 7), (1, ca.PRED_LT, 2400)]
    out_cols = [C["l_extendedprice"], C["l_discount"]]
    mask = sum(1 << c for c in out_cols)
    cnt = [(ca.AGG_COUNT_STAR, -1)]

    with ca.Reader(shard) as reader, reader.scan(cols_mask=mask, preds=preds) as s:
        t0 = time.time()
        s.stage(0)
        stage_s = time.time() - t0
        for _ in range(args.warmup):
            n_cnt = s.agg(cnt)[0].count
            res = s.select(cols=out_cols, want_nulls=False, device=True)
        assert res["n_rows"] == n_cnt, (res["n_rows"], n_cnt)
        n_rows = res["n_rows"]
        out_bytes = sum(t.numel() * t.element_size()
                        for t in res["values"].values())
        out_bytes += res["row_numbers"].numel() * 8

        keys = ("count_star_kernel_ms", "select_decode_ms", "select_mask_ms",
                "select_offsets_ms", "select_emit_ms", "select_total_ms")
        t = {k: [] for k in keys}
        reps = 0
        dev_ms = 0.0
        while True:
            s.agg(cnt)
            cs_ms = s.last_kernel_ms
            t["count_star_kernel_ms"].append(cs_ms)
            s.select(cols=out_cols, want_nulls=False, device=True)
            p = s.select_profile
            t["select_decode_ms"].append(p["decode_ms"])
            t["select_mask_ms"].append(p["mask_ms"])
            t["select_offsets_ms"].append(p["offsets_ms"])
            t["select_emit_ms"].append(p["emit_ms"])
            t["select_total_ms"].append(p["total_ms"])
            dev_ms += cs_ms + p["total_ms"]
            reps += 1
            if args.reps and reps >= args.reps:
                break
            if not args.reps and reps >= 20 and dev_ms >= 2000.0:
                break
            if reps >= 5000:
                break

    out = {"tool": "select_bench", "rows": args.rows,
           "compression": args.compression, "query": "q6 predicates",
           "reps": reps, "timed_device_ms": round(dev_ms, 1),
           "selected_rows": n_rows, "output_bytes": out_bytes,
           "staged_gen_s": round(gen_s, 1), "stage_s": round(stage_s, 2)}
    for k in keys:
        out[k] = spread(t[k])["median"]
        out[k + "_spread"] = spread(t[k])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
