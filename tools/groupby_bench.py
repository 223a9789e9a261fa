#!/usr/bin/env python3
"""
groupby_bench.py — device time of cstripe_scan_agg_hashed (hashed GROUP BY)
next to its yardsticks on the SAME staged scan: cstripe_scan_agg with a
single COUNT_STAR (the cost of just walking the rows) and, for the Q1 flag
query, cstripe_scan_agg_grouped.

Generates the bench's lineitem (default 100 M rows, sharded), stages once
per query, warms up, then alternates the calls. Queries, each with the Q1
aggregates:

  GROUP BY (l_discount, l_tax)            99 groups, I64 keys
  GROUP BY l_shipdate                     ~2.5 k groups
  GROUP BY l_orderkey                     one group per row: the scan is cut
                                          by `l_orderkey <= --orderkey-max`
                                          so the groups fit the capacity
  GROUP BY (l_returnflag, l_linestatus)   the Q1 shape, also via agg_grouped

With --sweep the flag and shipdate queries are also run under each
CSTRIPE_HASH_LDS_SLOTS value (the knob is read per call). All figures are
hipEvent times on the scan's stream as the library reports them; medians
over the repetitions with the min/max spread. Prints one JSON line.

  python tools/groupby_bench.py [--rows N] [--compression lz4|zstd]
                                [--reps K] [--sweep 0,16,64,256]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

KNOB = "CSTRIPE_HASH_LDS_SLOTS"


def spread(xs):
    return {"median": round(statistics.median(xs), 4),
            "min": round(min(xs), 4), "max": round(max(xs), 4)}


def med(xs):
    return round(statistics.median(xs), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--compression", default="lz4", choices=["lz4", "zstd"])
    ap.add_argument("--shards", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--orderkey-max", type=int, default=4_000_000,
                    help="GROUP BY l_orderkey scans l_orderkey <= this "
                         "(one group per row; must fit the capacity)")
    ap.add_argument("--sweep", default="",
                    help="comma-separated CSTRIPE_HASH_LDS_SLOTS values")
    args = ap.parse_args()

    import torch
    torch.cuda.is_available()       # torch's HIP view first (see bench.py)
    import citus_amd as ca
    assert ca.gpu_available(), "groupby_bench needs a visible MI355X"

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

    L = ca.LINEITEM_COLS
    q1 = [(ca.AGG_SUM_I64, 1), (ca.AGG_SUM_I64, 2),
          (ca.AGG_SUM_DISC_I64, 2, 3, -1, 100),
          (ca.AGG_SUM_DISC_TAX_I64, 2, 3, 4, 100),
          (ca.AGG_COUNT_STAR, -1)]
    cnt = [(ca.AGG_COUNT_STAR, -1)]
    okmax = min(args.orderkey_max, ca.MAX_HASH_GROUPS)
    queries = [
        ("discount_tax", [L["l_discount"], L["l_tax"]], 128, []),
        ("shipdate", [L["l_shipdate"]], 4096, []),
        ("orderkey", [L["l_orderkey"]], okmax,
         [(L["l_orderkey"], ca.PRED_LE, okmax)]),
        ("flags", [L["l_returnflag"], L["l_linestatus"]], 64, []),
    ]
    sweep = [v for v in args.sweep.split(",") if v != ""]
    os.environ.pop(KNOB, None)

    def timed(s, keys, cap):
        res = s.agg_hashed(q1, keys, cap)
        i_ms, s_ms, c_ms = s.last_hash_ms
        return res, {"decode_ms": s.last_decode_ms, "init_ms": i_ms,
                     "scan_ms": s_ms, "compact_ms": c_ms,
                     "total_ms": s.last_kernel_ms}

    out = {"tool": "groupby_bench", "rows": args.rows,
           "compression": args.compression, "aggs": "q1", "reps": args.reps,
           "gen_s": round(gen_s, 1), "queries": {}}
    for name, keys, cap, preds in queries:
        mask = ca.agg_cols_mask(q1)
        for k in keys:
            mask |= 1 << k
        with ca.Reader(shard) as reader, \
                reader.scan(cols_mask=mask, preds=preds) as s:
            t0 = time.time()
            s.stage(0)
            stage_s = time.time() - t0
            for _ in range(args.warmup):
                n_cnt = s.agg(cnt)[0].count
                res, _p = timed(s, keys, cap)
                if name == "flags":
                    s.agg_grouped(q1, keys)
            assert int(res["partials"]["count"][:, 4].sum()) == n_cnt
            t = {k: [] for k in ("count_star_ms", "decode_ms", "init_ms",
                                 "scan_ms", "compact_ms", "total_ms",
                                 "wall_ms", "grouped_ms")}
            for _ in range(args.reps):
                s.agg(cnt)
                t["count_star_ms"].append(s.last_kernel_ms)
                w0 = time.time()
                _r, p = timed(s, keys, cap)
                t["wall_ms"].append((time.time() - w0) * 1e3)
                for k, v in p.items():
                    t[k].append(v)
                if name == "flags":
                    s.agg_grouped(q1, keys)
                    t["grouped_ms"].append(s.last_kernel_ms)
            q = {"key_cols": keys, "capacity": cap, "rows_scanned": n_cnt,
                 "n_groups": int(res["n_groups"]), "stage_s": round(stage_s, 2)}
            for k, xs in t.items():
                if xs:
                    q[k] = med(xs)
                    q[k + "_spread"] = spread(xs)
            q["ratio_to_count_star"] = round(q["total_ms"] / q["count_star_ms"], 2)
            if name == "flags":
                q["ratio_to_agg_grouped"] = round(q["total_ms"] / q["grouped_ms"], 2)
            if sweep and name in ("flags", "shipdate", "discount_tax"):
                sw = {}
                for v in sweep:
                    os.environ[KNOB] = v
                    timed(s, keys, cap)
                    xs = [timed(s, keys, cap)[1]["scan_ms"]
                          for _ in range(max(3, args.reps // 2))]
                    sw[v] = spread(xs)
                os.environ.pop(KNOB, None)
                q["lds_slots_sweep_scan_ms"] = sw
            out["queries"][name] = q
    print(json.dumps(out))


if __name__ == "__main__":
    main()
