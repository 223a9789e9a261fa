#!/usr/bin/env python3
"""
lookup_bench.py — what a lookup (the device N:1 join with payload columns)
costs on the bench's lineitem: `l_orderkey` -> 1 or 2 payload columns, for map
sizes 10^3 .. 10^6, in both table forms, as host maps and as device maps.

Lookup work happens at stage (cstripe_scan_last_lookup_ms: table build; probe
= bitmap + rank scan + gather); the queries then read the derived column as an
ordinary sparse I64 column. Each case reports the stage split (median of
--stage-reps stages) next to the per-call kernel time (median of --reps calls)
of COUNT(*), SUM(derived) and a hashed GROUP BY on the derived column, whose
values are key % 4901 + 100 — the 4901 values 100..5000 of the generator's
l_quantity (a map smaller than that reaches fewer of them), on which the same
three queries run as the yardstick. Beside them: the set_probe_kernel time of
`l_orderkey NOT IN keys` (a full-table probe of the same key column and size)
and COUNT(*) over the key column alone. l_orderkey is 1..rows/shards in row
order inside every shard file; the keys are drawn from that range, so every
key matches one row per shard. No lookup here is INNER: nothing is pruned and
the probe walks the whole table.

All kernel figures are hipEvent times on the scan's stream as the library
reports them. Prints one JSON line; --out also writes it to a file.

  python tools/lookup_bench.py [--rows N] [--compression lz4|zstd] [--reps K]
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
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--stage-reps", type=int, default=3)
    ap.add_argument("--sizes", default="1000,10000,100000,1000000")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    torch.cuda.is_available()       # torch's HIP view first (see bench.py)
    import citus_amd as ca
    assert ca.gpu_available(), "lookup_bench needs a visible MI355X"

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

    KEY = ca.LINEITEM_COLS["l_orderkey"]
    QTY = ca.LINEITEM_COLS["l_quantity"]
    rng = np.random.default_rng(42)
    os.environ.pop("CSTRIPE_LOOKUP_FORM", None)
    os.environ.pop("CSTRIPE_SET_FORM", None)

    def time_queries(s, col):
        """COUNT(*), SUM(col), hashed GROUP BY col on a staged scan"""
        out = {}
        for name, fn in (("count_star", lambda: s.agg([(ca.AGG_COUNT_STAR, -1)])),
                         ("sum", lambda: s.agg([(ca.AGG_SUM_I64, col)])),
                         ("group_by", lambda: s.agg_hashed(
                             [(ca.AGG_COUNT_STAR, -1), (ca.AGG_SUM_I64, col)], [col], 1 << 16))):
            for _ in range(args.warmup):
                fn()
            ms = []
            for _ in range(max(1, args.reps)):
                res = fn()
                ms.append(s.last_kernel_ms)
            out[name + "_ms"] = spread(ms)
            if name == "count_star":
                out["count"] = res[0].count
            elif name == "sum":
                out["sum"] = res[0].i128
                out["sum_rows"] = res[0].count
            else:
                out["groups"] = int(res["n_groups"])
        return out

    cases = []
    with ca.Reader(shard) as reader:
        # yardsticks: the key column alone, and the table column l_quantity
        with reader.scan(cols_mask=1 << KEY) as s:
            s.stage(0)
            ms = []
            for i in range(args.warmup + max(1, args.reps)):
                s.agg([(ca.AGG_COUNT_STAR, -1)])
                if i >= args.warmup:
                    ms.append(s.last_kernel_ms)
            cases.append({"case": "count_star_key_column_only", "kernel_ms": spread(ms)})
        with reader.scan(cols_mask=(1 << KEY) | (1 << QTY)) as s:
            s.stage(0)
            row = {"case": "table_column_l_quantity"}
            row.update(time_queries(s, QTY))
            cases.append(row)

        per_shard = args.rows // args.shards
        for n_map in [int(x) for x in args.sizes.split(",")]:
            if n_map > per_shard or args.rows % args.shards:
                continue
            keys = rng.choice(per_shard, n_map, replace=False).astype(np.int64) + 1
            p0 = keys % 4901 + 100
            p1 = keys * 3 - 7
            want_rows = n_map * args.shards
            want_sum = int(p0.sum()) * args.shards
            # the value-set probe of the same key column and size, unpruned
            with reader.scan(cols_mask=1 << KEY, preds=[(KEY, ca.PRED_NOT_IN, keys)]) as s:
                b_ms, p_ms = [], []
                for _ in range(args.stage_reps):
                    s.stage(0)
                    b, p = s.last_set_ms()
                    b_ms.append(b)
                    p_ms.append(p)
                form, size = s.set_form(0)
                cases.append({"case": f"set_not_in_{n_map}", "set_form": form, "set_size": size,
                              "set_build_ms": spread(b_ms), "set_probe_ms": spread(p_ms)})
            dk, d0, d1 = (torch.from_numpy(a).to("cuda:0") for a in (keys, p0, p1))
            for where, (kk, q0, q1) in (("host", (keys, p0, p1)), ("device", (dk, d0, d1))):
                for form in ("hash", "direct"):
                    for n_pay in (1, 2):
                        if n_pay == 2 and where == "host":
                            continue        # the upload is outside both timers
                        os.environ["CSTRIPE_LOOKUP_FORM"] = form
                        lk = ca.Lookup(KEY, kk, [q0, q1][:n_pay])
                        with reader.scan(cols_mask=1 << KEY, lookups=[lk]) as s:
                            b_ms, p_ms, st_s = [], [], []
                            for _ in range(args.stage_reps):
                                t0 = time.time()
                                s.stage(0)
                                st_s.append(time.time() - t0)
                                b, p = s.last_lookup_ms()
                                b_ms.append(b)
                                p_ms.append(p)
                            got_form, size = s.lookup_form(0)
                            row = {"case": f"lookup_{n_map}_{where}_{form}_{n_pay}p",
                                   "map_entries": n_map, "map_memory": where,
                                   "payloads": n_pay,
                                   "form": {ca.LOOKUP_FORM_HASH: "hash",
                                            ca.LOOKUP_FORM_DIRECT: "direct"}[got_form],
                                   "form_size": size, "stage_s": spread(st_s),
                                   "build_ms": spread(b_ms), "probe_ms": spread(p_ms),
                                   "agg_path": None}
                            row.update(time_queries(s, s.derived(0, 0)))
                            row["agg_path"] = s.last_agg_path
                            assert row["count"] == args.rows, row
                            assert row["sum_rows"] == want_rows and row["sum"] == want_sum, row
                            cases.append(row)
            os.environ.pop("CSTRIPE_LOOKUP_FORM", None)

    line = json.dumps({"tool": "lookup_bench", "rows": args.rows,
                       "compression": args.compression, "reps": args.reps,
                       "stage_reps": args.stage_reps, "warmup": args.warmup,
                       "gen_s": round(gen_s, 1), "cases": cases})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
