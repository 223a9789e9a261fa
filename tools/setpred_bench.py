#!/usr/bin/env python3
"""
setpred_bench.py — what a set-membership predicate costs: COUNT(*) under
`l_orderkey IN S` (and NOT IN S) on the bench's lineitem, for |S| = 10, 10^3
and 10^6, as host sets and as device sets, in both table forms where legal.

Set work happens at stage (cstripe_scan_last_set_ms: table build, membership
probe); the query then reads a one-byte membership column. So each case
reports the stage split next to the per-call kernel time, and beside them the
yardsticks: COUNT(*) with no predicate, and for |S| = 10 the same list as an
OR group of EQ atoms. l_orderkey is 1..rows/shards in row order inside every
shard file, so S is drawn from that range, every element matches one row per
shard, and IN prunes every chunk group that holds no element
(`chunk_groups_filtered`); NOT IN never prunes and shows the full-table probe.

All kernel figures are hipEvent times on the scan's stream as the library
reports them, medians over --reps calls. Prints one JSON line.

  python tools/setpred_bench.py [--rows N] [--compression lz4|zstd] [--reps K]
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
    args = ap.parse_args()

    import numpy as np
    import torch
    torch.cuda.is_available()       # torch's HIP view first (see bench.py)
    import citus_amd as ca
    assert ca.gpu_available(), "setpred_bench needs a visible MI355X"

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
    cnt = [(ca.AGG_COUNT_STAR, -1)]
    rng = np.random.default_rng(42)
    os.environ.pop("CSTRIPE_SET_FORM", None)

    def run(reader, preds, label, extra=None):
        """stage one scan, time COUNT(*) on it"""
        with reader.scan(cols_mask=1 << KEY, preds=preds) as s:
            t0 = time.time()
            s.stage(0)
            stage_s = time.time() - t0
            for _ in range(args.warmup):
                n = s.agg(cnt)[0].count
            ms = []
            for _ in range(args.reps):
                s.agg(cnt)
                ms.append(s.last_kernel_ms)
            row = {"case": label, "count": n,
                   "chunk_groups_filtered": s.chunk_groups_filtered,
                   "agg_path": s.last_agg_path, "stage_s": round(stage_s, 3),
                   "kernel_ms": spread(ms)["median"], "kernel_ms_spread": spread(ms)}
            if any(p[1] in (ca.PRED_IN, ca.PRED_NOT_IN) for p in preds):
                b, p = s.last_set_ms()
                form, size = s.set_form(0)
                row.update({"set_build_ms": round(b, 4), "set_probe_ms": round(p, 4),
                            "set_form": {ca.SET_FORM_HASH: "hash",
                                         ca.SET_FORM_BITMAP: "bitmap"}.get(form, "none"),
                            "set_size": size})
            if extra:
                row.update(extra)
            return row

    cases = []
    with ca.Reader(shard) as reader:
        cases.append(run(reader, [], "count_star_no_predicate"))
        for n_set in (10, 1000, 1_000_000):
            per_shard = args.rows // args.shards
            if n_set > per_shard or args.rows % args.shards:
                continue
            # distinct values, so |S| is exactly n_set
            S = np.sort(rng.choice(per_shard, n_set, replace=False).astype(np.int64) + 1)
            want = len(S) * args.shards
            if n_set == 10:
                eq = [(KEY, ca.PRED_EQ, int(v), 1) for v in S]
                r = run(reader, eq, "or_group_of_eq_10")
                assert r["count"] == want, r
                cases.append(r)
            dev = torch.from_numpy(S).to("cuda:0")
            for where, values in (("host", S), ("device", dev)):
                for form in ("hash", "bitmap"):
                    os.environ["CSTRIPE_SET_FORM"] = form
                    for op, opname, expect in ((ca.PRED_IN, "in", want),
                                               (ca.PRED_NOT_IN, "not_in", args.rows - want)):
                        r = run(reader, [(KEY, op, values)],
                                f"{opname}_{n_set}_{where}_{form}_forced",
                                {"set_values": len(S), "set_memory": where})
                        assert r["count"] == expect, r
                        cases.append(r)
                os.environ.pop("CSTRIPE_SET_FORM", None)
                r = run(reader, [(KEY, ca.PRED_IN, values)], f"in_{n_set}_{where}_default",
                        {"set_values": len(S), "set_memory": where})
                assert r["count"] == want, r
                cases.append(r)

    print(json.dumps({"tool": "setpred_bench", "rows": args.rows,
                      "compression": args.compression, "reps": args.reps,
                      "warmup": args.warmup, "gen_s": round(gen_s, 1),
                      "cases": cases}))


if __name__ == "__main__":
    main()
