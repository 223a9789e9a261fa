#!/usr/bin/env python3
"""
groupby_topn_bench.py — cstripe_scan_agg_hashed_topn (GROUP BY ... [HAVING]
ORDER BY ... LIMIT on the device) next to cstripe_scan_agg_hashed, which
returns every group, on the SAME staged scan.

Generates the bench's lineitem (default 100 M rows, sharded), stages once per
query, warms up, then alternates the calls. Two GROUP BYs, each with the Q1
aggregates (agg 0 = sum(l_quantity), agg 1 = sum(l_extendedprice)):

  GROUP BY l_shipdate     ~2.5 k groups
  GROUP BY l_orderkey     one group per row, the scan cut by
                          `l_orderkey <= --orderkey-max` (4 M groups)

and per GROUP BY three calls:

  agg_hashed              every group comes back and is sorted on the host
  top10                   ORDER BY sum(l_quantity) DESC LIMIT 10
  q18                     the Q18 shape: HAVING sum(l_quantity) > c ORDER BY
                          sum(l_extendedprice) DESC, key LIMIT 100; c is the
                          90th percentile of the groups' sums, taken from the
                          agg_hashed result

Device figures are hipEvent times on the scan's stream as the library reports
them (front half: decode, table init, scan + hash aggregate, compaction; back
half: range / HAVING, key build + selection, gather); wall is the time inside
the Python call. Medians over the repetitions with the min/max spread. The
top-N results are checked against a numpy sort of the agg_hashed result.
Prints one JSON line and writes it to --out.

  python tools/groupby_topn_bench.py [--rows N] [--compression lz4|zstd]
                                     [--reps K] [--out FILE]
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--orderkey-max", type=int, default=4_000_000)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "hashagg_topn_100m.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    torch.cuda.is_available()       # torch's HIP view first (see bench.py)
    import citus_amd as ca
    assert ca.gpu_available(), "groupby_topn_bench needs a visible MI355X"

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
    okmax = min(args.orderkey_max, ca.MAX_HASH_GROUPS)
    queries = [
        ("shipdate", [L["l_shipdate"]], 4096, []),
        ("orderkey", [L["l_orderkey"]], okmax, [(L["l_orderkey"], ca.PRED_LE, okmax)]),
    ]
    os.environ.pop("CSTRIPE_HASH_LDS_SLOTS", None)
    top10 = dict(order=[("agg", 0, "desc")], limit=10)

    def front(s):
        i_ms, s_ms, c_ms = s.last_hash_ms
        return {"decode_ms": s.last_decode_ms, "init_ms": i_ms, "scan_ms": s_ms,
                "compact_ms": c_ms, "device_ms": s.last_kernel_ms}

    def run_hashed(s, keys, cap):
        w0 = time.time()
        res = s.agg_hashed(q1, keys, cap)
        p = front(s)
        p["wall_ms"] = (time.time() - w0) * 1e3
        return res, p

    def run_topn(s, keys, cap, order, limit, having=()):
        w0 = time.time()
        res = s.agg_hashed_topn(q1, keys, cap, order, limit, having=having)
        wall = (time.time() - w0) * 1e3
        p = front(s)
        n, kept, r_ms, s_ms, e_ms = s.last_group_topn
        p.update(range_ms=r_ms, select_ms=s_ms, emit_ms=e_ms, wall_ms=wall,
                 groups=n, kept=kept)
        return res, p

    def sums_of(res, a):
        # the bench's sums fit int64 (hi is the sign extension)
        return res["partials"]["i128_lo"][:, a].astype(np.int64)

    def summarize(samples):
        out = {}
        for k in samples[0]:
            xs = [p[k] for p in samples]
            if k in ("groups", "kept"):
                out[k] = int(xs[0])
            else:
                out[k] = round(statistics.median(xs), 4)
                out[k + "_spread"] = spread(xs)
        out["host_ms"] = round(out["wall_ms"] - out["device_ms"], 4)
        return out

    out = {"tool": "groupby_topn_bench", "rows": args.rows,
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
            full, _p = run_hashed(s, keys, cap)
            qty = sums_of(full, 0)
            thr = int(np.sort(qty)[int(0.9 * (len(qty) - 1))])
            q18 = dict(order=[("agg", 1, "desc"), ("key", 0)], limit=100,
                       having=[(0, ca.PRED_GT, thr)])
            # the top-N calls against a numpy sort of every group
            kv = full["keys"][0]
            want = np.lexsort((kv, -qty))[:10]
            got, _p = run_topn(s, keys, cap, **top10)
            assert np.array_equal(got["keys"][0], kv[want]), "top10 differs"
            price = sums_of(full, 1)
            keep = np.flatnonzero(qty > thr)
            want = keep[np.lexsort((kv[keep], -price[keep]))][:100]
            got, _p = run_topn(s, keys, cap, **q18)
            assert np.array_equal(got["keys"][0], kv[want]), "q18 differs"
            assert got["partials"].tobytes() == full["partials"][want].tobytes()
            for _ in range(args.warmup):
                run_hashed(s, keys, cap)
                run_topn(s, keys, cap, **top10)
                run_topn(s, keys, cap, **q18)
            t = {"agg_hashed": [], "top10": [], "q18": []}
            for _ in range(args.reps):
                t["agg_hashed"].append(run_hashed(s, keys, cap)[1])
                t["top10"].append(run_topn(s, keys, cap, **top10)[1])
                t["q18"].append(run_topn(s, keys, cap, **q18)[1])
            q = {"key_cols": keys, "capacity": cap, "n_groups": int(full["n_groups"]),
                 "stage_s": round(stage_s, 2), "q18_having_sum_quantity_gt": thr,
                 "result_bytes": {
                     "agg_hashed": int(full["n_groups"]) * (8 + 32 * len(q1)),
                     "top10": 10 * (24 + 32 * len(q1)),
                     "q18": 100 * (24 + 32 * len(q1))}}
            for call, samples in t.items():
                q[call] = summarize(samples)
            out["queries"][name] = q
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
