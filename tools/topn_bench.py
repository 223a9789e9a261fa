#!/usr/bin/env python3
"""
topn_bench.py — device time of cstripe_scan_select_topn for
`ORDER BY l_extendedprice DESC LIMIT 100` over the bench's lineitem, in two
settings: under the Q6 predicates, and with no predicate at all. Next to
each: cstripe_scan_agg with a single COUNT_STAR on the SAME staged scan
(the cost of reading the predicate columns), and what a user does today —
select(device=True) of the key column followed by torch.topk on it.

Generates the bench's lineitem (default 100 M rows, sharded), stages once
per setting, warms every path, then alternates the three. select_topn and
COUNT_STAR figures are hipEvent times on the scan's stream as the library
reports them; torch.topk is timed with torch.cuda events. Medians over the
repetitions with the min/max spread. Prints one JSON line.

  python tools/topn_bench.py [--rows N] [--compression lz4|zstd] [--reps K]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

LIMIT = 100


def spread(xs):
    return {"median": round(statistics.median(xs), 4),
            "min": round(min(xs), 4), "max": round(max(xs), 4)}


def run_setting(ca, torch, shard, preds, args):
    C = ca.LINEITEM_COLS
    key = C["l_extendedprice"]
    order = [(key, "desc")]
    cnt = [(ca.AGG_COUNT_STAR, -1)]
    keys = ("count_star_kernel_ms", "topn_decode_ms", "topn_mask_ms",
            "topn_key_ms", "topn_select_ms", "topn_emit_ms", "topn_total_ms",
            "topn_cold_total_ms", "select_mask_ms", "select_total_ms",
            "torch_topk_ms", "select_plus_topk_ms")
    t = {k: [] for k in keys}
    with ca.Reader(shard) as reader, \
            reader.scan(cols_mask=1 << key, preds=preds) as s:
        t0 = time.time()
        s.stage(0)
        stage_s = time.time() - t0
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)

        def once(record):
            s.agg(cnt)
            cs_ms = s.last_kernel_ms
            res = s.select_topn(order, LIMIT, cols=[key], want_nulls=False,
                                device=True)
            p = res["topn_profile"]
            sel = s.select(cols=[key], want_nulls=False, device=True)
            sp = s.select_profile
            e0.record()
            top = torch.topk(sel["values"][key], min(LIMIT, sel["n_rows"]))
            e1.record()
            torch.cuda.synchronize()
            tk_ms = e0.elapsed_time(e1)
            if record:
                m_ms = p["total_ms"] - p["decode_ms"] - p["key_ms"] - \
                    p["select_ms"] - p["emit_ms"]
                t["count_star_kernel_ms"].append(cs_ms)
                t["topn_decode_ms"].append(p["decode_ms"])
                t["topn_mask_ms"].append(max(m_ms, 0.0))
                t["topn_key_ms"].append(p["key_ms"])
                t["topn_select_ms"].append(p["select_ms"])
                t["topn_emit_ms"].append(p["emit_ms"])
                t["topn_total_ms"].append(p["total_ms"])
                # select() re-runs the mask pass on every call; select_topn is
                # served from the scan's cache after its first call. A cold
                # call runs that same pass, so it costs the sum.
                t["select_mask_ms"].append(sp["mask_ms"] + sp["offsets_ms"])
                t["topn_cold_total_ms"].append(p["total_ms"] + sp["mask_ms"] +
                                               sp["offsets_ms"])
                t["select_total_ms"].append(sp["total_ms"])
                t["torch_topk_ms"].append(tk_ms)
                t["select_plus_topk_ms"].append(sp["total_ms"] + tk_ms)
            return res, sel, top, cs_ms + p["total_ms"] + sp["total_ms"] + tk_ms

        for _ in range(args.warmup):
            res, sel, top, _ = once(False)
        # both paths return the same 100 prices
        got = res["values"][key].cpu().tolist()
        assert got == top.values.cpu().tolist(), "select_topn != select + topk"
        n_pass = sel["n_rows"]
        reps, dev_ms = 0, 0.0
        while True:
            dev_ms += once(True)[3]
            reps += 1
            if args.reps and reps >= args.reps:
                break
            if not args.reps and reps >= 20 and dev_ms >= 2000.0:
                break
            if reps >= 5000:
                break
    out = {"passing_rows": n_pass, "reps": reps, "stage_s": round(stage_s, 2),
           "timed_device_ms": round(dev_ms, 1), "key_array_bytes": 8 * n_pass}
    for k in keys:
        out[k] = spread(t[k])["median"]
        out[k + "_spread"] = spread(t[k])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--compression", default="lz4", choices=["lz4", "zstd"])
    ap.add_argument("--shards", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=0,
                    help="timed repetitions per setting (0 = auto: at least "
                         "20 and at least 2 s of device time)")
    args = ap.parse_args()

    import torch
    torch.cuda.is_available()       # torch's HIP view first (see bench.py)
    import citus_amd as ca
    assert ca.gpu_available(), "topn_bench needs a visible MI355X"

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

    q6 = [(5, ca.PRED_GE, 8766), (5, ca.PRED_LT, 9131),
          (3, ca.PRED_GE, 5), (3, ca.PRED_LE, 7), (1, ca.PRED_LT, 2400)]
    out = {"tool": "topn_bench", "rows": args.rows,
           "compression": args.compression,
           "query": f"ORDER BY l_extendedprice DESC LIMIT {LIMIT}",
           "staged_gen_s": round(gen_s, 1),
           "q6_predicates": run_setting(ca, torch, shard, q6, args),
           "no_predicate": run_setting(ca, torch, shard, [], args)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
