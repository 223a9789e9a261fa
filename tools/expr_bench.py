#!/usr/bin/env python3
"""
expr_bench.py — what a computed column (a postfix expression evaluated at
stage by expr_eval_kernel) costs on the bench's lineitem, for three programs:

  disc_price   l_extendedprice * (100 - l_discount)        two dense inputs
  q6_case      CASE WHEN shipdate, discount and quantity pass Q6's filter
               THEN l_extendedprice * l_discount ELSE 0 END    four inputs
  year         year(l_shipdate)

Expression work happens at stage (cstripe_scan_last_expr_ms: all evaluation
launches); the queries then read the computed column as an ordinary sparse
I64 column. Each case reports eval_ms (median and min-max of --stage-reps
stages) next to the per-call kernel time (median of --reps calls) of
SUM(computed), and beside them the yardsticks over the same input columns:
COUNT(*) and SUM of every input, the hard-wired SUM_DISC_I64 over the same
two columns, Q6 itself with its five predicates, and the lookup probe of one
10^6-key map on l_orderkey. Sums are cross-checked: SUM(disc_price) equals
SUM_DISC_I64, SUM(q6_case) equals Q6's revenue.

All kernel figures are hipEvent times on the scan's stream as the library
reports them. Prints one JSON line; --out also writes it to a file.

  python tools/expr_bench.py [--rows N] [--compression lz4|zstd] [--reps K]
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
    ap.add_argument("--stage-reps", type=int, default=5)
    ap.add_argument("--lookup-keys", type=int, default=1_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    torch.cuda.is_available()       # torch's HIP view first (see bench.py)
    import citus_amd as ca
    assert ca.gpu_available(), "expr_bench needs a visible MI355X"

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
    KEY, QTY, EXT, DISC, SHIP = (L["l_orderkey"], L["l_quantity"], L["l_extendedprice"],
                                 L["l_discount"], L["l_shipdate"])
    ext, disc, ship, qty = ca.col(EXT), ca.col(DISC), ca.col(SHIP), ca.col(QTY)
    q6_preds = [(SHIP, ca.PRED_GE, 8766), (SHIP, ca.PRED_LT, 9131),
                (DISC, ca.PRED_GE, 5), (DISC, ca.PRED_LE, 7), (QTY, ca.PRED_LT, 2400)]
    q6_cond = ship.ge(8766) & ship.lt(9131) & disc.ge(5) & disc.le(7) & qty.lt(2400)
    programs = [("disc_price", ext * (100 - disc), [EXT, DISC]),
                ("q6_case", ca.case(q6_cond, ext * disc, 0), [SHIP, DISC, QTY, EXT]),
                ("year", ship.year(), [SHIP])]

    def timed(s, aggs):
        for _ in range(args.warmup):
            s.agg(aggs)
        ms = []
        for _ in range(max(1, args.reps)):
            res = s.agg(aggs)
            ms.append(s.last_kernel_ms)
        return spread(ms), res

    cases = []
    sums = {}
    with ca.Reader(shard) as reader:
        for name, expr, inputs in programs:
            mask = 0
            for col in inputs:
                mask |= 1 << col
            # yardsticks over the same input columns
            with reader.scan(cols_mask=mask) as s:
                s.stage(0)
                row = {"case": f"inputs_of_{name}", "columns": inputs}
                row["count_star_ms"], _ = timed(s, [(ca.AGG_COUNT_STAR, -1)])
                row["sum_inputs_ms"], _ = timed(s, [(ca.AGG_SUM_I64, col) for col in inputs])
                row["agg_path"] = s.last_agg_path
                if name == "disc_price":
                    row["sum_disc_ms"], res = timed(s, [(ca.AGG_SUM_DISC_I64, EXT, DISC, -1, 100)])
                    sums["sum_disc"] = res[0].i128
                cases.append(row)
            with reader.scan(exprs=[expr]) as s:
                e_ms, st_s = [], []
                for _ in range(args.stage_reps):
                    t0 = time.time()
                    s.stage(0)
                    st_s.append(time.time() - t0)
                    e_ms.append(s.last_expr_ms())
                lo, hi, n_present = s.expr_range(0)
                row = {"case": f"expr_{name}", "ops": len(expr.ops), "inputs": len(inputs),
                       "eval_ms": spread(e_ms), "stage_s": spread(st_s),
                       "range": [lo, hi], "n_present": n_present}
                row["sum_computed_ms"], res = timed(s, [(ca.AGG_SUM_I64, s.computed(0))])
                row["agg_path"] = s.last_agg_path
                row["sum"] = res[0].i128
                sums[name] = res[0].i128
                assert n_present == args.rows, row
                cases.append(row)
        with reader.scan(cols_mask=ca.agg_cols_mask([(ca.AGG_SUM_PROD_I64, EXT, DISC)]),
                         preds=q6_preds) as s:
            s.stage(0)
            row = {"case": "q6_with_predicates"}
            row["kernel_ms"], res = timed(s, [(ca.AGG_SUM_PROD_I64, EXT, DISC)])
            row["agg_path"] = s.last_agg_path
            sums["q6"] = res[0].i128
            cases.append(row)
        # the lookup probe of DESIGN 5h at the same table size
        per_shard = args.rows // args.shards
        n_map = min(args.lookup_keys, per_shard)
        keys = np.random.default_rng(42).choice(per_shard, n_map, replace=False).astype(np.int64) + 1
        with reader.scan(cols_mask=1 << KEY, lookups=[ca.Lookup(KEY, keys, [keys % 4901 + 100])]) as s:
            b_ms, p_ms = [], []
            for _ in range(args.stage_reps):
                s.stage(0)
                b, p = s.last_lookup_ms()
                b_ms.append(b)
                p_ms.append(p)
            cases.append({"case": f"lookup_{n_map}_host", "form": s.lookup_form(0)[0],
                          "build_ms": spread(b_ms), "probe_ms": spread(p_ms)})
    assert sums["disc_price"] == sums["sum_disc"], sums
    assert sums["q6_case"] == sums["q6"], sums

    line = json.dumps({"tool": "expr_bench", "rows": args.rows,
                       "compression": args.compression, "reps": args.reps,
                       "stage_reps": args.stage_reps, "warmup": args.warmup,
                       "gen_s": round(gen_s, 1), "cases": cases})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
