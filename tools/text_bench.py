#!/usr/bin/env python3
"""
text_bench.py — what a CSTRIPE_VARTEXT column costs: the stage-time split of
the device dictionary build (decode / header walk / dictionary / rank remap,
cstripe_scan_last_text_ms) and, on the staged scan, a filter+aggregate and a
hashed GROUP BY on the text column — each next to the same query on a TWIN
file whose column holds the ranks as I32, and next to COUNT(*) on the same
staged scan (the cost of just walking the rows).

Table (default 10 M rows): v I64, l_shipmode VARTEXT (7 values),
l_shipinstruct VARTEXT (4 values). Queries:

  filter   WHERE l_shipmode IN ('AIR', 'MAIL') AND l_shipinstruct <> 'NONE'
           -> SUM(v), COUNT(*)
  groupby  GROUP BY l_shipmode -> SUM(v), COUNT(*)         (agg_hashed)

The query kernels are the same kernels on both files, so any text/twin gap
is a finding; the stage split is the baseline for work on the walk kernel.
All kernel figures are hipEvent times as the library reports them, medians
over the repetitions with the min/max spread. Prints one JSON line.

  python tools/text_bench.py [--rows N] [--compression none|lz4|zstd] [--reps K]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHIPMODE = [b"REG AIR", b"AIR", b"RAIL", b"SHIP", b"TRUCK", b"MAIL", b"FOB"]
SHIPINSTRUCT = [b"DELIVER IN PERSON", b"COLLECT COD", b"NONE", b"TAKE BACK RETURN"]


def spread(xs):
    return {"median": round(statistics.median(xs), 4),
            "min": round(min(xs), 4), "max": round(max(xs), 4)}


def text_column(np, codes, words):
    """(offsets, bytes) of words[codes] without a Python loop per row"""
    width = max(len(w) for w in words)
    mat = np.zeros((len(words), width), dtype=np.uint8)
    keep = np.zeros((len(words), width), dtype=bool)
    for i, w in enumerate(words):
        mat[i, :len(w)] = np.frombuffer(w, dtype=np.uint8)
        keep[i, :len(w)] = True
    lens = np.array([len(w) for w in words], dtype=np.uint64)
    offs = np.zeros(len(codes) + 1, dtype=np.uint64)
    np.cumsum(lens[codes], out=offs[1:])
    return offs, mat[codes][keep[codes]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--compression", default="lz4", choices=["none", "lz4", "zstd"])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()

    import numpy as np
    import torch
    torch.cuda.is_available()       # torch's HIP view first (see bench.py)
    import citus_amd as ca
    assert ca.gpu_available(), "text_bench needs a visible MI355X"

    comp = {"none": ca.COMP_NONE, "lz4": ca.COMP_LZ4, "zstd": ca.COMP_ZSTD}[args.compression]
    default_cache = ("/dev/shm/cstripe_bench" if os.path.isdir("/dev/shm")
                     else "/tmp/cstripe_bench")
    cache = os.environ.get("CSTRIPE_BENCH_DIR", default_cache)
    os.makedirs(cache, exist_ok=True)
    text_path = os.path.join(cache, f"text_{args.rows}_{args.compression}.cs")
    twin_path = os.path.join(cache, f"text_{args.rows}_{args.compression}_twin.cs")

    n = args.rows
    rng = np.random.default_rng(42)
    v = rng.integers(1, 100_000, n, dtype=np.int64)
    mode = rng.integers(0, len(SHIPMODE), n)
    instr = rng.integers(0, len(SHIPINSTRUCT), n)
    smode, sinstr = sorted(SHIPMODE), sorted(SHIPINSTRUCT)
    t0 = time.time()
    if not (os.path.exists(text_path) and os.path.exists(twin_path)):
        ca.write_table(text_path,
                       [("v", ca.I64, 0), ("l_shipmode", ca.VARTEXT, 0),
                        ("l_shipinstruct", ca.VARTEXT, 0)],
                       [v, text_column(np, mode, SHIPMODE),
                        text_column(np, instr, SHIPINSTRUCT)], compression=comp)
        rank_of = np.array([smode.index(w) for w in SHIPMODE], dtype=np.int32)
        rank_of2 = np.array([sinstr.index(w) for w in SHIPINSTRUCT], dtype=np.int32)
        ca.write_table(twin_path,
                       [("v", ca.I64, 0), ("l_shipmode", ca.I32, 0),
                        ("l_shipinstruct", ca.I32, 0)],
                       [v, rank_of[mode], rank_of2[instr]], compression=comp)
    gen_s = time.time() - t0

    aggs = [(ca.AGG_SUM_I64, 0), (ca.AGG_COUNT_STAR, -1)]
    cnt = [(ca.AGG_COUNT_STAR, -1)]
    text_preds = [(1, ca.PRED_EQ, b"AIR", 1), (1, ca.PRED_EQ, b"MAIL", 1),
                  (2, ca.PRED_NE, b"NONE")]
    twin_preds = [(1, ca.PRED_EQ, smode.index(b"AIR"), 1),
                  (1, ca.PRED_EQ, smode.index(b"MAIL"), 1),
                  (2, ca.PRED_NE, sinstr.index(b"NONE"))]
    # expected values from the generator arrays
    hit = ((mode == SHIPMODE.index(b"AIR")) | (mode == SHIPMODE.index(b"MAIL"))) & \
          (instr != SHIPINSTRUCT.index(b"NONE"))
    exp_filter = (int(v[hit].sum()), int(hit.sum()))
    exp_groups = [(int(v[mode == SHIPMODE.index(w)].sum()),
                   int((mode == SHIPMODE.index(w)).sum())) for w in smode]

    out = {"tool": "text_bench", "rows": n, "compression": args.compression,
           "reps": args.reps, "gen_s": round(gen_s, 1),
           "file_bytes": {"text": os.path.getsize(text_path),
                          "twin": os.path.getsize(twin_path)}}

    def run(path, preds, label):
        res = {}
        with ca.Reader(path) as reader:
            # ---- filter + aggregate ----
            with reader.scan(cols_mask=0b111, preds=preds) as s:
                stage_wall, split = [], {k: [] for k in ("decode_ms", "walk_ms",
                                                         "dict_ms", "remap_ms")}
                for _ in range(max(3, args.reps // 2)):
                    w0 = time.time()
                    s.stage(0)
                    stage_wall.append((time.time() - w0) * 1e3)
                    for k, x in zip(split, s.last_text_ms()):
                        split[k].append(x)
                res["stage_wall_ms"] = spread(stage_wall)
                if label == "text":
                    res["stage_text_ms"] = {k: spread(xs) for k, xs in split.items()}
                    res["stage_text_total_ms"] = round(
                        sum(statistics.median(xs) for xs in split.values()), 4)
                    res["dict_sizes"] = [len(s.text_dict(1)), len(s.text_dict(2))]
                res["staged_bytes"] = s.staged_bytes
                for _ in range(args.warmup):
                    parts = s.agg(aggs)
                assert (parts[0].i128, parts[1].count) == exp_filter, label
                f_ms, d_ms = [], []
                for _ in range(args.reps):
                    s.agg(aggs)
                    f_ms.append(s.last_kernel_ms)
                    d_ms.append(s.last_decode_ms)
                res["filter_agg_ms"] = spread(f_ms)
                res["filter_agg_decode_ms"] = spread(d_ms)
                res["filter_rows"] = exp_filter[1]
            # ---- GROUP BY + COUNT(*) on one staged predicate-free scan ----
            with reader.scan(cols_mask=0b011) as s:
                s.stage(0)
                for _ in range(args.warmup):
                    g = s.agg_hashed(aggs, [1], 16)
                    s.agg(cnt)
                assert g["n_groups"] == len(smode), label
                got = [(ca.partial_i128(g["partials"][i][0]), int(g["partials"][i][1]["count"]))
                       for i in range(g["n_groups"])]
                assert got == exp_groups, label
                assert list(g["keys"][0]) == list(range(len(smode))), label
                g_ms, gs_ms, c_ms = [], [], []
                for _ in range(args.reps):
                    s.agg(cnt)
                    c_ms.append(s.last_kernel_ms)
                    s.agg_hashed(aggs, [1], 16)
                    g_ms.append(s.last_kernel_ms)
                    gs_ms.append(s.last_hash_ms[1])
                res["groupby_ms"] = spread(g_ms)
                res["groupby_scan_ms"] = spread(gs_ms)
                res["count_star_ms"] = spread(c_ms)
        return res

    out["text"] = run(text_path, text_preds, "text")
    out["twin"] = run(twin_path, twin_preds, "twin")
    # totals include the per-call decode of the twin's LZ4/zstd I32 columns
    # (text ranks sit decoded in scratch); groupby_scan_ms is the kernel alone
    for q in ("filter_agg_ms", "groupby_ms", "groupby_scan_ms", "count_star_ms"):
        out[q.replace("_ms", "") + "_text_over_twin"] = round(
            out["text"][q]["median"] / out["twin"][q]["median"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
