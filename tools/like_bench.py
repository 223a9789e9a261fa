#!/usr/bin/env python3
"""
like_bench.py — what LIKE / NOT LIKE over a CSTRIPE_VARTEXT column costs at
cstripe_gpu_stage, in both read forms, next to the closest thing the library
could do before: the stage of the same column under an EQ predicate (decode +
walk + dictionary + remap).

Table (default 10 M rows): v I64, l_shipmode VARTEXT (7 values), p_type
VARTEXT (150 values), o_comment VARTEXT (near unique, 30-80 bytes). Cases:

  l_shipmode LIKE '%AIR'                      (7 values)
  p_type     LIKE 'PROMO%'                    (150 values, Q14)
  p_type     LIKE '%BRASS'                    (150 values, Q2)
  o_comment  NOT LIKE '%special%requests%'    (near unique, Q13)

For each case: the stage split (decode / walk / dict / remap / match / apply,
cstripe_scan_last_text_ms + cstripe_scan_last_like_ms) of the stream form
(the column is only pattern-matched), of the dictionary form (the column is
in cols_mask as well) and of an EQ predicate on the same column, then one
COUNT(*) on the staged scan, checked against the generator. Where the
dictionary cannot be built (more distinct values than
CSTRIPE_VARTEXT_MAX_DISTINCT) the error is recorded instead. On o_comment the
comparison predicate is NE: the values are unique and sorted by their row
number prefix, so an EQ would prune all but one chunk group and stage next to
nothing. All kernel
figures are hipEvent times as the library reports them, medians over the
repetitions with the min/max spread. Prints one JSON line and writes it to
profiles/like_<rows>.json (--out).

  python tools/like_bench.py [--rows N] [--compression none|lz4|zstd] [--reps K]
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
TYPE1 = [b"STANDARD", b"SMALL", b"MEDIUM", b"LARGE", b"ECONOMY", b"PROMO"]
TYPE2 = [b"ANODIZED", b"BURNISHED", b"PLATED", b"POLISHED", b"BRUSHED"]
TYPE3 = [b"TIN", b"NICKEL", b"BRASS", b"STEEL", b"COPPER"]
P_TYPE = [a + b" " + b + b" " + c for a in TYPE1 for b in TYPE2 for c in TYPE3]
WORDS = [b"special", b"requests", b"Customer", b"Complaints", b"furiously", b"pending",
         b"deposits", b"sleep", b"carefully", b"final", b"packages", b"ironic",
         b"accounts", b"express", b"blithely", b"regular"]
SLOT, SLOTS = 10, 8                 # a comment: 8 slots of 10 bytes, cut to 30-80


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


def comment_column(np, n, rng):
    """(offsets, bytes, hit): slot 0 holds the row number (so the values are
    unique), slots 1..7 a word each, space padded; the row is cut to a random
    length in [30, 80]. hit[i]: the row matches '%special%requests%', from the
    word codes — a cut word never completes a match."""
    wmat = np.full((len(WORDS), SLOT), 32, dtype=np.uint8)
    for i, w in enumerate(WORDS):
        wmat[i, :len(w)] = np.frombuffer(w, dtype=np.uint8)
    wlen = np.array([len(w) for w in WORDS])
    lens = rng.integers(30, 81, n)
    offs = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(lens.astype(np.uint64), out=offs[1:])
    data = np.empty(int(offs[-1]), dtype=np.uint8)
    hit = np.zeros(n, dtype=bool)
    step = 1_000_000
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        k = hi - lo
        codes = rng.integers(0, len(WORDS), (k, SLOTS))
        mat = wmat[codes].reshape(k, SLOTS * SLOT)
        ids = np.arange(lo, hi)
        for d in range(9):
            mat[:, d] = 48 + (ids // 10 ** (8 - d)) % 10
        mat[:, 9] = 32
        ln = lens[lo:hi]
        keep = np.arange(SLOTS * SLOT)[None, :] < ln[:, None]
        data[int(offs[lo]):int(offs[hi])] = mat[keep]
        whole = (np.arange(SLOTS)[None, :] * SLOT + wlen[codes]) <= ln[:, None]
        whole[:, 0] = False                      # the row number, not a word
        sp = whole & (codes == WORDS.index(b"special"))
        rq = whole & (codes == WORDS.index(b"requests"))
        first_sp = np.where(sp.any(1), sp.argmax(1), SLOTS)
        last_rq = np.where(rq.any(1), SLOTS - 1 - rq[:, ::-1].argmax(1), -1)
        hit[lo:hi] = first_sp < last_rq
    return offs, data, hit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--compression", default="lz4", choices=["none", "lz4", "zstd"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    torch.cuda.is_available()       # torch's HIP view first (see bench.py)
    import citus_amd as ca
    assert ca.gpu_available(), "like_bench needs a visible MI355X"

    comp = {"none": ca.COMP_NONE, "lz4": ca.COMP_LZ4, "zstd": ca.COMP_ZSTD}[args.compression]
    default_cache = ("/dev/shm/cstripe_bench" if os.path.isdir("/dev/shm")
                     else "/tmp/cstripe_bench")
    cache = os.environ.get("CSTRIPE_BENCH_DIR", default_cache)
    os.makedirs(cache, exist_ok=True)
    path = os.path.join(cache, f"like_{args.rows}_{args.compression}.cs")

    n = args.rows
    rng = np.random.default_rng(42)
    v = rng.integers(1, 100_000, n, dtype=np.int64)
    mode = rng.integers(0, len(SHIPMODE), n)
    ptype = rng.integers(0, len(P_TYPE), n)
    t0 = time.time()
    c_offs, c_data, c_hit = comment_column(np, n, rng)
    if not os.path.exists(path):
        ca.write_table(path,
                       [("v", ca.I64, 0), ("l_shipmode", ca.VARTEXT, 0),
                        ("p_type", ca.VARTEXT, 0), ("o_comment", ca.VARTEXT, 0)],
                       [v, text_column(np, mode, SHIPMODE), text_column(np, ptype, P_TYPE),
                        (c_offs, c_data)], compression=comp)
    gen_s = time.time() - t0

    def count_where(words, codes, test):
        ok = np.array([test(w) for w in words])
        return int(ok[codes].sum())

    # (name, column, op, pattern, expected COUNT(*),
    #  comparison op, its constant, its COUNT(*))
    cases = [
        ("shipmode_%AIR", 1, ca.PRED_LIKE, b"%AIR",
         count_where(SHIPMODE, mode, lambda w: w.endswith(b"AIR")),
         ca.PRED_EQ, b"AIR", count_where(SHIPMODE, mode, lambda w: w == b"AIR")),
        ("p_type_PROMO%", 2, ca.PRED_LIKE, b"PROMO%",
         count_where(P_TYPE, ptype, lambda w: w.startswith(b"PROMO")),
         ca.PRED_EQ, P_TYPE[7], count_where(P_TYPE, ptype, lambda w: w == P_TYPE[7])),
        ("p_type_%BRASS", 2, ca.PRED_LIKE, b"%BRASS",
         count_where(P_TYPE, ptype, lambda w: w.endswith(b"BRASS")),
         ca.PRED_EQ, P_TYPE[7], count_where(P_TYPE, ptype, lambda w: w == P_TYPE[7])),
        ("o_comment_NOT_%special%requests%", 3, ca.PRED_NOT_LIKE, b"%special%requests%",
         int((~c_hit).sum()), ca.PRED_NE, bytes(c_data[:int(c_offs[1])]), n - 1),
    ]

    out = {"tool": "like_bench", "rows": n, "compression": args.compression,
           "reps": args.reps, "gen_s": round(gen_s, 1),
           "file_bytes": os.path.getsize(path), "cases": {}}
    cnt = [(ca.AGG_COUNT_STAR, -1)]
    keys = ("decode_ms", "walk_ms", "dict_ms", "remap_ms", "match_ms", "apply_ms")

    def run(reader, cols_mask, preds, want_form, want_count):
        """stage `reps` times, then COUNT(*); a stage the library refuses is
        recorded as its error"""
        res = {}
        with reader.scan(cols_mask=cols_mask, preds=preds) as s:
            wall, split = [], {k: [] for k in keys}
            for _ in range(args.reps):
                w0 = time.time()
                try:
                    s.stage(0)
                except ca.CStripeError as e:
                    return {"error": str(e)}
                wall.append((time.time() - w0) * 1e3)
                for k, x in zip(keys, s.last_text_ms() + s.last_like_ms()):
                    split[k].append(x)
            assert s.like_form(preds[0][0]) == want_form, (preds, s.like_form(preds[0][0]))
            res["form"] = want_form
            res["chunk_groups_filtered"] = s.chunk_groups_filtered
            res["stage_wall_ms"] = spread(wall)
            res["stage_ms"] = {k: spread(xs) for k, xs in split.items()}
            res["stage_device_total_ms"] = round(
                sum(statistics.median(xs) for xs in split.values()), 4)
            c_ms = []
            for _ in range(args.reps + 1):
                parts = s.agg(cnt)
                c_ms.append(s.last_kernel_ms)
            assert parts[0].count == want_count, (preds, parts[0].count, want_count)
            res["count_star_ms"] = spread(c_ms[1:])
            res["count"] = want_count
        return res

    with ca.Reader(path) as reader:
        for name, col, op, pat, want, eq_op, eq_const, eq_want in cases:
            print(f"like_bench: {name} (generated in {gen_s:.0f} s)", file=sys.stderr, flush=True)
            out["cases"][name] = {
                "stream": run(reader, 1, [(col, op, pat)], "stream", want),
                "dict": run(reader, 1 | (1 << col), [(col, op, pat)], "dict", want),
                "eq": run(reader, 1, [(col, eq_op, eq_const)], None, eq_want),
            }
            out["cases"][name]["eq"]["op"] = "EQ" if eq_op == ca.PRED_EQ else "NE"
    for name, c in out["cases"].items():
        if "error" not in c["eq"]:
            c["stream_over_eq"] = round(c["stream"]["stage_device_total_ms"] /
                                        c["eq"]["stage_device_total_ms"], 3)
    line = json.dumps(out)
    print(line)
    dst = args.out or os.path.join(REPO, "profiles", f"like_{n // 1_000_000}m.json")
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
