"""
GPU stream-shape matrix (@pytest.mark.gpu): every entry of the stream-shape
catalogue (tests/shapes.py) through every device read path — scan_agg in all
hand-unrolled (n_preds, n_aggs) shapes, scan_agg_grouped, scan_select,
scan_agg_hashed, next_batch and read_row — against expectations computed in
numpy / Python ints from the arrays written (shapes.expect_agg), never from
the library. test_stream_shapes_cpu.py pins that each entry really is written
in its catalogued shape; the same footer check is repeated here before any
result is trusted, and Scan.last_fused is asserted so that a test cannot
silently run another kernel than the one it is about.

Each table holds the entry's column (0), a dense I64 helper from another
entry of the same codec and stream family (1) and an I8 key 0..4 (2).

Bar: counts, is_null, integers and int128 sums exact; float MIN/MAX and
selected values by bit pattern (NaN as NaN); SUM_F64 within 1e-6 relative of
math.fsum (BASELINE.json), NaN / infinite sums exact.
"""
import math

import numpy as np
import pytest

import citus_amd as ca
import shapes
from shapes import Col, SHAPES
from test_stream_shapes_cpu import footer_chunks

pytestmark = pytest.mark.gpu

X, H, K = 0, 1, 2
I64_MIN, I64_MAX = shapes.I64_MIN, shapes.I64_MAX
LT, LE, GT, GE, EQ, NE = (ca.PRED_LT, ca.PRED_LE, ca.PRED_GT, ca.PRED_GE,
                          ca.PRED_EQ, ca.PRED_NE)


@pytest.fixture(scope="module", autouse=True)
def require_gpu():
    assert ca.gpu_available(), "MI355X required for these tests"


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    """name -> (path, [Col x, Col h, Col k]); each table is written once and
    its footer checked against the catalogue before anything reads it"""
    root = tmp_path_factory.mktemp("shapes")
    cache = {}

    def get(name):
        if name not in cache:
            sh = SHAPES[name]
            path = str(root / f"{name}.cs")
            shapes.write_shape(path, sh, with_helpers=True)
            assert footer_chunks(path, X) == sh.chunks
            assert footer_chunks(path, H) == SHAPES[sh.helper].chunks
            cache[name] = (path, [Col(sh.values, sh.nulls),
                                  Col(SHAPES[sh.helper].values),
                                  Col(shapes.key_column(sh.n))])
        return cache[name]
    return get


# ------------------------------------------------------------------ queries
def consts(col):
    """predicate constants from the data: minimum, maximum, median, one
    present value c and its two neighbours c - 1 / c + 1 (floats: the
    adjacent doubles)"""
    pv = col.present_values()
    s = sorted(pv, key=shapes.pg_sort_key)
    c = pv[len(pv) // 3]
    if col.is_float:
        cm1, cp1 = float(np.nextafter(c, -np.inf)), float(np.nextafter(c, np.inf))
    else:
        cm1, cp1 = max(c - 1, I64_MIN), min(c + 1, I64_MAX)
    return {"mn": s[0], "mx": s[-1], "med": s[len(s) // 2], "c": c,
            "cm1": cm1, "cp1": cp1}


def agg_queries(cols):
    """[(preds, aggs)] in the shapes the kernels unroll by hand —
    (n_preds, n_aggs) = (0,1) (1,1) (2,2) (5,1) (5,2) (5,4) — plus the
    generic (3,3). All six operators occur; every aggregate kind valid for
    the column's type occurs, the product forms with the column as each
    operand. Float columns add NaN and +-inf constants."""
    x, h = consts(cols[X]), consts(cols[H])
    preds = [
        [],
        [(X, EQ, x["c"])],
        [(X, GE, x["med"]), (X, NE, x["c"])],
        # exactly the rows equal to c (when c has both neighbours)
        [(X, GT, x["cm1"]), (X, LT, x["cp1"]), (X, GE, x["mn"]), (X, LE, x["mx"]),
         (H, GE, h["mn"])],
        [(X, GE, x["mn"]), (X, LE, x["cp1"]), (X, NE, x["cm1"]), (H, GE, h["mn"]),
         (H, LE, h["mx"])],
        [(X, GE, x["mn"]), (X, LE, x["mx"]), (X, NE, x["c"]), (H, GE, h["mn"]),
         (H, LE, h["mx"])],
        [(X, LT, x["med"]), (X, NE, x["mn"]), (H, GE, h["med"])],
    ]
    if cols[X].is_float:
        aggs = [
            [(ca.AGG_SUM_F64, X)],
            [(ca.AGG_MIN_F64, X)],
            [(ca.AGG_MIN_F64, X), (ca.AGG_MAX_F64, X)],
            [(ca.AGG_COUNT_COL, X)],
            [(ca.AGG_SUM_F64, X), (ca.AGG_SUM_I64, H)],
            [(ca.AGG_COUNT_STAR, -1), (ca.AGG_SUM_F64, X), (ca.AGG_MIN_F64, X),
             (ca.AGG_MAX_F64, X)],
            [(ca.AGG_MAX_F64, X), (ca.AGG_SUM_F64, X), (ca.AGG_SUM_PROD_I64, H, H)],
        ]
        nan, inf = float("nan"), float("inf")
        preds += [[(X, LT, nan)], [(X, GE, nan)],
                  [(X, GT, -inf), (X, LT, inf)],
                  [(X, NE, nan), (X, GE, -inf), (X, LE, inf)]]
        aggs += [[(ca.AGG_SUM_F64, X)], [(ca.AGG_COUNT_STAR, -1)],
                 [(ca.AGG_MIN_F64, X), (ca.AGG_MAX_F64, X)],
                 [(ca.AGG_SUM_F64, X), (ca.AGG_MIN_F64, X), (ca.AGG_MAX_F64, X)]]
    else:
        aggs = [
            [(ca.AGG_SUM_PROD_I64, X, H)],
            [(ca.AGG_SUM_I64, X)],
            [(ca.AGG_MIN_I64, X), (ca.AGG_MAX_I64, X)],
            [(ca.AGG_COUNT_COL, X)],
            [(ca.AGG_SUM_PROD_I64, H, X), (ca.AGG_SUM_DISC_I64, X, H)],
            [(ca.AGG_SUM_DISC_I64, H, X), (ca.AGG_SUM_DISC_TAX_I64, X, H, H),
             (ca.AGG_SUM_DISC_TAX_I64, H, X, H), (ca.AGG_SUM_DISC_TAX_I64, H, H, X)],
            [(ca.AGG_COUNT_STAR, -1), (ca.AGG_SUM_I64, X), (ca.AGG_MIN_I64, H)],
        ]
    got = [(len(p), len(a)) for p, a in zip(preds, aggs)][:7]
    assert got == [(0, 1), (1, 1), (2, 2), (5, 1), (5, 2), (5, 4), (3, 3)]
    return [(p, shapes.with_one(cols, a)) for p, a in zip(preds, aggs)]


def grouped_queries(cols):
    """n_aggs in {1, 2, 4, 5} (unrolled in multi_grouped_kernel) and 3
    (generic), alternately unfiltered and filtered"""
    x = consts(cols[X])
    if cols[X].is_float:
        aggs = [
            [(ca.AGG_SUM_F64, X)],
            [(ca.AGG_MIN_F64, X), (ca.AGG_MAX_F64, X)],
            [(ca.AGG_COUNT_STAR, -1), (ca.AGG_SUM_F64, X), (ca.AGG_MIN_F64, X),
             (ca.AGG_COUNT_COL, X)],
            [(ca.AGG_SUM_F64, X), (ca.AGG_MIN_F64, X), (ca.AGG_MAX_F64, X),
             (ca.AGG_COUNT_STAR, -1), (ca.AGG_SUM_I64, H)],
            [(ca.AGG_MAX_F64, X), (ca.AGG_SUM_F64, X), (ca.AGG_MIN_I64, H)],
        ]
    else:
        aggs = [
            [(ca.AGG_SUM_I64, X)],
            [(ca.AGG_SUM_PROD_I64, X, H), (ca.AGG_COUNT_COL, X)],
            [(ca.AGG_MIN_I64, X), (ca.AGG_MAX_I64, X), (ca.AGG_SUM_DISC_I64, X, H),
             (ca.AGG_SUM_I64, H)],
            [(ca.AGG_SUM_I64, X), (ca.AGG_COUNT_STAR, -1), (ca.AGG_MIN_I64, X),
             (ca.AGG_MAX_I64, X), (ca.AGG_SUM_PROD_I64, H, X)],
            [(ca.AGG_SUM_DISC_TAX_I64, H, X, H), (ca.AGG_COUNT_STAR, -1),
             (ca.AGG_SUM_I64, X)],
        ]
    assert [len(a) for a in aggs] == [1, 2, 4, 5, 3]
    preds = [[], [(X, GE, x["med"])], [], [(X, NE, x["c"])], [(X, LE, x["med"])]]
    return [(p, shapes.with_one(cols, a)) for p, a in zip(preds, aggs)]


def fusable_col(sh):
    """stage rule (cstripe_gpu_stage, `fusable`): a projected column keeps the
    scan fusable only if every chunk is dense I64, comp_type LZ4, generic
    mode 0 in uniform 256 B segments; any canonical, raw, zstd or sparse
    chunk clears it"""
    return sh.ctype == ca.I64 and sh.dense and \
        all(ct == shapes.LZ4 and m == 0x00 for ct, m, _ in sh.chunks)


def run_agg(path, preds, aggs):
    with ca.Reader(path) as r, \
            r.scan(cols_mask=ca.agg_cols_mask(aggs), preds=preds) as s:
        s.stage()
        parts = [p.as_dict() for p in s.agg(aggs)]
        return parts, s.last_fused, s.chunk_groups_filtered


def projected(preds, aggs):
    cols = {p[0] for p in preds}
    for a in aggs:
        cols |= {c for c in a[1:4] if c >= 0}
    return cols or {0}


def check_agg_queries(name, path, cols, queries, fusable_by_col, n_chunks):
    """run every query, compare with the expectation, and assert the path.
    Returns the raw partials for the variant comparison."""
    out = []
    for qi, (preds, aggs) in enumerate(queries):
        parts, fused, pruned = run_agg(path, preds, aggs)
        rows = shapes.pass_mask(cols, preds)
        for ai, a in enumerate(aggs):
            shapes.check_partial(parts[ai], shapes.expect_agg(cols, a, rows), a[0],
                                 f"{name} query {qi} agg {ai} {a}")
        # scan_agg rule: the fused kernel runs iff the staged scan is fusable
        # (every projected column, see fusable_col; at most 4 of them) and
        # every aggregate is an integer kind
        want_fused = all(fusable_by_col[c] for c in projected(preds, aggs)) and \
            len(projected(preds, aggs)) <= 4 and \
            all(a[0] not in shapes.FLOAT_KINDS for a in aggs)
        if pruned == n_chunks:
            # min/max pruning removed every chunk group: no kernel runs at all
            assert not rows.any()
            want_fused = False
        assert fused == want_fused, \
            f"{name} query {qi}: last_fused {fused}, expected {want_fused}"
        out.append(parts)
    return out


def same_partials(a, b):
    def key(p):
        return (p["count"], p["is_null"], p["i128"], shapes.f64_bits(p["f64"]))
    return [[key(p) for p in q] for q in a] == [[key(p) for p in q] for q in b]


# ------------------------------------------------------------------ scan_agg
@pytest.mark.parametrize("name", shapes.NAMES)
def test_scan_agg(tables, monkeypatch, name):
    """dense entries take multi_agg_kernel (the L = 5 LZ4 ones the fused
    kernel), sparse twins filter_agg_kernel: stage's all_dense rule"""
    sh = SHAPES[name]
    path, cols = tables(name)
    fus = {X: fusable_col(sh), H: fusable_col(SHAPES[sh.helper]), K: False}
    if any(shapes.is_canonical_mode(m) for _, m, _ in sh.chunks):
        assert not fus[X]          # stage: a canonical chunk clears `fusable`
    monkeypatch.delenv("CSTRIPE_ZR_VARIANT", raising=False)
    queries = agg_queries(cols)
    base = check_agg_queries(name, path, cols, queries, fus, len(sh.chunks))
    if name in ("i64_l5a_lz4", "i64_l5b_lz4"):
        # the default writer's fusable shape: every query above ran fused
        assert fus[X] and fus[H]
    if any(m == 0x50 for _, m, _ in sh.chunks):
        # generic restricted-zstd frames: the decode kernel is chosen per
        # call by CSTRIPE_ZR_VARIANT; unset = zr_decode_lds2_kernel,
        # "1" = zr_decode_lds_kernel, "0" = zr_decode_kernel
        for v in ("1", "0"):
            monkeypatch.setenv("CSTRIPE_ZR_VARIANT", v)
            again = check_agg_queries(name, path, cols, queries, fus, len(sh.chunks))
            assert same_partials(base, again), f"{name}: CSTRIPE_ZR_VARIANT={v} differs"


# ---------------------------------------------------------- scan_agg_grouped
@pytest.mark.parametrize("name", shapes.NAMES)
def test_scan_agg_grouped(tables, name):
    path, cols = tables(name)
    key = cols[K].wide
    for qi, (preds, aggs) in enumerate(grouped_queries(cols)):
        with ca.Reader(path) as r, \
                r.scan(cols_mask=ca.agg_cols_mask(aggs) | (1 << K), preds=preds) as s:
            s.stage()
            res = s.agg_grouped(aggs, [K])
        rows = shapes.pass_mask(cols, preds)
        want_keys = sorted({int(k) for k in key[rows]})
        assert sorted(k[0] for k in res) == want_keys, f"{name} grouped {qi}"
        for g in want_keys:
            parts = res[(g, 0)]
            for ai, a in enumerate(aggs):
                shapes.check_partial(parts[ai],
                                     shapes.expect_agg(cols, a, rows & (key == g)),
                                     a[0], f"{name} grouped {qi} key {g} agg {ai} {a}")


# --------------------------------------------------------------- scan_select
@pytest.mark.parametrize("name", shapes.NAMES)
def test_scan_select(tables, name):
    sh = SHAPES[name]
    path, cols = tables(name)
    x = consts(cols[X])
    uint = sh.bits().dtype
    for preds in ([], [(X, GE, x["med"])], [(H, LE, consts(cols[H])["med"])]):
        with ca.Reader(path) as r, r.scan(cols_mask=1 << X, preds=preds) as s:
            s.stage()
            res = s.select(cols=[X])
        # a NULL operand fails its atom; with no predicate every row comes out
        rows = np.nonzero(shapes.pass_mask(cols, preds))[0]
        assert res["n_rows"] == len(rows)
        np.testing.assert_array_equal(res["row_numbers"], rows)
        want_null = (~cols[X].present[rows]).astype(np.uint8)
        np.testing.assert_array_equal(res["nulls"][X], want_null)
        want = sh.bits()[rows].copy()
        want[want_null.astype(bool)] = 0              # NULL slots are zero-filled
        np.testing.assert_array_equal(
            np.ascontiguousarray(res["values"][X]).view(uint), want)


# ----------------------------------------------------------- scan_agg_hashed
def expect_hashed(cols, key_cols, aggs, rows):
    """{key tuple (None = NULL): [expected partial per agg]}"""
    groups = {}
    for i in np.nonzero(rows)[0]:
        kt = tuple(int(cols[k].wide[i]) if cols[k].present[i] else None
                   for k in key_cols)
        groups.setdefault(kt, []).append(i)
    out = {}
    for kt, idx in groups.items():
        m = np.zeros(len(rows), dtype=bool)
        m[idx] = True
        out[kt] = [shapes.expect_agg(cols, a, m) for a in aggs]
    return out


def check_hashed(name, path, cols, key_cols, aggs, preds):
    mask = ca.agg_cols_mask(aggs)
    for k in key_cols:
        mask |= 1 << k
    n = len(cols[X].values)
    with ca.Reader(path) as r, r.scan(cols_mask=mask, preds=preds) as s:
        s.stage()
        res = s.agg_hashed(aggs, key_cols, n + 1)
    want = expect_hashed(cols, key_cols, aggs, shapes.pass_mask(cols, preds))
    got_keys = [tuple(None if res["key_nulls"][k][g] else int(res["keys"][k][g])
                      for k in range(len(key_cols)))
                for g in range(res["n_groups"])]
    # ascending by key tuple, signed, NULL last per column
    order = sorted(want, key=lambda kt: tuple((v is None, v or 0) for v in kt))
    assert got_keys == order, f"{name} hashed keys"
    for g, kt in enumerate(got_keys):
        for ai, a in enumerate(aggs):
            p = res["partials"][g, ai]
            got = {"count": int(p["count"]), "is_null": bool(p["is_null"]),
                   "i128": ca.partial_i128(p), "f64": float(p["f64"])}
            shapes.check_partial(got, want[kt][ai], a[0],
                                 f"{name} hashed key {kt} agg {ai} {a}")


@pytest.mark.parametrize("name", shapes.NAMES)
def test_scan_agg_hashed(tables, name):
    """the entry's column as an aggregate operand under the I8 key, and for
    integer types also as the key itself"""
    path, cols = tables(name)
    x = consts(cols[X])
    if cols[X].is_float:
        aggs = [(ca.AGG_COUNT_STAR, -1), (ca.AGG_SUM_F64, X), (ca.AGG_MIN_F64, X),
                (ca.AGG_MAX_F64, X), (ca.AGG_COUNT_COL, X)]
    else:
        aggs = [(ca.AGG_COUNT_STAR, -1), (ca.AGG_SUM_I64, X), (ca.AGG_MIN_I64, X),
                (ca.AGG_MAX_I64, X), (ca.AGG_SUM_PROD_I64, X, H),
                (ca.AGG_SUM_DISC_I64, H, X)]
    aggs = shapes.with_one(cols, aggs)
    check_hashed(name, path, cols, [K], aggs, [])
    check_hashed(name, path, cols, [K], aggs, [(X, NE, x["c"])])
    if not cols[X].is_float:
        check_hashed(name, path, cols, [X], aggs, [])
        check_hashed(name, path, cols, [K, X], aggs, [(X, GE, x["med"])])


# ------------------------------------------------------ next_batch / read_row
@pytest.mark.parametrize("name", shapes.NAMES)
def test_next_batch_and_read_row(tables, name):
    sh = SHAPES[name]
    path, cols = tables(name)
    uint = sh.bits().dtype
    bounds = sh.chunk_bounds()
    with ca.Reader(path) as r, r.scan(cols_mask=1 << X) as s:
        s.stage()
        vals = np.zeros(sh.cgrl, dtype=sh.values.dtype)
        nulls = np.zeros(sh.cgrl, dtype=np.uint8)
        for lo, hi in bounds:
            nr, first = s.next_batch({X: vals}, {X: nulls})
            assert (nr, first) == (hi - lo, lo)
            present = cols[X].present[lo:hi]
            np.testing.assert_array_equal(nulls[:nr], (~present).astype(np.uint8))
            np.testing.assert_array_equal(vals[:nr].view(uint)[present],
                                          sh.bits()[lo:hi][present])
        assert s.next_batch({X: vals}, {X: nulls}) is None

    # rows 0, 1, 2, the last row, and both sides of every chunk boundary
    want_rows = {0, 1, 2, sh.n - 1}
    for lo, _ in bounds[1:]:
        want_rows |= {lo - 1, lo}
    with ca.Reader(path) as r, r.scan(cols_mask=1 << X) as s:
        s.stage()
        for row in sorted(w for w in want_rows if 0 <= w < sh.n):
            got = s.read_row(row)[X]
            if not cols[X].present[row]:
                assert got is None, f"{name} row {row}"
            else:
                assert got is not None, f"{name} row {row}"
                gb = int(np.array([got], dtype=sh.values.dtype).view(uint)[0])
                assert gb == int(sh.bits()[row]), f"{name} row {row}: {got!r}"
        assert s.read_row(sh.n) is None


# ------------------------------------------------------- the fused kernel
FUSED_ROWS = (2, 31, 32, 33, 2047, 2048, 2049, 9985)


def fused_columns(source, rows, n_cols=2):
    """dense I64 columns that the writer stores as generic LZ4 in uniform
    256 B segments: with canonical=0 any compressible column does; under the
    default writer the catalogue's L = 5 formulas do (byte 4 varies, so no
    canonical parse applies)"""
    i = np.arange(rows, dtype=np.int64)
    if source == "canonical0":
        out = [(i * 2654435761) % 5000, (i * 40503) % 9000,
               (i * 7919) % 300, (i * 104729) % 70000]
        canonical = 0
    else:
        out = [shapes.l5_values(rows, "a"), shapes.l5_values(rows, "b"),
               shapes.l5_values(rows, "a")[::-1].copy(),
               shapes.l5_values(rows, "b")[::-1].copy()]
        canonical = 1
    return [c.astype(np.int64) for c in out[:n_cols]], canonical


def write_fused(path, source, rows, cgrl, n_cols=2):
    columns, canonical = fused_columns(source, rows, n_cols)
    defs = [(f"c{j}", ca.I64, 0) for j in range(n_cols)]
    ca.write_table(path, defs, [c.copy() for c in columns],
                   compression=ca.COMP_LZ4, canonical=canonical,
                   chunk_group_row_limit=cgrl)
    # every chunk generic LZ4 in 256 B segments, the precondition of `fusable`
    for j in range(n_cols):
        got = footer_chunks(path, j)
        want = [(shapes.LZ4, 0x00, math.ceil(min(cgrl, rows - s) * 8 / 256))
                for s in range(0, rows, cgrl)]
        assert got == want, f"column {j}: {got}"
    return [Col(c) for c in columns]


@pytest.mark.parametrize("source", ["canonical0", "l5_default"])
@pytest.mark.parametrize("rows", FUSED_ROWS + (2100,))
def test_fused_kernel_reached(tmp_path, source, rows):
    """one chunk per file at the tile (2048 rows) and lane-segment (32 rows)
    edges, rows % 32 == 1 included (8 B final segment), plus one file of
    three chunk groups (1000, 1000, 100): every integer query shape must run
    the fused decode+filter+aggregate kernel and be exact"""
    cgrl = 1000 if rows == 2100 else max(rows, 1000)
    path = str(tmp_path / "f.cs")
    cols = write_fused(path, source, rows, cgrl)
    cols.append(Col(shapes.key_column(rows)))         # not written, not used
    fus = {X: True, H: True, K: False}
    # stage: <= 4 projected columns, all dense I64 generic LZ4, integer
    # aggregates only -> check_agg_queries asserts last_fused for each query
    check_agg_queries(f"fused {source} {rows}", path, cols, agg_queries(cols), fus,
                      math.ceil(rows / cgrl))


@pytest.mark.parametrize("source", ["canonical0", "l5_default"])
def test_fused_four_projected_columns(tmp_path, source):
    """exactly 4 projected columns is the most the fused kernel takes
    (stage: n_proj > 4 clears `fusable`)"""
    rows = 2049
    path = str(tmp_path / "f4.cs")
    cols = write_fused(path, source, rows, rows, n_cols=4)
    c0 = consts(cols[0])
    preds = [(0, ca.PRED_NE, c0["c"]), (3, ca.PRED_GE, consts(cols[3])["med"])]
    aggs = shapes.with_one(cols, [(ca.AGG_SUM_DISC_TAX_I64, 0, 1, 2), (ca.AGG_SUM_I64, 3),
                                  (ca.AGG_MIN_I64, 2), (ca.AGG_COUNT_STAR, -1)])
    assert projected(preds, aggs) == {0, 1, 2, 3}
    parts, fused, _ = run_agg(path, preds, aggs)
    assert fused
    rowmask = shapes.pass_mask(cols, preds)
    for ai, a in enumerate(aggs):
        shapes.check_partial(parts[ai], shapes.expect_agg(cols, a, rowmask), a[0],
                             f"fused4 {source} agg {ai}")
