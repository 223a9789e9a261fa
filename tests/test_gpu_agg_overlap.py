"""The dense overlapped scan_agg body (multi_agg_kernel_ov, last_agg_path 4).

Every test writes its own small table, reads the footer back (tests/futil.py)
to pin which stream shapes are on disk — so a test cannot silently run the
fallback — asserts Scan.last_agg_path, and compares with exact Python-int
results computed from the numpy arrays that were written.

Three query shapes are run wherever row counts matter, because they are
three instances of the kernel: the TPC-H Q6 shape (specialised, 8 rows per
lane: a wave covers 512 rows, a block 2048), count(*) under one predicate
(specialised, same tiling) and an arbitrary query (the unspecialised
instance, 4 rows per lane: 256 / 1024).
"""
import json
import os

import numpy as np
import pytest

import citus_amd as ca
import futil

pytestmark = pytest.mark.gpu

PATH_NONE, PATH_FUSED, PATH_GENERAL, PATH_DENSE, PATH_OV = 0, 1, 2, 3, 4

LT, LE, GT, GE, EQ, NE = (ca.PRED_LT, ca.PRED_LE, ca.PRED_GT, ca.PRED_GE,
                          ca.PRED_EQ, ca.PRED_NE)
OPS = {LT: np.less, LE: np.less_equal, GT: np.greater, GE: np.greater_equal,
       EQ: np.equal, NE: np.not_equal}

OV_MODES = ({futil.SEGMODE_CONST, futil.SEGMODE_ZR_CONST} |
            {futil.SEGMODE_P_BASE | L for L in (1, 2, 3, 4)} |
            {futil.SEGMODE_ZRP_BASE | L for L in (1, 2, 3, 4)})


# ---------------------------------------------------------------- helpers

def write(path, cols, comp=ca.COMP_LZ4, nulls=None, **kw):
    types = {np.dtype(np.int64): ca.I64, np.dtype(np.float64): ca.F64,
             np.dtype(np.int8): ca.I8}
    defs = [(f"c{i}", types[c.dtype], 0) for i, c in enumerate(cols)]
    ca.write_table(str(path), defs, list(cols), nulls=nulls, compression=comp, **kw)
    return str(path)


def col_modes(path, col):
    """per chunk group, in scan order: the stream mode of the column's single
    segment, or None where the chunk is not a dense one-segment stream"""
    out = []
    for st in futil.read_footer(path)["stripes"]:
        for nd in st["nodes"][col]:
            ok = (nd["n_present"] == nd["row_count"] and nd["n_segs"] == 1 and
                  nd["comp_type"] in (ca.COMP_LZ4, ca.COMP_ZSTD))
            out.append(nd["segs"][0]["mode"] if ok else None)
    return out


def eligible(path, used_cols):
    return all(m in OV_MODES for c in used_cols for m in col_modes(path, c))


def used_columns(preds, aggs):
    cols = {p[0] for p in preds}
    for a in aggs:
        kind = a[0]
        n_ops = {ca.AGG_COUNT_STAR: 0, ca.AGG_SUM_PROD_I64: 2, ca.AGG_SUM_DISC_I64: 2,
                 ca.AGG_SUM_DISC_TAX_I64: 3}.get(kind, 1)
        cols |= set(a[1:1 + n_ops])
    return sorted(cols)


def pass_mask(cols, preds):
    """CNF over the written arrays: or_group 0 = its own conjunct"""
    n = len(cols[0])
    groups = {}
    for i, p in enumerate(preds):
        g = p[3] if len(p) > 3 and p[3] else ("solo", i)
        m = OPS[p[1]](cols[p[0]], p[2])
        groups[g] = groups.get(g, np.zeros(n, dtype=bool)) | m
    out = np.ones(n, dtype=bool)
    for m in groups.values():
        out &= m
    return out


def expected(cols, preds, aggs):
    """[(value or None, count)] in exact Python ints"""
    m = pass_mask(cols, preds)
    cnt = int(m.sum())
    v = [c[m].tolist() for c in cols]          # Python ints / floats
    out = []
    for a in aggs:
        kind = a[0]
        if kind == ca.AGG_COUNT_STAR:
            out.append((cnt, cnt))
            continue
        if cnt == 0:
            out.append((None, 0))
            continue
        x = v[a[1]]
        if kind == ca.AGG_SUM_I64:
            val = sum(x)
        elif kind == ca.AGG_MIN_I64:
            val = min(x)
        elif kind == ca.AGG_MAX_I64:
            val = max(x)
        elif kind == ca.AGG_SUM_PROD_I64:
            val = sum(p * q for p, q in zip(x, v[a[2]]))
        elif kind == ca.AGG_SUM_DISC_I64:
            one = a[4]
            val = sum(p * (one - q) for p, q in zip(x, v[a[2]]))
        elif kind == ca.AGG_SUM_DISC_TAX_I64:
            one = a[4]
            val = sum(p * (one - q) * (one + r) for p, q, r in zip(x, v[a[2]], v[a[3]]))
        elif kind == ca.AGG_SUM_F64:
            val = float(np.sum(np.asarray(x, dtype=np.float64)))
        else:
            raise AssertionError(kind)
        out.append((val, cnt))
    return out


def wrap128(x):
    """what a 128-bit two's complement accumulator holds"""
    x &= (1 << 128) - 1
    return x - (1 << 128) if x >> 127 else x


def check_parts(parts, aggs, exp, what=""):
    for i, (a, (val, cnt)) in enumerate(zip(aggs, exp)):
        p = parts[i]
        tag = f"{what} agg {i} kind {a[0]}"
        assert p.count == cnt, f"{tag}: count {p.count} != {cnt}"
        if a[0] == ca.AGG_COUNT_STAR:
            continue
        if val is None:
            assert p.is_null, f"{tag}: expected NULL"
            continue
        assert not p.is_null, f"{tag}: unexpected NULL"
        if a[0] == ca.AGG_SUM_F64:
            assert p.f64 == pytest.approx(val, rel=1e-12), tag
        else:
            assert p.i128 == wrap128(val), f"{tag}: {p.i128} != {val}"


def run(path, preds, aggs, extra_mask=0):
    """-> (parts, last_agg_path, chunk_groups_filtered)"""
    with ca.Reader(path) as r, \
         r.scan(cols_mask=ca.agg_cols_mask(aggs) | extra_mask, preds=preds) as s:
        s.stage()
        parts = s.agg(aggs)
        return parts, s.last_agg_path, s.chunk_groups_filtered


def check(path, cols, preds, aggs, want_path=None, what=""):
    """run one query, assert the body that ran and the exact result; the
    expected body follows from the on-disk shapes unless given"""
    if want_path is None:
        want_path = PATH_OV if eligible(path, used_columns(preds, aggs)) else PATH_DENSE
    parts, got_path, filt = run(path, preds, aggs)
    assert got_path == want_path, f"{what}: last_agg_path {got_path}, expected {want_path}"
    check_parts(parts, aggs, expected(cols, preds, aggs), what)
    return filt


# the three instances --------------------------------------------------

def q6_query(a_lo, a_hi, b_lo, b_hi, c_hi):
    """TPC-H Q6 over columns A=0, B=1, C=2, D=3: the specialised instance"""
    preds = [(0, GE, a_lo), (0, LT, a_hi), (1, GE, b_lo), (1, LE, b_hi), (2, LT, c_hi)]
    aggs = [(ca.AGG_SUM_PROD_I64, 3, 1), (ca.AGG_COUNT_STAR, -1)]
    return preds, aggs


def any_query(a_lo, a_hi):
    """same rows through the unspecialised instance (4 aggregates)"""
    preds = [(0, GE, a_lo), (0, LT, a_hi)]
    aggs = [(ca.AGG_SUM_I64, 3), (ca.AGG_COUNT_STAR, -1),
            (ca.AGG_MIN_I64, 1), (ca.AGG_MAX_I64, 3)]
    return preds, aggs


def count_query(a_lo):
    return [(0, GE, a_lo)], [(ca.AGG_COUNT_STAR, -1)]


def edge_table(n, rng):
    """A = base + 2*i: strictly increasing with a gap after every value, so
    'one row' and 'no row inside [min, max]' are both expressible and never
    refuted by min/max pruning. B, C, D vary in their low 1, 2 and 3 bytes."""
    A = (1 << 20) + 2 * np.arange(n, dtype=np.int64)
    B = rng.integers(0, 200, n, dtype=np.int64)
    C = 70000 + rng.integers(0, 60000, n, dtype=np.int64)
    D = (5 << 40) + rng.integers(0, 1 << 23, n, dtype=np.int64)
    return [A, B, C, D]


# ---------------------------------------------------------------- tests

EDGE_N = [3, 7, 8, 9, 15, 16, 17, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025,
          2047, 2048, 2049, 4095, 4096, 4097]


@pytest.mark.parametrize("n", EDGE_N)
def test_row_count_edges(tmp_path, n):
    """single chunk group of n rows: rows 0/1 of the stream, the R-row edge,
    one wave, one block, and the old 4096-row tile — all rows, no row, only
    the first, only the last row passing"""
    rng = np.random.default_rng(n)
    cols = edge_table(n, rng)
    path = write(tmp_path / "t.cs", cols, chunk_group_row_limit=10000)
    A = cols[0]
    first, last = int(A[0]), int(A[-1])
    ranges = {"all": (first, last + 1), "none": (first + 1, first + 2),
              "first": (first, first + 1), "last": (last, last + 1)}
    if n >= 8:
        # from 8 rows on every column must be canonical: the fallback may
        # not stand in for the body under test
        assert eligible(path, [0, 1, 2, 3])
    for name, (lo, hi) in ranges.items():
        p, a = q6_query(lo, hi, -5, 1000, 1 << 40)
        assert check(path, cols, p, a, what=f"n={n} {name} q6") == 0
        p, a = any_query(lo, hi)
        check(path, cols, p, a, what=f"n={n} {name} any")
    for lo in (first, last, first + 1):
        p, a = count_query(lo)
        check(path, cols, p, a, what=f"n={n} count>={lo}")


def big_table(n, rng):
    A = 8000 + rng.integers(0, 2500, n, dtype=np.int64)          # L=2
    B = rng.integers(0, 11, n, dtype=np.int64)                   # L=1
    C = rng.integers(1, 51, n, dtype=np.int64) * 100             # L=2
    D = rng.integers(90000, 10500000, n, dtype=np.int64)         # L=3
    return [A, B, C, D]


Q6ISH = q6_query(8766, 9131, 5, 7, 2400)


@pytest.mark.parametrize("cgrl,n", [(40, 200_017), (1000, 25_017), (10000, 25_017)])
def test_multi_item_walk(tmp_path, cgrl, n):
    """more work items than the grid has blocks (limit 40), ragged last
    groups, several tiles per group (limit 10000)"""
    rng = np.random.default_rng(cgrl)
    cols = big_table(n, rng)
    path = write(tmp_path / "t.cs", cols, chunk_group_row_limit=cgrl,
                 stripe_row_limit=max(cgrl * 7, 20000))
    assert eligible(path, [0, 1, 2, 3])
    assert len(col_modes(path, 0)) >= n // cgrl
    check(path, cols, *Q6ISH, want_path=PATH_OV, what="q6")
    check(path, cols, *any_query(8766, 9131), want_path=PATH_OV, what="any")
    check(path, cols, *count_query(9000), want_path=PATH_OV, what="count")


@pytest.mark.parametrize("comp", [ca.COMP_LZ4, ca.COMP_ZSTD], ids=["lz4", "zstd"])
def test_multi_item_walk_two_tiles(tmp_path, comp):
    """both load forms (lz4: lane-contiguous, zstd: per-lane windows) with a
    block walking several work items, so that the words loaded one trip ahead
    and the rotate at the loop's end are what the next trip reads: 520 chunk
    groups of 2049 rows (two tiles at R = 8, three at R = 4, the last holding
    one row) and a last group of 9 rows, the shortest the writer stores
    canonically in every case. 1042 / 1563 work items against a fixed grid of
    four blocks per CU (1024 on 256 CUs)."""
    cg, n_full, tail = 2049, 520, 9
    n = cg * n_full + tail
    rng = np.random.default_rng(21)
    cols = big_table(n, rng)
    path = write(tmp_path / "t.cs", cols, comp=comp, chunk_group_row_limit=cg,
                 stripe_row_limit=64 * cg)
    assert eligible(path, [0, 1, 2, 3])
    P = futil.SEGMODE_ZRP_BASE if comp == ca.COMP_ZSTD else futil.SEGMODE_P_BASE
    assert {m & ~0xF for m in col_modes(path, 0)} == {P}
    assert len(col_modes(path, 0)) == n_full + 1
    check(path, cols, *Q6ISH, want_path=PATH_OV, what="q6")
    check(path, cols, *any_query(8766, 9131), want_path=PATH_OV, what="any")
    check(path, cols, *count_query(9000), want_path=PATH_OV, what="count")


@pytest.mark.parametrize("where", ["leading", "middle", "trailing"])
def test_pruned_groups(tmp_path, where):
    """chunk groups removed by min/max pruning before the kernel runs"""
    n, cgrl = 30_000, 1000
    rng = np.random.default_rng(7)
    cols = big_table(n, rng)
    A = np.sort(cols[0])                       # clustered: groups prune
    cols[0] = A
    path = write(tmp_path / "t.cs", cols, chunk_group_row_limit=cgrl,
                 stripe_row_limit=7000)
    lo, hi = {"leading": (int(A[12_500]), int(A[-1]) + 1),
              "middle": (int(A[0]), int(A[-1]) + 1),
              "trailing": (int(A[0]), int(A[17_500]))}[where]
    preds, aggs = q6_query(lo, hi, 0, 10, 1 << 30)
    if where == "middle":                      # A outside the middle third
        preds = [(0, LT, int(A[10_000]), 1), (0, GT, int(A[20_000]), 1),
                 (1, GE, 0), (1, LE, 10), (2, LT, 1 << 30)]
    assert eligible(path, [0, 1, 2, 3])
    filt = check(path, cols, preds, aggs, want_path=PATH_OV, what=where)
    assert 5 <= filt <= 13, f"{where}: {filt} chunk groups filtered"


def test_three_shards(tmp_path):
    """a directory of 3 shard files scanned as one table (ragged last group
    in every shard), and the per-shard partials combined"""
    rng = np.random.default_rng(11)
    n = 9_037
    shards, parts_list = [], []
    preds, aggs = Q6ISH
    d = tmp_path / "table"
    d.mkdir()
    for k in range(3):
        cols = big_table(n + k, rng)
        path = write(d / f"shard{k:02d}.cs", cols, chunk_group_row_limit=1000)
        assert eligible(path, [0, 1, 2, 3])
        parts, agg_path, _ = run(path, preds, aggs)
        assert agg_path == PATH_OV
        shards.append(cols)
        parts_list.append(parts)
    whole = [np.concatenate([s[i] for s in shards]) for i in range(4)]
    exp = expected(whole, preds, aggs)
    check_parts(ca.combine(aggs, parts_list), aggs, exp, "combined")
    parts, agg_path, _ = run(str(d), preds, aggs)
    assert agg_path == PATH_OV
    check_parts(parts, aggs, exp, "directory")


def ranged(n, rng, L, base):
    """values whose low L bytes vary and whose high bytes are base's"""
    v = base + rng.integers(0, 1 << (8 * L), n, dtype=np.int64)
    v[0], v[1] = base, base + (1 << (8 * L)) - 1      # force exactly L
    return v


@pytest.mark.parametrize("comp", [ca.COMP_LZ4, ca.COMP_ZSTD])
def test_every_stream_shape(tmp_path, comp):
    """L = 1..4 per column in one query, CONST as predicate column and as
    operand, for lz4 and zstd canonical streams"""
    n, cgrl = 5_037, 1000
    rng = np.random.default_rng(3)
    zr = comp == ca.COMP_ZSTD
    P, K = (futil.SEGMODE_ZRP_BASE, futil.SEGMODE_ZR_CONST) if zr else \
           (futil.SEGMODE_P_BASE, futil.SEGMODE_CONST)
    cols = [ranged(n, rng, 1, 3 << 8), ranged(n, rng, 2, -(5 << 16)),
            ranged(n, rng, 3, 9 << 24), ranged(n, rng, 4, -(1 << 32)),
            np.full(n, 77, dtype=np.int64)]
    path = write(tmp_path / "t.cs", cols, comp=comp, chunk_group_row_limit=cgrl)
    for c, L in enumerate((1, 2, 3, 4)):
        assert set(col_modes(path, c)) <= {P | l for l in range(1, L + 1)}
        assert col_modes(path, c)[0] == P | L
    assert set(col_modes(path, 4)) == {K}
    # four P(L) slots, different L per column
    preds = [(0, GE, (3 << 8) + 40), (1, LT, -(5 << 16) + 50000), (3, NE, -(1 << 32) + 5)]
    aggs = [(ca.AGG_SUM_PROD_I64, 2, 3), (ca.AGG_MIN_I64, 1), (ca.AGG_MAX_I64, 0),
            (ca.AGG_SUM_I64, 3)]
    check(path, cols, preds, aggs, want_path=PATH_OV, what="L1234")
    # CONST as a predicate column and as an operand; a predicate that is
    # false on a constant is always refuted by min/max, so that scan is empty
    check(path, cols, [(4, EQ, 77), (2, GT, (9 << 24) + 1000)],
          [(ca.AGG_SUM_PROD_I64, 4, 2), (ca.AGG_SUM_I64, 4), (ca.AGG_COUNT_STAR, -1)],
          want_path=PATH_OV, what="const")
    check(path, cols, [(4, NE, 77), (0, GE, 0)], [(ca.AGG_SUM_I64, 4)],
          want_path=PATH_NONE, what="const false")
    check(path, cols, [(4, GE, 70)], [(ca.AGG_COUNT_STAR, -1)],
          want_path=PATH_OV, what="const count")


@pytest.mark.parametrize("comp", [ca.COMP_LZ4, ca.COMP_ZSTD])
def test_L_changes_between_groups(tmp_path, comp):
    """one column whose L differs from chunk group to chunk group, CONST
    groups included"""
    cgrl = 1000
    rng = np.random.default_rng(5)
    base = 1 << 36
    pieces = [ranged(cgrl, rng, L, base) for L in (1, 3, 2, 4, 1)]
    pieces.insert(2, np.full(cgrl, base + 9, dtype=np.int64))
    pieces.append(ranged(337, rng, 2, base))
    X = np.concatenate(pieces)
    Y = -5000 + rng.integers(0, 2000, len(X), dtype=np.int64)
    cols = [X, Y]
    path = write(tmp_path / "t.cs", cols, comp=comp, chunk_group_row_limit=cgrl)
    assert eligible(path, [0, 1])
    low = [m & 0xF for m in col_modes(path, 0)]
    assert [m >> 4 for m in col_modes(path, 0)].count(2 if comp == ca.COMP_LZ4 else 7) == 1
    assert {1, 2, 3, 4} <= set(low)
    check(path, cols, [(0, GE, base + 100), (1, LT, -4500)],
          [(ca.AGG_SUM_PROD_I64, 0, 1), (ca.AGG_MAX_I64, 0), (ca.AGG_COUNT_STAR, -1)],
          want_path=PATH_OV, what="mixed L")
    check(path, cols, [(0, GE, base + 100)], [(ca.AGG_COUNT_STAR, -1)],
          want_path=PATH_OV, what="mixed L count")


def test_slot_deduplication(tmp_path):
    """a column named many times is one slot: predicate column that is also
    proj_a, proj_b and proj_c; operands shared between aggregates; five
    predicates on one column; OR groups spanning two columns"""
    n = 6_037
    rng = np.random.default_rng(9)
    X = rng.integers(1, 120, n, dtype=np.int64)
    Y = 1000 + rng.integers(0, 3000, n, dtype=np.int64)
    Z = (1 << 33) + rng.integers(0, 100000, n, dtype=np.int64)
    cols = [X, Y, Z]
    path = write(tmp_path / "t.cs", cols, chunk_group_row_limit=1000)
    assert eligible(path, [0, 1, 2])
    one = 100
    check(path, cols, [(0, GT, 10), (0, LT, 90)],
          [(ca.AGG_SUM_DISC_TAX_I64, 0, 0, 0, one), (ca.AGG_SUM_PROD_I64, 0, 0),
           (ca.AGG_SUM_DISC_I64, 1, 0, -1, one), (ca.AGG_MIN_I64, 0)],
          want_path=PATH_OV, what="pred col as a, b, c")
    check(path, cols, [(1, GE, 1500)],
          [(ca.AGG_SUM_I64, 2), (ca.AGG_MIN_I64, 2), (ca.AGG_MAX_I64, 2),
           (ca.AGG_SUM_PROD_I64, 2, 1)],
          want_path=PATH_OV, what="shared operand")
    check(path, cols, [(0, GT, 5), (0, LT, 110), (0, NE, 50), (0, GE, 7), (0, LE, 100)],
          [(ca.AGG_SUM_I64, 1), (ca.AGG_COUNT_STAR, -1)],
          want_path=PATH_OV, what="five preds one column")
    check(path, cols, [(0, LT, 20, 1), (1, GT, 3500, 1), (2, GE, (1 << 33) + 50000, 2), (0, EQ, 60, 2),
                       (1, NE, 1234)],
          [(ca.AGG_SUM_PROD_I64, 2, 0), (ca.AGG_COUNT_STAR, -1)],
          want_path=PATH_OV, what="OR groups over two columns")


def test_128_bit_carries(tmp_path):
    """products near +-2^80 and +-2^100: the low half wraps many times, in
    both directions"""
    n = 4_099
    rng = np.random.default_rng(13)
    sign = np.where(rng.integers(0, 2, n) == 1, 1, -1).astype(np.int64)
    # per column the high bytes are shared within a sign, so each sign gets
    # its own column pair: values near +2^40 and near -2^40
    Pp = (1 << 40) + rng.integers(0, 1 << 30, n, dtype=np.int64)
    Pn = -(1 << 40) + rng.integers(0, 1 << 30, n, dtype=np.int64)
    Q = (1 << 40) - rng.integers(1, 1 << 24, n, dtype=np.int64)
    T = rng.integers(0, 9, n, dtype=np.int64)
    cols = [Pp, Pn, Q, T, sign]
    path = write(tmp_path / "t.cs", cols, chunk_group_row_limit=1000)
    assert eligible(path, [0, 1, 2, 3])
    one = 1 << 20
    aggs = [(ca.AGG_SUM_PROD_I64, 0, 2), (ca.AGG_SUM_PROD_I64, 1, 2),
            (ca.AGG_SUM_DISC_TAX_I64, 1, 2, 3, one), (ca.AGG_SUM_DISC_TAX_I64, 0, 1, 2, one)]
    exp = expected(cols, [(3, GE, 0)], aggs)
    assert abs(exp[0][0]) > 1 << 90 and exp[1][0] < -(1 << 90)
    check(path, cols, [(3, GE, 0)], aggs, want_path=PATH_OV, what="carries")
    check(path, cols, [(3, GE, 3), (3, LE, 5)], aggs, want_path=PATH_OV, what="carries sel")


def fallback_table(n, rng):
    X = 500 + rng.integers(0, 100, n, dtype=np.int64)
    Y = rng.integers(0, 1 << 20, n, dtype=np.int64)
    F = rng.random(n)
    return [X, Y, F]


FB_PREDS = [(0, GE, 520)]
FB_AGGS = [(ca.AGG_SUM_PROD_I64, 1, 0), (ca.AGG_COUNT_STAR, -1)]


def test_fallback_null(tmp_path):
    """one NULL in one chunk group of a referenced column: general body"""
    n = 5_000
    cols = fallback_table(n, np.random.default_rng(1))
    nulls = [None, np.zeros(n, dtype=np.uint8), None]
    nulls[1][2_345] = 1
    path = write(tmp_path / "t.cs", cols, nulls=nulls, chunk_group_row_limit=1000)
    assert col_modes(path, 1).count(None) == 1
    parts, agg_path, _ = run(path, FB_PREDS, FB_AGGS)
    assert agg_path == PATH_GENERAL
    keep = [np.delete(c, 2_345) for c in cols]      # a NULL operand drops the row...
    exp = expected(keep, FB_PREDS, FB_AGGS)
    exp[1] = expected(cols, FB_PREDS, FB_AGGS)[1]   # ...from the sum, not count(*)
    assert parts[0].i128 == exp[0][0] and parts[1].count == exp[1][1]
    # the same table through a column the NULL is not in: still not eligible
    # as a scan (it is not all-dense), and still exact
    parts, agg_path, _ = run(path, FB_PREDS, [(ca.AGG_SUM_I64, 0)], extra_mask=2)
    assert agg_path == PATH_GENERAL
    check_parts(parts, [(ca.AGG_SUM_I64, 0)], expected(cols, FB_PREDS, [(ca.AGG_SUM_I64, 0)]))


def test_fallback_high_entropy_chunk(tmp_path):
    """one chunk group whose values vary in more than 4 bytes: the writer
    stores it generic or raw, the scan takes the windowed body"""
    n = 5_000
    rng = np.random.default_rng(2)
    cols = fallback_table(n, rng)
    cols[1][3_000:4_000] = rng.integers(0, 1 << 62, 1000, dtype=np.int64)
    path = write(tmp_path / "t.cs", cols, chunk_group_row_limit=1000)
    modes = col_modes(path, 1)
    assert [m in OV_MODES for m in modes] == [True, True, True, False, True]
    check(path, cols, FB_PREDS, FB_AGGS, want_path=PATH_DENSE, what="entropy")
    # a query that does not touch that column is eligible on the same file
    check(path, cols, FB_PREDS, [(ca.AGG_SUM_I64, 0)], want_path=PATH_OV, what="other col")


def test_fallback_non_canonical(tmp_path):
    n = 5_000
    cols = fallback_table(n, np.random.default_rng(4))
    path = write(tmp_path / "t.cs", cols, chunk_group_row_limit=1000, canonical=0)
    assert not eligible(path, [0, 1])
    parts, agg_path, _ = run(path, FB_PREDS, FB_AGGS)
    assert agg_path in (PATH_FUSED, PATH_DENSE)
    check_parts(parts, FB_AGGS, expected(cols, FB_PREDS, FB_AGGS))


def test_fallback_float(tmp_path):
    """an F64 predicate, and SUM_F64, keep the windowed body"""
    n = 5_000
    cols = fallback_table(n, np.random.default_rng(6))
    path = write(tmp_path / "t.cs", cols, chunk_group_row_limit=1000)
    assert eligible(path, [0, 1])
    preds = FB_PREDS + [(2, LT, 0.5)]
    parts, agg_path, _ = run(path, preds, FB_AGGS)
    assert agg_path == PATH_DENSE
    check_parts(parts, FB_AGGS, expected(cols, preds, FB_AGGS))
    aggs = [(ca.AGG_SUM_I64, 1), (ca.AGG_SUM_F64, 2)]
    parts, agg_path, _ = run(path, FB_PREDS, aggs)
    assert agg_path == PATH_DENSE
    check_parts(parts, aggs, expected(cols, FB_PREDS, aggs))


def test_repeatable(tmp_path):
    """the same agg three times, interleaved with agg_grouped, on one scan"""
    n = 20_037
    rng = np.random.default_rng(8)
    cols = big_table(n, rng) + [rng.integers(0, 5, n).astype(np.int8)]
    path = write(tmp_path / "t.cs", cols, chunk_group_row_limit=1000)
    assert eligible(path, [0, 1, 2, 3])
    preds, aggs = Q6ISH
    exp = expected(cols, preds, aggs)
    seen = []
    with ca.Reader(path) as r, r.scan(cols_mask=0x1F, preds=preds) as s:
        s.stage()
        for _ in range(3):
            parts = s.agg(aggs)
            assert s.last_agg_path == PATH_OV
            check_parts(parts, aggs, exp)
            seen.append([(p.i128, p.count) for p in parts])
            grouped = s.agg_grouped(aggs, (4,))
            assert sum(g[1].count for g in grouped.values()) == exp[1][1]
            assert sum(g[0].i128 for g in grouped.values() if not g[0].is_null) == exp[0][0]
    assert seen[0] == seen[1] == seen[2]


@pytest.mark.parametrize("variant", ["none", "lz4", "zstd"])
def test_golden_q6(variant):
    here = os.path.dirname(os.path.abspath(__file__))
    exp = json.load(open(os.path.join(here, "golden", "expected.json")))["q6"]
    path = os.path.join(here, "golden", f"lineitem12k_{variant}.cs")
    preds = [(5, GE, exp["shipdate_ge"]), (5, LT, exp["shipdate_lt"]),
             (3, GE, 5), (3, LE, 7), (1, LT, 2400)]
    aggs = [(ca.AGG_SUM_PROD_I64, 2, 3), (ca.AGG_COUNT_STAR, -1)]
    parts, agg_path, _ = run(path, preds, aggs)
    want = PATH_OV if eligible(path, [1, 2, 3, 5]) else None
    if want is not None:
        assert agg_path == want
    else:
        assert agg_path in (PATH_FUSED, PATH_GENERAL, PATH_DENSE)
    assert parts[0].i128 == exp["revenue_scale4"]
