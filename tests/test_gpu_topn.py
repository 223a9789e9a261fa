"""
GPU tests (@pytest.mark.gpu) for cstripe_scan_select_topn — device ORDER BY
... LIMIT over a scan (topn_key / topn_hist / topn_pick / topn_refine /
topn_final / topn_keygather / topn_permute kernels around the select ones).

Expectations always come from numpy over the arrays the test itself wrote:
np.lexsort with the row number as the last tie-break; never from the
library. Values are copied, not computed, so every comparison is bit-exact
(floats are compared as bit patterns).
"""
import ctypes as C

import numpy as np
import pytest

import citus_amd as ca

pytestmark = pytest.mark.gpu

BITS = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


@pytest.fixture(scope="module", autouse=True)
def require_gpu():
    assert ca.gpu_available(), "MI355X required for these tests"


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(BITS[a.dtype.itemsize])


def dense_rank(v):
    """ascending ranks with ties equal: ints signed, floats in PG order (NaN
    greatest and equal to itself, -0.0 = +0.0), lists of bytes by memcmp"""
    if isinstance(v, list):
        u = {b: i for i, b in enumerate(sorted(set(x for x in v if x is not None)))}
        return np.array([0 if x is None else u[x] for x in v], dtype=np.int64)
    v = np.asarray(v)
    if v.dtype.kind == "f":
        f = v.astype(np.float64)        # exact for float32
        nan = np.isnan(f)
        u = np.unique(f[~nan])          # -0.0 == 0.0 dedups to one entry
        rank = np.searchsorted(u, np.where(nan, 0.0, f)).astype(np.int64)
        rank[nan] = len(u)
        return rank
    u = np.unique(v)
    return np.searchsorted(u, v).astype(np.int64)


def np_topn(order, limit, mask, columns, nulls=None):
    """row indices of ORDER BY order LIMIT limit over the rows in mask:
    order = [(col, desc, nulls_first)]; ties by ascending row number"""
    nulls = nulls or {}
    n = len(mask)
    keys = [np.arange(n)]                       # least significant
    for c, desc, first in reversed(order):
        isnull = nulls[c].astype(bool) if nulls.get(c) is not None else np.zeros(n, bool)
        rank = dense_rank(columns[c])
        if desc:
            rank = -rank
        rank = np.where(isnull, 0, rank)
        keys.append(rank)
        keys.append(np.where(isnull, 0, 1) if first else isnull.astype(np.int64))
    idx = np.lexsort(keys)
    idx = idx[mask[idx]]
    return idx[:limit]


def check(res, idx, columns, nulls=None, row_numbers=None):
    """res = select_topn() output; idx = expected row indices in final order;
    row_numbers = table-wide numbers of those rows (default: idx itself)"""
    nulls = nulls or {}
    assert res["n_rows"] == len(idx)
    if res["row_numbers"] is not None:
        np.testing.assert_array_equal(
            res["row_numbers"], idx if row_numbers is None else row_numbers)
    for c, got in res["values"].items():
        full = columns[c]
        if isinstance(full, list):
            continue                    # VARTEXT ranks: checked through text
        assert got.dtype == full.dtype and len(got) == len(idx)
        exp = full[idx].copy()
        expn = np.zeros(len(idx), dtype=np.uint8)
        if nulls.get(c) is not None:
            expn = nulls[c][idx]
            exp[expn == 1] = 0          # NULL slots are zero-filled
        np.testing.assert_array_equal(bits(got), bits(exp), err_msg=f"col {c}")
        if res["nulls"]:
            np.testing.assert_array_equal(res["nulls"][c], expn, err_msg=f"nulls {c}")


class Tab:
    """one written table and one staged scan over it"""

    def __init__(self, path, defs, columns, nulls=None, preds=(), cols_mask=None, **opt):
        self.columns = dict(enumerate(columns))
        self.nulls = dict(enumerate(nulls)) if nulls else {}
        ca.write_table(path, defs, list(columns), nulls=nulls,
                       compression=opt.pop("compression", ca.COMP_LZ4), **opt)
        self.n = len(columns[0])
        self.reader = ca.Reader(path)
        mask = (1 << len(defs)) - 1 if cols_mask is None else cols_mask
        self.scan = self.reader.scan(cols_mask=mask, preds=list(preds))
        self.scan.stage()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.scan.end()
        self.reader.close()

    def topn(self, order, limit, mask=None, **kw):
        """run select_topn and check it against numpy"""
        res = self.scan.select_topn(order, limit, **kw)
        mask = np.ones(self.n, bool) if mask is None else mask
        idx = np_topn(ca.parse_order(order), limit, mask, self.columns, self.nulls)
        check(res, idx, self.columns, self.nulls)
        return res, idx


KV = [("k", ca.I64, 0), ("v", ca.I64, 0)]


# ---------------- slice, tile and chunk-group edges ----------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4096, 4097, 10001, 25017])
def test_edges(tmp_path, n):
    rng = np.random.default_rng(100 + n)
    k = rng.integers(-2**40, 2**40, n).astype(np.int64)
    v = rng.integers(-2**62, 2**62, n).astype(np.int64)
    with Tab(str(tmp_path / "e.cs"), KV, [k, v]) as t:
        for limit in sorted({1, 2, 64, n - 1, n, n + 5}):
            if limit < 1:
                continue
            res, idx = t.topn([0], limit)
            assert res["n_rows"] == min(limit, n) == len(idx)
            assert len(res["values"][1]) == min(limit, n)


# ---------------- ties decide everything ----------------

def test_all_keys_equal_returns_first_rows(tmp_path):
    n = 25017
    k = np.full(n, 77, dtype=np.int64)
    v = np.arange(n, dtype=np.int64) * 3 - 5
    with Tab(str(tmp_path / "eq.cs"), KV, [k, v]) as t:
        # mid slice, tile boundary, chunk-group boundary, last partial chunk
        for limit in (1, 100, 4096, 4097, 10000, 20001, 25000, n):
            for order in ([0], [(0, "desc")]):
                res, idx = t.topn(order, limit)
                np.testing.assert_array_equal(idx, np.arange(limit))
                np.testing.assert_array_equal(res["row_numbers"], np.arange(limit))


def test_cut_inside_a_tie_run(tmp_path):
    n = 25017
    rng = np.random.default_rng(7)
    k = rng.integers(0, 3, n).astype(np.int64)
    v = rng.integers(-2**50, 2**50, n).astype(np.int64)
    with Tab(str(tmp_path / "tie.cs"), KV, [k, v], chunk_group_row_limit=1000,
             stripe_row_limit=3000) as t:
        zeros = int((k == 0).sum())
        # the limit-th row is the last 1 before row R: mid 64-row slice, a
        # 4096 multiple, a chunk-group (= tile) boundary, a stripe boundary,
        # the last partial chunk
        for R in (12345 + 37 - 12345 % 64, 4096, 7000, 9000, 25010):
            limit = zeros + int((k[:R] == 1).sum())
            res, idx = t.topn([0], limit)
            assert (k[idx[zeros:]] == 1).all() and idx[zeros:].max() < R
            res, idx = t.topn([0], limit + 1)
            assert k[idx[-1]] == 2 or idx[-1] >= R
        # descending: the cut falls inside the run of 1s from the other side
        twos = int((k == 2).sum())
        t.topn([(0, "desc")], twos + int((k[:7000] == 1).sum()))


# ---------------- every radix digit ----------------

@pytest.mark.parametrize("shape", ["low_byte", "high_byte", "every_byte", "bits64"])
def test_radix_digits(tmp_path, shape):
    n = 10001
    rng = np.random.default_rng(21)
    if shape == "low_byte":
        k = (5 * 2**40 + rng.integers(0, 256, n)).astype(np.int64)
    elif shape == "high_byte":
        k = (rng.integers(0, 201, n) << 24).astype(np.int64)    # 32-bit span
    elif shape == "every_byte":
        k = rng.integers(-2**61, 2**61, n).astype(np.int64)
    else:
        # span 2^63, + 1 NULL code: exactly 64 bits
        k = rng.integers(-2**62, 2**62, n).astype(np.int64)
        k[17] = -2**62
        k[n - 3] = 2**62
    v = np.arange(n, dtype=np.int64)
    with Tab(str(tmp_path / "rx.cs"), KV, [k, v]) as t:
        for limit in (1, 37, 5000, n - 1):
            t.topn([0], limit)
            t.topn([(0, "desc", "last")], limit)
            t.topn([(0, "asc", "first")], limit)


def test_full_range_i64_needs_65_bits(tmp_path):
    n = 5000
    k = np.random.default_rng(22).integers(-2**62, 2**62, n).astype(np.int64)
    k[5] = np.iinfo(np.int64).min
    k[4000] = np.iinfo(np.int64).max
    with Tab(str(tmp_path / "w.cs"), KV, [k, np.arange(n, dtype=np.int64)]) as t:
        with pytest.raises(ca.CStripeError, match=r"rc=-5.*65 bits"):
            t.scan.select_topn([0], 10)
        # ... and the scan still answers other calls
        assert t.scan.select_count() == n


# ---------------- direction and NULLs ----------------

@pytest.fixture(scope="module")
def null_tab(tmp_path_factory):
    n = 9001
    rng = np.random.default_rng(31)
    k = rng.integers(-50, 50, n).astype(np.int64)
    nk = (rng.random(n) < 0.3).astype(np.uint8)
    nk[2000:3000] = 1                                   # an all-NULL chunk group
    v = rng.integers(-2**40, 2**40, n).astype(np.int64)
    nv = (rng.random(n) < 0.2).astype(np.uint8)
    z = np.zeros(n, dtype=np.int32)                     # an only-NULL column
    nz = np.ones(n, dtype=np.uint8)
    path = str(tmp_path_factory.mktemp("topn_nulls") / "nulls.cs")
    with Tab(path, [("k", ca.I64, 0), ("v", ca.I64, 0), ("z", ca.I32, 0)],
             [k, v, z], nulls=[nk, nv, nz], chunk_group_row_limit=1000) as t:
        yield t


@pytest.mark.parametrize("nulls", ["first", "last"])
@pytest.mark.parametrize("direction", ["asc", "desc"])
def test_direction_and_nulls(null_tab, direction, nulls):
    t = null_tab
    non_null = int((t.nulls[0] == 0).sum())
    for limit in (1, 50, 1500, non_null - 1, non_null, non_null + 1,
                  non_null + 700, t.n):
        res, idx = t.topn([(0, direction, nulls)], limit)
        got_nulls = int(res["nulls"][0].sum())
        if nulls == "first":
            assert got_nulls == min(limit, t.n - non_null)
        else:
            assert got_nulls == max(0, limit - non_null)


def test_pg_default_null_placement(null_tab):
    t = null_tab
    res, _ = t.topn([(0, "asc")], 10)
    assert not res["nulls"][0].any()
    res, _ = t.topn([(0, "desc")], 10)
    assert res["nulls"][0].all()


def test_only_null_column(null_tab):
    t = null_tab
    for order in ([2], [(2, "desc")], [(2, "asc", "first")]):
        res, idx = t.topn(order, 300)
        np.testing.assert_array_equal(idx, np.arange(300))
        assert res["nulls"][2].all() and not res["values"][2].any()
    # as a leading column it decides nothing: the second column orders
    t.topn([(2, "desc"), (0, "asc", "last")], 1234)


# ---------------- types ----------------

def test_integer_tuples_mixed_directions(tmp_path):
    n = 12001
    rng = np.random.default_rng(41)
    c8 = rng.integers(-128, 128, n).astype(np.int8)
    c16 = rng.integers(-300, 300, n).astype(np.int16)
    c32 = rng.integers(-3, 4, n).astype(np.int32)
    c64 = rng.integers(-2**33, 2**33, n).astype(np.int64)
    n16 = (rng.random(n) < 0.1).astype(np.uint8)
    defs = [("a", ca.I8, 0), ("b", ca.I16, 0), ("c", ca.I32, 0), ("d", ca.I64, 0)]
    with Tab(str(tmp_path / "ints.cs"), defs, [c8, c16, c32, c64],
             nulls=[None, n16, None, None], chunk_group_row_limit=5000) as t:
        for order in ([(2, "asc"), (0, "desc")],
                      [(0, "desc"), (1, "asc", "first"), (3, "desc")],
                      [(2, "desc"), (1, "desc"), (0, "asc"), (3, "asc")],
                      [(1, "asc"), (2, "asc")],
                      [(3, "desc")]):
            for limit in (1, 777, 6000):
                t.topn(order, limit)


SPECIALS = [np.nan, np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324, 2.5e-310,
            1.0, -1.0]


@pytest.mark.parametrize("ftype", [ca.F64, ca.F32])
def test_float_pg_order(tmp_path, ftype):
    n = 8200
    rng = np.random.default_rng(43)
    f = rng.normal(size=n)
    pick = rng.random(n) < 0.5
    f[pick] = rng.choice(SPECIALS, int(pick.sum()))
    # a NaN with a payload and the sign bit set still equals every NaN
    f[11] = np.frombuffer(np.uint64(0xFFF8000000000123).tobytes(), np.float64)[0]
    if ftype == ca.F32:
        f = f.astype(np.float32)        # f64 denormals flush to +-0.0 here
        f[13], f[14] = np.float32(1e-45), np.float32(-1e-45)
    nf = (rng.random(n) < 0.1).astype(np.uint8)
    v = np.arange(n, dtype=np.int64)
    defs = [("f", ftype, 0), ("v", ca.I64, 0)]
    with Tab(str(tmp_path / "fl.cs"), defs, [f, v], nulls=[nf, None],
             chunk_group_row_limit=3000) as t:
        for order in ([0], [(0, "desc")], [(0, "desc", "last")], [(0, "asc", "first")]):
            for limit in (1, 100, 4000, n):
                t.topn(order, limit)


WORDS = [b"", b"a", b"ab", b"abc", b"b", b"\x7f", b"\x80", b"\xff\xfe",
         b"x" * 126, b"x" * 127, b"x" * 200, b"x" * 199 + b"y", b"zebra"]


def test_vartext_key_and_i32_twin(tmp_path):
    n = 6001
    rng = np.random.default_rng(47)
    pick = rng.integers(0, len(WORDS), n)
    words = [WORDS[i] for i in pick]
    for i in np.flatnonzero(rng.random(n) < 0.1):
        words[i] = None
    nt = np.array([1 if w is None else 0 for w in words], np.uint8)
    rank = dense_rank(words).astype(np.int32)
    v = rng.integers(0, 5, n).astype(np.int64)
    defs = [("t", ca.VARTEXT, 0), ("r", ca.I32, 0), ("v", ca.I64, 0)]
    path = str(tmp_path / "vt.cs")
    with Tab(path, defs, [list(words), rank, v], nulls=[None, nt, None],
             chunk_group_row_limit=2000) as t:
        t.columns[0] = words
        t.nulls[0] = nt
        for dirn, nulls in (("asc", "last"), ("desc", "first"), ("desc", "last"),
                            ("asc", "first")):
            for limit in (1, 250, 3000, n):
                res, idx = t.topn([(2, "asc"), (0, dirn, nulls)], limit,
                                  decode_text=True)
                twin = t.scan.select_topn([(2, "asc"), (1, dirn, nulls)], limit)
                np.testing.assert_array_equal(res["row_numbers"], twin["row_numbers"])
                assert res["text"][0].tolist() == [words[i] for i in idx]
                assert res["text_cols"] == [0]
        # single text key: memcmp order, the empty string first, NULL last
        res, idx = t.topn([0], n, decode_text=True)
        seen = [w for w in res["text"][0].tolist() if w is not None]
        assert seen == sorted(seen) and seen[0] == b"" and len(seen[-1]) < 200
        assert max(len(w) for w in seen) == 200


# ---------------- predicates and pruning ----------------

def test_pruned_chunks_and_row_numbers(tmp_path):
    n = 12345
    p = np.arange(n, dtype=np.int64)
    v = (p * 7919) % 100003
    # (p>=1500 AND p<2200) OR (p>=7300 AND p<9100), distributed into CNF
    preds = [(0, ca.PRED_GE, 1500, 1), (0, ca.PRED_GE, 7300, 1),
             (0, ca.PRED_GE, 1500, 2), (0, ca.PRED_LT, 9100, 2),
             (0, ca.PRED_LT, 2200, 3), (0, ca.PRED_GE, 7300, 3),
             (0, ca.PRED_LT, 2200, 4), (0, ca.PRED_LT, 9100, 4)]
    mask = ((p >= 1500) & (p < 2200)) | ((p >= 7300) & (p < 9100))
    with Tab(str(tmp_path / "pr.cs"), [("p", ca.I64, 0), ("v", ca.I64, 0)], [p, v],
             preds=preds, chunk_group_row_limit=1000) as t:
        assert t.scan.chunk_groups_filtered >= 3
        passing = int(mask.sum())
        for limit in (1, 100, 2000, passing - 1, passing, passing + 9):
            res, idx = t.topn([(1, "desc")], limit, mask=mask)
            assert mask[res["row_numbers"]].all()
            res, idx = t.topn([1, (0, "desc")], limit, mask=mask)
            assert res["n_rows"] == min(limit, passing)


def test_zero_rows_and_zero_groups(tmp_path):
    n = 3000
    p = np.arange(n, dtype=np.int64)
    v = p * 2
    defs = [("p", ca.I64, 0), ("v", ca.I64, 0)]
    # every chunk group pruned
    with Tab(str(tmp_path / "z1.cs"), defs, [p, v], preds=[(0, ca.PRED_GT, 10**6)],
             chunk_group_row_limit=1000) as t:
        assert t.scan.chunk_groups_filtered == 3
        res = t.scan.select_topn([1], 10)
        assert res["n_rows"] == 0 and len(res["values"][1]) == 0
        assert len(res["row_numbers"]) == 0
    # groups survive (min <= 777 <= max) but no row passes
    with Tab(str(tmp_path / "z2.cs"), defs, [p * 2, v],
             preds=[(0, ca.PRED_EQ, 777)]) as t:
        res = t.scan.select_topn([1], 10)
        assert res["n_rows"] == 0 and len(res["row_numbers"]) == 0


def test_fewer_passing_rows_than_limit(tmp_path):
    n = 20011
    rng = np.random.default_rng(53)
    a = rng.integers(0, 2000, n).astype(np.int64)
    b = rng.integers(-99, 99, n).astype(np.int64)
    with Tab(str(tmp_path / "few.cs"), KV, [a, b], preds=[(0, ca.PRED_LT, 5)]) as t:
        mask = a < 5
        res, idx = t.topn([(1, "desc"), 0], 4096, mask=mask)
        assert 0 < res["n_rows"] == int(mask.sum()) < 4096
        assert t.scan.last_topn_ms[1] == 0.0        # no selection needed


def test_key_range_comes_from_selected_groups_only(tmp_path):
    """the whole column spans the full int64 range (65 bits); the chunk
    groups the predicate keeps span far less"""
    n = 4000
    sel = np.arange(n, dtype=np.int64) // 1000          # chunk group id
    k = np.random.default_rng(59).integers(-2**30, 2**30, n).astype(np.int64)
    k[10] = np.iinfo(np.int64).min                      # group 0
    k[3500] = np.iinfo(np.int64).max                    # group 3
    defs = [("g", ca.I64, 0), ("k", ca.I64, 0)]
    path = str(tmp_path / "rng.cs")
    with Tab(path, defs, [sel, k], chunk_group_row_limit=1000,
             preds=[(0, ca.PRED_GE, 1), (0, ca.PRED_LE, 2)]) as t:
        assert t.scan.chunk_groups_filtered == 2
        mask = (sel >= 1) & (sel <= 2)
        for limit in (1, 500, 1999):
            t.topn([1], limit, mask=mask)
            t.topn([(1, "desc")], limit, mask=mask)
    with ca.Reader(path) as r, r.scan(cols_mask=0b11) as s:
        s.stage()
        with pytest.raises(ca.CStripeError, match=r"rc=-5.*65 bits"):
            s.select_topn([1], 5)


# ---------------- every stream shape of the key column ----------------

@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("comp,canonical", [
    (ca.COMP_NONE, 1), (ca.COMP_LZ4, 1), (ca.COMP_LZ4, 0),
    (ca.COMP_ZSTD, 1), (ca.COMP_ZSTD, 0)])
def test_key_stream_shapes(tmp_path, comp, canonical, sparse):
    """raw, canonical P / CONST / width-4 frames, greedy LZ4, generic zstd —
    dense, and sparse (NULLs: rank-indexed value streams)"""
    n = 5000
    rng = np.random.default_rng(47)
    pe = (10**9 + rng.integers(0, 300, n)).astype(np.int64)     # shared high bytes
    const = np.full(n, -424242, dtype=np.int64)
    i32 = rng.integers(0, 3, n).astype(np.int32)
    i8 = rng.integers(-3, 3, n).astype(np.int8)
    he = rng.integers(-2**45, 2**45, n).astype(np.int64)        # high entropy
    nulls = None
    if sparse:
        nulls = [(rng.random(n) < 0.15).astype(np.uint8), None,
                 (rng.random(n) < 0.15).astype(np.uint8),
                 (rng.random(n) < 0.15).astype(np.uint8), None]
    defs = [("pe", ca.I64, 0), ("c", ca.I64, 0), ("f", ca.I32, 0),
            ("b", ca.I8, 0), ("he", ca.I64, 0)]
    with Tab(str(tmp_path / "shape.cs"), defs, [pe, const, i32, i8, he], nulls=nulls,
             compression=comp, canonical=canonical) as t:
        t.topn([0], 37)
        t.topn([(2, "desc"), (3, "asc"), (1, "asc"), (0, "desc", "last")], 37)
        t.topn([(4, "desc")], 37)
        t.topn([1], 37)


# ---------------- destinations ----------------

def test_device_destinations_and_round_trip(tmp_path):
    import torch
    n = 40000
    rng = np.random.default_rng(61)
    a = (10**6 + rng.integers(0, 5000, n)).astype(np.int64)
    b = rng.integers(-2**45, 2**45, n).astype(np.int64)
    f = rng.normal(size=n) * 100
    defs = [("a", ca.I64, 0), ("b", ca.I64, 0), ("f", ca.F64, 0)]
    dst = str(tmp_path / "dst.cs")
    with Tab(str(tmp_path / "src.cs"), defs, [a, b, f],
             preds=[(0, ca.PRED_GE, 10**6 + 1000)]) as t:
        mask = a >= 10**6 + 1000
        order = [(0, "asc"), (1, "desc")]       # 13 + 47 bits
        limit = 12000
        t.topn([(2, "desc")], limit, mask=mask)     # f64 alone: 64 bits
        hres, idx = t.topn(order, limit, mask=mask)
        dres = t.scan.select_topn(order, limit, device=True)
        assert dres["n_rows"] == limit
        for c in range(3):
            tt = dres["values"][c]
            assert tt.is_cuda and len(tt) == limit
            np.testing.assert_array_equal(bits(tt.cpu().numpy()), bits(hres["values"][c]))
            np.testing.assert_array_equal(dres["nulls"][c].cpu().numpy(), hres["nulls"][c])
        assert dres["row_numbers"].dtype == torch.int64
        np.testing.assert_array_equal(dres["row_numbers"].cpu().numpy(),
                                      hres["row_numbers"])
        ca.write_table_device(dst, defs,
                              [dres["values"][c].data_ptr() for c in range(3)], limit)
        torch.cuda.synchronize()
    with ca.Reader(dst) as r, r.scan(cols_mask=0b111) as s:
        assert r.row_count == limit
        s.stage()
        back = s.select()
    for c, full in enumerate((a, b, f)):
        np.testing.assert_array_equal(bits(back["values"][c]), bits(full[idx]))


# ---------------- repeat and interleave ----------------

def test_repeat_and_interleave(tmp_path):
    n = 30011
    rng = np.random.default_rng(67)
    p = rng.integers(0, 100, n).astype(np.int64)
    k = rng.integers(-500, 500, n).astype(np.int64)
    g = rng.integers(0, 40, n).astype(np.int32)
    defs = [("p", ca.I64, 0), ("k", ca.I64, 0), ("g", ca.I32, 0)]
    preds = [(0, ca.PRED_LT, 60)]
    aggs = [(ca.AGG_COUNT_STAR, -1), (ca.AGG_SUM_I64, 1)]
    o1, o2 = [(1, "desc"), (2, "asc")], [(2, "asc"), (1, "asc", "first")]
    path = str(tmp_path / "il.cs")

    def fresh(fn):
        with ca.Reader(path) as r, r.scan(cols_mask=0b111, preds=preds) as s:
            s.stage()
            return fn(s)

    def same_rows(x, y):
        assert x["n_rows"] == y["n_rows"]
        np.testing.assert_array_equal(x["row_numbers"], y["row_numbers"])
        for c in x["values"]:
            np.testing.assert_array_equal(bits(x["values"][c]), bits(y["values"][c]))
            np.testing.assert_array_equal(x["nulls"][c], y["nulls"][c])

    def same_parts(x, y):
        for a_, b_ in zip(x, y):
            assert (a_.i128, a_.count, a_.is_null) == (b_.i128, b_.count, b_.is_null)

    with Tab(path, defs, [p, k, g], preds=preds) as t:
        mask = p < 60
        t1, _ = t.topn(o1, 500, mask=mask)
        s1 = t.scan.select()
        a1 = t.scan.agg(aggs)
        h1 = t.scan.agg_hashed(aggs, [2], 64)
        t2, _ = t.topn(o2, 7000, mask=mask)
        s2 = t.scan.select()
        t3, _ = t.topn(o1, 500, mask=mask)
        assert t.scan.last_kernel_ms > 0 and t.scan.last_topn_ms[1] > 0
    same_rows(s1, s2)           # the cached pass mask and bases are untouched
    same_rows(t1, t3)
    assert s1["n_rows"] == int(mask.sum())
    np.testing.assert_array_equal(s1["row_numbers"], np.flatnonzero(mask))
    same_rows(s1, fresh(lambda s: s.select()))
    same_rows(t1, fresh(lambda s: s.select_topn(o1, 500)))
    same_rows(t2, fresh(lambda s: s.select_topn(o2, 7000)))
    same_parts(a1, fresh(lambda s: s.agg(aggs)))
    fh = fresh(lambda s: s.agg_hashed(aggs, [2], 64))
    assert h1["n_groups"] == fh["n_groups"] == 40
    np.testing.assert_array_equal(h1["keys"][0], fh["keys"][0])
    assert h1["partials"].tobytes() == fh["partials"].tobytes()


# ---------------- argument errors ----------------

def test_argument_errors(tmp_path):
    n = 5000
    p = np.arange(n, dtype=np.int64)
    txt = ca.text_slots(["A", "N"] * (n // 2))
    defs = [("p", ca.I64, 0), ("v", ca.I64, 0), ("w", ca.I64, 0), ("t", ca.TEXT, 0)]
    with Tab(str(tmp_path / "arg.cs"), defs, [p, p * 11, p * 13, txt],
             cols_mask=0b1011) as t:
        s = t.scan
        arg = r"rc=-5"
        with pytest.raises(ca.CStripeError, match=arg):
            s.select_topn([0], 0)
        with pytest.raises(ca.CStripeError, match=arg):
            s.select_topn([0], 2**20 + 1)
        assert s.select_topn([0], 2**20, cols=[0])["n_rows"] == n   # the largest limit
        with pytest.raises(ca.CStripeError, match=arg):
            s.select_topn([], 5)
        with pytest.raises(ca.CStripeError, match=arg):
            s.select_topn([0, 1, 0, 1, 0], 5)                       # n_order 5
        with pytest.raises(ca.CStripeError, match=arg + r".*whole-slot"):
            s.select_topn([3], 5, cols=[0])                         # a TEXT key
        with pytest.raises(ca.CStripeError, match=arg + r".*not projected"):
            s.select_topn([2], 5, cols=[0])                         # unprojected key
        with pytest.raises(ca.CStripeError, match=arg + r".*repeated"):
            s.select_topn([0, (1, "desc"), 0], 5, cols=[0])
        with pytest.raises(ca.CStripeError, match=arg):
            s.select_topn([9], 5, cols=[0])                         # out of range
        with pytest.raises(ca.CStripeError, match=arg + r".*not projected"):
            s.select_topn([0], 5, cols=[0, 2])                      # wanted col 2
        # nothing above disturbed the scan
        res, _ = t.topn([(1, "desc")], 10, cols=[0, 1])
        assert res["values"][0].tolist() == list(range(n - 1, n - 11, -1))
        # the raw entry point leaves the destinations alone on an error
        SENT = 0x5A
        vals = np.full(8, SENT, dtype=np.int64)
        rows = ca.Rows()
        vp = (C.c_void_p * 4)()
        vp[1] = vals.ctypes.data
        rows.col_values = vp
        ok = (ca.OrderKey * 1)()
        ok[0].column, ok[0].flags = 0, 4                            # unknown flag
        assert ca._select_topn(s._h, ok, 1, 8, C.byref(rows), 0) == ca.ERR_ARG
        assert (vals == SENT).all()
        ok[0].flags = ca.ORDER_DESC
        assert ca._select_topn(s._h, ok, 1, 8, C.byref(rows), 0) == ca.OK
        assert rows.n_rows == 8
        np.testing.assert_array_equal(vals, (p * 11)[::-1][:8])


# ---------------- shards ----------------

def test_three_shards_merge_topn(tmp_path):
    rng = np.random.default_rng(71)
    parts = []
    d = tmp_path / "all"
    d.mkdir()
    for i, n in enumerate((2500, 1777, 3100)):
        k = rng.integers(0, 40, n).astype(np.int64)     # heavy ties across shards
        f = 1.0 + rng.integers(0, 17, n) / 4.0          # [1, 5]: 54 key bits
        nk = (rng.random(n) < 0.1).astype(np.uint8)
        path = str(d / f"shard{i:02d}.cs")
        ca.write_table(path, [("k", ca.I64, 0), ("f", ca.F64, 0)],
                       [k, f], nulls=[nk, None], chunk_group_row_limit=1000)
        parts.append((path, k, f, nk))
    order = [(0, "desc"), (1, "asc")]
    limit, offset = 300, 25
    results = []
    for path, _, _, _ in parts:
        with ca.Reader(path) as r, r.scan(cols_mask=0b11) as s:
            s.stage()
            results.append(s.select_topn(order, limit + offset))
    m = ca.merge_topn(results, order, limit, offset=offset)
    # numpy over the concatenation: (part, row number) is concatenation order
    K = np.concatenate([x[1] for x in parts])
    F = np.concatenate([x[2] for x in parts])
    NK = np.concatenate([x[3] for x in parts])
    idx = np_topn(ca.parse_order(order), limit + offset, np.ones(len(K), bool),
                  {0: K, 1: F}, {0: NK})[offset:]
    starts = np.cumsum([0] + [len(x[1]) for x in parts])
    exp_part = np.searchsorted(starts, idx, side="right") - 1
    assert m["n_rows"] == limit
    np.testing.assert_array_equal(m["part"], exp_part)
    np.testing.assert_array_equal(m["row_numbers"], idx - starts[exp_part])
    exp_k = K[idx].copy()
    exp_k[NK[idx] == 1] = 0
    np.testing.assert_array_equal(m["values"][0], exp_k)
    np.testing.assert_array_equal(bits(m["values"][1]), bits(F[idx]))
    np.testing.assert_array_equal(m["nulls"][0], NK[idx])
    # one scan over the 3-file shard directory: row numbers continue across files
    with ca.Reader(str(d)) as r, r.scan(cols_mask=0b11) as s:
        s.stage()
        whole = s.select_topn(order, limit + offset)
    np.testing.assert_array_equal(whole["row_numbers"][offset:], idx)
