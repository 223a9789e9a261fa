"""
GPU tests (@pytest.mark.gpu) for cstripe_scan_select — device-side filtered
row materialisation (select_mask / select_offsets / select_emit kernels).

Expected results are computed in numpy from the arrays the test itself
wrote: expected = column[mask], row_numbers = np.flatnonzero(mask); never
from the library. Values are copied, not computed, so every comparison is
bit-exact (floats are compared as bit patterns).
"""
import ctypes as C
import os

import numpy as np
import pytest

import citus_amd as ca
import oracle

from conftest import q6_preds

pytestmark = pytest.mark.gpu

NP_OF = {ca.I8: np.int8, ca.I16: np.int16, ca.I32: np.int32, ca.I64: np.int64,
         ca.F32: np.float32, ca.F64: np.float64, ca.TEXT: np.uint32}
BITS = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


@pytest.fixture(scope="module", autouse=True)
def require_gpu():
    assert ca.gpu_available(), "MI355X required for these tests"


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(BITS[a.dtype.itemsize])


def pg_cmp(a, op, c):
    """`a op c` under PG float ordering: NaN is the greatest value and
    equal to itself (float8_cmp_internal)."""
    a = np.asarray(a, dtype=np.float64)
    an = np.isnan(a)
    if np.isnan(c):
        eq = an
        lt = ~an
    else:
        with np.errstate(invalid="ignore"):
            eq = ~an & (a == c)
            lt = ~an & (a < c)
    gt = ~eq & ~lt
    return {ca.PRED_LT: lt, ca.PRED_LE: lt | eq, ca.PRED_GT: gt,
            ca.PRED_GE: gt | eq, ca.PRED_EQ: eq, ca.PRED_NE: ~eq}[op]


def check(res, mask, columns, nulls=None):
    """res = Scan.select() output; columns = {col: full array written};
    nulls = {col: uint8 array written, 1 = null}."""
    nulls = nulls or {}
    idx = np.flatnonzero(mask)
    assert res["n_rows"] == len(idx)
    if res["row_numbers"] is not None:
        np.testing.assert_array_equal(res["row_numbers"], idx)
    for c, full in columns.items():
        got = res["values"][c]
        assert got.dtype == full.dtype and len(got) == len(idx)
        exp = full[idx].copy()
        expn = np.zeros(len(idx), dtype=np.uint8)
        if nulls.get(c) is not None:
            expn = nulls[c][idx]
            exp[expn == 1] = 0              # NULL slots are zero-filled
        np.testing.assert_array_equal(bits(got), bits(exp), err_msg=f"col {c}")
        if res["nulls"]:
            np.testing.assert_array_equal(res["nulls"][c], expn,
                                          err_msg=f"nulls {c}")


def select_of(path, preds, cols_mask, **kw):
    with ca.Reader(path) as r, r.scan(cols_mask=cols_mask, preds=preds) as s:
        s.stage()
        res = s.select(**kw)
        filtered = s.chunk_groups_filtered
    return res, filtered


# ---------------- slice and tile edges ----------------

EDGE_RNG = np.random.default_rng(11)


def edge_masks(n):
    i = np.arange(n)
    return {"none": np.zeros(n, bool), "all": np.ones(n, bool),
            "alt": i % 2 == 0, "last": i == n - 1, "first": i == 0,
            "rand3": np.random.default_rng(n).random(n) < 0.03}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4096, 4097, 10000, 10001,
                               25017])
def test_slice_and_tile_edges(tmp_path, n):
    """64-row ballot slices, 4096-row tiles, 10 000-row chunk groups: one
    I64 predicate column + one I64 payload column."""
    v = EDGE_RNG.integers(-2**62, 2**62, n).astype(np.int64)
    i = np.arange(n)
    for name, mask in edge_masks(n).items():
        # passing rows hold 5; the others straddle it so min/max cannot
        # refute `p == 5` wherever two non-passing rows share a chunk
        p = np.where(mask, 5, np.where(i % 2 == 0, 0, 9)).astype(np.int64)
        path = str(tmp_path / f"e_{name}.cs")
        ca.write_table(path, [("p", ca.I64, 0), ("v", ca.I64, 0)], [p, v],
                       compression=ca.COMP_LZ4)
        res, _ = select_of(path, [(0, ca.PRED_EQ, 5)], 0b11)
        check(res, mask, {0: p, 1: v})


def test_many_groups_and_stripes(tmp_path):
    """partial last chunk and partial last stripe keep row numbers right"""
    n = 7777
    rng = np.random.default_rng(3)
    p = rng.integers(0, 100, n).astype(np.int64)
    v = rng.integers(-2**40, 2**40, n).astype(np.int64)
    path = str(tmp_path / "mg.cs")
    ca.write_table(path, [("p", ca.I64, 0), ("v", ca.I64, 0)], [p, v],
                   compression=ca.COMP_LZ4, chunk_group_row_limit=1000,
                   stripe_row_limit=3000)
    res, _ = select_of(path, [(0, ca.PRED_LT, 17)], 0b11)
    check(res, p < 17, {0: p, 1: v})


def test_pruned_chunks_count_in_row_numbers(tmp_path):
    """min/max pruning removes leading, middle and trailing chunk groups; a
    surviving chunk's row base still counts the pruned ones before it."""
    n = 12345
    p = np.arange(n, dtype=np.int64)
    v = (p * 7919) % 100003
    path = str(tmp_path / "pr.cs")
    ca.write_table(path, [("p", ca.I64, 0), ("v", ca.I64, 0)], [p, v],
                   compression=ca.COMP_LZ4, chunk_group_row_limit=1000)
    # (p>=1500 AND p<2200) OR (p>=7300 AND p<9100), distributed into CNF
    preds = [(0, ca.PRED_GE, 1500, 1), (0, ca.PRED_GE, 7300, 1),
             (0, ca.PRED_GE, 1500, 2), (0, ca.PRED_LT, 9100, 2),
             (0, ca.PRED_LT, 2200, 3), (0, ca.PRED_GE, 7300, 3),
             (0, ca.PRED_LT, 2200, 4), (0, ca.PRED_LT, 9100, 4)]
    mask = ((p >= 1500) & (p < 2200)) | ((p >= 7300) & (p < 9100))
    res, filtered = select_of(path, preds, 0b11)
    assert filtered > 0
    # leading chunk 0, middle chunk 4 and the trailing chunks are refuted
    assert filtered >= 3
    check(res, mask, {0: p, 1: v})


# ---------------- every stream shape ----------------

@pytest.mark.parametrize("comp,canonical", [
    (ca.COMP_NONE, 1), (ca.COMP_LZ4, 1), (ca.COMP_LZ4, 0),
    (ca.COMP_ZSTD, 1), (ca.COMP_ZSTD, 0)])
def test_stream_shapes(tmp_path, comp, canonical):
    """raw, canonical P/CONST/LIT, greedy LZ4, generic zstd, width-4 flag
    frames: P-eligible and high-entropy I64, a constant column and a TEXT
    flag column, all gathered through col_value."""
    n = 25017
    rng = np.random.default_rng(5)
    pe = (10**9 + rng.integers(0, 50000, n)).astype(np.int64)    # shared high bytes
    he = rng.integers(-2**63, 2**63 - 1, n).astype(np.int64)      # high entropy
    const = np.full(n, 424242, dtype=np.int64)
    flag = ca.text_slots([["A", "N", "R"][k] for k in rng.integers(0, 3, n)])
    cflag = ca.text_slots(["F"] * n)
    path = str(tmp_path / "shape.cs")
    defs = [("pe", ca.I64, 0), ("he", ca.I64, 0), ("c", ca.I64, 0),
            ("f", ca.TEXT, 0), ("cf", ca.TEXT, 0)]
    ca.write_table(path, defs, [pe, he, const, flag, cflag], compression=comp,
                   canonical=canonical)
    cols = {0: pe, 1: he, 2: const, 3: flag, 4: cflag}
    lo = 10**9 + 20000
    res, _ = select_of(path, [(0, ca.PRED_GE, lo), (0, ca.PRED_LT, lo + 900)],
                       0b11111)
    check(res, (pe >= lo) & (pe < lo + 900), cols)
    # predicate on the high-entropy column and on the flag column
    res, _ = select_of(path, [(1, ca.PRED_GT, 2**62),
                              (3, ca.PRED_EQ, ca.text_slot("N"))], 0b11111)
    check(res, (he > 2**62) & (flag == ca.text_slot("N")), cols)


def test_all_types_and_mixed_predicates(tmp_path):
    n = 12001
    rng = np.random.default_rng(9)
    c8 = rng.integers(-128, 128, n).astype(np.int8)
    c16 = rng.integers(-2**15, 2**15, n).astype(np.int16)
    c32 = rng.integers(-1000, 1000, n).astype(np.int32)
    c64 = rng.integers(-2**50, 2**50, n).astype(np.int64)
    f32 = rng.normal(size=n).astype(np.float32)
    f64 = rng.normal(size=n)
    txt = ca.text_slots([["A", "N", "R", "xy", "abc"][k]
                         for k in rng.integers(0, 5, n)])
    defs = [("a", ca.I8, 0), ("b", ca.I16, 0), ("c", ca.I32, 0),
            ("d", ca.I64, 0), ("e", ca.F32, 0), ("f", ca.F64, 0),
            ("t", ca.TEXT, 0)]
    arrs = [c8, c16, c32, c64, f32, f64, txt]
    path = str(tmp_path / "types.cs")
    ca.write_table(path, defs, arrs, compression=ca.COMP_LZ4,
                   chunk_group_row_limit=5000)
    preds = [(2, ca.PRED_GE, -500), (4, ca.PRED_LT, 0.5),
             (6, ca.PRED_NE, ca.text_slot("N"))]
    mask = ((c32 >= -500) & (f32.astype(np.float64) < 0.5) &
            (txt != ca.text_slot("N")))
    res, _ = select_of(path, preds, 0x7F)
    check(res, mask, dict(enumerate(arrs)))


# ---------------- NULLs ----------------

@pytest.mark.parametrize("comp", [ca.COMP_NONE, ca.COMP_LZ4, ca.COMP_ZSTD])
def test_nulls(tmp_path, comp):
    """NULL predicate operands never pass; NULL payload slots come back
    zero-filled with nulls == 1; an all-NULL payload column."""
    n = 9001
    rng = np.random.default_rng(13)
    p = rng.integers(0, 1000, n).astype(np.int64)
    np_ = (rng.random(n) < 0.3).astype(np.uint8)
    v = rng.integers(-2**40, 2**40, n).astype(np.int64)
    nv = (rng.random(n) < 0.2).astype(np.uint8)
    f = rng.normal(size=n)
    nf = (rng.random(n) < 0.5).astype(np.uint8)
    z = np.zeros(n, dtype=np.int32)
    nz = np.ones(n, dtype=np.uint8)
    path = str(tmp_path / "nulls.cs")
    ca.write_table(path, [("p", ca.I64, 0), ("v", ca.I64, 0), ("f", ca.F64, 0),
                          ("z", ca.I32, 0)], [p, v, f, z],
                   nulls=[np_, nv, nf, nz], compression=comp,
                   chunk_group_row_limit=3000)
    mask = (np_ == 0) & (p >= 100)
    res, _ = select_of(path, [(0, ca.PRED_GE, 100)], 0b1111)
    check(res, mask, {0: p, 1: v, 2: f, 3: z}, {0: np_, 1: nv, 2: nf, 3: nz})
    assert res["nulls"][3].all() and not res["values"][3].any()
    assert not res["nulls"][0].any()


# ---------------- OR groups and NaN ----------------

def test_or_groups(tmp_path):
    n = 20011
    rng = np.random.default_rng(17)
    a = rng.integers(0, 200, n).astype(np.int64)
    b = rng.integers(0, 1000, n).astype(np.int64)
    path = str(tmp_path / "or.cs")
    ca.write_table(path, [("a", ca.I64, 0), ("b", ca.I64, 0)], [a, b],
                   compression=ca.COMP_LZ4)
    preds = [(0, ca.PRED_LT, 100, 1), (1, ca.PRED_GT, 500, 1),
             (0, ca.PRED_GE, 50, 2), (1, ca.PRED_EQ, 7, 2)]
    mask = ((a < 100) | (b > 500)) & ((a >= 50) | (b == 7))
    res, _ = select_of(path, preds, 0b11)
    check(res, mask, {0: a, 1: b})


@pytest.mark.parametrize("const", [0.25, float("nan")])
@pytest.mark.parametrize("op", [ca.PRED_GT, ca.PRED_EQ, ca.PRED_NE])
def test_nan_pg_order(tmp_path, op, const):
    n = 8200
    rng = np.random.default_rng(19)
    f = rng.integers(-4, 5, n) / 4.0            # exact quarters, hits 0.25
    f[rng.random(n) < 0.1] = np.nan
    v = np.arange(n, dtype=np.int64) * 3
    path = str(tmp_path / "nan.cs")
    ca.write_table(path, [("f", ca.F64, 0), ("v", ca.I64, 0)], [f, v],
                   compression=ca.COMP_LZ4, chunk_group_row_limit=3000)
    res, _ = select_of(path, [(0, op, const)], 0b11)
    check(res, pg_cmp(f, op, const), {0: f, 1: v})


# ---------------- no predicates == next_batch ----------------

def test_no_predicates_equals_next_batch(tmp_path):
    n = 10500
    rng = np.random.default_rng(23)
    a = rng.integers(-2**40, 2**40, n).astype(np.int64)
    na = (rng.random(n) < 0.2).astype(np.uint8)
    b = rng.normal(size=n).astype(np.float32)
    path = str(tmp_path / "nb.cs")
    ca.write_table(path, [("a", ca.I64, 0), ("b", ca.F32, 0)], [a, b],
                   nulls=[na, None], compression=ca.COMP_LZ4,
                   stripe_row_limit=6000, chunk_group_row_limit=2000)
    with ca.Reader(path) as r, r.scan(cols_mask=0b11) as s:
        s.stage()
        res = s.select()
        va, vb = np.zeros(2000, np.int64), np.zeros(2000, np.float32)
        ea, eb = np.zeros(2000, np.uint8), np.zeros(2000, np.uint8)
        ca_, cb_, cna, cnb, crn = [], [], [], [], []
        while True:
            nb = s.next_batch({0: va, 1: vb}, {0: ea, 1: eb})
            if nb is None:
                break
            k, first = nb
            ca_.append(va[:k].copy()); cb_.append(vb[:k].copy())
            cna.append(ea[:k].copy()); cnb.append(eb[:k].copy())
            crn.append(first + np.arange(k))
    assert res["n_rows"] == n
    np.testing.assert_array_equal(res["values"][0], np.concatenate(ca_))
    np.testing.assert_array_equal(bits(res["values"][1]), bits(np.concatenate(cb_)))
    np.testing.assert_array_equal(res["nulls"][0], np.concatenate(cna))
    np.testing.assert_array_equal(res["nulls"][1], np.concatenate(cnb))
    np.testing.assert_array_equal(res["row_numbers"], np.concatenate(crn))
    check(res, np.ones(n, bool), {0: a, 1: b}, {0: na})


# ---------------- golden pin ----------------

@pytest.mark.parametrize("variant", ["lz4", "none", "zstd"])
def test_q6_golden_select(golden_dir, expected, variant):
    path = os.path.join(golden_dir, f"lineitem12k_{variant}.cs")
    preds = q6_preds(ca, expected)
    with oracle.OracleTable(path) as t:
        op, _ = t.scan_agg(preds, [(ca.AGG_COUNT_STAR, -1)])
    res, _ = select_of(path, preds, (1 << 2) | (1 << 3), cols=[2, 3])
    price, disc = res["values"][2], res["values"][3]
    rev = sum(int(a) * int(b) for a, b in zip(price, disc))
    assert rev == expected["q6"]["revenue_scale4"] == 2432777858
    assert res["n_rows"] == op[0].count
    assert not res["nulls"][2].any() and not res["nulls"][3].any()
    assert (np.diff(res["row_numbers"]) > 0).all()


# ---------------- shard directory ----------------

def test_shard_directory_row_numbers(tmp_path):
    d = tmp_path / "shards"
    d.mkdir()
    rng = np.random.default_rng(29)
    parts = []
    for i, n in enumerate((2500, 1777)):
        p = rng.integers(0, 50, n).astype(np.int64)
        v = rng.integers(-2**30, 2**30, n).astype(np.int64)
        ca.write_table(str(d / f"shard{i:02d}.cs"),
                       [("p", ca.I64, 0), ("v", ca.I64, 0)], [p, v],
                       compression=ca.COMP_LZ4, chunk_group_row_limit=1000)
        parts.append((p, v))
    p = np.concatenate([x[0] for x in parts])
    v = np.concatenate([x[1] for x in parts])
    mask = p < 5
    with ca.Reader(str(d)) as r:
        assert r.row_count == 4277
        with r.scan(cols_mask=0b11, preds=[(0, ca.PRED_LT, 5)]) as s:
            s.stage()
            res = s.select()
        check(res, mask, {0: p, 1: v})
        rns = res["row_numbers"]
        assert rns[0] < 2500 <= rns[-1]        # continues across the files
        with r.scan(cols_mask=0b11) as s:
            s.stage()
            for k in (0, 1, len(rns) // 2, len(rns) - 2, len(rns) - 1):
                row = s.read_row(int(rns[k]))
                assert row == {0: int(res["values"][0][k]),
                               1: int(res["values"][1][k])}


# ---------------- capacity and arguments ----------------

def test_capacity_and_unprojected(tmp_path):
    n = 5000
    p = np.arange(n, dtype=np.int64)
    v = p * 11
    w = p * 13
    path = str(tmp_path / "cap.cs")
    ca.write_table(path, [("p", ca.I64, 0), ("v", ca.I64, 0), ("w", ca.I64, 0)],
                   [p, v, w], compression=ca.COMP_LZ4)
    with ca.Reader(path) as r, r.scan(cols_mask=0b011,
                                      preds=[(0, ca.PRED_LT, 1234)]) as s:
        s.stage()
        k = s.select_count()
        assert k == 1234
        SENT = 0x5A
        vals = np.full(k, SENT, dtype=np.int64)
        nul = np.full(k, SENT, dtype=np.uint8)
        rn = np.full(k, SENT, dtype=np.int64)
        rows = ca.Rows()
        vp = (C.c_void_p * 3)()
        vp[1] = vals.ctypes.data
        npn = (C.c_void_p * 3)()
        npn[1] = nul.ctypes.data
        rows.col_values, rows.col_nulls = vp, npn
        rows.row_numbers = rn.ctypes.data
        rc = ca._select(s._h, C.byref(rows), k - 1, 0)
        assert rc == ca.ERR_ARG
        assert "1233" in ca.errmsg() and "1234" in ca.errmsg()
        assert (vals == SENT).all() and (nul == SENT).all() and (rn == SENT).all()
        # exact capacity works
        assert ca._select(s._h, C.byref(rows), k, 0) == ca.OK
        assert rows.n_rows == k
        np.testing.assert_array_equal(vals, v[:k])
        np.testing.assert_array_equal(rn, np.arange(k))
        assert not nul.any()
        # column 2 was never projected
        with pytest.raises(ca.CStripeError, match=r"rc=-5"):
            s.select(cols=[2])


def test_zero_selected_groups(tmp_path):
    n = 3000
    p = np.arange(n, dtype=np.int64)
    path = str(tmp_path / "zero.cs")
    ca.write_table(path, [("p", ca.I64, 0)], [p], compression=ca.COMP_LZ4,
                   chunk_group_row_limit=1000)
    res, filtered = select_of(path, [(0, ca.PRED_GT, 10**6)], 0b1)
    assert filtered == 3
    assert res["n_rows"] == 0 and len(res["values"][0]) == 0
    assert len(res["row_numbers"]) == 0


# ---------------- stability and interleaving ----------------

def test_stable_and_interleaved(golden_dir, expected):
    """select -> agg -> select -> agg_grouped -> select on ONE scan: the
    selects are identical, the aggregates equal a fresh scan's."""
    path = os.path.join(golden_dir, "lineitem12k_lz4.cs")
    preds = q6_preds(ca, expected)
    aggs = [(ca.AGG_SUM_PROD_I64, 2, 3), (ca.AGG_COUNT_STAR, -1)]
    gaggs = [(ca.AGG_SUM_I64, 1), (ca.AGG_COUNT_STAR, -1)]
    mask = ca.agg_cols_mask(aggs) | (1 << 1) | (1 << 6) | (1 << 7)

    def same(x, y):
        assert x["n_rows"] == y["n_rows"]
        np.testing.assert_array_equal(x["row_numbers"], y["row_numbers"])
        for c in x["values"]:
            np.testing.assert_array_equal(bits(x["values"][c]), bits(y["values"][c]))
            np.testing.assert_array_equal(x["nulls"][c], y["nulls"][c])

    with ca.Reader(path) as r:
        with r.scan(cols_mask=mask, preds=preds) as s:
            s.stage()
            fresh_agg = s.agg(aggs)
        with r.scan(cols_mask=mask, preds=preds) as s:
            s.stage()
            fresh_grp = s.agg_grouped(gaggs, (6, 7))
        with r.scan(cols_mask=mask, preds=preds) as s:
            s.stage()
            s1 = s.select()
            a1 = s.agg(aggs)
            s2 = s.select()
            g1 = s.agg_grouped(gaggs, (6, 7))
            s3 = s.select()
            assert s.last_kernel_ms > 0
    same(s1, s2)
    same(s1, s3)
    assert s1["n_rows"] == fresh_agg[1].count > 0
    for x, y in zip(a1, fresh_agg):
        assert (x.i128, x.count, x.is_null) == (y.i128, y.count, y.is_null)
    assert set(g1) == set(fresh_grp)
    for k in g1:
        for x, y in zip(g1[k], fresh_grp[k]):
            assert (x.i128, x.count, x.is_null) == (y.i128, y.count, y.is_null)


# ---------------- device round trip (the CTAS loop) ----------------

def test_device_round_trip_ctas(tmp_path):
    """scan -> filter -> compact -> write with the rows never leaving HBM:
    select(device=True) feeds write_table_device; the new file holds exactly
    the selected rows."""
    import torch
    n = 40000
    rng = np.random.default_rng(31)
    a = (10**6 + rng.integers(0, 5000, n)).astype(np.int64)
    b = rng.integers(-2**45, 2**45, n).astype(np.int64)
    f = rng.normal(size=n) * 100
    src = str(tmp_path / "src.cs")
    defs = [("a", ca.I64, 0), ("b", ca.I64, 0), ("f", ca.F64, 0)]
    ca.write_table(src, defs, [a, b, f], compression=ca.COMP_LZ4)
    preds = [(0, ca.PRED_GE, 10**6 + 1000), (0, ca.PRED_LT, 10**6 + 3500)]
    mask = (a >= 10**6 + 1000) & (a < 10**6 + 3500)
    dst = str(tmp_path / "dst.cs")
    with ca.Reader(src) as r, r.scan(cols_mask=0b111, preds=preds) as s:
        s.stage()
        dres = s.select(device=True)
        hres = s.select()
        k = dres["n_rows"]
        assert k == int(mask.sum()) > 10000
        for c in range(3):
            t = dres["values"][c]
            assert t.is_cuda and len(t) == k
        assert dres["row_numbers"].dtype == torch.int64
        ca.write_table_device(dst, defs,
                              [dres["values"][c].data_ptr() for c in range(3)], k)
        torch.cuda.synchronize()
        # copied back, the device tensors equal the host-mode select exactly
        for c in range(3):
            np.testing.assert_array_equal(bits(dres["values"][c].cpu().numpy()),
                                          bits(hres["values"][c]))
            np.testing.assert_array_equal(dres["nulls"][c].cpu().numpy(),
                                          hres["nulls"][c])
        np.testing.assert_array_equal(dres["row_numbers"].cpu().numpy(),
                                      hres["row_numbers"])
    check(hres, mask, {0: a, 1: b, 2: f})

    aggs = [(ca.AGG_COUNT_STAR, -1), (ca.AGG_SUM_I64, 0), (ca.AGG_MIN_I64, 1),
            (ca.AGG_MAX_I64, 1), (ca.AGG_SUM_I64, 1), (ca.AGG_SUM_F64, 2),
            (ca.AGG_MIN_F64, 2), (ca.AGG_MAX_F64, 2)]
    with oracle.OracleTable(dst) as t:
        assert t.row_count == k
        new, _ = t.scan_agg([], aggs)
    with oracle.OracleTable(src) as t:
        old, _ = t.scan_agg(preds, aggs)
    for i, ag in enumerate(aggs):
        assert new[i].count == old[i].count and new[i].is_null == old[i].is_null
        if ag[0] == ca.AGG_SUM_F64:
            # same rows, possibly another association across chunk groups:
            # the project's float-SUM bar (1e-6 relative)
            assert abs(new[i].f64 - old[i].f64) <= 1e-6 * abs(old[i].f64)
        elif ag[0] in (ca.AGG_MIN_F64, ca.AGG_MAX_F64):
            assert new[i].f64 == old[i].f64
        else:
            assert new[i].i128 == old[i].i128
