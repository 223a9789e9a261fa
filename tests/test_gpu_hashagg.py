"""
GPU tests (@pytest.mark.gpu) for cstripe_scan_agg_hashed — the device hash
GROUP BY over integer keys (hash_init / hash_agg / hash_compact kernels) —
and its merge, cagg_combine_groups.

Expected results are computed in numpy / Python ints from the arrays the
test itself wrote (group by a Python dict of key tuples, exact Python-int
sums), never from the library. Integers, counts, min/max and f64 min/max
bit patterns are compared exactly; f64 sums within the project's 1e-6
relative tolerance, on positive inputs so nothing cancels.

CSTRIPE_HASH_LDS_SLOTS is read per call: unset = the default per-block LDS
table, "0" = no LDS table (every row goes to the global table), "16" = a
16-slot LDS table that overflows into the global one.
"""
import math
import os
import struct

import numpy as np
import pytest

import citus_amd as ca

pytestmark = pytest.mark.gpu

LDS_MODES = [None, "0", "16"]
PROD_KINDS = (ca.AGG_SUM_PROD_I64, ca.AGG_SUM_DISC_I64, ca.AGG_SUM_DISC_TAX_I64)
F64_KINDS = (ca.AGG_SUM_F64, ca.AGG_MIN_F64, ca.AGG_MAX_F64)
SC = [(ca.AGG_COUNT_STAR, -1), (ca.AGG_SUM_I64, 1)]


@pytest.fixture(scope="module", autouse=True)
def require_gpu():
    assert ca.gpu_available(), "MI355X required for these tests"


def set_lds(monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv("CSTRIPE_HASH_LDS_SLOTS", raising=False)
    else:
        monkeypatch.setenv("CSTRIPE_HASH_LDS_SLOTS", mode)


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


# ---------------- the numpy / Python-int reference ----------------

def ref_agg(agg, idx, cols, nulls):
    kind, c_a, c_b, c_c, one = (tuple(agg) + (-1, -1, -1, 0)[len(agg) - 1:])[:5]
    if kind == ca.AGG_COUNT_STAR:
        return {"count": len(idx), "null": False, "i128": len(idx)}

    def present(c):
        nl = nulls.get(c)
        return np.ones(len(idx), bool) if nl is None else nl[idx] == 0
    ok = present(c_a)
    if kind in PROD_KINDS:
        ok &= present(c_b)
    if kind == ca.AGG_SUM_DISC_TAX_I64:
        ok &= present(c_c)
    sel = idx[ok]
    cnt = len(sel)
    if kind == ca.AGG_COUNT_COL:
        return {"count": cnt, "null": False, "i128": cnt}
    if cnt == 0:
        return {"count": 0, "null": True}
    a = cols[c_a][sel]
    out = {"count": cnt, "null": False}
    if kind == ca.AGG_SUM_I64:
        out["i128"] = sum(a.tolist())
    elif kind == ca.AGG_MIN_I64:
        out["i128"] = int(a.min())
    elif kind == ca.AGG_MAX_I64:
        out["i128"] = int(a.max())
    elif kind == ca.AGG_SUM_F64:
        out["f64"] = math.fsum(a.tolist())
    elif kind == ca.AGG_MIN_F64:        # PG order: NaN is the greatest float
        nn = a[~np.isnan(a)]
        out["f64"] = float(nn.min()) if len(nn) else float("nan")
    elif kind == ca.AGG_MAX_F64:
        out["f64"] = float("nan") if np.isnan(a).any() else float(a.max())
    elif kind == ca.AGG_SUM_PROD_I64:
        out["i128"] = sum(x * y for x, y in zip(a.tolist(), cols[c_b][sel].tolist()))
    elif kind == ca.AGG_SUM_DISC_I64:
        out["i128"] = sum(x * (one - y)
                          for x, y in zip(a.tolist(), cols[c_b][sel].tolist()))
    else:
        out["i128"] = sum(x * (one - y) * (one + z)
                          for x, y, z in zip(a.tolist(), cols[c_b][sel].tolist(),
                                             cols[c_c][sel].tolist()))
    return out


def ref_groups(key_cols, mask, aggs, cols, nulls=None):
    """{key tuple (None = NULL): [ref_agg per agg]} over rows where mask"""
    nulls = nulls or {}
    kl = [(cols[c].tolist(), None if nulls.get(c) is None else nulls[c].tolist())
          for c in key_cols]
    groups = {}
    for i in np.flatnonzero(mask).tolist():
        t = tuple(None if (nl is not None and nl[i]) else v[i] for v, nl in kl)
        groups.setdefault(t, []).append(i)
    return {t: [ref_agg(a, np.array(ix), cols, nulls) for a in aggs]
            for t, ix in groups.items()}


def sort_key(t):
    """ascending, signed, per column NULL last"""
    return tuple((1, 0) if v is None else (0, v) for v in t)


def result_keys(res):
    nk = len(res["keys"])
    return [tuple(None if res["key_nulls"][k][g] else int(res["keys"][k][g])
                  for k in range(nk)) for g in range(res["n_groups"])]


def check(res, exp, aggs):
    order = sorted(exp, key=sort_key)
    got = result_keys(res)
    assert res["n_groups"] == len(order)
    assert got == order                       # sorted, each key exactly once
    for k in range(len(res["keys"])):         # NULL keys carry value 0
        assert not res["keys"][k][res["key_nulls"][k] == 1].any()
    assert res["partials"].shape == (len(order), len(aggs))
    for g, t in enumerate(order):
        for a, agg in enumerate(aggs):
            p, e, kind = res["partials"][g, a], exp[t][a], agg[0]
            where = (t, a)
            assert p["count"] == e["count"], where
            if kind in (ca.AGG_COUNT_STAR, ca.AGG_COUNT_COL):
                assert p["is_null"] == 0 and p["i128_lo"] == e["count"], where
                continue
            assert bool(p["is_null"]) == e["null"], where
            if e["null"]:
                continue
            if kind == ca.AGG_SUM_F64:
                assert abs(p["f64"] - e["f64"]) <= 1e-6 * abs(e["f64"]), where
            elif kind in F64_KINDS:
                if math.isnan(e["f64"]):
                    assert math.isnan(p["f64"]), where
                else:
                    assert f64_bits(p["f64"]) == f64_bits(e["f64"]), where
            else:
                assert ca.partial_i128(p) == e["i128"], where


def same_result(a, b):
    assert a["n_groups"] == b["n_groups"]
    for k in range(len(a["keys"])):
        np.testing.assert_array_equal(a["keys"][k], b["keys"][k])
        np.testing.assert_array_equal(a["key_nulls"][k], b["key_nulls"][k])
    assert a["partials"].tobytes() == b["partials"].tobytes()


def open_scan(path, cols_mask, preds=()):
    r = ca.Reader(path)
    s = r.scan(cols_mask=cols_mask, preds=preds)
    s.stage()
    return r, s


def hashed(path, cols_mask, aggs, key_cols, capacity, preds=()):
    r, s = open_scan(path, cols_mask, preds)
    try:
        return s.agg_hashed(aggs, key_cols, capacity)
    finally:
        s.end()
        r.close()


# ---------------- slice, tile and chunk-group edges ----------------

EDGE_RNG = np.random.default_rng(21)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4097, 10001, 25017])
def test_edges(tmp_path, monkeypatch, n):
    """64-row waves, 4096-row tiles, 10 000-row chunk groups; I64 key i % m;
    the three LDS settings must agree bit for bit."""
    v = EDGE_RNG.integers(-2**40, 2**40, n).astype(np.int64)
    for m in (1, 7, 1000):
        k = (np.arange(n) % m).astype(np.int64)
        path = str(tmp_path / f"e{m}.cs")
        ca.write_table(path, [("k", ca.I64, 0), ("v", ca.I64, 0)], [k, v],
                       compression=ca.COMP_LZ4)
        exp = ref_groups([0], np.ones(n, bool), SC, {0: k, 1: v})
        r, s = open_scan(path, 0b11)
        try:
            results = []
            for mode in LDS_MODES:
                set_lds(monkeypatch, mode)
                results.append(s.agg_hashed(SC, [0], 1000))
        finally:
            s.end()
            r.close()
        check(results[0], exp, SC)
        same_result(results[0], results[1])
        same_result(results[0], results[2])


# ---------------- LDS overflow and flush ----------------

@pytest.mark.parametrize("mode", LDS_MODES)
def test_all_distinct_keys_overflow_every_lds_table(tmp_path, monkeypatch, mode):
    """25 017 distinct keys: every 4096-row tile holds more keys than any
    LDS table, so most rows take the bounded-probe exit to the global table"""
    n = 25017
    rng = np.random.default_rng(31)
    k = (rng.permutation(n).astype(np.int64) - 12000) * 3
    v = rng.integers(-2**50, 2**50, n).astype(np.int64)
    path = str(tmp_path / "d.cs")
    ca.write_table(path, [("k", ca.I64, 0), ("v", ca.I64, 0)], [k, v],
                   compression=ca.COMP_LZ4)
    set_lds(monkeypatch, mode)
    res = hashed(path, 0b11, SC, [0], 32768)
    assert res["n_groups"] == n
    order = np.argsort(k)
    np.testing.assert_array_equal(res["keys"][0], k[order])
    assert not res["key_nulls"][0].any()
    np.testing.assert_array_equal(res["partials"]["count"][:, 0], np.ones(n))
    np.testing.assert_array_equal(res["partials"]["i128_lo"][:, 1], v[order])
    np.testing.assert_array_equal(res["partials"]["i128_hi"][:, 1], v[order] >> 63)
    assert not res["partials"]["is_null"].any()


@pytest.mark.parametrize("mode", LDS_MODES)
def test_one_key_in_every_tile_and_chunk_group(tmp_path, monkeypatch, mode):
    """one key spread over every block's tiles (plus a sprinkle of others):
    the flush merge across blocks, with sums that carry past 64 bits"""
    n = 25017
    k = np.where(np.arange(n) % 5 == 4, np.arange(n) % 11, 777).astype(np.int64)
    v = np.full(n, 2**62 + 12345, dtype=np.int64)
    path = str(tmp_path / "one.cs")
    ca.write_table(path, [("k", ca.I64, 0), ("v", ca.I64, 0)], [k, v],
                   compression=ca.COMP_LZ4, chunk_group_row_limit=1000)
    aggs = SC + [(ca.AGG_MIN_I64, 1), (ca.AGG_MAX_I64, 1)]
    set_lds(monkeypatch, mode)
    res = hashed(path, 0b11, aggs, [0], 64)
    exp = ref_groups([0], np.ones(n, bool), aggs, {0: k, 1: v})
    check(res, exp, aggs)
    g = result_keys(res).index((777,))
    assert res["partials"][g, 1]["i128_hi"] > 0       # carried


# ---------------- small tables: collisions and wrap-around ----------------

CAPS = (1, 2, 3, 5, 8)


@pytest.mark.parametrize("seed", range(32))
def test_small_tables(tmp_path, seed):
    """2..16-slot global tables holding exactly `capacity` distinct random
    keys: linear-probe collisions and wrap-around. One scan per seed, one
    key column per capacity."""
    rng = np.random.default_rng(1000 + seed)
    n = 100
    cols = {}
    for j, cap in enumerate(CAPS):
        distinct = set()
        while len(distinct) < cap:
            distinct.add(int(rng.integers(-2**61, 2**61)))
        distinct = np.array(sorted(distinct), dtype=np.int64)
        pick = np.concatenate([np.arange(cap), rng.integers(0, cap, n - cap)])
        cols[j] = distinct[rng.permutation(pick)]
    vcol = len(CAPS)
    cols[vcol] = rng.integers(-2**40, 2**40, n).astype(np.int64)
    defs = [(f"k{j}", ca.I64, 0) for j in range(len(CAPS))] + [("v", ca.I64, 0)]
    path = str(tmp_path / "s.cs")
    ca.write_table(path, defs, [cols[j] for j in range(vcol + 1)],
                   compression=ca.COMP_NONE)
    aggs = [(ca.AGG_COUNT_STAR, -1), (ca.AGG_SUM_I64, vcol)]
    r, s = open_scan(path, (1 << (vcol + 1)) - 1)
    try:
        for j, cap in enumerate(CAPS):
            res = s.agg_hashed(aggs, [j], cap)
            assert res["n_groups"] == cap
            check(res, ref_groups([j], np.ones(n, bool), aggs, cols), aggs)
    finally:
        s.end()
        r.close()


# ---------------- capacity errors ----------------

def test_capacity_errors(tmp_path):
    n = 6000
    k1000 = (np.arange(n) % 1000).astype(np.int64) * 7 - 3000
    k5000 = (np.arange(n) % 5000).astype(np.int64)
    v = np.ones(n, dtype=np.int64)
    path = str(tmp_path / "cap.cs")
    ca.write_table(path, [("a", ca.I64, 0), ("b", ca.I64, 0), ("v", ca.I64, 0)],
                   [k1000, k5000, v], compression=ca.COMP_LZ4)
    aggs = [(ca.AGG_COUNT_STAR, -1), (ca.AGG_SUM_I64, 2)]
    cols = {0: k1000, 1: k5000, 2: v}
    r, s = open_scan(path, 0b111)
    try:
        # 1000 groups into capacity 999: the table (2048 slots) does not
        # fill, so the message names the exact count and the capacity
        with pytest.raises(ca.CStripeError) as ei:
            s.agg_hashed(aggs, [0], 999)
        assert "rc=-5" in str(ei.value)
        assert "1000" in str(ei.value) and "999" in str(ei.value)
        res = s.agg_hashed(aggs, [0], 1000)
        check(res, ref_groups([0], np.ones(n, bool), aggs, cols), aggs)
        # 5000 groups into capacity 1000: the 2048-slot table fills; every
        # probe loop is bounded, so the call returns
        with pytest.raises(ca.CStripeError) as ei:
            s.agg_hashed(aggs, [1], 1000)
        assert "rc=-5" in str(ei.value) and "more than 2048 groups" in str(ei.value)
        # the scan is still usable afterwards
        res = s.agg_hashed(aggs, [1], 5000)
        assert res["n_groups"] == 5000
        for bad in (0, ca.MAX_HASH_GROUPS + 1):
            with pytest.raises(ca.CStripeError, match="rc=-5"):
                s.agg_hashed(aggs, [0], bad)
    finally:
        s.end()
        r.close()


# ---------------- keys ----------------

def test_null_keys_and_all_null_chunk_group(tmp_path):
    """NULL keys form their own group (sorted last); chunk group 1 holds
    nothing but NULL keys (no min/max in its skip node); NULL aggregate
    operands give is_null partials with COUNT 0."""
    n = 9000
    rng = np.random.default_rng(41)
    k = rng.integers(-50, 50, n).astype(np.int64)
    nk = (rng.random(n) < 0.2).astype(np.uint8)
    nk[3000:6000] = 1
    v = rng.integers(-2**40, 2**40, n).astype(np.int64)
    nv = (rng.random(n) < 0.3).astype(np.uint8)
    nv[k == 7] = 1                       # a whole group of NULL operands
    path = str(tmp_path / "nk.cs")
    ca.write_table(path, [("k", ca.I64, 0), ("v", ca.I64, 0)], [k, v],
                   nulls=[nk, nv], compression=ca.COMP_LZ4,
                   chunk_group_row_limit=3000)
    aggs = [(ca.AGG_COUNT_STAR, -1), (ca.AGG_COUNT_COL, 1), (ca.AGG_SUM_I64, 1),
            (ca.AGG_MIN_I64, 1)]
    res = hashed(path, 0b11, aggs, [0], 128)
    exp = ref_groups([0], np.ones(n, bool), aggs, {0: k, 1: v}, {0: nk, 1: nv})
    check(res, exp, aggs)
    assert result_keys(res)[-1] == (None,)
    g7 = result_keys(res).index((7,))
    assert res["partials"][g7, 2]["is_null"] == 1
    assert res["partials"][g7, 1]["is_null"] == 0 and res["partials"][g7, 1]["count"] == 0


def test_only_null_keys(tmp_path):
    n = 500
    k = np.zeros(n, dtype=np.int32)
    v = np.arange(n, dtype=np.int64)
    path = str(tmp_path / "on.cs")
    ca.write_table(path, [("k", ca.I32, 0), ("v", ca.I64, 0)], [k, v],
                   nulls=[np.ones(n, dtype=np.uint8), None])
    res = hashed(path, 0b11, SC, [0], 1)
    assert result_keys(res) == [(None,)]
    assert res["partials"][0, 0]["count"] == n
    assert ca.partial_i128(res["partials"][0, 1]) == n * (n - 1) // 2


@pytest.mark.parametrize("key_cols", [(0, 3), (4, 1, 2), (2, 4, 0, 1), (3,)])
def test_mixed_type_key_columns(tmp_path, key_cols):
    """I8 / I16 / I32 / I64 / TEXT keys, negative values, NULLs in two of
    them, a predicate on the measure; keys equal to each recorded min/max"""
    n = 12001
    rng = np.random.default_rng(43)
    c8 = rng.integers(-128, -120, n).astype(np.int8)
    c16 = rng.integers(-3, 3, n).astype(np.int16)
    c32 = (rng.integers(0, 4, n) * 1000 - 2**31).astype(np.int32)
    c64 = (rng.integers(0, 5, n) - 2).astype(np.int64) * 10**12
    txt = ca.text_slots([["A", "N", "R", "xy", "abc"][j]
                         for j in rng.integers(0, 5, n)])
    v = rng.integers(1, 10**9, n).astype(np.int64)
    n16 = (rng.random(n) < 0.1).astype(np.uint8)
    ntx = (rng.random(n) < 0.1).astype(np.uint8)
    defs = [("a", ca.I8, 0), ("b", ca.I16, 0), ("c", ca.I32, 0),
            ("d", ca.I64, 0), ("t", ca.TEXT, 0), ("v", ca.I64, 0)]
    cols = {0: c8, 1: c16, 2: c32, 3: c64, 4: txt, 5: v}
    nulls = {1: n16, 4: ntx}
    path = str(tmp_path / "mixed.cs")
    ca.write_table(path, defs, [cols[c] for c in range(6)],
                   nulls=[nulls.get(c) for c in range(6)],
                   compression=ca.COMP_LZ4, chunk_group_row_limit=5000)
    aggs = [(ca.AGG_COUNT_STAR, -1), (ca.AGG_SUM_I64, 5), (ca.AGG_MAX_I64, 5)]
    preds = [(5, ca.PRED_GE, 10**8)]
    res = hashed(path, 0x3F, aggs, list(key_cols), 4096, preds)
    exp = ref_groups(list(key_cols), v >= 10**8, aggs, cols, nulls)
    check(res, exp, aggs)
    assert res["n_groups"] > 4 or len(key_cols) == 1


def test_two_text_key_columns_pack_by_order_key(tmp_path):
    """two TEXT keys are 66 bits as whole slots; they pack by the order key
    the skip nodes record instead. Keys still come back as slots, sorted by
    slot value; a slot that is no canonical short varlena cannot pack."""
    n = 9001
    rng = np.random.default_rng(45)
    words = ["A", "N", "R", "xy", "abc", "b"]
    t0 = ca.text_slots([words[j] for j in rng.integers(0, 6, n)])
    t1 = ca.text_slots([["O", "F", "zz"][j] for j in rng.integers(0, 3, n)])
    nt1 = (rng.random(n) < 0.1).astype(np.uint8)
    v = rng.integers(-2**40, 2**40, n).astype(np.int64)
    defs = [("t0", ca.TEXT, 0), ("t1", ca.TEXT, 0), ("v", ca.I64, 0)]
    path = str(tmp_path / "tt.cs")
    ca.write_table(path, defs, [t0, t1, v], nulls=[None, nt1, None],
                   compression=ca.COMP_ZSTD, chunk_group_row_limit=2000)
    aggs = [(ca.AGG_COUNT_STAR, -1), (ca.AGG_SUM_I64, 2)]
    res = hashed(path, 0b111, aggs, [0, 1], 64)
    check(res, ref_groups([0, 1], np.ones(n, bool), aggs, {0: t0, 1: t1, 2: v},
                          {1: nt1}), aggs)
    assert res["n_groups"] == 6 * 4
    bad = t0.copy()
    bad[5000] = 0x00004107            # header says 2 payload bytes, only 'A' there
    path = str(tmp_path / "bad.cs")
    ca.write_table(path, defs, [bad, t1, v], compression=ca.COMP_NONE)
    with pytest.raises(ca.CStripeError, match="rc=-5"):
        hashed(path, 0b111, aggs, [0, 1], 64)
    # one TEXT key still groups by whole slot, whatever the slot holds
    res = hashed(path, 0b111, aggs, [0], 64)
    check(res, ref_groups([0], np.ones(n, bool), aggs, {0: bad, 2: v}), aggs)


def test_argument_errors(tmp_path):
    n = 100
    k = np.arange(n, dtype=np.int64)
    f = np.arange(n, dtype=np.float64)
    f32 = np.arange(n, dtype=np.float32)
    path = str(tmp_path / "arg.cs")
    ca.write_table(path, [("k", ca.I64, 0), ("f", ca.F64, 0), ("g", ca.F32, 0),
                          ("u", ca.I64, 0)], [k, f, f32, k.copy()])
    r, s = open_scan(path, 0b0111)
    try:
        agg = [(ca.AGG_COUNT_STAR, -1)]
        for keys in ([1], [2], [0, 1], [], [0, 0, 0, 0, 0], [3], [9]):
            with pytest.raises(ca.CStripeError, match="rc=-5"):
                s.agg_hashed(agg, keys, 128)
        assert s.agg_hashed(agg, [0, 0, 0, 0], 128)["n_groups"] == n
    finally:
        s.end()
        r.close()


# ---------------- the 63-bit key budget ----------------

def one_col_table(tmp_path, name, arrs, **kw):
    path = str(tmp_path / name)
    defs = [(f"c{j}", ca.I64, 0) for j in range(len(arrs))]
    ca.write_table(path, defs, list(arrs), **kw)
    return path


def test_bit_budget(tmp_path):
    agg = [(ca.AGG_COUNT_STAR, -1)]
    base = np.array([0, 5, 2**40, 5, 0], dtype=np.int64)
    # lo = 0, hi = 2^63 - 2: codes need exactly 63 bits
    a = base.copy()
    a[2] = 2**63 - 2
    res = hashed(one_col_table(tmp_path, "b63.cs", [a]), 1, agg, [0], 8)
    assert result_keys(res) == [(0,), (5,), (2**63 - 2,)]
    assert res["partials"]["count"][:, 0].tolist() == [2, 2, 1]
    # hi = 2^63 - 1: 64 bits, no room for the EMPTY marker
    b = base.copy()
    b[2] = 2**63 - 1
    with pytest.raises(ca.CStripeError) as ei:
        hashed(one_col_table(tmp_path, "b64.cs", [b]), 1, agg, [0], 8)
    assert "rc=-5" in str(ei.value) and "64 bits" in str(ei.value)
    # two columns of range 2^40 each: 41 + 41 bits
    c = np.array([0, 2**40 - 1, 17], dtype=np.int64)
    path = one_col_table(tmp_path, "b2.cs", [c, c[::-1].copy()])
    with pytest.raises(ca.CStripeError) as ei:
        hashed(path, 0b11, agg, [0, 1], 8)
    assert "rc=-5" in str(ei.value) and "41 bits" in str(ei.value)
    assert hashed(path, 0b11, agg, [0], 8)["n_groups"] == 3


def test_key_range_comes_from_selected_chunk_groups_only(tmp_path):
    """the table's full key range does not fit 63 bits, but the predicate
    prunes it to chunk groups that do"""
    n = 3000
    k = (np.arange(n) % 10).astype(np.int64)
    k[1000:2000] = np.where(np.arange(1000) % 2 == 0, -2**63, 2**63 - 1)
    p = np.zeros(n, dtype=np.int64)
    p[1000:2000] = 1
    path = str(tmp_path / "pr.cs")
    ca.write_table(path, [("k", ca.I64, 0), ("p", ca.I64, 0)], [k, p],
                   chunk_group_row_limit=1000)
    with pytest.raises(ca.CStripeError, match="rc=-5"):
        hashed(path, 0b11, SC, [0], 64)
    r, s = open_scan(path, 0b11, [(1, ca.PRED_EQ, 0)])
    try:
        assert s.chunk_groups_filtered == 1
        res = s.agg_hashed(SC, [0], 64)
    finally:
        s.end()
        r.close()
    check(res, ref_groups([0], p == 0, SC, {0: k, 1: p}), SC)


def test_zero_groups(tmp_path):
    n = 2000
    k = np.arange(n, dtype=np.int64)
    path = one_col_table(tmp_path, "z.cs", [k, k.copy()])
    # every chunk group pruned
    res = hashed(path, 0b11, SC, [0], 16, [(0, ca.PRED_LT, -5)])
    assert res["n_groups"] == 0 and res["partials"].shape == (0, 2)
    # chunk survives min/max, no row passes
    k2 = (np.arange(n) * 2).astype(np.int64)
    path = one_col_table(tmp_path, "z2.cs", [k2, k2.copy()])
    res = hashed(path, 0b11, SC, [0], 16, [(0, ca.PRED_EQ, 777)])
    assert res["n_groups"] == 0


# ---------------- every stream shape of the key column ----------------

@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("comp,canonical", [
    (ca.COMP_NONE, 1), (ca.COMP_LZ4, 1), (ca.COMP_LZ4, 0),
    (ca.COMP_ZSTD, 1), (ca.COMP_ZSTD, 0)])
def test_key_stream_shapes(tmp_path, comp, canonical, sparse):
    """raw, canonical P / CONST / width-4 flag frames, greedy LZ4, generic
    zstd — dense, and sparse (NULLs: rank-indexed value streams)"""
    n = 25017
    rng = np.random.default_rng(47)
    pe = (10**9 + rng.integers(0, 300, n)).astype(np.int64)     # shared high bytes
    const = np.full(n, -424242, dtype=np.int64)
    flag = ca.text_slots([["A", "N", "R"][j] for j in rng.integers(0, 3, n)])
    i8 = rng.integers(-3, 3, n).astype(np.int8)
    v = rng.integers(1, 2**45, n).astype(np.int64)
    cols = {0: pe, 1: const, 2: flag, 3: i8, 4: v}
    nulls = {}
    if sparse:
        nulls = {c: (rng.random(n) < 0.15).astype(np.uint8) for c in (0, 2, 3)}
    defs = [("pe", ca.I64, 0), ("c", ca.I64, 0), ("f", ca.TEXT, 0),
            ("b", ca.I8, 0), ("v", ca.I64, 0)]
    path = str(tmp_path / "shape.cs")
    ca.write_table(path, defs, [cols[c] for c in range(5)],
                   nulls=[nulls.get(c) for c in range(5)] if sparse else None,
                   compression=comp, canonical=canonical)
    aggs = [(ca.AGG_COUNT_STAR, -1), (ca.AGG_SUM_I64, 4)]
    r, s = open_scan(path, 0b11111)
    try:
        res_pe = s.agg_hashed(aggs, [0], 512)
        res_mix = s.agg_hashed(aggs, [2, 3, 1], 64)
    finally:
        s.end()
        r.close()
    every = np.ones(n, bool)
    check(res_pe, ref_groups([0], every, aggs, cols, nulls), aggs)
    check(res_mix, ref_groups([2, 3, 1], every, aggs, cols, nulls), aggs)


# ---------------- all 11 aggregate kinds ----------------

@pytest.mark.parametrize("mode", LDS_MODES)
def test_all_agg_kinds(tmp_path, monkeypatch, mode):
    """every kind at once (the runtime-n_aggs kernel): NaN under PG order,
    int128 sums that carry past 64 bits — positive, negative, and both
    signs within one group — NULL operands, positive f64 sums"""
    n = 10001
    rng = np.random.default_rng(53)
    k = rng.integers(0, 4, n).astype(np.int64)
    big = rng.integers(2**61, 2**62, n).astype(np.int64)
    sign = np.where(k == 0, 1, np.where(k == 1, -1, rng.choice([-1, 1], n)))
    a = (big * sign).astype(np.int64)
    a[k == 3] = rng.integers(-1000, 1000, int((k == 3).sum()))
    b = rng.integers(0, 11, n).astype(np.int64)
    c = rng.integers(0, 9, n).astype(np.int64)
    price = rng.integers(1, 10**7, n).astype(np.int64)
    f = rng.random(n) + 0.5                               # positive
    fm = rng.integers(-40, 40, n) / 8.0 + 0.0625          # exact, never -0.0
    fm[rng.random(n) < 0.1] = np.nan
    fm[k == 2] = np.nan                                   # an all-NaN group
    na = (rng.random(n) < 0.1).astype(np.uint8)
    nb = (rng.random(n) < 0.1).astype(np.uint8)
    nf = (rng.random(n) < 0.2).astype(np.uint8)
    cols = {0: k, 1: a, 2: b, 3: c, 4: price, 5: f, 6: fm}
    nulls = {1: na, 2: nb, 6: nf}
    defs = [("k", ca.I64, 0), ("a", ca.I64, 0), ("b", ca.I64, 2), ("c", ca.I64, 2),
            ("p", ca.I64, 2), ("f", ca.F64, 0), ("fm", ca.F64, 0)]
    path = str(tmp_path / "kinds.cs")
    ca.write_table(path, defs, [cols[j] for j in range(7)],
                   nulls=[nulls.get(j) for j in range(7)],
                   compression=ca.COMP_LZ4, chunk_group_row_limit=3000)
    aggs = [(ca.AGG_COUNT_STAR, -1), (ca.AGG_COUNT_COL, 1), (ca.AGG_SUM_I64, 1),
            (ca.AGG_SUM_F64, 5), (ca.AGG_MIN_I64, 1), (ca.AGG_MAX_I64, 1),
            (ca.AGG_MIN_F64, 6), (ca.AGG_MAX_F64, 6),
            (ca.AGG_SUM_PROD_I64, 1, 2), (ca.AGG_SUM_DISC_I64, 4, 2, -1, 100),
            (ca.AGG_SUM_DISC_TAX_I64, 4, 2, 3, 100)]
    set_lds(monkeypatch, mode)
    res = hashed(path, 0x7F, aggs, [0], 16)
    exp = ref_groups([0], np.ones(n, bool), aggs, cols, nulls)
    check(res, exp, aggs)
    # the sums really left 64 bits, in both directions
    assert exp[(0,)][2]["i128"] > 2**64 and exp[(1,)][2]["i128"] < -2**64
    assert math.isnan(exp[(2,)][6]["f64"])                # MIN over only NaN


# ---------------- reference pin: TPC-H Q1 ----------------

def q1_aggs():
    return [(ca.AGG_SUM_I64, 1), (ca.AGG_SUM_I64, 2),
            (ca.AGG_SUM_DISC_I64, 2, 3, -1, 100),
            (ca.AGG_SUM_DISC_TAX_I64, 2, 3, 4, 100),
            (ca.AGG_COUNT_STAR, -1)]


@pytest.mark.parametrize("variant", ["none", "lz4", "zstd"])
def test_q1_reference_pin(golden_dir, expected, variant):
    """hashed GROUP BY (returnflag, linestatus) reproduces the reference's
    own Q1 result table (multi_tpch_query1.out, via expected.json) digit for
    digit, and equals agg_grouped partial for partial"""
    path = os.path.join(golden_dir, f"lineitem12k_{variant}.cs")
    q1 = expected["q1"]
    aggs = q1_aggs()
    preds = [(5, ca.PRED_LE, q1["shipdate_le"])]
    r, s = open_scan(path, ca.agg_cols_mask(aggs) | (1 << 6) | (1 << 7), preds)
    try:
        res = s.agg_hashed(aggs, [6, 7], 64)
        grouped = s.agg_grouped(aggs, (6, 7))
    finally:
        s.end()
        r.close()
    rf = expected["flag_codes"]["returnflag"]
    ls = expected["flag_codes"]["linestatus"]
    want = {(rf[key.split(",")[0]], ls[key.split(",")[1]]): vals
            for key, vals in q1["groups"].items()}
    got = result_keys(res)
    assert got == sorted(want)
    for g, t in enumerate(got):
        p = res["partials"][g]
        assert [ca.partial_i128(p[0]), ca.partial_i128(p[1]), ca.partial_i128(p[2]),
                ca.partial_i128(p[3]), int(p[4]["count"])] == want[t]
        for a in range(len(aggs)):
            q = grouped[t][a]
            assert (int(p[a]["i128_lo"]), int(p[a]["i128_hi"]), int(p[a]["count"]),
                    int(p[a]["is_null"])) == (q.i128_lo, q.i128_hi, q.count, q.is_null)
    assert len(grouped) == len(got)


# ---------------- shards + combine_groups ----------------

def test_shards_group_by_shipdate(tmp_path):
    """2 lineitem shards, GROUP BY l_shipdate: expected from the columns a
    predicate-free select() returns; per-shard results merged by
    combine_groups equal the whole-directory result"""
    d = str(tmp_path / "shards")
    ca.gen_lineitem_shards(d, 20000, 2, chunk_rows=4000)
    aggs = q1_aggs()
    mask = ca.agg_cols_mask(aggs) | (1 << 5)
    r, s = open_scan(d, mask)
    try:
        sel = s.select(cols=[1, 2, 3, 4, 5], want_nulls=False,
                       want_row_numbers=False)
        whole = s.agg_hashed(aggs, [5], 8192)
    finally:
        s.end()
        r.close()
    n = sel["n_rows"]
    assert n == 20000
    cols = {c: np.asarray(a) for c, a in sel["values"].items()}
    check(whole, ref_groups([5], np.ones(n, bool), aggs, cols), aggs)
    assert whole["n_groups"] > 1000
    per_shard = []
    for name in sorted(f for f in os.listdir(d) if f.endswith(".cs")):
        per_shard.append(hashed(os.path.join(d, name), mask, aggs, [5], 8192))
    assert len(per_shard) == 2 and all(p["n_groups"] > 0 for p in per_shard)
    same_result(ca.combine_groups(aggs, 1, per_shard), whole)
    same_result(ca.combine_groups(aggs, 1, per_shard[::-1]), whole)


# ---------------- repeat and interleave ----------------

def test_repeat_and_interleave(tmp_path):
    n = 25017
    rng = np.random.default_rng(59)
    k = rng.integers(0, 3, n).astype(np.int8)
    w = rng.integers(-500, 500, n).astype(np.int64)
    v = rng.integers(-2**40, 2**40, n).astype(np.int64)
    path = str(tmp_path / "il.cs")
    ca.write_table(path, [("k", ca.I8, 0), ("w", ca.I64, 0), ("v", ca.I64, 0)],
                   [k, w, v], compression=ca.COMP_LZ4)
    aggs = [(ca.AGG_COUNT_STAR, -1), (ca.AGG_SUM_I64, 2), (ca.AGG_MIN_I64, 2)]
    preds = [(1, ca.PRED_GE, -400)]
    cols = {0: k, 1: w, 2: v}
    r, s = open_scan(path, 0b111, preds)
    try:
        def others():
            a = [(p.i128, p.count, p.is_null) for p in s.agg(aggs)]
            g = {key: [(p.i128, p.count, p.is_null) for p in ps]
                 for key, ps in s.agg_grouped(aggs, (0,)).items()}
            sl = s.select()
            return a, g, sl
        a0, g0, s0 = others()
        h1 = s.agg_hashed(aggs, [1], 1024)
        assert s.last_kernel_ms > 0 and s.last_hash_ms[1] > 0
        a1, g1, s1 = others()
        h2 = s.agg_hashed(aggs, [1], 1024)
        hk = s.agg_hashed(aggs, [0, 1], 4096)
        h3 = s.agg_hashed(aggs, [1], 2048)        # the table grows in place
        a2, g2, s2 = others()
    finally:
        s.end()
        r.close()
    same_result(h1, h2)
    same_result(h1, h3)
    exp = ref_groups([1], w >= -400, aggs, cols)
    check(h1, exp, aggs)
    check(hk, ref_groups([0, 1], w >= -400, aggs, cols), aggs)
    assert a0 == a1 == a2 and g0 == g1 == g2
    for sa, sb in ((s0, s1), (s0, s2)):
        assert sa["n_rows"] == sb["n_rows"]
        np.testing.assert_array_equal(sa["row_numbers"], sb["row_numbers"])
        for c_ in sa["values"]:
            np.testing.assert_array_equal(sa["values"][c_], sb["values"][c_])
