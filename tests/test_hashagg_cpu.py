"""
CPU tests (no GPU) for the hashed GROUP BY surface: cagg_combine_groups —
the per-group coordinator merge — and the entry-point contract of
cstripe_scan_agg_hashed that holds without a device.

Expected values are computed here in Python ints / dicts from the inputs
the test itself builds, never from the library.
"""
import ctypes as C

import numpy as np
import pytest

import citus_amd as ca

PD = ca.partial_dtype()
M64 = (1 << 64) - 1


def test_partial_dtype_mirrors_the_c_struct():
    assert PD.itemsize == C.sizeof(ca.Partial) == 40
    for name in ("i128_lo", "i128_hi", "f64", "count", "is_null"):
        assert PD.fields[name][1] == getattr(ca.Partial, name).offset


def test_abi_version_is_still_2():
    ca._lib.cstripe_abi_version.restype = C.c_uint32
    assert ca._lib.cstripe_abi_version() == 2


def sum_partial(v, count=1):
    """SUM_I64-style partial holding the signed 128-bit value v"""
    p = np.zeros((), dtype=PD)
    lo = v & M64
    p["i128_lo"] = lo - (1 << 64) if lo >> 63 else lo
    p["i128_hi"] = v >> 64
    p["count"] = count
    return p


def count_partial(n):
    p = np.zeros((), dtype=PD)
    p["i128_lo"] = n
    p["count"] = n
    return p


def null_partial():
    p = np.zeros((), dtype=PD)
    p["is_null"] = 1
    return p


def f64_partial(x, count=1):
    p = np.zeros((), dtype=PD)
    p["f64"] = x
    p["count"] = count
    return p


def make_part(n_key_cols, rows):
    """rows: list of (key tuple with None = NULL, [partial per agg])"""
    n = len(rows)
    n_aggs = len(rows[0][1]) if rows else 1
    keys = [np.zeros(n, dtype=np.int64) for _ in range(n_key_cols)]
    nulls = [np.zeros(n, dtype=np.uint8) for _ in range(n_key_cols)]
    parts = np.zeros((n, n_aggs), dtype=PD)
    for g, (key, ps) in enumerate(rows):
        for k in range(n_key_cols):
            if key[k] is None:
                nulls[k][g] = 1
                keys[k][g] = 12345        # garbage under a NULL must not matter
            else:
                keys[k][g] = key[k]
        for a, p in enumerate(ps):
            parts[g, a] = p
    return {"n_groups": n, "keys": keys, "key_nulls": nulls, "partials": parts}


def result_keys(res, n_key_cols):
    return [tuple(None if res["key_nulls"][k][g] else int(res["keys"][k][g])
                  for k in range(n_key_cols)) for g in range(res["n_groups"])]


def sort_key(t):
    """ascending, signed, per column NULL last"""
    return tuple((1, 0) if v is None else (0, v) for v in t)


AGGS_SC = [(ca.AGG_SUM_I64, 0), (ca.AGG_COUNT_STAR, -1)]


def check_sum_count(res, n_key_cols, inputs):
    """inputs: every (key, sum-or-None, count) fed in, over all parts"""
    exp = {}
    for key, sm, cnt in inputs:
        e = exp.setdefault(key, [None, 0])
        if sm is not None:
            e[0] = sm if e[0] is None else e[0] + sm
        e[1] += cnt
    order = sorted(exp, key=sort_key)
    assert result_keys(res, n_key_cols) == order
    for g, key in enumerate(order):
        sp, cp = res["partials"][g, 0], res["partials"][g, 1]
        if exp[key][0] is None:
            assert sp["is_null"] == 1
        else:
            assert sp["is_null"] == 0 and ca.partial_i128(sp) == exp[key][0]
        assert cp["is_null"] == 0 and cp["count"] == exp[key][1]
        # NULL keys come back as value 0 under key_nulls = 1
        for k in range(n_key_cols):
            if key[k] is None:
                assert res["keys"][k][g] == 0


def rows_of(inputs):
    return [(k, [null_partial() if s is None else sum_partial(s), count_partial(c)])
            for k, s, c in inputs]


def test_disjoint_overlapping_and_duplicate_keys():
    a = [((5,), 10, 1), ((1,), 20, 2), ((9,), 30, 3)]
    b = [((7,), 1, 1), ((1,), 2, 1)]                       # 1 overlaps a
    c = [((9,), 100, 4), ((9,), 1000, 5), ((-3,), 7, 1)]   # 9 twice in one part
    res = ca.combine_groups(AGGS_SC, 1, [make_part(1, rows_of(p)) for p in (a, b, c)])
    assert res["n_groups"] == 5
    check_sum_count(res, 1, a + b + c)


def test_null_keys_merge_and_sort_last():
    a = [((None,), 1, 1), ((2,), 2, 1), ((-2**63,), 3, 1)]
    b = [((2**63 - 1,), 4, 1), ((None,), 5, 2)]
    res = ca.combine_groups(AGGS_SC, 1, [make_part(1, rows_of(p)) for p in (a, b)])
    assert result_keys(res, 1) == [(-2**63,), (2,), (2**63 - 1,), (None,)]
    check_sum_count(res, 1, a + b)


@pytest.mark.parametrize("nk", [1, 2, 3, 4])
def test_one_to_four_key_columns(nk):
    rng = np.random.default_rng(100 + nk)
    vals = [None, -5, 0, 3]
    parts_in = []
    for _ in range(3):
        rows = []
        for _ in range(40):
            key = tuple(vals[i] for i in rng.integers(0, len(vals), nk))
            rows.append((key, int(rng.integers(-1000, 1000)), int(rng.integers(1, 9))))
        parts_in.append(rows)
    res = ca.combine_groups(AGGS_SC, nk, [make_part(nk, rows_of(p)) for p in parts_in])
    check_sum_count(res, nk, [r for p in parts_in for r in p])
    # each distinct tuple exactly once
    ks = result_keys(res, nk)
    assert len(ks) == len(set(ks))


def test_strict_null_partials_and_count_null_to_zero():
    aggs = [(ca.AGG_SUM_I64, 0), (ca.AGG_COUNT_COL, 0), (ca.AGG_MIN_F64, 1)]
    cnull = null_partial()
    a = make_part(1, [((1,), [null_partial(), cnull, null_partial()]),
                      ((2,), [null_partial(), cnull, f64_partial(3.5)])])
    b = make_part(1, [((1,), [null_partial(), cnull, null_partial()]),
                      ((2,), [sum_partial(-4), count_partial(2), null_partial()])])
    res = ca.combine_groups(aggs, 1, [a, b])
    assert result_keys(res, 1) == [(1,), (2,)]
    g1, g2 = res["partials"][0], res["partials"][1]
    # key 1: nothing but NULL partials -> strict aggs NULL, COUNT 0 not NULL
    assert g1[0]["is_null"] == 1 and g1[2]["is_null"] == 1
    assert g1[1]["is_null"] == 0 and g1[1]["count"] == 0
    # key 2: the first non-null partial initialises
    assert g2[0]["is_null"] == 0 and ca.partial_i128(g2[0]) == -4
    assert g2[1]["is_null"] == 0 and g2[1]["count"] == 2
    assert g2[2]["is_null"] == 0 and g2[2]["f64"] == 3.5


def test_int128_carry_across_parts():
    big = 2**63 - 1
    ins = [[((1,), big, 1), ((2,), -2**63, 1)],
           [((1,), big, 1), ((2,), -2**63, 1)],
           [((1,), big, 1), ((2,), -2**63, 1), ((1,), 2**100, 1)]]
    res = ca.combine_groups(AGGS_SC, 1, [make_part(1, rows_of(p)) for p in ins])
    assert ca.partial_i128(res["partials"][0, 0]) == 3 * big + 2**100
    assert ca.partial_i128(res["partials"][1, 0]) == -3 * 2**63
    assert res["partials"][0, 0]["i128_hi"] != 0        # carried past 64 bits
    check_sum_count(res, 1, [r for p in ins for r in p])


def test_float_min_max_follow_pg_nan_order():
    aggs = [(ca.AGG_MIN_F64, 0), (ca.AGG_MAX_F64, 0)]
    nan = float("nan")
    a = make_part(1, [((1,), [f64_partial(nan), f64_partial(2.0)])])
    b = make_part(1, [((1,), [f64_partial(7.0), f64_partial(nan)])])
    res = ca.combine_groups(aggs, 1, [a, b])
    assert res["partials"][0, 0]["f64"] == 7.0          # NaN is the greatest
    assert np.isnan(res["partials"][0, 1]["f64"])


def test_output_sorted_signed_with_column_0_most_significant():
    rng = np.random.default_rng(5)
    rows = [((int(a), int(b)), 1, 1)
            for a, b in zip(rng.integers(-4, 4, 200), rng.integers(-2**62, 2**62, 200))]
    rows += [((None, 1), 1, 1), ((0, None), 1, 1), ((None, None), 1, 1)]
    order = rng.permutation(len(rows))
    shuffled = [rows[i] for i in order]
    res = ca.combine_groups(AGGS_SC, 2, [make_part(2, rows_of(shuffled[:90])),
                                         make_part(2, rows_of(shuffled[90:]))])
    ks = result_keys(res, 2)
    assert ks == sorted(set(r[0] for r in rows), key=sort_key)
    assert ks[-1] == (None, None)


def test_empty_inputs_give_zero_groups():
    res = ca.combine_groups(AGGS_SC, 1, [])
    assert res["n_groups"] == 0
    empty = make_part(1, [])
    empty["partials"] = np.zeros((0, 2), dtype=PD)
    res = ca.combine_groups(AGGS_SC, 1, [empty, empty])
    assert res["n_groups"] == 0


def test_capacity_error_reports_the_needed_count_and_writes_nothing():
    a = rows_of([((k,), k, 1) for k in range(10)])
    b = rows_of([((k,), k, 1) for k in range(5, 17)])       # union: 17 keys
    parts = [make_part(1, a), make_part(1, b)]
    with pytest.raises(ca.CStripeError) as ei:
        ca.combine_groups(AGGS_SC, 1, parts, capacity=16)
    assert "17" in str(ei.value) and "16" in str(ei.value)
    assert ca.combine_groups(AGGS_SC, 1, parts, capacity=17)["n_groups"] == 17

    # raw ABI: out->n_groups carries the needed count, nothing else is written
    arr = ca.make_aggs(AGGS_SC)
    hparts = (ca.HGroups * 2)()
    for i, p in enumerate(parts):
        hparts[i].n_groups = p["n_groups"]
        hparts[i].keys[0] = p["keys"][0].ctypes.data
        hparts[i].key_nulls[0] = p["key_nulls"][0].ctypes.data
        hparts[i].partials = p["partials"].ctypes.data
    ok = np.full(16, -77, dtype=np.int64)
    on = np.full(16, 9, dtype=np.uint8)
    op = np.zeros((16, 2), dtype=PD)
    op["count"] = -77
    out = ca.HGroups()
    out.keys[0], out.key_nulls[0], out.partials = ok.ctypes.data, on.ctypes.data, op.ctypes.data
    rc = ca._combine_groups(arr, 2, 1, hparts, 2, C.byref(out), 16)
    assert rc == ca.ERR_ARG
    assert out.n_groups == 17
    assert (ok == -77).all() and (on == 9).all() and (op["count"] == -77).all()


def test_bad_key_column_counts_are_rejected():
    p = make_part(1, rows_of([((1,), 1, 1)]))
    for nk in (0, 5):
        with pytest.raises(ca.CStripeError):
            ca.combine_groups(AGGS_SC, nk, [p])


def test_agg_hashed_on_an_unstaged_scan_is_err_nogpu(tmp_path):
    """the staged check comes first — before any argument check"""
    path = str(tmp_path / "t.cs")
    k = np.arange(100, dtype=np.int64) % 7
    ca.write_table(path, [("k", ca.I64, 0)], [k])
    with ca.Reader(path) as r, r.scan(cols_mask=1) as s:
        arr = ca.make_aggs([(ca.AGG_COUNT_STAR, -1)])
        kc = (C.c_uint32 * 1)(0)
        out = ca.HGroups()
        assert ca._scan_agg_hashed(s._h, arr, 1, kc, 1, 16, C.byref(out)) == ca.ERR_NOGPU
        # even with arguments that would otherwise be ERR_ARG
        assert ca._scan_agg_hashed(s._h, arr, 1, kc, 0, 0, C.byref(out)) == ca.ERR_NOGPU
        with pytest.raises(ca.CStripeError, match="not staged"):
            s.agg_hashed([(ca.AGG_COUNT_STAR, -1)], [0], 16)
        i, sc, c = s.last_hash_ms
        assert (i, sc, c) == (0.0, 0.0, 0.0)
