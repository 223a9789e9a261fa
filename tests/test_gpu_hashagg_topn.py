"""
GPU tests (@pytest.mark.gpu) for cstripe_scan_agg_hashed_topn — GROUP BY ...
[HAVING] ORDER BY ... LIMIT over the device group table (gtopn_range /
gtopn_key / radix select / gtopn_gather kernels) — and merge_groups_topn.

Expected results come from gtutil: numpy / Python ints over the arrays the
test itself wrote (group in a dict, exact Python-int sums, HAVING, the
documented total order, a slice), never from the library. Everything is
compared exactly; SUM_F64 runs over integer-valued doubles, whose sums are
exact in any order.
"""
import ctypes as C
import os

import numpy as np
import pytest

import citus_amd as ca
import gtutil as gt

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_MODES = [None, "0", "16"]
OPS = (ca.PRED_LT, ca.PRED_LE, ca.PRED_GT, ca.PRED_GE, ca.PRED_EQ, ca.PRED_NE)
CS = [(ca.AGG_COUNT_STAR, -1), (ca.AGG_SUM_I64, 1)]
KV = [("k", ca.I64, 0), ("v", ca.I64, 0)]


@pytest.fixture(scope="module", autouse=True)
def require_gpu():
    assert ca.gpu_available(), "MI355X required for these tests"


def set_lds(monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv("CSTRIPE_HASH_LDS_SLOTS", raising=False)
    else:
        monkeypatch.setenv("CSTRIPE_HASH_LDS_SLOTS", mode)


class staged:
    """with staged(path, mask, preds, lookups) as s: a staged scan"""

    def __init__(self, path, cols_mask, preds=(), lookups=()):
        self.r = ca.Reader(path)
        self.s = self.r.scan(cols_mask=cols_mask, preds=preds, lookups=lookups)

    def __enter__(self):
        self.s.stage()
        return self.s

    def __exit__(self, *a):
        self.s.end()
        self.r.close()


def run_case(s, groups, aggs, key_cols, cap, order, limit, having=()):
    """one call, checked against the reference; returns the result"""
    res = s.agg_hashed_topn(aggs, key_cols, cap, order, limit, having=having)
    want = gt.ref_topn(groups, aggs, order, limit, having)
    gt.check_topn(res, groups, want, aggs)
    n_groups, n_kept = s.last_group_topn[:2]
    assert n_groups == len(groups)
    assert n_kept == len(gt.ref_having(groups, aggs, having))
    return res


# ---------------- wave, tile and chunk-group edges; limits around the count ----------------

EDGE_RNG = np.random.default_rng(31)


@pytest.mark.parametrize("n", [1, 64, 65, 4097, 10001])
def test_edges(tmp_path, monkeypatch, n):
    """64-row waves, 4096-row tiles, default and 1 000-row chunk groups; more
    groups (up to 300) than one 256-thread block of the group kernels; limit
    1, groups - 1, groups, groups + 1"""
    set_lds(monkeypatch, None)
    m = min(n, 300)
    k = (np.arange(n) * 7 % m).astype(np.int64)
    v = EDGE_RNG.integers(-2**30, 2**30, n).astype(np.int64)
    groups = gt.ref_groups([0], CS, {0: k, 1: v})
    assert len(groups) == m
    for cg in (10000, 1000):
        path = str(tmp_path / f"e{cg}.cs")
        ca.write_table(path, KV, [k, v], chunk_group_row_limit=cg)
        with staged(path, 0b11) as s:
            for limit in sorted({1, m - 1, m, m + 1} - {0}):
                for order in ([("agg", 1, "desc")], [("agg", 0), ("agg", 1)]):
                    run_case(s, groups, CS, [0], 512, order, limit)


def test_lds_modes_agree(tmp_path, monkeypatch):
    n = 10001
    k = (np.arange(n) % 97).astype(np.int64)
    v = EDGE_RNG.integers(-2**30, 2**30, n).astype(np.int64)
    path = str(tmp_path / "lds.cs")
    ca.write_table(path, KV, [k, v])
    groups = gt.ref_groups([0], CS, {0: k, 1: v})
    with staged(path, 0b11) as s:
        results = []
        for mode in LDS_MODES:
            set_lds(monkeypatch, mode)
            # 10 001 = 97 * 103 + 10: ten groups count 104 and survive
            results.append(run_case(s, groups, CS, [0], 128, [("agg", 1, "desc")], 4,
                                    having=[(0, ca.PRED_GT, 103)]))
            results.append(run_case(s, groups, CS, [0], 128, [("agg", 1), ("key", 0)], 40))
    for i in (2, 4):
        gt.same_bytes(results[0], results[i])
        gt.same_bytes(results[1], results[i + 1])


# ---------------- a tie straddling the limit ----------------

def test_tie_straddles_the_limit(tmp_path):
    """ORDER BY count(*): most of the 80 groups share the threshold count, so
    the cut and the output order inside it follow the key tuple, NULL last;
    three calls return the same bytes"""
    rows_a, rows_b, na, nb = [], [], [], []
    for a in range(-1, 9):                  # -1 stands for NULL
        for b in range(-1, 7):
            cnt = 5 if (a + b) % 9 == 0 else (1 if (a * b) % 7 == 3 else 3)
            rows_a += [max(a, 0)] * cnt
            rows_b += [max(b, 0) * 1000] * cnt
            na += [1 if a < 0 else 0] * cnt
            nb += [1 if b < 0 else 0] * cnt
    perm = np.random.default_rng(5).permutation(len(rows_a))
    ka, kb = np.array(rows_a, np.int64)[perm], np.array(rows_b, np.int64)[perm]
    na, nb = np.array(na, np.uint8)[perm], np.array(nb, np.uint8)[perm]
    v = np.arange(len(ka), dtype=np.int64)
    path = str(tmp_path / "tie.cs")
    defs = [("a", ca.I64, 0), ("b", ca.I64, 0), ("v", ca.I64, 0)]
    ca.write_table(path, defs, [ka, kb, v], nulls=[na, nb, None], chunk_group_row_limit=100)
    aggs = [(ca.AGG_COUNT_STAR, -1), (ca.AGG_SUM_I64, 2)]
    groups = gt.ref_groups([0, 1], aggs, {0: ka, 1: kb, 2: v}, {0: na, 1: nb})
    counts = sorted(es[0]["v"] for es in groups.values())
    assert len(groups) == 80 and counts.count(3) > 40
    with staged(path, 0b111) as s:
        for order in ([("agg", 0, "desc")], [("agg", 0)]):
            for limit in (20, 33, 47):
                want = gt.ref_topn(groups, aggs, order, limit)
                assert groups[want[-1]][0]["v"] == 3      # the cut is inside the tie
                got = [run_case(s, groups, aggs, [0, 1], 128, order, limit)
                       for _ in range(3)]
                gt.same_bytes(got[0], got[1])
                gt.same_bytes(got[0], got[2])
        # NULL keys really are among the tied groups that were taken and cut
        want = gt.ref_topn(groups, aggs, [("agg", 0, "desc")], 47)
        assert any(None in t for t in want)


# ---------------- every radix round decides ----------------

@pytest.mark.parametrize("direction", ["asc", "desc"])
def test_radix_digits(tmp_path, direction):
    """group sums spread over 47 bits with neighbours of the threshold at
    every digit distance (T +- 256^j), so each of the six rounds of the order
    word separates some group from the threshold"""
    T = 0x2A5A5A5A5A5A
    rng = np.random.default_rng(8)
    sums = {T}
    for j in range(6):
        sums |= {T + 256**j, T - 256**j}
    while len(sums) < 300:
        sums.add(int(rng.integers(-2**46, 2**46)))
    sums = sorted(sums)
    k = np.repeat(np.arange(len(sums), dtype=np.int64), 2)
    half = np.array([s // 2 for s in sums], dtype=np.int64)
    v = np.stack([half, np.array(sums, dtype=np.int64) - half], axis=1).reshape(-1)
    perm = rng.permutation(len(k))
    k, v = k[perm], v[perm]
    path = str(tmp_path / "radix.cs")
    ca.write_table(path, KV, [k, v], chunk_group_row_limit=100)
    groups = gt.ref_groups([0], CS, {0: k, 1: v})
    rank = sums.index(T) if direction == "asc" else len(sums) - 1 - sums.index(T)
    with staged(path, 0b11) as s:
        for limit in range(rank - 5, rank + 8):
            run_case(s, groups, CS, [0], 512, [("agg", 1, direction)], limit)


# ---------------- every aggregate kind as the order term ----------------

def kinds_table(tmp_path_factory):
    n, ng = 2000, 24
    rng = np.random.default_rng(12)
    g = (np.arange(n) % ng).astype(np.int64)
    a = rng.integers(-500, 500, n).astype(np.int64)
    b = rng.integers(0, 11, n).astype(np.int64)
    c = rng.integers(0, 9, n).astype(np.int64)
    fi = rng.integers(-1000, 1000, n).astype(np.float64)     # integer-valued doubles
    f = rng.integers(-50, 50, n).astype(np.float64) / 4
    an = (rng.random(n) < 0.2).astype(np.uint8)
    fn = (rng.random(n) < 0.2).astype(np.uint8)
    an[g == 0] = 1                          # group 0: every operand NULL
    fn[g == 0] = 1
    a[g == 7] = 3                           # groups 7 and 8 tie on most kinds
    a[g == 8] = 3
    an[g == 7] = an[g == 8] = 0
    f[g == 1] = np.nan
    f[g == 2] = np.inf
    f[(g == 2) & (np.arange(n) % 48 == 2)] = 1.0
    f[g == 3] = -np.inf
    f[g == 4] = -0.0
    f[g == 5] = 0.0
    f[(g == 6) & (np.arange(n) % 48 == 6)] = np.nan
    fn[(g >= 1) & (g <= 6)] = 0
    path = str(tmp_path_factory.mktemp("kinds") / "kinds.cs")
    defs = [("g", ca.I64, 0), ("a", ca.I64, 0), ("b", ca.I64, 0), ("c", ca.I64, 0),
            ("fi", ca.F64, 0), ("f", ca.F64, 0)]
    ca.write_table(path, defs, [g, a, b, c, fi, f], nulls=[None, an, None, None, fn, fn],
                   chunk_group_row_limit=500)
    return path, {0: g, 1: a, 2: b, 3: c, 4: fi, 5: f}, {1: an, 4: fn, 5: fn}


@pytest.fixture(scope="module")
def kinds_tab(tmp_path_factory):
    return kinds_table(tmp_path_factory)


KIND_SPECS = {
    ca.AGG_COUNT_STAR: (ca.AGG_COUNT_STAR, -1), ca.AGG_COUNT_COL: (ca.AGG_COUNT_COL, 1),
    ca.AGG_SUM_I64: (ca.AGG_SUM_I64, 1), ca.AGG_SUM_F64: (ca.AGG_SUM_F64, 4),
    ca.AGG_MIN_I64: (ca.AGG_MIN_I64, 1), ca.AGG_MAX_I64: (ca.AGG_MAX_I64, 1),
    ca.AGG_MIN_F64: (ca.AGG_MIN_F64, 5), ca.AGG_MAX_F64: (ca.AGG_MAX_F64, 5),
    ca.AGG_SUM_PROD_I64: (ca.AGG_SUM_PROD_I64, 1, 2),
    ca.AGG_SUM_DISC_I64: (ca.AGG_SUM_DISC_I64, 1, 2, -1, 100),
    ca.AGG_SUM_DISC_TAX_I64: (ca.AGG_SUM_DISC_TAX_I64, 1, 2, 3, 100),
}


@pytest.mark.parametrize("kind", gt.ALL_KINDS)
def test_every_kind_as_order_term(kinds_tab, kind):
    path, cols, nulls = kinds_tab
    aggs = [KIND_SPECS[kind], (ca.AGG_COUNT_STAR, -1)]
    groups = gt.ref_groups([0], aggs, cols, nulls)
    if kind not in gt.COUNT_KINDS:
        assert groups[(0,)][0]["null"]                      # the all-NULL group
    with staged(path, 0b111111) as s:
        for opts in (("asc",), ("desc",), ("asc", "nulls_first"), ("desc", "nulls_first")):
            for limit in (1, 9, 24, 30):
                run_case(s, groups, aggs, [0], 64, [("agg", 0) + opts], limit)


def test_f64_specials_order(kinds_tab):
    """MAX_F64 DESC: NaN first, then +inf, ..., -0.0 and +0.0 tie (key order),
    -inf, the NULL group last"""
    path, cols, nulls = kinds_tab
    aggs = [(ca.AGG_MAX_F64, 5)]
    with staged(path, 0b100001) as s:
        res = s.agg_hashed_topn(aggs, [0], 64, [("agg", 0, "desc")], 24)
    keys = res["keys"][0].tolist()
    assert keys[:3] == [1, 6, 2] and keys[-2:] == [3, 0]
    assert keys.index(5) == keys.index(4) + 1
    assert res["partials"][-1, 0]["is_null"] == 1


# ---------------- mixed terms ----------------

def test_mixed_key_only_and_no_terms(tmp_path):
    n = 6000
    rng = np.random.default_rng(14)
    a = rng.integers(-4, 5, n).astype(np.int32)
    b = rng.integers(0, 12, n).astype(np.int16)
    v = rng.integers(0, 3, n).astype(np.int64)           # small sums: many ties
    na = (rng.random(n) < 0.1).astype(np.uint8)
    nb = (rng.random(n) < 0.1).astype(np.uint8)
    path = str(tmp_path / "mixed.cs")
    defs = [("a", ca.I32, 0), ("b", ca.I16, 0), ("v", ca.I64, 0)]
    ca.write_table(path, defs, [a, b, v], nulls=[na, nb, None], chunk_group_row_limit=1000)
    aggs = [(ca.AGG_SUM_I64, 2), (ca.AGG_COUNT_STAR, -1)]
    groups = gt.ref_groups([0, 1], aggs, {0: a, 1: b, 2: v}, {0: na, 1: nb})
    assert len(groups) == 130
    orders = [[("agg", 1, "desc"), ("key", 1)],
              [("agg", 1, "desc"), ("key", 1, "desc", "nulls_first"), ("key", 0, "desc")],
              [("key", 1, "desc"), ("key", 0)],
              [("key", 0, "asc", "nulls_first")],
              [("key", 1), ("agg", 0, "desc"), ("agg", 1), ("key", 0, "desc")],
              []]
    with staged(path, 0b111) as s:
        for order in orders:
            for limit in (7, 64, 130, 200):
                run_case(s, groups, aggs, [0, 1], 256, order, limit)


# ---------------- HAVING ----------------

@pytest.fixture(scope="module")
def having_tab(tmp_path_factory):
    n, ng = 3000, 40
    rng = np.random.default_rng(16)
    k = rng.integers(0, ng, n).astype(np.int64)
    v = rng.integers(-100, 100, n).astype(np.int64)
    f = rng.integers(-40, 40, n).astype(np.float64) / 8
    fn = (rng.random(n) < 0.3).astype(np.uint8)
    fn[k == 3] = 1                          # a NULL f64 max
    f[(k == 5) & (fn == 0)] = np.nan
    path = str(tmp_path_factory.mktemp("having") / "having.cs")
    ca.write_table(path, [("k", ca.I64, 0), ("v", ca.I64, 0), ("f", ca.F64, 0)],
                   [k, v, f], nulls=[None, None, fn], chunk_group_row_limit=1000)
    aggs = [(ca.AGG_COUNT_STAR, -1), (ca.AGG_SUM_I64, 1), (ca.AGG_MAX_F64, 2)]
    return path, aggs, gt.ref_groups([0], aggs, {0: k, 1: v, 2: f}, {2: fn})


@pytest.mark.parametrize("op", OPS)
def test_having_ops(having_tab, op):
    """each operator against a constant some group holds exactly, on a count,
    an int sum and an f64 max; then two atoms ANDed"""
    path, aggs, groups = having_tab
    consts = [groups[(11,)][0]["v"], groups[(12,)][1]["v"], groups[(13,)][2]["v"]]
    assert groups[(3,)][2]["null"] and np.isnan(groups[(5,)][2]["v"])
    order = [("agg", 1, "desc")]
    with staged(path, 0b111) as s:
        for a in range(3):
            for limit in (5, 64):
                run_case(s, groups, aggs, [0], 64, order, limit, having=[(a, op, consts[a])])
        run_case(s, groups, aggs, [0], 64, order, 64,
                 having=[(0, op, consts[0]), (2, ca.PRED_GT, -1.0)])
        run_case(s, groups, aggs, [0], 64, order, 64,
                 having=[(2, op, float("nan")), (1, ca.PRED_NE, consts[1])])


def test_having_on_a_sum_beyond_int64(tmp_path):
    """group 1 sums four values near 2^62 to just under 2^64: HAVING compares
    the int128 exactly; as an order term the sum is rejected by name"""
    big = 2**62 - 5
    k = np.array([1, 1, 1, 1, 2, 2, 3, 4, 4], dtype=np.int64)
    v = np.array([big, big, big, big, 2**62, 2**62 - 1, -7, -2**61, -2**61], dtype=np.int64)
    path = str(tmp_path / "big.cs")
    ca.write_table(path, KV, [k, v])
    groups = gt.ref_groups([0], CS, {0: k, 1: v})
    assert groups[(1,)][1]["v"] == 4 * big > 2**63
    assert groups[(2,)][1]["v"] == 2**63 - 1
    with staged(path, 0b11) as s:
        by_key = [("key", 0)]
        res = run_case(s, groups, CS, [0], 16, by_key, 9, having=[(1, ca.PRED_GT, 2**63 - 1)])
        assert gt.result_keys(res) == [(1,)]
        res = run_case(s, groups, CS, [0], 16, by_key, 9, having=[(1, ca.PRED_GE, 2**63 - 1)])
        assert gt.result_keys(res) == [(1,), (2,)]
        res = run_case(s, groups, CS, [0], 16, by_key, 9, having=[(1, ca.PRED_LE, -2**62)])
        assert gt.result_keys(res) == [(4,)]
        res = run_case(s, groups, CS, [0], 16, by_key, 9, having=[(1, ca.PRED_LT, -2**63)])
        assert gt.result_keys(res) == []
        res = run_case(s, groups, CS, [0], 16, by_key, 9, having=[(1, ca.PRED_LT, 0)])
        assert gt.result_keys(res) == [(3,), (4,)]
        with pytest.raises(ca.CStripeError, match=r"rc=-5.*order term 0: agg 1 \(kind 2\).*int64"):
            s.agg_hashed_topn(CS, [0], 16, [("agg", 1, "desc")], 2)
        # with the group filtered out the same order term is fine
        run_case(s, groups, CS, [0], 16, [("agg", 1, "desc")], 2,
                 having=[(1, ca.PRED_LE, 2**63 - 1)])


def test_having_removes_every_group(having_tab):
    path, aggs, groups = having_tab
    with staged(path, 0b111) as s:
        res = s.agg_hashed_topn(aggs, [0], 64, [("agg", 1, "desc")], 5,
                                having=[(0, ca.PRED_LT, 0)])
        assert res["n_groups"] == 0 and res["partials"].shape == (0, 3)
        assert s.last_group_topn[:2] == (len(groups), 0)


# ---------------- the 64-bit order word ----------------

def bitlen(x):
    return int(x).bit_length()


def test_two_wide_terms_exceed_the_order_word(tmp_path):
    n = 500
    rng = np.random.default_rng(18)
    k = np.arange(n, dtype=np.int64) % 50
    v = rng.integers(-2**44, 2**44, n).astype(np.int64)
    path = str(tmp_path / "wide.cs")
    ca.write_table(path, KV, [k, v])
    aggs = [(ca.AGG_SUM_I64, 1), (ca.AGG_MIN_I64, 1), (ca.AGG_COUNT_STAR, -1)]
    groups = gt.ref_groups([0], aggs, {0: k, 1: v})
    bits = []
    for a in range(3):
        vals = [es[a]["v"] for es in groups.values()]
        bits.append(bitlen(max(vals) - min(vals) + 1))
    assert bits[0] + bits[1] > 64 and bits[2] == 1
    with staged(path, 0b11) as s:
        with pytest.raises(ca.CStripeError) as ei:
            s.agg_hashed_topn(aggs, [0], 64, [("agg", 0, "desc"), ("agg", 1), ("agg", 2)], 5)
        msg = str(ei.value)
        assert "rc=-5" in msg and f"needs {sum(bits)} bits > 64" in msg
        for t in range(3):
            assert f"term {t} (agg {t}): {bits[t]} bits" in msg
        # either wide term alone, or with the narrow ones, fits
        run_case(s, groups, aggs, [0], 64, [("agg", 0, "desc"), ("agg", 2), ("key", 0)], 5)
        run_case(s, groups, aggs, [0], 64, [("agg", 1), ("agg", 2)], 5)


# ---------------- argument errors ----------------

def raw_call(s, aggs, key_cols, capacity, having, n_having, order, n_order, limit,
             n_aggs=None, n_key_cols=None):
    arr = ca.make_aggs(aggs)
    kc = (C.c_uint32 * max(1, len(key_cols)))(*key_cols)
    bufs, hg = ca._alloc_hgroups(4, max(1, len(aggs)), 16)
    rc = ca._scan_agg_hashed_topn(
        s._h, arr, len(aggs) if n_aggs is None else n_aggs, kc,
        len(key_cols) if n_key_cols is None else n_key_cols, capacity,
        having, n_having, order, n_order, limit, C.byref(hg))
    return rc, ca.errmsg()


def test_argument_errors(tmp_path):
    n = 300
    k = (np.arange(n) % 9).astype(np.int64)
    v = np.arange(n, dtype=np.int64)
    f = np.arange(n, dtype=np.float64)
    t = ca.text_slots([["A", "N", "R"][i % 3] for i in range(n)])
    u = ca.text_slots([["O", "F"][i % 2] for i in range(n)])
    path = str(tmp_path / "args.cs")
    defs = [("k", ca.I64, 0), ("v", ca.I64, 0), ("f", ca.F64, 0), ("t", ca.TEXT, 0),
            ("u", ca.TEXT, 0), ("w", ca.I64, 0)]
    ca.write_table(path, defs, [k, v, f, t, u, v])
    order1, _ = ca.make_group_order([("agg", 0, "desc")])
    with staged(path, 0b11111) as s:
        def bad(msg, **kw):
            args = dict(aggs=CS, key_cols=[0], capacity=16, having=None, n_having=0,
                        order=order1, n_order=1, limit=5)
            args.update(kw)
            rc, err = raw_call(s, **args)
            assert rc == ca.ERR_ARG, (kw, rc, err)
            assert msg in err, (kw, err)

        bad("limit 0 outside", limit=0)
        bad("limit 1048577 outside", limit=ca.MAX_TOPN + 1)
        five = (ca.GroupOrder * 5)()
        bad("5 order terms", order=five, n_order=5)
        bad("5 HAVING atoms", having=(ca.Having * 5)(), n_having=5)
        for kind, index, flags, msg in ((2, 0, 0, "bad kind 2"), (0, 2, 0, "agg index 2"),
                                        (1, 1, 0, "key index 1"), (0, 0, 4, "unknown flags 0x4")):
            o = (ca.GroupOrder * 1)()
            o[0].kind, o[0].index, o[0].flags = kind, index, flags
            bad(msg, order=o)
        rep, _ = ca.make_group_order([("agg", 1), ("key", 0), ("agg", 1, "desc")])
        bad("order term 2 repeats term 0", order=rep, n_order=3)
        hv, _ = ca.make_having([(2, ca.PRED_GT, 1)])
        bad("agg 2 out of range", having=hv, n_having=1)
        hv, _ = ca.make_having([(0, 6, 1)])
        bad("bad op 6", having=hv, n_having=1)
        # a TEXT key column as a KEY order term: select_topn's message
        keyterm, _ = ca.make_group_order([("key", 1)])
        bad("is TEXT — its row-level order in this ABI is whole-slot, not collation",
            key_cols=[0, 3], order=keyterm)
        # two char(1) TEXT keys only pack through the order-key fallback
        bad("use cstripe_scan_agg_hashed", key_cols=[3, 4])
        assert s.agg_hashed(CS, [3, 4], 16)["n_groups"] == 6
        # one TEXT key packs by slot and is fine, ordered by an aggregate
        res = s.agg_hashed_topn(CS, [3], 16, [("agg", 1, "desc")], 2)
        assert [ca.slot_text(int(x)) for x in res["keys"][0]] == ["R", "N"]
        # everything agg_hashed rejects, with its messages
        bad("bad args", n_aggs=0)
        bad("0 key columns", n_key_cols=0)
        bad("5 key columns", key_cols=[0, 1, 0, 1, 0])
        bad("key col 2 must be", key_cols=[2])
        bad("key col 5 not projected", key_cols=[5])
        bad("bad kind 11", aggs=[(11, 0)])
        # the capacity errors are agg_hashed's own
        for cap in (0, ca.MAX_HASH_GROUPS + 1, 8, 1):
            with pytest.raises(ca.CStripeError) as e1:
                s.agg_hashed(CS, [0], cap)
            m1 = ca.errmsg()
            with pytest.raises(ca.CStripeError) as e2:
                s.agg_hashed_topn(CS, [0], cap, [("agg", 0)], 3)
            assert ca.errmsg() == m1 and "rc=-5" in str(e1.value) and "rc=-5" in str(e2.value)
        assert s.agg_hashed_topn(CS, [0], 9, [("agg", 0)], 3)["n_groups"] == 3


def test_empty_selections(tmp_path):
    k = np.arange(50, dtype=np.int64)
    path = str(tmp_path / "empty.cs")
    ca.write_table(path, KV, [k, k])
    # zero selected chunk groups, then zero passing rows
    for preds in ([(0, ca.PRED_GT, 1000)], [(0, ca.PRED_GE, 10), (1, ca.PRED_LT, 10)]):
        with staged(path, 0b11, preds) as s:
            res = s.agg_hashed_topn(CS, [0], 64, [("agg", 1, "desc")], 5)
            assert res["n_groups"] == 0
            assert s.last_group_topn == (0, 0, 0.0, 0.0, 0.0)


# ---------------- differential against agg_hashed on the same scan ----------------

def random_query(rng, n_aggs, n_keys):
    terms = [("agg", a) for a in range(n_aggs)] + [("key", c) for c in range(n_keys)]
    picks = rng.permutation(len(terms))[:rng.integers(0, 5)]
    order = []
    for i in picks:
        opts = (("desc",) if rng.random() < 0.5 else ()) + \
               (("nulls_first",) if rng.random() < 0.5 else ())
        order.append(terms[i] + opts)
    return order


@pytest.mark.parametrize("seed", range(16))
def test_differential_random(tmp_path, seed):
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(200, 3000))
    n_keys = int(rng.integers(1, 4))
    keys = [rng.integers(-3, int(rng.integers(2, 12)), n).astype(np.int64) for _ in range(3)]
    knull = [(rng.random(n) < 0.1).astype(np.uint8) for _ in range(3)]
    v = rng.integers(-5, 6, n).astype(np.int64)
    vn = (rng.random(n) < 0.3).astype(np.uint8)
    # one binade, 17 values 2^-30 apart: the f64 term's order codes span 27
    # bits, so any four terms fit the 64-bit order word (floats of both signs,
    # which need all 64 bits alone, are test_every_kind_as_order_term's)
    f = 1.0 + rng.integers(0, 17, n).astype(np.float64) / 2**30
    fn = (rng.random(n) < 0.3).astype(np.uint8)
    path = str(tmp_path / "d.cs")
    defs = [("k0", ca.I64, 0), ("k1", ca.I64, 0), ("k2", ca.I64, 0), ("v", ca.I64, 0),
            ("f", ca.F64, 0)]
    ca.write_table(path, defs, keys + [v, f], nulls=knull + [vn, fn],
                   chunk_group_row_limit=1000)
    aggs = [(ca.AGG_COUNT_STAR, -1), (ca.AGG_SUM_I64, 3), (ca.AGG_MAX_F64, 4),
            (ca.AGG_MIN_I64, 3)]
    preds = [(3, ca.PRED_NE, 0)] if seed % 2 else []
    key_cols = list(range(n_keys))
    with staged(path, 0b11111, preds) as s:
        full = s.agg_hashed(aggs, key_cols, 4096)
        for _ in range(4):
            order = random_query(rng, len(aggs), n_keys)
            limit = int(rng.integers(1, full["n_groups"] + 3))
            having = []
            if rng.random() < 0.5:
                having.append((0, OPS[rng.integers(0, 6)], int(rng.integers(1, 8))))
            if rng.random() < 0.3:
                having.append((2, OPS[rng.integers(0, 6)],
                               1.0 + float(rng.integers(0, 17)) / 2**30))
            got = s.agg_hashed_topn(aggs, key_cols, 4096, order, limit, having=having)
            gt.same_bytes(got, gt.py_topn_of_hashed(full, aggs, order, limit, having))
        gt.same_bytes(s.agg_hashed(aggs, key_cols, 4096), full)


@pytest.mark.parametrize("codec", ["none", "lz4", "zstd"])
def test_golden_lineitem(codec):
    """GROUP BY l_shipdate ORDER BY sum(l_quantity) DESC, l_shipdate LIMIT 10"""
    path = os.path.join(REPO, "tests", "golden", f"lineitem12k_{codec}.cs")
    qty, date = ca.LINEITEM_COLS["l_quantity"], ca.LINEITEM_COLS["l_shipdate"]
    aggs = [(ca.AGG_SUM_I64, qty), (ca.AGG_COUNT_STAR, -1)]
    order = [("agg", 0, "desc"), ("key", 0)]
    with staged(path, (1 << qty) | (1 << date)) as s:
        full = s.agg_hashed(aggs, [date], 4096)
        got = s.agg_hashed_topn(aggs, [date], 4096, order, 10)
    assert full["n_groups"] > 100 and got["n_groups"] == 10
    gt.same_bytes(got, gt.py_topn_of_hashed(full, aggs, order, 10))


# ---------------- other surfaces ----------------

def test_vartext_key_ordered_by_rank(tmp_path):
    words = [b"pear", b"apple", b"fig", b"banana", b"", b"cherry", b"apricot", None]
    n = 4000
    rng = np.random.default_rng(20)
    pick = rng.integers(0, len(words), n)
    t = [words[i] for i in pick]
    v = rng.integers(0, 100, n).astype(np.int64)
    path = str(tmp_path / "vt.cs")
    ca.write_table(path, [("t", ca.VARTEXT, 0), ("v", ca.I64, 0)], [t, v],
                   chunk_group_row_limit=1000)
    aggs = [(ca.AGG_COUNT_STAR, -1), (ca.AGG_SUM_I64, 1)]
    present = sorted(w for w in words if w is not None)
    with staged(path, 0b11) as s:
        res = s.agg_hashed_topn(aggs, [0], 16, [("key", 0, "desc")], 3, decode_text=True)
        assert list(res["text_keys"][0]) == present[::-1][:3]
        res = s.agg_hashed_topn(aggs, [0], 16, [("key", 0, "asc", "nulls_first")], 3,
                                decode_text=True)
        assert list(res["text_keys"][0]) == [None] + present[:2]
        res = s.agg_hashed_topn(aggs, [0], 16, [("agg", 1, "desc")], 8, decode_text=True)
    sums = {}
    for w, x in zip(t, v.tolist()):
        sums[w] = sums.get(w, 0) + x
    want = sorted(sums, key=lambda w: (-sums[w], w is None, w or b""))
    assert list(res["text_keys"][0]) == want
    assert [ca.partial_i128(p) for p in res["partials"][:, 1]] == [sums[w] for w in want]


def test_lookup_derived_keys_q3_shape(tmp_path):
    """SELECT l_orderkey, sum(price * (1 - disc)), o_date, o_prio FROM lineitem
    JOIN orders ... GROUP BY l_orderkey, o_date, o_prio ORDER BY 2 DESC,
    o_date LIMIT 10"""
    n_orders, n = 400, 5000
    rng = np.random.default_rng(22)
    o_key = np.arange(n_orders, dtype=np.int64) * 3 + 1
    o_date = rng.integers(9000, 9050, n_orders).astype(np.int64)
    o_prio = rng.integers(0, 5, n_orders).astype(np.int64)
    l_key = rng.integers(0, n_orders * 3 + 3, n).astype(np.int64)
    price = (rng.integers(1, 20, n) * 1000).astype(np.int64)      # many equal revenues
    disc = rng.integers(0, 3, n).astype(np.int64)
    path = str(tmp_path / "l.cs")
    ca.write_table(path, [("l_key", ca.I64, 0), ("price", ca.I64, 0), ("disc", ca.I64, 0)],
                   [l_key, price, disc], chunk_group_row_limit=1000)
    pos = {int(x): i for i, x in enumerate(o_key)}
    hit = np.array([int(x) in pos for x in l_key])
    d_date = np.array([o_date[pos[int(x)]] if int(x) in pos else 0 for x in l_key], np.int64)
    d_prio = np.array([o_prio[pos[int(x)]] if int(x) in pos else 0 for x in l_key], np.int64)
    DATE, PRIO = 3, 4
    aggs = [(ca.AGG_SUM_DISC_I64, 1, 2, -1, 100), (ca.AGG_COUNT_STAR, -1)]
    cols = {0: l_key, 1: price, 2: disc, DATE: d_date, PRIO: d_prio}
    groups = gt.ref_groups([0, DATE, PRIO], aggs, cols, mask=hit)
    order = [("agg", 0, "desc"), ("key", 1)]
    with staged(path, 0b111, lookups=[ca.Lookup(0, o_key, [o_date, o_prio], inner=True)]) as s:
        assert (s.derived(0, 0), s.derived(0, 1)) == (DATE, PRIO)
        res = run_case(s, groups, aggs, [0, DATE, PRIO], 1024, order, 10)
        run_case(s, groups, aggs, [0, DATE, PRIO], 1024, order, 10,
                 having=[(1, ca.PRED_GT, 12)])
    revenue = [ca.partial_i128(p) for p in res["partials"][:, 0]]
    assert revenue == sorted(revenue, reverse=True)


def test_pruned_scan_ranges_come_from_selected_chunks(tmp_path):
    """ascending keys in 1 000-row chunk groups; the predicate prunes all but
    two of them, so the key range (and the tie word) is that of the survivors"""
    n = 10000
    k = (np.arange(n, dtype=np.int64) // 10) * 2**30
    v = (np.arange(n, dtype=np.int64) * 37) % 11
    path = str(tmp_path / "pruned.cs")
    ca.write_table(path, KV, [k, v], chunk_group_row_limit=1000)
    preds = [(0, ca.PRED_GE, int(k[3500])), (0, ca.PRED_LT, int(k[4800]))]
    mask = (k >= k[3500]) & (k < k[4800])
    groups = gt.ref_groups([0], CS, {0: k, 1: v}, mask=mask)
    with staged(path, 0b11, preds) as s:
        assert s.chunk_groups_filtered == 8
        for order in ([("agg", 1, "desc")], [("key", 0, "desc")], [("agg", 1), ("key", 0, "desc")]):
            run_case(s, groups, CS, [0], 256, order, 17)


# ---------------- shards with disjoint keys ----------------

def test_disjoint_shards_merge_to_the_single_table_result(tmp_path):
    n = 9000
    rng = np.random.default_rng(24)
    k = rng.integers(0, 300, n).astype(np.int64)
    v = rng.integers(-3, 4, n).astype(np.int64)
    whole = str(tmp_path / "whole.cs")
    ca.write_table(whole, KV, [k, v], chunk_group_row_limit=1000)
    order, limit, having = [("agg", 1, "desc"), ("agg", 0)], 12, [(0, ca.PRED_GE, 25)]
    groups = gt.ref_groups([0], CS, {0: k, 1: v})
    with staged(whole, 0b11) as s:
        single = run_case(s, groups, CS, [0], 512, order, limit, having=having)
    parts = []
    for sh in range(3):                      # shard = key % 3: disjoint groups
        sel = k % 3 == sh
        path = str(tmp_path / f"shard{sh}.cs")
        ca.write_table(path, KV, [k[sel], v[sel]], chunk_group_row_limit=1000)
        with staged(path, 0b11) as s:
            parts.append(s.agg_hashed_topn(CS, [0], 512, order, limit, having=having))
    merged = ca.merge_groups_topn(CS, 1, parts, order, limit)
    gt.same_bytes(merged, single)
    # the coordinator's offset slices the same total order
    want = gt.ref_topn(groups, CS, order, 5, having, offset=4)
    got = ca.merge_groups_topn(CS, 1, parts, order, 5, offset=4)
    gt.check_topn(got, groups, want, CS)


# ---------------- interleaving ----------------

def test_interleaving_changes_nobodys_result(tmp_path):
    n = 8000
    rng = np.random.default_rng(26)
    k = rng.integers(0, 200, n).astype(np.int64)
    v = rng.integers(-1000, 1000, n).astype(np.int64)
    path = str(tmp_path / "il.cs")
    ca.write_table(path, KV, [k, v], chunk_group_row_limit=1000)
    preds = [(1, ca.PRED_GT, -900)]
    groups = gt.ref_groups([0], CS, {0: k, 1: v}, mask=v > -900)
    order = [("agg", 1, "desc")]

    def rows_bytes(res):
        return (res["n_rows"], res["row_numbers"].tobytes(),
                tuple(res["values"][c].tobytes() for c in sorted(res["values"])))

    with staged(path, 0b11, preds) as s:
        base = {
            "topn": s.agg_hashed_topn(CS, [0], 256, order, 10),
            "topn_having": s.agg_hashed_topn(CS, [0], 256, [("key", 0, "desc")], 300,
                                             having=[(1, ca.PRED_LT, 0)]),
            "hashed": s.agg_hashed(CS, [0], 256),
            "agg": [p.as_dict() for p in s.agg(CS)],
            "select": rows_bytes(s.select(cols=[0, 1])),
            "select_topn": rows_bytes(s.select_topn([(1, "desc"), 0], 25, cols=[0, 1])),
        }
        gt.check_topn(base["topn"], groups, gt.ref_topn(groups, CS, order, 10), CS)
        for _ in range(2):
            gt.same_bytes(s.agg_hashed_topn(CS, [0], 256, order, 10), base["topn"])
            assert rows_bytes(s.select_topn([(1, "desc"), 0], 25, cols=[0, 1])) == \
                base["select_topn"]
            gt.same_bytes(s.agg_hashed_topn(CS, [0], 256, [("key", 0, "desc")], 300,
                                            having=[(1, ca.PRED_LT, 0)]), base["topn_having"])
            gt.same_bytes(s.agg_hashed(CS, [0], 256), base["hashed"])
            assert [p.as_dict() for p in s.agg(CS)] == base["agg"]
            gt.same_bytes(s.agg_hashed_topn(CS, [0], 200, order, 10), base["topn"])
            assert rows_bytes(s.select(cols=[0, 1])) == base["select"]
