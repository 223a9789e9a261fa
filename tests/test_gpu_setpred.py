"""
Set-membership predicates on the device (@pytest.mark.gpu): PRED_IN /
PRED_NOT_IN through cstripe_scan_begin_sets, the stage-time membership column
(build + probe kernels) and every query surface that then reads it as an
ordinary integer atom. Expected rows come from numpy over the arrays the test
wrote (np.isin and the null masks), never from the library; every comparison
is exact.
"""
import numpy as np
import pytest

import citus_amd as ca
import shapes
from shapes import Col, SHAPES

pytestmark = pytest.mark.gpu

IN, NOT_IN = ca.PRED_IN, ca.PRED_NOT_IN
HASH, BITMAP = ca.SET_FORM_HASH, ca.SET_FORM_BITMAP
I64_MIN, I64_MAX = shapes.I64_MIN, shapes.I64_MAX
PATH_GENERAL, PATH_DENSE = 2, 3
SIZES = (0, 1, 3, 17, 1000)


@pytest.fixture(scope="module", autouse=True)
def require_gpu():
    assert ca.gpu_available(), "MI355X required for these tests"


def force_form(monkeypatch, form):
    if form is None:
        monkeypatch.delenv("CSTRIPE_SET_FORM", raising=False)
    else:
        monkeypatch.setenv("CSTRIPE_SET_FORM", {HASH: "hash", BITMAP: "bitmap"}[form])


def member_mask(values, nulls, S, op):
    """rows that pass `x op S`: a NULL operand fails either atom"""
    present = np.ones(len(values), bool) if nulls is None else (np.asarray(nulls) == 0)
    isin = np.isin(np.asarray(values).astype(np.int64), np.asarray(S, dtype=np.int64))
    return present & (isin if op == IN else ~isin)


def draw_set(values, nulls, n, lo, hi):
    """n distinct int64 set elements by a fixed formula: every other element
    is one of the column's own present values (spread over their sorted
    order), the rest are values absent from the column, next to present ones
    where the type's range [lo, hi] has room"""
    present = values if nulls is None else values[np.asarray(nulls) == 0]
    pv = sorted(set(int(v) for v in present))
    have = set(pv)
    own = []
    if pv:
        step = max(1, len(pv) // (n // 2 + 1))
        own = pv[::step][:(n + 1) // 2]
    out = list(own)
    seen = set(out)
    bases = pv[::max(1, len(pv) // 8)] or [0]
    d = 1
    while len(out) < n:
        for b in bases:
            for c in (b + d, b - d):
                if len(out) < n and lo <= c <= hi and c not in have and c not in seen:
                    out.append(c)
                    seen.add(c)
        d += 1
        assert d < 100000
    # a fixed shuffle: sets arrive unsorted
    return [out[(i * 7919) % len(out)] for i in range(len(out))] if out else []


def bitmap_legal(S):
    return not S or max(S) - min(S) < (1 << 32)


def check_select(path, col, values, nulls, S, op, want_form, cols=None):
    mask = member_mask(values, nulls, S, op)
    with ca.Reader(path) as r, r.scan(cols_mask=1 << col, preds=[(col, op, S)]) as s:
        s.stage()
        assert s.set_form(0)[0] == want_form, (s.set_form(0), want_form)
        assert s.select_count() == int(mask.sum())
        res = s.select(cols=[col])
    assert res["n_rows"] == int(mask.sum())
    assert np.array_equal(res["row_numbers"], np.nonzero(mask)[0])
    assert np.array_equal(res["values"][col], values[mask])
    assert not res["nulls"][col].any()
    return res


# ------------------------------------------------- key stream shapes, both forms
INT_SHAPES = [n for n, sh in SHAPES.items() if sh.ctype in (ca.I32, ca.I64)]
TYPE_RANGE = {ca.I8: (-128, 127), ca.I32: (-(1 << 31), (1 << 31) - 1),
              ca.I64: (I64_MIN, I64_MAX)}


@pytest.fixture(scope="module")
def shape_tables(tmp_path_factory):
    root = tmp_path_factory.mktemp("setshapes")
    cache = {}

    def get(name):
        if name not in cache:
            path = str(root / f"{name}.cs")
            shapes.write_shape(path, SHAPES[name])
            cache[name] = path
        return cache[name]
    return get


def run_forms(monkeypatch, path, values, nulls, ctype):
    lo, hi = TYPE_RANGE[ctype]
    hits = 0
    for n in SIZES:
        S = draw_set(values, nulls, n, lo, hi)
        assert len(S) == n and len(set(S)) == n
        for op in (IN, NOT_IN):
            got = []
            for form in (HASH, BITMAP):
                force_form(monkeypatch, form)
                want = form if form == HASH or bitmap_legal(S) else HASH
                got.append(check_select(path, 0, values, nulls, S, op, want))
            assert np.array_equal(got[0]["row_numbers"], got[1]["row_numbers"])
            if op == IN:
                hits += got[0]["n_rows"]
    assert hits > 0              # the formula does draw present values


@pytest.mark.parametrize("name", INT_SHAPES)
def test_shapes_in_and_not_in(name, shape_tables, monkeypatch):
    sh = SHAPES[name]
    run_forms(monkeypatch, shape_tables(name), sh.values, sh.nulls, sh.ctype)


@pytest.mark.parametrize("codec", [ca.COMP_LZ4, ca.COMP_ZSTD, ca.COMP_NONE])
@pytest.mark.parametrize("mask", [None, "third", "word64", "first"])
def test_i8_keys(codec, mask, tmp_path, monkeypatch):
    i = np.arange(shapes.N, dtype=np.int64)
    v = ((i * 37 + i // 11) % 201 - 100).astype(np.int8)       # -100 .. 100
    nulls = None if mask is None else shapes.null_mask(mask)
    path = str(tmp_path / "i8.cs")
    ca.write_table(path, [("x", ca.I8, 0)], [v], nulls=None if nulls is None else [nulls],
                   compression=codec, chunk_group_row_limit=shapes.CG)
    lo, hi = TYPE_RANGE[ca.I8]
    for n in (0, 1, 3, 17):
        S = draw_set(v, nulls, n, lo, hi)
        for op in (IN, NOT_IN):
            for form in (HASH, BITMAP):
                force_form(monkeypatch, form)
                check_select(path, 0, v, nulls, S, op, form)
    # values outside the column's range never match: 261 = 5 + 256
    force_form(monkeypatch, None)
    S = [5, 300, -200, 261, 1 << 40, I64_MIN]
    res = check_select(path, 0, v, nulls, S, IN, HASH)
    assert set(res["values"][0].tolist()) <= {5}
    S = [5, 300, -200, 261]
    check_select(path, 0, v, nulls, S, NOT_IN, BITMAP)


# ------------------------------------------------------- sentinel and extremes
@pytest.mark.parametrize("with_m1", [True, False])
def test_sentinel_and_extremes(with_m1, tmp_path, monkeypatch):
    """-1 is the hash table's EMPTY pattern: it must be found when it is in
    the set and not found when it is not"""
    i = np.arange(shapes.N, dtype=np.int64)
    v = (i * 2654435761) % 1000003 - 500000
    v[::7] = I64_MIN
    v[1::7] = I64_MAX
    v[2::7] = 0
    v[3::7] = -1
    nulls = shapes.null_mask("third")
    path = str(tmp_path / "ext.cs")
    ca.write_table(path, [("x", ca.I64, 0)], [v], nulls=[nulls],
                   chunk_group_row_limit=shapes.CG)
    S = [I64_MAX, 0, I64_MIN, 12345678901] + ([-1] if with_m1 else [-2])
    force_form(monkeypatch, HASH)
    for op in (IN, NOT_IN):
        res = check_select(path, 0, v, nulls, S, op, HASH)
        assert (-1 in res["values"][0].tolist()) == (with_m1 == (op == IN))
    # a forced bitmap over a range beyond 2^32 falls back to hash
    force_form(monkeypatch, BITMAP)
    check_select(path, 0, v, nulls, S, IN, HASH)


def test_collision_chains(tmp_path, monkeypatch):
    rng = np.random.default_rng(20240607)
    v = rng.integers(0, 10**6, 20000, dtype=np.int64)
    S = rng.integers(0, 10**6, 1000, dtype=np.int64)          # duplicates allowed
    path = str(tmp_path / "coll.cs")
    ca.write_table(path, [("x", ca.I64, 0)], [v], chunk_group_row_limit=4096)
    force_form(monkeypatch, HASH)
    with ca.Reader(path) as r, r.scan(preds=[(0, IN, S)]) as s:
        s.stage()
        assert s.set_form(0) == (HASH, 2048)
        res = s.select()
    mask = np.isin(v, S)
    assert mask.sum() > 0
    assert np.array_equal(res["row_numbers"], np.nonzero(mask)[0])
    force_form(monkeypatch, None)                     # range 10^6 > 128 * 1000: hash
    check_select(path, 0, v, None, S.tolist(), NOT_IN, HASH)


# ------------------------------------------------------------- every surface
K, V, G = 0, 1, 2


def surface_table(path, nullable):
    i = np.arange(shapes.N, dtype=np.int64)
    k = (i * 48271) % 997
    v = (i * 31 + 7) % 5003 - 2500
    g = shapes.key_column(shapes.N)
    nulls = [shapes.null_mask("third") if nullable else None, None, None]
    ca.write_table(path, [("k", ca.I64, 0), ("v", ca.I64, 0), ("g", ca.I8, 0)],
                   [k, v, g], nulls=nulls if nullable else None,
                   chunk_group_row_limit=shapes.CG)
    return [Col(k, nulls[0]), Col(v), Col(g)], nulls[0]


@pytest.mark.parametrize("nullable", [True, False])
@pytest.mark.parametrize("op", [IN, NOT_IN])
def test_every_surface(nullable, op, tmp_path):
    path = str(tmp_path / "surf.cs")
    cols, knulls = surface_table(path, nullable)
    k, v, g = (c.values for c in cols)
    S = [int(x) for x in range(3, 997, 5)] + [5000, -1]
    rows = member_mask(k, knulls, S, op)
    assert 0 < rows.sum() < shapes.N
    aggs = shapes.with_one(cols, [(ca.AGG_COUNT_STAR, -1), (ca.AGG_SUM_I64, V),
                                  (ca.AGG_MIN_I64, V), (ca.AGG_MAX_I64, V)])
    with ca.Reader(path) as r, r.scan(cols_mask=0b111, preds=[(K, op, S)]) as s:
        s.stage()
        parts = s.agg(aggs)
        assert s.last_agg_path == (PATH_GENERAL if nullable else PATH_DENSE)
        assert s.last_agg_path in (PATH_GENERAL, PATH_DENSE)
        for a, p in zip(aggs, parts):
            shapes.check_partial(p, shapes.expect_agg(cols, a, rows), a[0], f"agg {a}")
        # scan_agg_grouped
        grouped = s.agg_grouped(aggs, [G])
        keys = sorted(int(x) for x in np.unique(g[rows]))
        assert sorted(kk[0] for kk in grouped) == keys
        for kk, ps in grouped.items():
            for a, p in zip(aggs, ps):
                shapes.check_partial(p, shapes.expect_agg(cols, a, rows & (g == kk[0])),
                                     a[0], f"grouped {kk} {a}")
        # scan_agg_hashed
        hashed = s.agg_hashed(aggs, [G], 64)
        assert hashed["keys"][0].tolist() == keys
        for gi, key in enumerate(keys):
            for ai, a in enumerate(aggs):
                p = hashed["partials"][gi][ai]
                got = {"count": int(p["count"]), "is_null": bool(p["is_null"]),
                       "i128": ca.partial_i128(p), "f64": float(p["f64"])}
                shapes.check_partial(got, shapes.expect_agg(cols, a, rows & (g == key)),
                                     a[0], f"hashed {key} {a}")
        # select_count / select
        assert s.select_count() == int(rows.sum())
        res = s.select(cols=[K, V])
        assert np.array_equal(res["row_numbers"], np.nonzero(rows)[0])
        assert np.array_equal(res["values"][K], k[rows])
        assert np.array_equal(res["values"][V], v[rows])
        assert not res["nulls"][K].any()
        # select_topn: ORDER BY v DESC, row number breaks ties
        top = s.select_topn([(V, "desc")], 25, cols=[V])
        idx = np.nonzero(rows)[0]
        order = idx[np.lexsort((idx, -v[idx]))][:25]
        assert np.array_equal(top["row_numbers"], order)
        assert np.array_equal(top["values"][V], v[order])


# ------------------------------------------------------------------------- CNF
def test_cnf(tmp_path):
    path = str(tmp_path / "cnf.cs")
    cols, knulls = surface_table(path, True)
    k, v, g = (c.values for c in cols)
    S = list(range(0, 997, 3))
    T = list(range(0, 997, 7)) + [10**12]
    c = -1000
    present = knulls == 0
    want = ((member_mask(k, knulls, S, IN) | (v < c)) & member_mask(k, knulls, T, NOT_IN))
    assert (want & ~member_mask(k, knulls, S, IN)).any()      # the OR matters
    preds = [(K, IN, S, 9), (V, ca.PRED_LT, c, 9), (K, NOT_IN, T)]
    with ca.Reader(path) as r, r.scan(cols_mask=0b11, preds=preds) as s:
        s.stage()
        assert s.set_form(0)[0] and s.set_form(1)[0]
        res = s.select(cols=[K])
        assert np.array_equal(res["row_numbers"], np.nonzero(want)[0])
        assert s.agg([(ca.AGG_COUNT_STAR, -1)])[0].count == int(want.sum())
    # one set, two columns: g IN U AND v IN U
    U = [int(v[10]), int(v[500]), int(v[1200]), 0, 1, 2, 3, 4, 10**10]
    want = np.isin(g.astype(np.int64), U) & np.isin(v, U)
    assert want.any()
    with ca.Reader(path) as r, r.scan(preds=[(G, IN, U), (V, IN, U)]) as s:
        s.stage()
        assert s.set_form(0)[0] != ca.SET_FORM_NONE
        with pytest.raises(ca.CStripeError):
            s.set_form(1)                                    # U is one set
        res = s.select(cols=[V])
        assert np.array_equal(res["row_numbers"], np.nonzero(want)[0])
    # the same set on one column as IN and NOT IN in one OR group: every
    # non-NULL row
    with ca.Reader(path) as r, r.scan(preds=[(K, IN, S, 1), (K, NOT_IN, S, 1)]) as s:
        s.stage()
        assert s.select_count() == int(present.sum())


# ------------------------------------------------------------------- text keys
def test_text_slots(tmp_path):
    words = ["A", "B", "AB", "ABC", "N", "R", "zz", "a"]
    i = np.arange(shapes.N)
    pick = (i * 5 + i // 13) % len(words)
    slots = ca.text_slots([words[j] for j in pick])
    nulls = shapes.null_mask("third")
    path = str(tmp_path / "t.cs")
    ca.write_table(path, [("c", ca.TEXT, 0)], [slots.view(np.int32)], nulls=[nulls],
                   chunk_group_row_limit=shapes.CG)
    S_words = ["AB", "N", "a", "QQ", "zzz"]
    in_S = np.array([words[j] in S_words for j in pick])
    for op in (IN, NOT_IN):
        want = (nulls == 0) & (in_S if op == IN else ~in_S)
        with ca.Reader(path) as r, r.scan(preds=[(0, op, ca.text_slots(S_words))]) as s:
            s.stage()
            res = s.select()
            assert np.array_equal(res["row_numbers"], np.nonzero(want)[0])
            assert np.array_equal(res["values"][0], slots[want])


def test_text_reference_fixture_rows_and_device_set(tmp_path):
    """the reference's IN-list pushdown fixture
    (columnar_chunk_filtering.out:1085-1121) through PRED_IN: rows {3,7,8},
    2 groups removed by a host set. A device set of slots is known by its raw
    slot range only, which says nothing about the lex-key min/max of TEXT skip
    nodes: it must remove no chunk (slot("AL") lies above every lex key of
    the {AL,AU} chunk) and still return the same rows."""
    import torch
    ids = np.arange(1, 9, dtype=np.int64)
    countries = ["AL", "AU", "BR", "BT", "PK", "PA", "USA", "ZW"]
    path = str(tmp_path / "push.cs")
    ca.write_table(path, [("id", ca.I64, 0), ("country", ca.TEXT, 0)],
                   [ids, ca.text_slots(countries).view(np.int32)],
                   compression=ca.COMP_LZ4, stripe_row_limit=2, chunk_group_row_limit=2)
    for S, want_ids, host_pruned in ((["USA", "BR", "ZW"], [3, 7, 8], 2),
                                     (["AL", "ZW"], [1, 8], 2),
                                     (["AL"], [1], 3)):
        slots = ca.text_slots(S).astype(np.int64)
        dev = torch.from_numpy(slots).to("cuda:0")
        for values, pruned in ((slots, host_pruned), (dev, 0)):
            with ca.Reader(path) as r, \
                    r.scan(cols_mask=0b11, preds=[(1, IN, values)]) as s:
                assert s.chunk_groups_filtered == pruned
                s.stage()
                res = s.select(cols=[0])
                assert res["values"][0].tolist() == want_ids
                assert res["row_numbers"].tolist() == [i - 1 for i in want_ids]
                parts = s.agg([(ca.AGG_COUNT_STAR, -1), (ca.AGG_SUM_I64, 0)])
                assert parts[0].count == len(want_ids) and parts[1].i128 == sum(want_ids)
    # an empty device set is an empty set on TEXT too
    with ca.Reader(path) as r, \
            r.scan(cols_mask=0b11, preds=[(1, NOT_IN, dev[:0].contiguous())]) as s:
        s.stage()
        assert s.select_count() == 8


def test_vartext(tmp_path, monkeypatch):
    vocab = [b"", b"a", b"ab", b"abc" * 50, b"lineitem", b"lineitem2", b"orders",
             b"x" * 127, b"x" * 128, b"zebra", b"\xff\xfe"]
    i = np.arange(shapes.N)
    pick = (i * 7 + i // 17) % len(vocab)
    vals = [None if j % 5 == 4 else vocab[pick[j]] for j in range(shapes.N)]
    path = str(tmp_path / "vt.cs")
    ca.write_table(path, [("id", ca.I64, 0), ("t", ca.VARTEXT, 0)],
                   [np.arange(shapes.N, dtype=np.int64), vals],
                   chunk_group_row_limit=shapes.CG)
    S = [vocab[j] for j in (0, 2, 3, 5, 7, 9)] + \
        [b"absent%d" % j for j in range(30)] + [b"lineite", b"x" * 129, "orders", b"ab"]
    assert len(S) == 40
    Sset = {x.encode() if isinstance(x, str) else x for x in S}
    for form in (None, HASH, BITMAP):
        force_form(monkeypatch, form)
        for op in (IN, NOT_IN):
            want = np.array([x is not None and ((x in Sset) == (op == IN)) for x in vals])
            with ca.Reader(path) as r, r.scan(cols_mask=0b11, preds=[(1, op, S)]) as s:
                s.stage()
                res = s.select(cols=[0, 1], decode_text=True)
                assert np.array_equal(res["row_numbers"], np.nonzero(want)[0])
                assert list(res["text"][1]) == [vals[j] for j in np.nonzero(want)[0]]
    # a set none of whose strings the table holds, and the empty set
    for S0 in ([b"nope", b"nada"], []):
        with ca.Reader(path) as r, r.scan(cols_mask=0b11, preds=[(1, NOT_IN, S0)]) as s:
            s.stage()
            assert s.select_count() == sum(x is not None for x in vals)
        with ca.Reader(path) as r, r.scan(cols_mask=0b11, preds=[(1, IN, S0)]) as s:
            s.stage()
            assert s.select_count() == 0


# ---------------------------------------------------------- semi-join on device
def test_semi_join_device_set(tmp_path):
    """orders filtered by a range -> select(device=True) of its key -> the
    lineitem scan's PRED_IN set, never leaving the device"""
    import torch
    o_key = np.arange(500, dtype=np.int64) * 3 + 1
    o_date = (np.arange(500, dtype=np.int64) * 7919) % 1000
    o_date[:260] = 999                         # the filter keeps keys >= 781 only
    opath, lpath = str(tmp_path / "orders.cs"), str(tmp_path / "lineitem.cs")
    ca.write_table(opath, [("o_orderkey", ca.I64, 0), ("o_date", ca.I64, 0)],
                   [o_key, o_date], chunk_group_row_limit=200)
    i = np.arange(shapes.N, dtype=np.int64)
    l_key = i * 5 // 7                         # ascending: chunks cover key ranges
    l_price = (i * 131) % 10007
    ca.write_table(lpath, [("l_orderkey", ca.I64, 0), ("l_price", ca.I64, 0)],
                   [l_key, l_price], chunk_group_row_limit=shapes.CG)
    keep = (o_date >= 100) & (o_date < 600)
    keys = o_key[keep]
    assert len(keys) > 50 and keys.min() >= 781
    aggs = [(ca.AGG_COUNT_STAR, -1), (ca.AGG_SUM_I64, 1), (ca.AGG_MIN_I64, 1),
            (ca.AGG_MAX_I64, 1)]
    with ca.Reader(opath) as ro, \
            ro.scan(cols_mask=0b11, preds=[(1, ca.PRED_GE, 100), (1, ca.PRED_LT, 600)]) as so:
        so.stage()
        dev_keys = so.select(cols=[0], want_nulls=False, want_row_numbers=False,
                             device=True)["values"][0]
    assert isinstance(dev_keys, torch.Tensor) and dev_keys.is_cuda
    assert np.array_equal(dev_keys.cpu().numpy(), keys)

    rows = np.isin(l_key, keys)
    assert 0 < rows.sum() < shapes.N
    cols = [Col(l_key), Col(l_price)]
    bounds = [(int(l_key[a]), int(l_key[b - 1])) for a, b in
              ((0, 1000), (1000, 2000), (2000, 2100))]
    by_range = sum(int(keys.max()) < mn or int(keys.min()) > mx for mn, mx in bounds)
    assert by_range == 1                       # chunk 0 holds keys 0..713 only
    with ca.Reader(lpath) as rl:
        with rl.scan(cols_mask=0b11, preds=[(0, IN, dev_keys)]) as s:
            assert s.chunk_groups_filtered == by_range
            s.stage()
            dev_parts = s.agg(shapes.with_one(cols, aggs))
            assert s.set_form(0)[0] in (HASH, BITMAP)
            build_ms, probe_ms = s.last_set_ms()
            assert build_ms > 0 and probe_ms > 0
        with rl.scan(cols_mask=0b11, preds=[(0, IN, keys)]) as s:
            s.stage()
            host_parts = s.agg(shapes.with_one(cols, aggs))
    for a, d, h in zip(shapes.with_one(cols, aggs), dev_parts, host_parts):
        shapes.check_partial(d, shapes.expect_agg(cols, a, rows), a[0], f"device set {a}")
        assert bytes(d) == bytes(h)            # bit-identical partials
    # an empty device set
    empty = dev_keys[:0].contiguous()
    with ca.Reader(lpath) as rl, rl.scan(preds=[(0, NOT_IN, empty)]) as s:
        s.stage()
        assert s.select_count() == shapes.N


# ------------------------------------------------ pruned chunks, shard directory
def test_pruned_chunks_in_a_shard_directory(tmp_path):
    d = tmp_path / "shards"
    d.mkdir()
    i = np.arange(2 * shapes.N, dtype=np.int64)
    key = i // 3 * 2                             # ascending, even
    val = (i * 17) % 1009
    for f, sl in (("a.cs", slice(0, shapes.N)), ("b.cs", slice(shapes.N, None))):
        ca.write_table(str(d / f), [("k", ca.I64, 0), ("v", ca.I64, 0)],
                       [key[sl], val[sl]], chunk_group_row_limit=shapes.CG)
    S = [0, 2, 5, 700, 702, 1500, 1501, 2796, 2798]     # 5 and 1501 are absent
    mask = np.isin(key, S)
    starts = list(range(0, shapes.N, shapes.CG))
    bounds = [(int(key[b + a]), int(key[min(b + a + shapes.CG, b + shapes.N) - 1]))
              for b in (0, shapes.N) for a in starts]
    pruned = sum(not any(mn <= x <= mx for x in S) for mn, mx in bounds)
    assert len(bounds) == 6 and 0 < pruned < 6
    with ca.Reader(str(d)) as r, r.scan(cols_mask=0b11, preds=[(0, IN, S)]) as s:
        assert s.chunk_groups_filtered == pruned
        s.stage()
        res = s.select(cols=[0, 1])
        assert np.array_equal(res["row_numbers"], np.nonzero(mask)[0])   # table-wide
        assert np.array_equal(res["values"][1], val[mask])
        assert s.agg([(ca.AGG_SUM_I64, 1)])[0].i128 == int(val[mask].sum())


# ------------------------------------------------ re-invocation and interleaving
def test_reinvocation_interleaving_and_restage(tmp_path):
    path = str(tmp_path / "re.cs")
    cols, knulls = surface_table(path, True)
    k, v, g = (c.values for c in cols)
    S = list(range(1, 997, 4))
    rows = member_mask(k, knulls, S, IN)
    aggs = [(ca.AGG_COUNT_STAR, -1), (ca.AGG_SUM_I64, V)]

    def snapshot(s):
        res = s.select(cols=[K, V])
        return (bytes(b"".join(bytes(p) for p in s.agg(aggs))),
                res["row_numbers"].tobytes(), res["values"][K].tobytes(),
                res["values"][V].tobytes(),
                s.agg_hashed(aggs, [G], 16)["partials"].tobytes())

    with ca.Reader(path) as r, r.scan(cols_mask=0b111, preds=[(K, IN, S)]) as s, \
            r.scan(cols_mask=0b111) as twin:
        s.stage()
        twin.stage()
        first = snapshot(s)
        assert np.frombuffer(first[1], np.int64).tolist() == np.nonzero(rows)[0].tolist()
        assert snapshot(s) == first
        # the predicate-free twin reads the same rows through next_batch / read_row
        bufs = {c: np.zeros(shapes.CG, dt) for c, dt in ((K, np.int64), (V, np.int64), (G, np.int8))}
        nb = {c: np.zeros(shapes.CG, np.uint8) for c in bufs}
        n, first_row = twin.next_batch(bufs, nb)
        assert (n, first_row) == (shapes.CG, 0)
        assert np.array_equal(bufs[V][:n], v[:n])
        assert np.array_equal(nb[K][:n], knulls[:n])
        assert twin.read_row(1501)[V] == int(v[1501])
        assert snapshot(s) == first
        assert twin.read_row(7)[G] == int(g[7])
        s.stage()                                   # restage rebuilds the set
        assert s.set_form(0)[0] != ca.SET_FORM_NONE
        assert snapshot(s) == first


# ------------------------------------------------------------------ stage errors
def test_member_slots_count_against_the_projection(tmp_path):
    n_cols = 16
    a = np.arange(50, dtype=np.int64)
    path = str(tmp_path / "wide.cs")
    ca.write_table(path, [(f"c{j}", ca.I64, 0) for j in range(n_cols)],
                   [a + j for j in range(n_cols)])
    with ca.Reader(path) as r:
        # 16 table columns + 1 membership column: one slot too many
        with r.scan(cols_mask=(1 << 16) - 1, preds=[(0, IN, [1, 2, 3])]) as s:
            with pytest.raises(ca.CStripeError, match=r"rc=-5"):
                s.stage()
            with pytest.raises(ca.CStripeError, match=r"rc=-4"):   # left unstaged
                s.agg([(ca.AGG_COUNT_STAR, -1)])
            assert s.set_form(0) == (ca.SET_FORM_NONE, 0)
        # 14 + two distinct (column, set) pairs = 16 fits; a repeated pair is one slot
        S = [1, 2, 3]
        preds = [(0, IN, S), (1, NOT_IN, S), (0, NOT_IN, S, 5), (1, ca.PRED_GT, 2, 5)]
        with r.scan(cols_mask=(1 << 14) - 1, preds=preds) as s:
            s.stage()
            want = np.isin(a, S) & ~np.isin(a + 1, S) & (~np.isin(a, S) | (a + 1 > 2))
            assert want.sum() == 1
            assert s.select_count() == int(want.sum())
        with r.scan(cols_mask=(1 << 15) - 1, preds=preds) as s:
            with pytest.raises(ca.CStripeError, match=r"rc=-5"):
                s.stage()
