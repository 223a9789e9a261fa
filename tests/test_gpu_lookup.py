"""
Lookups on the device (@pytest.mark.gpu): the N:1 join of
cstripe_scan_begin_lookups — table build, probe, rank scan and gather at
stage — and every query surface that then reads a derived column as an
ordinary sparse I64 column. Expected rows come from a Python dict over the
arrays the test wrote (numpy / Python ints), never from the library; every
comparison is exact.
"""
import numpy as np
import pytest

import citus_amd as ca
import shapes
from shapes import Col, SHAPES

pytestmark = pytest.mark.gpu

HASH, DIRECT = ca.LOOKUP_FORM_HASH, ca.LOOKUP_FORM_DIRECT
I64_MIN, I64_MAX = shapes.I64_MIN, shapes.I64_MAX
PATH_GENERAL = 2
SIZES = (0, 1, 3, 17, 1000)
SPECIALS = (I64_MIN, I64_MAX, -1, 0)


@pytest.fixture(scope="module", autouse=True)
def require_gpu():
    assert ca.gpu_available(), "MI355X required for these tests"


def force_form(monkeypatch, form):
    if form is None:
        monkeypatch.delenv("CSTRIPE_LOOKUP_FORM", raising=False)
    else:
        monkeypatch.setenv("CSTRIPE_LOOKUP_FORM", {HASH: "hash", DIRECT: "direct"}[form])


def pay(k):
    """the payload of build key k: a fixed formula that reaches I64_MIN,
    I64_MAX, -1 and 0"""
    k = int(k)
    if k % 7 < 4:
        return SPECIALS[k % 7]
    u = (k * 0x9E3779B97F4A7C15 + 12345) & ((1 << 64) - 1)
    return u - (1 << 64) if u >> 63 else u


def join(values, nulls, keys, payload):
    """the dict join: (int64 values with 0 in NULL slots, uint8 null bytes)"""
    d = {int(k): int(p) for k, p in zip(keys, payload)}
    assert len(d) == len(keys)
    n = len(values)
    out = np.zeros(n, dtype=np.int64)
    onull = np.ones(n, dtype=np.uint8)
    for i in range(n):
        if nulls is not None and nulls[i]:
            continue
        k = int(values[i])
        if k in d:
            out[i] = d[k]
            onull[i] = 0
    return out, onull


def draw_keys(values, nulls, n, lo, hi):
    """n distinct build keys by a fixed formula, as the value-set tests draw
    sets: half are present keys of the column (spread over their sorted
    order), half are absent from it"""
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
    return [out[(i * 7919) % len(out)] for i in range(len(out))] if out else []


def direct_legal(keys):
    return not keys or max(keys) - min(keys) < (1 << 32) - 1


def select_derived(path, key_col, keys, payloads, want_form=None, inner=False, extra=()):
    with ca.Reader(path) as r, \
            r.scan(lookups=[ca.Lookup(key_col, keys, payloads, inner=inner)]) as s:
        s.stage()
        if want_form is not None:
            assert s.lookup_form(0)[0] == want_form, (s.lookup_form(0), want_form)
        ds = [s.derived(0, p) for p in range(len(payloads))]
        res = s.select(cols=ds + list(extra))
        return res, ds


def check_join(res, d, want_vals, want_nulls, rows=None):
    rows = np.ones(len(want_vals), bool) if rows is None else rows
    assert res["n_rows"] == int(rows.sum())
    assert np.array_equal(res["row_numbers"], np.nonzero(rows)[0])
    assert np.array_equal(res["nulls"][d], want_nulls[rows])
    assert np.array_equal(res["values"][d], want_vals[rows])


# ------------------------------------------------- key stream shapes, both forms
INT_SHAPES = [n for n, sh in SHAPES.items() if sh.ctype in (ca.I32, ca.I64)]
TYPE_RANGE = {ca.I8: (-128, 127), ca.I16: (-(1 << 15), (1 << 15) - 1),
              ca.I32: (-(1 << 31), (1 << 31) - 1), ca.I64: (I64_MIN, I64_MAX)}


@pytest.fixture(scope="module")
def shape_tables(tmp_path_factory):
    root = tmp_path_factory.mktemp("lookupshapes")
    cache = {}

    def get(name):
        if name not in cache:
            path = str(root / f"{name}.cs")
            shapes.write_shape(path, SHAPES[name])
            cache[name] = path
        return cache[name]
    return get


@pytest.mark.parametrize("name", INT_SHAPES)
def test_key_stream_shapes(name, shape_tables, monkeypatch):
    sh = SHAPES[name]
    path = shape_tables(name)
    lo, hi = TYPE_RANGE[sh.ctype]
    hits = 0
    for n in SIZES:
        keys = draw_keys(sh.values, sh.nulls, n, lo, hi)
        assert len(keys) == n and len(set(keys)) == n
        payload = [pay(k) for k in keys]
        want_vals, want_nulls = join(sh.values, sh.nulls, keys, payload)
        got = []
        for form in (HASH, DIRECT):
            force_form(monkeypatch, form)
            want_form = form if form == HASH or direct_legal(keys) else HASH
            res, (d,) = select_derived(path, 0, keys, [payload], want_form)
            check_join(res, d, want_vals, want_nulls)
            got.append(res)
        assert np.array_equal(got[0]["values"][d], got[1]["values"][d])
        assert np.array_equal(got[0]["nulls"][d], got[1]["nulls"][d])
        assert np.array_equal(got[0]["row_numbers"], got[1]["row_numbers"])
        hits += int((want_nulls == 0).sum())
    assert hits > 0              # the formula does draw present keys


# ------------------------------------------------------------ bitmap / rank edges
EDGE_PATTERNS = ("all", "none", "first", "last", "alternating", "null_complement")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129, 1000])
def test_bitmap_and_rank_edges(n, tmp_path, monkeypatch):
    i = np.arange(n, dtype=np.int64)
    k = i * 2 + 10
    kn_nulls = (i % 2).astype(np.uint8)          # NULL in the odd rows
    path = str(tmp_path / "edge.cs")
    ca.write_table(path, [("k", ca.I64, 0), ("kn", ca.I64, 0)], [k, k],
                   nulls=[None, kn_nulls], chunk_group_row_limit=1000)
    for pattern in EDGE_PATTERNS:
        key_col, knulls = 0, None
        keys = {"all": k.tolist(), "none": [11, 13, -5], "first": [int(k[0]), 7],
                "last": [int(k[n - 1]), 7], "alternating": k[::2].tolist() + [9],
                "null_complement": k.tolist()}[pattern]
        if pattern == "null_complement":
            key_col, knulls = 1, kn_nulls
        payload = [pay(x) for x in keys]
        want_vals, want_nulls = join(k, knulls, keys, payload)
        matched = want_nulls == 0
        assert int(matched.sum()) == {"all": n, "none": 0, "first": 1, "last": 1,
                                      "alternating": (n + 1) // 2,
                                      "null_complement": (n + 1) // 2}[pattern]
        cols = [Col(k), Col(k, kn_nulls), Col(want_vals, want_nulls)]
        for form in (HASH, DIRECT):
            force_form(monkeypatch, form)
            with ca.Reader(path) as r, \
                    r.scan(lookups=[ca.Lookup(key_col, keys, [payload])]) as s:
                s.stage()
                assert s.lookup_form(0)[0] == form
                D = s.derived(0, 0)
                assert D == 2
                res = s.select(cols=[D])
                check_join(res, D, want_vals, want_nulls)
                aggs = shapes.with_one(cols, [(ca.AGG_COUNT_COL, D), (ca.AGG_SUM_I64, D),
                                              (ca.AGG_MIN_I64, D), (ca.AGG_MAX_I64, D),
                                              (ca.AGG_COUNT_STAR, -1)])
                rows = np.ones(n, bool)
                for a, p in zip(aggs, s.agg(aggs)):
                    shapes.check_partial(p, shapes.expect_agg(cols, a, rows), a[0],
                                         f"{pattern} n={n} {a}")
                assert s.last_agg_path == PATH_GENERAL


# ------------------------------------------------------------ sentinels and chains
@pytest.mark.parametrize("present", [True, False])
def test_sentinel_keys(present, tmp_path, monkeypatch):
    """-1 is the hash table's EMPTY pattern: found when it is a build key, not
    found when it is not; likewise the int64 extremes and 0"""
    i = np.arange(shapes.N, dtype=np.int64)
    v = (i * 2654435761) % 1000003 - 500000
    v[::7] = I64_MIN
    v[1::7] = I64_MAX
    v[2::7] = 0
    v[3::7] = -1
    v[v == -2] = 5
    nulls = shapes.null_mask("third")
    path = str(tmp_path / "ext.cs")
    ca.write_table(path, [("x", ca.I64, 0)], [v], nulls=[nulls],
                   chunk_group_row_limit=shapes.CG)
    keys = ([-1, I64_MIN, I64_MAX, 0] if present else [-2, I64_MIN + 1, I64_MAX - 1, 1]) \
        + [12345678901, int(v[4])]
    payload = [I64_MAX, -1, 0, I64_MIN, 77, 78]
    want_vals, want_nulls = join(v, nulls, keys, payload)
    force_form(monkeypatch, HASH)
    res, (d,) = select_derived(path, 0, keys, [payload], HASH)
    check_join(res, d, want_vals, want_nulls)
    hit = set(v[want_nulls == 0].tolist())
    assert ({-1, I64_MIN, I64_MAX, 0} <= hit) == present
    assert present or not ({-1, I64_MIN, I64_MAX, 0} & hit)
    # a forced direct over a range beyond 2^32 falls back to hash
    force_form(monkeypatch, DIRECT)
    res, (d,) = select_derived(path, 0, keys, [payload], HASH)
    check_join(res, d, want_vals, want_nulls)


def test_collision_chains(tmp_path, monkeypatch):
    rng = np.random.default_rng(20240607)
    v = rng.integers(0, 10**6, 20000, dtype=np.int64)
    keys = np.unique(rng.integers(0, 10**6, 1000, dtype=np.int64))[:1000]
    rng.shuffle(keys)
    payload = [pay(k) for k in keys]
    path = str(tmp_path / "coll.cs")
    ca.write_table(path, [("x", ca.I64, 0)], [v], chunk_group_row_limit=4096)
    want_vals, want_nulls = join(v, None, keys, payload)
    assert (want_nulls == 0).sum() > 0
    force_form(monkeypatch, HASH)
    with ca.Reader(path) as r, r.scan(lookups=[ca.Lookup(0, keys, [payload])]) as s:
        s.stage()
        slots = 2
        while slots < 2 * len(keys):
            slots *= 2
        assert s.lookup_form(0) == (HASH, slots)
        D = s.derived(0, 0)
        check_join(s.select(cols=[D]), D, want_vals, want_nulls)
    force_form(monkeypatch, None)                     # range 10^6 > max(2^16, 4n): hash
    res, (d,) = select_derived(path, 0, keys, [payload], HASH)
    check_join(res, d, want_vals, want_nulls)
    # a dense key range takes the direct form by itself
    dk = np.arange(1000, 3000, dtype=np.int64)
    res, (d,) = select_derived(path, 0, dk, [[pay(k) for k in dk]], DIRECT)
    wv, wn = join(v, None, dk, [pay(k) for k in dk])
    check_join(res, d, wv, wn)


@pytest.mark.parametrize("ctype,dtype", [(ca.I8, np.int8), (ca.I16, np.int16)])
@pytest.mark.parametrize("mask", [None, "third"])
def test_narrow_key_columns(ctype, dtype, mask, tmp_path, monkeypatch):
    i = np.arange(shapes.N, dtype=np.int64)
    span = 201 if ctype == ca.I8 else 40001
    v = ((i * 37 + i // 11) % span - span // 2).astype(dtype)
    nulls = None if mask is None else shapes.null_mask(mask)
    path = str(tmp_path / "narrow.cs")
    ca.write_table(path, [("x", ctype, 0)], [v], nulls=None if nulls is None else [nulls],
                   chunk_group_row_limit=shapes.CG)
    lo, hi = TYPE_RANGE[ctype]
    # keys outside the type's range never match: 261 = 5 + 256, 65541 = 5 + 65536
    keys = [5, -3, 261, 65541, hi + 1, lo - 1, 1 << 40, I64_MIN, int(v[7]) if v[7] not in (5, -3) else 9]
    payload = [pay(k) + 1 if pay(k) != I64_MAX else 3 for k in keys]
    want_vals, want_nulls = join(v, nulls, keys, payload)
    assert set(v[want_nulls == 0].tolist()) <= {5, -3, int(v[7]), 9}
    assert (want_nulls == 0).any()
    for form in (HASH, DIRECT):
        force_form(monkeypatch, form)
        res, (d,) = select_derived(path, 0, keys, [payload], HASH)   # range > 2^32
        check_join(res, d, want_vals, want_nulls)
    small = [5, -3, 100, -100, 77]
    want_vals, want_nulls = join(v, nulls, small, small)
    for form in (HASH, DIRECT):
        force_form(monkeypatch, form)
        res, (d,) = select_derived(path, 0, small, [small], form)
        check_join(res, d, want_vals, want_nulls)


# ------------------------------------------------------------- every surface
K, V, G, K2 = 0, 1, 2, 3
D0, D1, E0 = 4, 5, 6


def surface_table(path, nullable):
    i = np.arange(shapes.N, dtype=np.int64)
    k = (i * 48271) % 997
    v = (i * 31 + 7) % 5003 - 2500
    g = shapes.key_column(shapes.N)
    k2 = ((i * 7 + i // 13) % 300 - 150).astype(np.int32)
    nulls = [shapes.null_mask("third") if nullable else None, None, None, None]
    ca.write_table(path, [("k", ca.I64, 0), ("v", ca.I64, 0), ("g", ca.I8, 0),
                          ("k2", ca.I32, 0)],
                   [k, v, g, k2], nulls=nulls if nullable else None,
                   chunk_group_row_limit=shapes.CG)
    return [Col(k, nulls[0]), Col(v), Col(g), Col(k2)], nulls[0]


def surface_maps():
    keys = [int(x) for x in range(3, 997, 3)] + [5000, -1, 10**12]
    keys = [keys[(i * 101) % len(keys)] for i in range(len(keys))]
    p0 = [k % 11 - 5 for k in keys]                     # few distinct: a GROUP BY key
    p1 = [k * 1000003 - 7 for k in keys]
    keys2 = [int(x) for x in range(-150, 150, 2)] + [1 << 33]
    q0 = [k * k - 9 if abs(k) < 1000 else 77 for k in keys2]
    return keys, p0, p1, keys2, q0


def topn_expect(rows, dvals, dnulls, desc, nulls_first, limit):
    idx = np.nonzero(rows)[0]
    isnull = dnulls[idx] == 1
    val = np.where(isnull, 0, dvals[idx])
    if desc:
        val = -val
    nk = (~isnull).astype(np.int64) if nulls_first else isnull.astype(np.int64)
    return idx[np.lexsort((idx, val, nk))][:limit]


def hashed_dict(res, n_keys):
    out = {}
    for gi in range(res["n_groups"]):
        key = tuple(None if res["key_nulls"][k][gi] else int(res["keys"][k][gi])
                    for k in range(n_keys))
        out[key] = res["partials"][gi]
    assert len(out) == res["n_groups"]
    return out


def check_hashed(res, key_cols, cols, aggs, rows, what):
    got = hashed_dict(res, len(key_cols))
    want_keys = set()
    for i in np.nonzero(rows)[0]:
        want_keys.add(tuple(None if not cols[c].present[i] else int(cols[c].wide[i])
                            for c in key_cols))
    assert set(got) == want_keys, what
    for key, ps in got.items():
        m = rows.copy()
        for c, kv in zip(key_cols, key):
            m &= ~cols[c].present if kv is None else (cols[c].present & (cols[c].wide == kv))
        for ai, a in enumerate(aggs):
            p = ps[ai]
            g = {"count": int(p["count"]), "is_null": bool(p["is_null"]),
                 "i128": ca.partial_i128(p), "f64": float(p["f64"])}
            shapes.check_partial(g, shapes.expect_agg(cols, a, m), a[0], f"{what} {key} {a}")


@pytest.mark.parametrize("nullable", [True, False])
@pytest.mark.parametrize("inner", [False, True])
def test_every_surface(nullable, inner, tmp_path):
    path = str(tmp_path / "surf.cs")
    cols, knulls = surface_table(path, nullable)
    keys, p0, p1, keys2, q0 = surface_maps()
    cols.append(Col(*join(cols[K].values, knulls, keys, p0)))      # D0
    cols.append(Col(*join(cols[K].values, knulls, keys, p1)))      # D1
    cols.append(Col(*join(cols[K2].values, None, keys2, q0)))      # E0
    v = cols[V].values
    rows = cols[D0].present.copy() if inner else np.ones(shapes.N, bool)
    assert 0 < cols[D0].present.sum() < shapes.N
    assert 0 < cols[E0].present.sum() < shapes.N
    lks = [ca.Lookup(K, keys, [p0, p1], inner=inner), ca.Lookup(K2, keys2, [q0])]
    aggs = shapes.with_one(cols, [
        (ca.AGG_COUNT_STAR, -1), (ca.AGG_COUNT_COL, D0), (ca.AGG_COUNT_COL, E0),
        (ca.AGG_SUM_I64, D1), (ca.AGG_MIN_I64, D1), (ca.AGG_MAX_I64, D1),
        (ca.AGG_SUM_PROD_I64, D0, V), (ca.AGG_SUM_PROD_I64, V, E0),
        (ca.AGG_SUM_DISC_I64, V, D0), (ca.AGG_SUM_DISC_TAX_I64, D0, G, E0),
        (ca.AGG_SUM_I64, V)])
    with ca.Reader(path) as r, r.scan(cols_mask=0b1111, lookups=lks) as s:
        assert (s.derived(0, 0), s.derived(0, 1), s.derived(1, 0)) == (D0, D1, E0)
        assert s.column_count() == 7
        s.stage()
        build_ms, probe_ms = s.last_lookup_ms()
        assert build_ms > 0 and probe_ms > 0
        parts = s.agg(aggs)
        assert s.last_agg_path == PATH_GENERAL
        for a, p in zip(aggs, parts):
            shapes.check_partial(p, shapes.expect_agg(cols, a, rows), a[0], f"agg {a}")
        # hashed: keyed by a derived column alone, and with a table column
        h_aggs = aggs[:6] + aggs[10:]
        res = s.agg_hashed(h_aggs, [D0], 64)
        check_hashed(res, [D0], cols, h_aggs, rows, "hashed D0")
        null_group = any(bool(x) for x in res["key_nulls"][0])
        assert null_group == (not inner)            # the unmatched rows' group
        res = s.agg_hashed(h_aggs, [G, D0], 256)
        check_hashed(res, [G, D0], cols, h_aggs, rows, "hashed G,D0")
        res = s.agg_hashed(h_aggs[:3], [E0, D0], 4096)
        check_hashed(res, [E0, D0], cols, h_aggs[:3], rows, "hashed E0,D0")
        # select_count / select
        assert s.select_count() == int(rows.sum())
        sel = s.select(cols=[K, V, D0, D1, E0])
        assert np.array_equal(sel["row_numbers"], np.nonzero(rows)[0])
        assert np.array_equal(sel["values"][V], v[rows])
        for d in (D0, D1, E0):
            check_join(sel, d, cols[d].values, (~cols[d].present).astype(np.uint8), rows)
        every = s.select()                          # default: projected + derived
        assert sorted(every["values"]) == [K, V, G, K2, D0, D1, E0]
        # select_topn ordered by a derived column
        dn = (~cols[D1].present).astype(np.uint8)
        for desc in (False, True):
            for first in (False, True):
                top = s.select_topn([(D1, "desc" if desc else "asc",
                                      "first" if first else "last")], 40, cols=[D1, V])
                order = topn_expect(rows, cols[D1].values // 1000003, dn, desc, first, 40)
                assert np.array_equal(top["row_numbers"], order), (desc, first)
                assert np.array_equal(top["values"][D1], cols[D1].values[order])
                assert np.array_equal(top["nulls"][D1], dn[order])
        # a derived column as the second order key, after a table column
        top = s.select_topn([(G, "asc"), (D0, "desc", "last")], 30, cols=[G, D0])
        idx = np.nonzero(rows)[0]
        d0n = ~cols[D0].present[idx]
        order = idx[np.lexsort((idx, np.where(d0n, 0, -cols[D0].values[idx]), d0n,
                                cols[G].wide[idx]))][:30]
        assert np.array_equal(top["row_numbers"], order)
        # errors: grouped keys, and the scan still works afterwards
        with pytest.raises(ca.CStripeError, match=r"rc=-5"):
            s.agg_grouped(aggs[:1], [D0])
        grouped = s.agg_grouped(aggs[:2], [G])
        for kk, ps in grouped.items():
            for a, p in zip(aggs[:2], ps):
                shapes.check_partial(p, shapes.expect_agg(cols, a, rows & (cols[G].values == kk[0])),
                                     a[0], f"grouped {kk} {a}")
        assert s.select_count() == int(rows.sum())


OPS = (ca.PRED_LT, ca.PRED_LE, ca.PRED_GT, ca.PRED_GE, ca.PRED_EQ, ca.PRED_NE)


@pytest.mark.parametrize("nullable", [True, False])
@pytest.mark.parametrize("inner", [False, True])
def test_predicates_on_derived_columns(nullable, inner, tmp_path):
    path = str(tmp_path / "pred.cs")
    cols, knulls = surface_table(path, nullable)
    keys, p0, p1, keys2, q0 = surface_maps()
    cols.append(Col(*join(cols[K].values, knulls, keys, p0)))
    cols.append(Col(*join(cols[K].values, knulls, keys, p1)))
    lks = [ca.Lookup(K, keys, [p0, p1], inner=inner)]
    matched = cols[D0].present
    with ca.Reader(path) as r:
        for op in OPS:
            # standalone: a NULL operand fails the atom (inner-join semantics),
            # so INNER changes nothing here
            want = shapes.pred_mask(cols[D0], op, 2)
            assert 0 < want.sum() < shapes.N and not (want & ~matched).any()
            with r.scan(cols_mask=0b11, preds=[(D0, op, 2)], lookups=lks) as s:
                s.stage()
                assert s.select_count() == int(want.sum())
                res = s.select(cols=[D0, D1])
                check_join(res, D1, cols[D1].values, (~cols[D1].present).astype(np.uint8), want)
                assert s.agg([(ca.AGG_COUNT_STAR, -1)])[0].count == int(want.sum())
            # in an or_group with a table column: unmatched rows pass through
            # the table atom, unless INNER drops them
            want = shapes.pred_mask(cols[D0], op, 2) | shapes.pred_mask(cols[V], ca.PRED_LT, -2000)
            assert (want & ~matched).any()
            if inner:
                want = want & matched
            with r.scan(cols_mask=0b11, preds=[(D0, op, 2, 7), (V, ca.PRED_LT, -2000, 7)],
                        lookups=lks) as s:
                s.stage()
                res = s.select(cols=[D0])
                check_join(res, D0, cols[D0].values, (~cols[D0].present).astype(np.uint8), want)
        # two conjuncts on two payloads of one lookup, plus INNER
        want = shapes.pred_mask(cols[D0], ca.PRED_GE, 0) & \
            shapes.pred_mask(cols[D1], ca.PRED_LT, 500 * 1000003)
        assert 0 < want.sum()
        with r.scan(preds=[(D0, ca.PRED_GE, 0), (D1, ca.PRED_LT, 500 * 1000003)],
                    lookups=[ca.Lookup(K, keys, [p0, p1], inner=True)]) as s:
            s.stage()
            assert np.array_equal(s.select(cols=[D0])["row_numbers"], np.nonzero(want)[0])


@pytest.mark.parametrize("nullable", [True, False])
@pytest.mark.parametrize("inner", [False, True])
def test_lookup_plus_in_set(nullable, inner, tmp_path):
    path = str(tmp_path / "mix.cs")
    cols, knulls = surface_table(path, nullable)
    keys, p0, p1, keys2, q0 = surface_maps()
    cols.append(Col(*join(cols[K].values, knulls, keys, p0)))
    S = list(range(0, 997, 2))
    in_S = cols[K].present & np.isin(cols[K].values, S)
    dn = (~cols[D0].present).astype(np.uint8)
    with ca.Reader(path) as r:
        # the set alone: unmatched rows stay (NULL) unless INNER drops them
        want = in_S & cols[D0].present if inner else in_S
        assert (in_S & ~cols[D0].present).any()
        with r.scan(cols_mask=0b11, preds=[(K, ca.PRED_IN, S)],
                    lookups=[ca.Lookup(K, keys, [p0], inner=inner)]) as s:
            s.stage()
            res = s.select(cols=[K, D0])
            check_join(res, D0, cols[D0].values, dn, want)
            assert s.agg([(ca.AGG_COUNT_COL, D0)])[0].count == int((in_S & cols[D0].present).sum())
        # the set AND a predicate on the derived column
        want = in_S & shapes.pred_mask(cols[D0], ca.PRED_NE, 0)
        assert 0 < want.sum() < in_S.sum()
        with r.scan(cols_mask=0b11, preds=[(K, ca.PRED_IN, S), (D0, ca.PRED_NE, 0)],
                    lookups=[ca.Lookup(K, keys, [p0], inner=inner)]) as s:
            s.stage()
            assert s.set_form(0)[0] != ca.SET_FORM_NONE and s.lookup_form(0)[0] != 0
            res = s.select(cols=[K, D0])
            check_join(res, D0, cols[D0].values, dn, want)
            assert np.array_equal(res["values"][K], cols[K].values[want])
    # IN on a derived id is refused at begin
    with ca.Reader(path) as r:
        with pytest.raises(ca.CStripeError, match="derived"):
            r.scan(preds=[(D0, ca.PRED_IN, [1, 2])], lookups=[ca.Lookup(K, keys, [p0])])


# ------------------------------------------------------------------ stage errors
def test_device_map_duplicates_and_recovery(tmp_path, monkeypatch):
    import torch
    path = str(tmp_path / "dup.cs")
    cols, knulls = surface_table(path, True)
    keys, p0, p1, keys2, q0 = surface_maps()
    dup_keys = list(keys)
    assert len(keys) > 250
    dup_keys[17] = dup_keys[200]
    for form in (HASH, DIRECT):
        force_form(monkeypatch, form)
        with ca.Reader(path) as r:
            dk = torch.tensor(dup_keys, dtype=torch.int64, device="cuda:0")
            dp = torch.arange(len(dk), dtype=torch.int64, device="cuda:0")
            with r.scan(lookups=[ca.Lookup(K, dk, [dp])]) as s:
                with pytest.raises(ca.CStripeError, match=r"rc=-5.*lookup 0"):
                    s.stage()
                with pytest.raises(ca.CStripeError, match=r"rc=-4"):   # left unstaged
                    s.agg([(ca.AGG_COUNT_STAR, -1)])
                assert s.lookup_form(0) == (ca.LOOKUP_FORM_NONE, 0)
            # the sentinel key twice (hash form's flag word)
            dk = torch.tensor([-1, 5, -1], dtype=torch.int64, device="cuda:0")
            with r.scan(lookups=[ca.Lookup(K, dk, [dk.clone()])]) as s:
                with pytest.raises(ca.CStripeError, match=r"rc=-5"):
                    s.stage()
            # a later correct scan on the same reader works
            gk = torch.tensor(keys, dtype=torch.int64, device="cuda:0")
            gp = torch.tensor(p0, dtype=torch.int64, device="cuda:0")
            wv, wn = join(cols[K].values, knulls, keys, p0)
            with r.scan(lookups=[ca.Lookup(K, gk, [gp])]) as s:
                s.stage()
                check_join(s.select(cols=[D0]), D0, wv, wn)


def _two_devices():
    try:
        import torch
        return torch.cuda.is_available() and torch.cuda.device_count() >= 2
    except Exception:
        return False


if _two_devices():
    def test_device_map_on_the_wrong_device(tmp_path):
        import torch
        path = str(tmp_path / "dev.cs")
        surface_table(path, False)
        dk = torch.tensor([3, 6, 9], dtype=torch.int64, device="cuda:1")
        with ca.Reader(path) as r, r.scan(lookups=[ca.Lookup(K, dk, [dk.clone()])]) as s:
            with pytest.raises(ca.CStripeError, match=r"rc=-5"):
                s.stage(0)
            s.stage(1)
            assert s.select_count() == shapes.N


def test_derived_slots_count_against_the_projection(tmp_path):
    n_cols = 16
    a = np.arange(50, dtype=np.int64)
    path = str(tmp_path / "wide.cs")
    ca.write_table(path, [(f"c{j}", ca.I64, 0) for j in range(n_cols)],
                   [a + j for j in range(n_cols)])
    keys, p = [1, 2, 3, 60], [10, 20, 30, 40]
    with ca.Reader(path) as r:
        # 15 table columns + 2 payloads: one slot too many
        with r.scan(cols_mask=(1 << 15) - 1, lookups=[ca.Lookup(0, keys, [p, p])]) as s:
            with pytest.raises(ca.CStripeError, match=r"rc=-5"):
                s.stage()
            with pytest.raises(ca.CStripeError, match=r"rc=-4"):   # left unstaged
                s.agg([(ca.AGG_COUNT_STAR, -1)])
        # 14 + 2 = 16 fits; the key column is projected implicitly
        with r.scan(cols_mask=((1 << 14) - 1) << 1, lookups=[ca.Lookup(0, keys, [p, p])]) as s:
            with pytest.raises(ca.CStripeError, match=r"rc=-5"):
                s.stage()                      # 14 + the key column + 2
        with r.scan(cols_mask=(1 << 14) - 1, lookups=[ca.Lookup(0, keys, [p, p])]) as s:
            s.stage()
            D = s.derived(0, 1)
            assert D == 17
            wv, wn = join(a, None, keys, p)
            check_join(s.select(cols=[D]), D, wv, wn)


# ----------------------------------------------- device build side: the Q3 shape
def q3_tables(tmp_path):
    j = np.arange(3000, dtype=np.int64)
    o_key = j * 3 + 1
    o_date = (j * 7919) % 1000
    o_date[:1400] = 999                       # kept keys start at 4201
    o_date[2667:2799] = 999                   # no kept key in 8000..8396
    o_prio = (j * 13 + j // 9) % 5
    opath, lpath = str(tmp_path / "orders.cs"), str(tmp_path / "lineitem.cs")
    ca.write_table(opath, [("o_key", ca.I64, 0), ("o_date", ca.I64, 0), ("o_prio", ca.I64, 0)],
                   [o_key, o_date, o_prio], chunk_group_row_limit=200)
    i = np.arange(shapes.N, dtype=np.int64)
    l_key = i * 4                             # ascending: chunks cover key ranges
    l_price = (i * 131) % 10007
    ca.write_table(lpath, [("l_key", ca.I64, 0), ("l_price", ca.I64, 0)],
                   [l_key, l_price], chunk_group_row_limit=shapes.CG)
    return opath, lpath, (o_key, o_date, o_prio), (l_key, l_price)


def test_q3_shape_device_build_side(tmp_path):
    """SELECT o_prio, SUM(l_price), COUNT(*) FROM lineitem JOIN orders ON
    l_key = o_key WHERE o_date in [100, 600) AND o_date < 450 GROUP BY o_prio
    ORDER BY o_prio — orders filtered on the device, its columns going
    straight into the lookup"""
    import torch
    opath, lpath, (o_key, o_date, o_prio), (l_key, l_price) = q3_tables(tmp_path)
    keep = (o_date >= 100) & (o_date < 600)
    keys, dates, prios = o_key[keep], o_date[keep], o_prio[keep]
    assert len(keys) > 100 and keys.min() >= 4201 and keys.max() > 8396
    with ca.Reader(opath) as ro, \
            ro.scan(cols_mask=0b111, preds=[(1, ca.PRED_GE, 100), (1, ca.PRED_LT, 600)]) as so:
        so.stage()
        dev = so.select(cols=[0, 1, 2], want_nulls=False, want_row_numbers=False,
                        device=True)["values"]
    assert all(isinstance(dev[c], torch.Tensor) and dev[c].is_cuda for c in (0, 1, 2))
    assert np.array_equal(dev[0].cpu().numpy(), keys)

    DATE, PRIO = 2, 3
    cols = [Col(l_key), Col(l_price), Col(*join(l_key, None, keys, dates)),
            Col(*join(l_key, None, keys, prios))]
    rows = cols[DATE].present & shapes.pred_mask(cols[DATE], ca.PRED_LT, 450)
    assert 0 < rows.sum() < cols[DATE].present.sum()
    bounds = [(int(l_key[a]), int(l_key[b - 1])) for a, b in
              ((0, 1000), (1000, 2000), (2000, 2100))]
    by_range = sum(int(keys.max()) < mn or int(keys.min()) > mx for mn, mx in bounds)
    exact = sum(not any(mn <= int(x) <= mx for x in keys) for mn, mx in bounds)
    assert (by_range, exact) == (1, 2)
    aggs = shapes.with_one(cols, [(ca.AGG_SUM_I64, 1), (ca.AGG_COUNT_STAR, -1)])
    preds = [(DATE, ca.PRED_LT, 450)]
    out = []
    with ca.Reader(lpath) as rl:
        for kk, pp, pruned in ((dev[0], [dev[1], dev[2]], by_range),
                               (keys, [dates, prios], exact)):
            with rl.scan(cols_mask=0b11, preds=preds,
                         lookups=[ca.Lookup(0, kk, pp, inner=True)]) as s:
                assert s.chunk_groups_filtered == pruned
                s.stage()
                res = s.agg_hashed(aggs, [PRIO], 16)
                check_hashed(res, [PRIO], cols, aggs, rows, "q3")
                assert res["keys"][0].tolist() == sorted(set(prios[np.isin(keys, l_key[rows])].tolist()))
                top = s.select_topn([(PRIO, "asc"), (1, "desc")], 10, cols=[PRIO, 1, DATE])
                idx = np.nonzero(rows)[0]
                order = idx[np.lexsort((idx, -l_price[idx], cols[PRIO].values[idx]))][:10]
                assert np.array_equal(top["row_numbers"], order)
                assert np.array_equal(top["values"][DATE], cols[DATE].values[order])
                out.append((res["keys"][0].tobytes(), res["key_nulls"][0].tobytes(),
                            res["partials"].tobytes(), top["row_numbers"].tobytes(),
                            top["values"][PRIO].tobytes()))
    assert out[0] == out[1]                    # the host-map twin: the same bytes


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
    keys = [0, 2, 5, 700, 702, 1500, 1501, 2796, 2798]     # 5 and 1501 are absent
    payload = [pay(k) for k in keys]
    wv, wn = join(key, None, keys, payload)
    rows = wn == 0
    starts = list(range(0, shapes.N, shapes.CG))
    bounds = [(int(key[b + a]), int(key[min(b + a + shapes.CG, b + shapes.N) - 1]))
              for b in (0, shapes.N) for a in starts]
    pruned = sum(not any(mn <= x <= mx for x in keys) for mn, mx in bounds)
    assert len(bounds) == 6 and 0 < pruned < 6
    with ca.Reader(str(d)) as r, \
            r.scan(cols_mask=0b11, lookups=[ca.Lookup(0, keys, [payload], inner=True)]) as s:
        assert s.chunk_groups_filtered == pruned
        s.stage()
        D = s.derived(0, 0)
        res = s.select(cols=[1, D])
        check_join(res, D, wv, wn, rows)                       # table-wide row numbers
        assert np.array_equal(res["values"][1], val[rows])
        assert s.agg([(ca.AGG_SUM_I64, 1)])[0].i128 == int(val[rows].sum())


@pytest.mark.parametrize("batch_rows", [1, 1000, 1999, 2000, 5000])
def test_probe_batches(batch_rows, tmp_path, monkeypatch):
    """probe, rank scan and gather run over batches of chunk groups
    (CSTRIPE_LOOKUP_BATCH_ROWS): one group per batch, two groups then one,
    everything in one — the same column every time"""
    path = str(tmp_path / "batch.cs")
    cols, knulls = surface_table(path, True)
    keys, p0, p1, keys2, q0 = surface_maps()
    wv0, wn0 = join(cols[K].values, knulls, keys, p0)
    wv1, wn1 = join(cols[K].values, knulls, keys, p1)
    monkeypatch.setenv("CSTRIPE_LOOKUP_BATCH_ROWS", str(batch_rows))
    for form in (HASH, DIRECT):
        force_form(monkeypatch, form)
        res, (d0, d1) = select_derived(path, K, keys, [p0, p1])
        check_join(res, d0, wv0, wn0)
        check_join(res, d1, wv1, wn1)


# ------------------------------------------------ re-invocation and interleaving
def test_reinvocation_interleaving_and_restage(tmp_path):
    import torch
    path = str(tmp_path / "re.cs")
    cols, knulls = surface_table(path, True)
    k, v, g = (cols[c].values for c in (K, V, G))
    keys, p0, p1, keys2, q0 = surface_maps()
    gk = torch.tensor(keys, dtype=torch.int64, device="cuda:0")
    gp = torch.tensor(p0, dtype=torch.int64, device="cuda:0")
    aggs = [(ca.AGG_COUNT_STAR, -1), (ca.AGG_SUM_I64, V), (ca.AGG_SUM_I64, D0)]

    def snapshot(s):
        res = s.select(cols=[K, V, D0])
        top = s.select_topn([(D0, "desc", "last"), (V, "asc")], 20, cols=[D0])
        return (bytes(b"".join(bytes(p) for p in s.agg(aggs))),
                res["row_numbers"].tobytes(), res["values"][D0].tobytes(),
                res["nulls"][D0].tobytes(), res["values"][V].tobytes(),
                s.agg_hashed(aggs, [D0], 64)["partials"].tobytes(),
                top["row_numbers"].tobytes())

    def expect(payload):
        wv, wn = join(k, knulls, keys, payload)
        rows = (wn == 0) & (v > -2000)
        return wv, wn, rows

    with ca.Reader(path) as r, \
            r.scan(cols_mask=0b1111, preds=[(V, ca.PRED_GT, -2000)],
                   lookups=[ca.Lookup(K, gk, [gp], inner=True)]) as s, \
            r.scan(cols_mask=0b111) as twin:
        s.stage()
        twin.stage()
        wv, wn, rows = expect(p0)
        first = snapshot(s)
        assert np.frombuffer(first[1], np.int64).tolist() == np.nonzero(rows)[0].tolist()
        assert np.frombuffer(first[2], np.int64).tolist() == wv[rows].tolist()
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
        s.stage()                                   # restage rebuilds everything
        assert s.lookup_form(0)[0] != ca.LOOKUP_FORM_NONE
        assert snapshot(s) == first
        # the device payload changes between stages (inside its begin-time
        # range): results follow it
        new_p = p0[::-1]
        assert new_p != p0 and min(new_p) == min(p0) and max(new_p) == max(p0)
        gp.copy_(torch.tensor(new_p, dtype=torch.int64))
        torch.cuda.synchronize()
        s.stage()
        wv2, wn2, rows2 = expect(new_p)
        second = snapshot(s)
        assert second != first
        assert np.frombuffer(second[1], np.int64).tolist() == np.nonzero(rows2)[0].tolist()
        assert np.frombuffer(second[2], np.int64).tolist() == wv2[rows2].tolist()
        assert s.agg(aggs)[2].i128 == int(wv2[rows2].sum())
        # a payload value outside the begin-time range: the packed-key
        # surfaces refuse it, the others still read it
        gp[0] = max(p0) + 1000
        torch.cuda.synchronize()
        s.stage()
        hit = (k == keys[0]) & (knulls == 0) & (v > -2000)
        if hit.any():
            with pytest.raises(ca.CStripeError, match=r"rc=-3"):
                s.agg_hashed(aggs, [D0], 64)
        assert s.select_count() == int(rows2.sum())
