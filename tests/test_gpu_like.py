"""CSTRIPE_PRED_LIKE / NOT_LIKE on the GPU: both read forms (the dictionary
form and the dictionary-free stream form) on every query surface, against the
recursive statement of the rules in likeutil. Every comparison is exact."""
import numpy as np
import pytest

import citus_amd as ca
import futil
import likeutil
import vtutil

pytestmark = pytest.mark.gpu

N = 5000
CHUNK, STRIPE = 1000, 3000          # 2 stripes, 5 chunk groups
CODECS = {"none": ca.COMP_NONE, "lz4": ca.COMP_LZ4, "zstd": ca.COMP_ZSTD}
DEFS = [("id", ca.I64, 0), ("val", ca.I64, 0), ("t", ca.VARTEXT, 0),
        ("u", ca.VARTEXT, 0), ("m", ca.I32, 0)]
LIKE, NOT_LIKE = ca.PRED_LIKE, ca.PRED_NOT_LIKE
FORMS = ["dict", "stream"]
T, U = 2, 3


def make_pool():
    """100 distinct strings: p_type-like words, every header / padding edge
    length, the wildcard and escape bytes as data, multi-byte characters"""
    pool = {b"", b"ab", b"abc", b"%", b"_", b"\\", b"100%", b"a_c", b"a\\c",
            "é".encode(), "€uro".encode(), "a😀c".encode(), "été".encode(), b"MAIL"}
    for a in (b"PROMO", b"STANDARD", b"SMALL", b"ECONOMY"):
        for b in (b"PLATED", b"BRUSHED", b"ANODIZED"):
            for c in (b"BRASS", b"TIN", b"STEEL"):
                pool.add(a + b" " + b + b" " + c)
    for n in vtutil.EDGE_LENS:
        pool.add(bytes((97 + (n + i) % 26) for i in range(n)))
    i = 0
    while len(pool) < 100:
        pool.add(b"w%02d" % i)
        i += 1
    return sorted(pool)


POOL = make_pool()
WORDS = [b"special", b"requests", b"Customer", b"Complaints", b"furiously", b"pending",
         b"deposits", b"sleep", b"carefully", b"final", "café".encode(), "€".encode()]


class Table:
    def __init__(self):
        rng = np.random.default_rng(11)
        self.ids = np.arange(N, dtype=np.int64)
        self.val = rng.integers(-10**9, 10**9, N, dtype=np.int64)
        self.val_null = (rng.random(N) < 0.1).astype(np.uint8)
        t = [POOL[i] for i in rng.integers(0, len(POOL), N)]
        for i in range(N):
            if 3000 <= i < 4000:
                t[i] = b"MAIL"                              # chunk group 3: one value
            if rng.random() < 0.1 or 2000 <= i < 3000:      # chunk group 2: all NULL
                t[i] = None
        self.t = t
        # comment-like, near unique, 30-80 bytes
        u = []
        for i in range(N):
            words = [WORDS[k] for k in rng.integers(0, len(WORDS), 6)]
            c = (b"%05d " % i) + b" ".join(words)
            u.append(c[:80].ljust(30, b"."))
        for i in range(0, N, 37):
            u[i] = None
        self.u = u
        self.m = (self.ids % 3).astype(np.int32)

    def write(self, path, codec, rows=None):
        sl = slice(None) if rows is None else rows
        ca.write_table(path, DEFS,
                       [self.ids[sl], self.val[sl], self.t[sl], self.u[sl], self.m[sl]],
                       nulls=[None, self.val_null[sl], None, None, None],
                       chunk_group_row_limit=CHUNK, stripe_row_limit=STRIPE,
                       compression=codec)


@pytest.fixture(scope="module")
def tab():
    t = Table()
    assert len({v for v in t.t if v is not None}) == 100
    assert len({v for v in t.u if v is not None}) > 4800
    assert all(30 <= len(v) <= 80 for v in t.u if v is not None)
    return t


@pytest.fixture(scope="module", params=list(CODECS))
def path(request, tab, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("like") / f"t_{request.param}.cs")
    tab.write(p, CODECS[request.param])
    if request.param != "none":     # the codec really is exercised
        ft = futil.read_footer(p)
        kinds = {n["comp_type"] for st in ft["stripes"] for n in st["nodes"][U]}
        assert kinds == {CODECS[request.param]}
    return p


@pytest.fixture(scope="module")
def lz4_path(tab, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("like1") / "lz4.cs")
    tab.write(p, ca.COMP_LZ4)
    return p


@pytest.fixture(scope="module")
def masks(tab):
    """memo of likeutil masks: (col, pattern, negate) -> bool array"""
    memo = {}

    def get(col, pat, negate=False):
        pat = pat.encode() if isinstance(pat, str) else pat
        if (col, pat) not in memo:
            m = likeutil.like_mask(tab.t if col == T else tab.u, pat)
            m.setflags(write=False)
            memo[(col, pat)] = m
        if not negate:
            return memo[(col, pat)]
        present = np.array([v is not None for v in (tab.t if col == T else tab.u)])
        return present & ~memo[(col, pat)]
    return get


def force(monkeypatch, form):
    if form is None:
        monkeypatch.delenv("CSTRIPE_LIKE_FORM", raising=False)
    else:
        monkeypatch.setenv("CSTRIPE_LIKE_FORM", form)


AGGS = [(ca.AGG_COUNT_STAR, -1), (ca.AGG_SUM_I64, 1)]


def check_aggs(tab, parts, rows):
    live = [i for i in rows if not tab.val_null[i]]
    assert (parts[0].count, parts[0].is_null) == (len(rows), 0)
    assert parts[1].is_null == (0 if live else 1)
    if live:
        assert parts[1].i128 == sum(int(tab.val[i]) for i in live)
        assert parts[1].count == len(live)


def check_hashed(tab, res, rows):
    """GROUP BY m: COUNT(*), SUM(val)"""
    groups = {}
    for i in rows:
        groups.setdefault(int(tab.m[i]), []).append(i)
    assert res["n_groups"] == len(groups)
    for g, key in enumerate(sorted(groups)):
        assert res["keys"][0][g] == key and res["key_nulls"][0][g] == 0
        live = [i for i in groups[key] if not tab.val_null[i]]
        p = res["partials"][g]
        assert (p[0]["count"], p[0]["is_null"]) == (len(groups[key]), 0)
        assert p[1]["is_null"] == (0 if live else 1)
        if live:
            assert ca.partial_i128(p[1]) == sum(int(tab.val[i]) for i in live)


def check_surfaces(tab, s, want):
    """select, agg, agg_hashed and select_topn of a staged scan against the
    passing row numbers `want` (ascending)"""
    rows = s.select(cols=[0], want_nulls=False)
    assert rows["n_rows"] == len(want)
    assert np.array_equal(rows["row_numbers"], want)
    assert np.array_equal(rows["values"][0], want)
    check_aggs(tab, s.agg(AGGS), [int(i) for i in want])
    check_hashed(tab, s.agg_hashed(AGGS, [4], 16), [int(i) for i in want])
    top = s.select_topn([(0, "desc")], 7, cols=[0], want_nulls=False)
    assert np.array_equal(top["row_numbers"], want[::-1][:7])


SURFACE_PATTERNS = [(T, "PROMO%"), (T, "%BRASS"), (T, "%L_ PLATED%"), (T, "_"), (T, "%\\%"),
                    (U, "%special%requests%"), (U, "%Customer%Complaints%"), (U, "0001_ %é%")]


@pytest.mark.parametrize("op", [LIKE, NOT_LIKE], ids=["like", "not_like"])
@pytest.mark.parametrize("form", FORMS)
def test_every_surface(tab, lz4_path, masks, monkeypatch, form, op):
    force(monkeypatch, form)
    with ca.Reader(lz4_path) as r:
        for col, pat in SURFACE_PATTERNS:
            want = np.flatnonzero(masks(col, pat, op == NOT_LIKE))
            assert 0 < len(want) < N, (col, pat)
            # the column is only pattern-matched: the stream form is legal
            with r.scan(cols_mask=0b10011, preds=[(col, op, pat)]) as s:
                assert s.like_form(col) is None
                s.stage(0)
                assert s.like_form(col) == form
                check_surfaces(tab, s, want)
            # the caller reads the column too: the dictionary form, always
            if col == T:
                with r.scan(cols_mask=0b10111, preds=[(col, op, pat)]) as s:
                    s.stage(0)
                    assert s.like_form(col) == "dict"
                    check_surfaces(tab, s, want)
                    got = s.select(cols=[T], decode_text=True)
                    assert list(got["text"][T]) == [tab.t[i] for i in want]


@pytest.mark.parametrize("form", FORMS)
def test_codecs_and_both_columns(tab, path, masks, monkeypatch, form):
    force(monkeypatch, form)
    preds = [(T, LIKE, "%A%"), (U, NOT_LIKE, "%special%requests%"), (0, ca.PRED_GE, 150)]
    want = np.flatnonzero(masks(T, "%A%") & masks(U, "%special%requests%", True) &
                          (tab.ids >= 150))
    assert 100 < len(want) < N
    with ca.Reader(path) as r, r.scan(cols_mask=0b10011, preds=preds) as s:
        s.stage(0)
        assert (s.like_form(T), s.like_form(U)) == (form, form)
        check_surfaces(tab, s, want)


EDGE_CHUNK = 16


def edge_values():
    """every EDGE_LENS length as a run of a's and as one ending in b; one value
    of 65535 a's; NULLs; chunk group 1 (rows 16..31) all NULL"""
    vals = []
    for n in vtutil.EDGE_LENS:
        vals.append(b"a" * n)
        vals.append(b"a" * max(n - 1, 0) + b"b")
        if len(vals) % 5 == 0:
            vals.append(None)
    vals = vals[:16] + [None] * 16 + vals[16:]
    vals.append(b"a" * 65535)
    vals.append(b"x" + b"a" * 300 + b"b")
    vals.append("é".encode() * 64)
    return vals


EDGE_PATTERNS = ["%aaaaaaab", "%a", "%", "", "_", "_%", "%b", "a%b", "%_a_", "no such value",
                 "a" * 126, "a" * 127 + "_", "%" + "é" * 3, "_" * 64]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("codec", list(CODECS))
def test_value_lengths(tmp_path, monkeypatch, codec, form):
    force(monkeypatch, form)
    vals = edge_values()
    n = len(vals)
    assert vals[16:32] == [None] * 16 and any(v is None for v in vals[:16])
    p = str(tmp_path / "edge.cs")
    ca.write_table(p, [("id", ca.I64, 0), ("t", ca.VARTEXT, 0)],
                   [np.arange(n, dtype=np.int64), vals],
                   chunk_group_row_limit=EDGE_CHUNK, stripe_row_limit=2 * EDGE_CHUNK,
                   compression=CODECS[codec])
    with ca.Reader(p) as r:
        for pat in EDGE_PATTERNS:
            for op in (LIKE, NOT_LIKE):
                want = np.flatnonzero(likeutil.like_mask(vals, pat, op == NOT_LIKE))
                with r.scan(cols_mask=1, preds=[(1, op, pat)]) as s:
                    s.stage(0)
                    assert s.like_form(1) == form
                    rows = s.select(cols=[0], want_nulls=False)
                    assert np.array_equal(rows["row_numbers"], want), (pat, op)
                    assert s.agg([(ca.AGG_COUNT_STAR, -1)])[0].count == len(want)
        # the long value is really decided by the matcher
        assert likeutil.match(b"%a", b"a" * 65535)
        assert not likeutil.match(b"%aaaaaaab", b"a" * 65535)
        # a zero-row selection
        with r.scan(cols_mask=1, preds=[(1, LIKE, "no such value")]) as s:
            s.stage(0)
            assert s.select_count() == 0
            assert s.select(cols=[0])["n_rows"] == 0


@pytest.mark.parametrize("form", FORMS)
def test_two_shard_directory(tab, tmp_path, masks, monkeypatch, form):
    force(monkeypatch, form)
    d = tmp_path / "shards"
    d.mkdir()
    tab.write(str(d / "shard00.cs"), ca.COMP_LZ4, slice(0, 3000))
    tab.write(str(d / "shard01.cs"), ca.COMP_ZSTD, slice(3000, N))
    with ca.Reader(str(d)) as r:
        for col, pat in ((T, "%BRASS"), (U, "%special%requests%")):
            want = np.flatnonzero(masks(col, pat))
            with r.scan(cols_mask=0b10011, preds=[(col, LIKE, pat)]) as s:
                s.stage(0)
                assert s.like_form(col) == form
                check_surfaces(tab, s, want)


@pytest.mark.parametrize("form", FORMS)
def test_pruned_chunk_groups(tmp_path, monkeypatch, form):
    force(monkeypatch, form)
    vals = sorted(bytes([97 + i // 250]) + b"-%04d" % ((i * 7919) % 2000) for i in range(2000))
    vals[5] = None
    p = str(tmp_path / "sorted.cs")
    ca.write_table(p, [("id", ca.I64, 0), ("t", ca.VARTEXT, 0)],
                   [np.arange(2000, dtype=np.int64), vals],
                   chunk_group_row_limit=200, stripe_row_limit=1000, compression=ca.COMP_LZ4)
    bounds = []
    for k in range(0, 2000, 200):
        present = [v for v in vals[k:k + 200] if v is not None]
        bounds.append((vtutil.prefix_key(min(present)), vtutil.prefix_key(max(present))))
    with ca.Reader(p) as r:
        for pat, some in (("c%", True), ("c-1%3", True), ("e-0__5", True), ("%3", False),
                          ("z%", True)):
            want = np.flatnonzero(likeutil.like_mask(vals, pat))
            pruned = sum(likeutil.refuted(pat.encode(), mn, mx) for mn, mx in bounds)
            assert (pruned > 0) == some
            with r.scan(cols_mask=1, preds=[(1, LIKE, pat)]) as s:
                assert s.chunk_groups_filtered == pruned, pat
                s.stage(0)
                rows = s.select(cols=[0], want_nulls=False)
                assert np.array_equal(rows["row_numbers"], want), pat
                assert np.array_equal(rows["values"][0], want), pat


def test_cnf(tab, lz4_path, masks, monkeypatch):
    force(monkeypatch, None)
    eq_mail = np.array([v == b"MAIL" for v in tab.t])
    with ca.Reader(lz4_path) as r:
        # LIKE OR EQ in one or_group: the EQ needs ranks
        preds = [(T, LIKE, "%TIN", 1), (T, ca.PRED_EQ, b"MAIL", 1)]
        with r.scan(cols_mask=0b10011, preds=preds) as s:
            s.stage(0)
            assert s.like_form(T) == "dict"
            check_surfaces(tab, s, np.flatnonzero(masks(T, "%TIN") | eq_mail))
        # LIKE OR an integer atom: still only pattern-matched
        preds = [(T, LIKE, "%TIN", 1), (0, ca.PRED_LT, 40, 1)]
        with r.scan(cols_mask=0b10011, preds=preds) as s:
            s.stage(0)
            assert s.like_form(T) == "stream"
            check_surfaces(tab, s, np.flatnonzero(masks(T, "%TIN") | (tab.ids < 40)))
        # LIKE AND NOT LIKE of the same pattern: nothing
        preds = [(T, LIKE, "PROMO%"), (T, NOT_LIKE, "PROMO%")]
        with r.scan(cols_mask=0b10011, preds=preds) as s:
            s.stage(0)
            assert s.select_count() == 0
            assert s.agg([(ca.AGG_COUNT_STAR, -1)])[0].count == 0
        # ... of different patterns
        preds = [(T, LIKE, "PROMO%"), (T, NOT_LIKE, "%BRASS"), (U, LIKE, "%final%")]
        want = np.flatnonzero(masks(T, "PROMO%") & masks(T, "%BRASS", True) &
                              masks(U, "%final%"))
        assert len(want) > 20
        with r.scan(cols_mask=0b10011, preds=preds) as s:
            s.stage(0)
            assert (s.like_form(T), s.like_form(U)) == ("stream", "stream")
            check_surfaces(tab, s, want)
        # next to an IN text set on the same column: the dictionary form
        members = [b"MAIL", POOL[20], POOL[60], b"absent"]
        preds = [(T, NOT_LIKE, "%A%"), (T, ca.PRED_IN, members)]
        in_set = np.array([v in members for v in tab.t])
        want = np.flatnonzero(masks(T, "%A%", True) & in_set)
        with r.scan(cols_mask=0b10011, preds=preds) as s:
            s.stage(0)
            assert s.like_form(T) == "dict"
            assert s.set_form(0)[0] != ca.SET_FORM_NONE
            check_surfaces(tab, s, want)
        # next to a predicate on a lookup-derived column
        lk = ca.Lookup(4, np.array([0, 1], np.int64), [np.array([10, 20], np.int64)])
        preds = [(U, LIKE, "%sleep%"), (5, ca.PRED_GE, 20)]
        want = np.flatnonzero(masks(U, "%sleep%") & (tab.m == 1))
        assert len(want) > 50
        with r.scan(cols_mask=0b10011, preds=preds, lookups=[lk]) as s:
            s.stage(0)
            assert s.like_form(U) == "stream"
            check_surfaces(tab, s, want)


WIDE = 15                            # I8 columns, then one VARTEXT column


def wide_table(path):
    n = 300
    vals = [POOL[(i * 7) % len(POOL)] for i in range(n)]
    defs = [(f"c{i}", ca.I8, 0) for i in range(WIDE)] + [("t", ca.VARTEXT, 0)]
    cols = [((np.arange(n) + i) % 100).astype(np.int8) for i in range(WIDE)] + [vals]
    ca.write_table(path, defs, cols, chunk_group_row_limit=100, stripe_row_limit=300,
                   compression=ca.COMP_LZ4)
    return vals


@pytest.mark.parametrize("form", FORMS)
def test_member_slots_and_overflow(tmp_path, monkeypatch, form):
    force(monkeypatch, form)
    p = str(tmp_path / "wide.cs")
    vals = wide_table(p)
    fourteen = (1 << 14) - 1
    with ca.Reader(p) as r:
        # 14 integer columns + the text column + ONE member slot = 16: LIKE and
        # NOT LIKE of one pattern share it
        preds = [(WIDE, LIKE, "PROMO%"), (WIDE, NOT_LIKE, "PROMO%")]
        with r.scan(cols_mask=fourteen, preds=preds) as s:
            s.stage(0)
            assert s.select_count() == 0
        # one pattern, given as two constants: still one slot
        preds = [(WIDE, LIKE, "PROMO%"), (WIDE, LIKE, b"PROMO%")]
        with r.scan(cols_mask=fourteen, preds=preds) as s:
            s.stage(0)
            assert s.select_count() == int(likeutil.like_mask(vals, "PROMO%").sum())
        # two patterns need two: 17 slots
        preds = [(WIDE, LIKE, "PROMO%"), (WIDE, NOT_LIKE, "%TIN")]
        with r.scan(cols_mask=fourteen, preds=preds) as s:
            with pytest.raises(ca.CStripeError, match=r"rc=-5.*LIKE.*16 slots"):
                s.stage(0)
        # sixteen projected columns plus one LIKE
        with r.scan(cols_mask=(1 << 16) - 1, preds=[(WIDE, LIKE, "PROMO%")]) as s:
            with pytest.raises(ca.CStripeError, match=r"rc=-5.*LIKE.*16 slots"):
                s.stage(0)
            assert s.like_form(WIDE) is None
            with pytest.raises(ca.CStripeError, match="rc=-4"):      # left unstaged
                s.agg([(ca.AGG_COUNT_STAR, -1)])
        # fifteen plus one LIKE fit
        want = np.flatnonzero(likeutil.like_mask(vals, "%BRASS"))
        with r.scan(cols_mask=(1 << 14) - 1, preds=[(WIDE, LIKE, "%BRASS")]) as s:
            s.stage(0)
            assert np.array_equal(s.select(cols=[0])["row_numbers"], want)


def test_stream_form_has_no_distinct_limit(tab, lz4_path, masks, monkeypatch):
    force(monkeypatch, None)
    monkeypatch.setenv("CSTRIPE_VARTEXT_MAX_DISTINCT", "4")
    with ca.Reader(lz4_path) as r:
        for col, pat in ((T, "%STEEL"), (U, "%Customer%Complaints%")):
            want = np.flatnonzero(masks(col, pat))
            assert len(want) > 10
            with r.scan(cols_mask=0b10011, preds=[(col, LIKE, pat)]) as s:
                s.stage(0)
                assert s.like_form(col) == "stream"
                assert s.last_text_ms()[2:] == (0.0, 0.0)        # no dict, no remap
                check_surfaces(tab, s, want)
            # the same scan with the column in cols_mask needs the dictionary
            with r.scan(cols_mask=0b10011 | (1 << col), preds=[(col, LIKE, pat)]) as s:
                with pytest.raises(ca.CStripeError,
                                   match=rf"rc=-5.*column {col} .*\b4\b.*MAX_DISTINCT"):
                    s.stage(0)
                assert s.like_form(col) is None
        # forced dict is subject to the limit too
        monkeypatch.setenv("CSTRIPE_LIKE_FORM", "dict")
        with r.scan(cols_mask=0b10011, preds=[(T, LIKE, "%STEEL")]) as s:
            with pytest.raises(ca.CStripeError, match="rc=-5.*MAX_DISTINCT"):
                s.stage(0)


def test_stream_column_is_refused_elsewhere(tab, lz4_path, monkeypatch):
    force(monkeypatch, None)
    with ca.Reader(lz4_path) as r, \
            r.scan(cols_mask=0b10011, preds=[(T, LIKE, "PROMO%")]) as s:
        s.stage(0)
        assert s.like_form(T) == "stream"
        calls = [
            lambda: s.text_dict(T),
            lambda: s.select(cols=[0, T]),
            lambda: s.select_topn([(0, "asc")], 5, cols=[T]),
            lambda: s.select_topn([(T, "asc")], 5, cols=[0]),
            lambda: s.agg_hashed(AGGS, [T], 256),
            lambda: s.agg_hashed_topn(AGGS, [T], 256, [("agg", 0, "desc")], 3),
            lambda: s.agg([(ca.AGG_COUNT_COL, T)]),
        ]
        for k, call in enumerate(calls):
            with pytest.raises(ca.CStripeError, match="rc=-5") as e:
                call()
            m = ca.errmsg()
            assert "column 2" in m and "add it to cols_mask" in m, (k, m, str(e.value))
        # the scan still answers
        assert s.select_count() == sum(v is not None and v.startswith(b"PROMO") for v in tab.t)
    # with the column in cols_mask every one of them works
    with ca.Reader(lz4_path) as r, \
            r.scan(cols_mask=0b10111, preds=[(T, LIKE, "PROMO%")]) as s:
        s.stage(0)
        assert all(v.startswith(b"PROMO") for v in s.select(cols=[T], decode_text=True)["text"][T])
        assert s.agg([(ca.AGG_COUNT_COL, T)])[0].count == s.select_count()
        assert s.agg_hashed(AGGS, [T], 256)["n_groups"] == 9


def test_form_timing_and_restage(tab, lz4_path, masks, monkeypatch):
    force(monkeypatch, None)
    want = np.flatnonzero(masks(T, "%BRASS"))
    with ca.Reader(lz4_path) as r:
        with r.scan(cols_mask=0b10011, preds=[(0, ca.PRED_GE, 5)]) as s:      # no LIKE atom
            s.stage(0)
            assert s.last_like_ms() == (0.0, 0.0)
            assert s.like_form(T) is None and s.like_form(0) is None
        with r.scan(cols_mask=0b10011, preds=[(T, LIKE, "%BRASS")]) as s:
            assert s.like_form(T) is None and s.last_like_ms() == (0.0, 0.0)
            s.stage(0)
            match_ms, apply_ms = s.last_like_ms()
            assert s.like_form(T) == "stream" and s.like_form(U) is None
            assert s.like_form(0) is None and s.like_form(99) is None
            assert match_ms > 0 and apply_ms == 0
            first = s.select(cols=[0])["row_numbers"]
            assert np.array_equal(first, want)
            # a restage re-evaluates, and reads the switch again
            monkeypatch.setenv("CSTRIPE_LIKE_FORM", "dict")
            s.stage(0)
            match_ms, apply_ms = s.last_like_ms()
            assert s.like_form(T) == "dict"
            assert match_ms > 0 and apply_ms > 0
            assert np.array_equal(s.select(cols=[0])["row_numbers"], first)
            # forced stream on a column that needs ranks falls back to dict
        monkeypatch.setenv("CSTRIPE_LIKE_FORM", "stream")
        with r.scan(cols_mask=0b10111, preds=[(T, LIKE, "%BRASS")]) as s:
            s.stage(0)
            assert s.like_form(T) == "dict"
            assert np.array_equal(s.select(cols=[0])["row_numbers"], want)
            assert s.text_dict(T) == sorted({v for v in tab.t if v is not None})


@pytest.mark.parametrize("form", FORMS)
def test_interleaved_calls_are_stable(tab, lz4_path, masks, monkeypatch, form):
    force(monkeypatch, form)
    preds = [(U, NOT_LIKE, "%special%requests%"), (T, LIKE, "%E%")]
    want = np.flatnonzero(masks(U, "%special%requests%", True) & masks(T, "%E%"))
    assert len(want) > 100
    with ca.Reader(lz4_path) as r, r.scan(cols_mask=0b10011, preds=preds) as s:
        s.stage(0)
        for _ in range(2):
            check_aggs(tab, s.agg(AGGS), [int(i) for i in want])
            assert np.array_equal(s.select(cols=[0])["row_numbers"], want)
            check_hashed(tab, s.agg_hashed(AGGS, [4], 16), [int(i) for i in want])
