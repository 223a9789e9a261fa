"""CSTRIPE_VARTEXT on the GPU: the per-scan device dictionary (decode -> header
walk -> hash table -> gather -> host sort -> rank remap) and everything that
reads the column as dictionary ranks — predicates with string constants,
scan_agg, scan_select, scan_agg_hashed — against Python. Expected values come
from Python (bytes comparison is memcmp order); every comparison is exact."""
import bisect
import math
import os
import shutil

import numpy as np
import pytest

import citus_amd as ca
import futil
import vtutil

pytestmark = pytest.mark.gpu

N = 5000
CHUNK, STRIPE = 1000, 3000          # 2 stripes, 5 chunk groups
OPS = (ca.PRED_LT, ca.PRED_LE, ca.PRED_GT, ca.PRED_GE, ca.PRED_EQ, ca.PRED_NE)
CODECS = {"none": ca.COMP_NONE, "lz4": ca.COMP_LZ4, "zstd": ca.COMP_ZSTD}
DEFS = [("id", ca.I64, 0), ("val", ca.I64, 0), ("t", ca.VARTEXT, 0),
        ("u", ca.VARTEXT, 0), ("m", ca.I32, 0)]
TWIN_DEFS = [("id", ca.I64, 0), ("val", ca.I64, 0), ("t", ca.I32, 0),
             ("u", ca.VARTEXT, 0), ("m", ca.I32, 0)]
AGGS = [(ca.AGG_COUNT_STAR, -1), (ca.AGG_SUM_I64, 1), (ca.AGG_COUNT_COL, 2)]


def make_pool():
    """40 distinct strings: every header/padding edge length, b"", the pair
    b"ab" / b"abc", two values sharing a 7-byte prefix"""
    pool = {b"", b"ab", b"abc", b"AIR", b"MAIL", b"SHIP", b"TRUCK", b"RAIL",
            b"REG AIR", b"FOB", b"DELIVER IN PERSON", b"COLLECT COD",
            b"TAKE BACK RETURN", b"prefix7A", b"prefix7B", b"\xc3\xa9t\xc3\xa9"}
    for n in vtutil.EDGE_LENS:
        pool.add(bytes((97 + (n + i) % 26) for i in range(n)))
    i = 0
    while len(pool) < 40:
        pool.add(b"w%02d" % i)
        i += 1
    return sorted(pool)


POOL = make_pool()
V127 = next(v for v in POOL if len(v) == 127)
ONLY = b"MAIL"                      # chunk group 3 holds just this value


class Table:
    def __init__(self):
        rng = np.random.default_rng(7)
        self.ids = np.arange(N, dtype=np.int64)
        self.val = rng.integers(-10**9, 10**9, N, dtype=np.int64)
        self.val_null = (rng.random(N) < 0.1).astype(np.uint8)
        t = [POOL[i] for i in rng.integers(0, len(POOL), N)]
        for i in range(N):
            if 3000 <= i < 4000:
                t[i] = ONLY
            if rng.random() < 0.1 or 2000 <= i < 3000:      # chunk group 2: all NULL
                t[i] = None
        self.t = t
        perm = rng.permutation(N)
        self.u = [b"k%05d" % perm[i] + b"x" * (perm[i] % 9) for i in range(N)]
        self.m = (self.ids % 3).astype(np.int32)
        self.dict_t = sorted({v for v in t if v is not None})

    def columns(self, t=None):
        return [self.ids, self.val, list(self.t if t is None else t), list(self.u), self.m]

    def nulls(self):
        return [None, self.val_null, None, None, None]

    def write(self, path, codec, rows=None):
        sl = slice(None) if rows is None else rows
        ca.write_table(path, DEFS,
                       [self.ids[sl], self.val[sl], self.t[sl], self.u[sl], self.m[sl]],
                       nulls=[None, self.val_null[sl], None, None, None],
                       chunk_group_row_limit=CHUNK, stripe_row_limit=STRIPE,
                       compression=codec)

    def rank(self, v):
        return None if v is None else bisect.bisect_left(self.dict_t, v)


@pytest.fixture(scope="module")
def tab():
    return Table()


@pytest.fixture(scope="module", params=list(CODECS))
def path(request, tab, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("vt") / f"t_{request.param}.cs")
    tab.write(p, CODECS[request.param])
    if request.param != "none":     # the codec really is exercised
        ft = futil.read_footer(p)
        kinds = {n["comp_type"] for st in ft["stripes"] for n in st["nodes"][2]
                 if n["n_present"] > 1 and n["row_count"] == CHUNK and n["min_i"] != n["max_i"]}
        assert kinds == {CODECS[request.param]}
    return p


@pytest.fixture(scope="module")
def none_path(tab, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("vtn") / "none.cs")
    tab.write(p, ca.COMP_NONE)
    return p


def mask_of(tab, preds):
    """Python CNF over (col, op, const[, or_group]) on cols 0, 1, 2"""
    cols = {0: tab.ids, 2: tab.t}
    ok = np.ones(N, dtype=bool)
    groups = {}
    for i, p in enumerate(preds):
        groups.setdefault(p[3] if len(p) > 3 and p[3] else -1 - i, []).append(p)
    for members in groups.values():
        g = np.zeros(N, dtype=bool)
        for c, op, k, *_ in members:
            if c == 1:
                g |= np.array([not tab.val_null[i] and vtutil.py_pred(op, int(tab.val[i]), k)
                               for i in range(N)])
            else:
                g |= np.array([vtutil.py_pred(op, cols[c][i] if c == 2 else int(cols[c][i]), k)
                               for i in range(N)])
        ok &= g
    return ok


def expect_aggs(tab, rows):
    """[(count,), (i128 or None, contributing), (count,)] for AGGS over rows"""
    live = [i for i in rows if not tab.val_null[i]]
    return (len(rows), (sum(int(tab.val[i]) for i in live), len(live)),
            sum(tab.t[i] is not None for i in rows))


def check_partials(parts, exp):
    cnt, (sm, contributing), cc = exp
    assert (parts[0].count, parts[0].is_null) == (cnt, 0)
    assert parts[1].is_null == (1 if contributing == 0 else 0)
    if contributing:
        assert parts[1].i128 == sm and parts[1].count == contributing
    assert (parts[2].count, parts[2].is_null) == (cc, 0)


def expect_groups(tab, rows, with_m):
    """sorted [(key tuple, expect_aggs)]: text ascending by memcmp, NULL last"""
    groups = {}
    for i in rows:
        key = (tab.t[i],) + ((int(tab.m[i]),) if with_m else ())
        groups.setdefault(key, []).append(i)
    order = sorted(groups, key=lambda k: ((k[0] is None, k[0] or b""),) + k[1:])
    return [(k, expect_aggs(tab, groups[k])) for k in order]


def check_groups(res, exp, with_m):
    assert res["n_groups"] == len(exp)
    for g, (key, e) in enumerate(exp):
        assert res["text_keys"][0][g] == key[0], g
        assert res["key_nulls"][0][g] == (1 if key[0] is None else 0)
        if with_m:
            assert res["keys"][1][g] == key[1] and res["key_nulls"][1][g] == 0
        p = res["partials"][g]
        cnt, (sm, contributing), cc = e
        assert (p[0]["count"], p[0]["is_null"]) == (cnt, 0)
        assert p[1]["is_null"] == (1 if contributing == 0 else 0)
        if contributing:
            assert ca.partial_i128(p[1]) == sm and p[1]["count"] == contributing
        assert (p[2]["count"], p[2]["is_null"]) == (cc, 0)


def test_dictionary_and_round_trip(tab, path):
    with ca.Reader(path) as r, r.scan(cols_mask=0b01101) as s:
        s.stage(0)
        assert s.text_dict(2) == tab.dict_t
        assert s.text_dict(3) == sorted(tab.u)
        rows = s.select(decode_text=True)
        assert rows["n_rows"] == N
        assert np.array_equal(rows["row_numbers"], tab.ids)
        assert np.array_equal(rows["values"][0], tab.ids)
        assert list(rows["text"][2]) == tab.t
        assert list(rows["text"][3]) == tab.u
        assert rows["values"][2].dtype == np.int32
        want_nulls = np.array([v is None for v in tab.t], dtype=np.uint8)
        assert np.array_equal(rows["nulls"][2], want_nulls)
        assert not rows["values"][2][want_nulls == 1].any()       # NULL gives 0
        assert all(math.isfinite(x) and x >= 0 for x in s.last_text_ms())
        with pytest.raises(ca.CStripeError, match="rc=-5"):
            s.text_dict(0)


def test_six_operators(tab, path):
    between = POOL[10] + b"\x01"
    assert between not in POOL and POOL[10] < between < POOL[11]
    consts = [b"TRUCK", between, b"\x01", b"\xff\xff", b"", b"ab", V127]
    assert consts[2] < POOL[1] and consts[3] > POOL[-1]
    with ca.Reader(path) as r:
        for c in consts:
            for op in OPS:
                want = np.flatnonzero(mask_of(tab, [(2, op, c)]))
                with r.scan(cols_mask=1, preds=[(2, op, c)]) as s:
                    s.stage(0)
                    rows = s.select(cols=[0], want_nulls=False)
                assert np.array_equal(rows["row_numbers"], want), (op, c)
                assert np.array_equal(rows["values"][0], want), (op, c)


def test_cnf_in_list_and_integer_range(tab, path):
    preds = [(2, ca.PRED_EQ, b"AIR", 1), (2, ca.PRED_EQ, b"abc", 1), (2, ca.PRED_EQ, V127, 1),
             (2, ca.PRED_EQ, b"no such value", 1),
             (0, ca.PRED_GE, 500), (0, ca.PRED_LT, 4600)]
    want = [int(i) for i in np.flatnonzero(mask_of(tab, preds))]
    assert 50 < len(want) < 1000
    with ca.Reader(path) as r, r.scan(cols_mask=0b110, preds=preds) as s:
        s.stage(0)
        check_partials(s.agg(AGGS), expect_aggs(tab, want))
    # text range AND text inequality AND a nullable integer column
    preds = [(2, ca.PRED_GE, b"SHIP"), (2, ca.PRED_NE, b"ab"), (1, ca.PRED_GT, 0)]
    want = [int(i) for i in np.flatnonzero(mask_of(tab, preds))]
    assert len(want) > 100
    with ca.Reader(path) as r, r.scan(cols_mask=0b110, preds=preds) as s:
        s.stage(0)
        check_partials(s.agg(AGGS), expect_aggs(tab, want))


@pytest.mark.parametrize("lds", [None, "0"])
def test_agg_hashed_group_by_text(tab, path, monkeypatch, lds):
    if lds is None:
        monkeypatch.delenv("CSTRIPE_HASH_LDS_SLOTS", raising=False)
    else:
        monkeypatch.setenv("CSTRIPE_HASH_LDS_SLOTS", lds)
    with ca.Reader(path) as r, r.scan(cols_mask=0b10110) as s:
        s.stage(0)
        res = s.agg_hashed(AGGS, [2], 64, decode_text=True)
        check_groups(res, expect_groups(tab, range(N), False), False)
        assert res["n_groups"] == len(POOL) + 1 and res["text_keys"][0][-1] is None
        # keys are the ranks: ascending, so group order is memcmp order
        assert list(res["keys"][0][:-1]) == list(range(len(POOL)))
        res = s.agg_hashed(AGGS, [2, 4], 256, decode_text=True)
        check_groups(res, expect_groups(tab, range(N), True), True)
    preds = [(2, ca.PRED_LT, b"b"), (0, ca.PRED_GE, 100)]
    want = [int(i) for i in np.flatnonzero(mask_of(tab, preds))]
    with ca.Reader(path) as r, r.scan(cols_mask=0b10110, preds=preds) as s:
        s.stage(0)
        res = s.agg_hashed(AGGS, [2, 4], 256, decode_text=True)
        check_groups(res, expect_groups(tab, want, True), True)


def test_twin_differential(tab, path, tmp_path):
    """the same table with col 2 stored as its ranks in an I32 column: select
    and agg_hashed under the translated integer predicates are identical"""
    twin = str(tmp_path / "twin.cs")
    ranks = np.array([tab.rank(v) or 0 for v in tab.t], dtype=np.int32)
    ca.write_table(twin, TWIN_DEFS, [tab.ids, tab.val, ranks, list(tab.u), tab.m],
                   nulls=[None, tab.val_null,
                          np.array([v is None for v in tab.t], dtype=np.uint8), None, None],
                   chunk_group_row_limit=CHUNK, stripe_row_limit=STRIPE,
                   compression=ca.COMP_LZ4)
    d = tab.dict_t

    def translate(op, c):
        lb, ub = bisect.bisect_left(d, c), bisect.bisect_right(d, c)
        return {ca.PRED_EQ: (ca.PRED_EQ, lb if lb != ub else -1),
                ca.PRED_NE: (ca.PRED_NE, lb if lb != ub else -1),
                ca.PRED_LT: (ca.PRED_LT, lb), ca.PRED_LE: (ca.PRED_LT, ub),
                ca.PRED_GE: (ca.PRED_GT, lb - 1), ca.PRED_GT: (ca.PRED_GT, ub - 1)}[op]

    cases = [[], [(2, ca.PRED_GE, b"MAIL"), (0, ca.PRED_LT, 4500)],
             [(2, ca.PRED_EQ, b"abc", 1), (2, ca.PRED_GT, b"prefix7A", 1)],
             [(2, ca.PRED_NE, b"missing")], [(2, ca.PRED_LE, b"ab"), (1, ca.PRED_LT, 0)]]
    with ca.Reader(path) as rt, ca.Reader(twin) as ri:
        for preds in cases:
            ipreds = [(p[0],) + translate(p[1], p[2]) + tuple(p[3:]) if p[0] == 2 else p
                      for p in preds]
            with rt.scan(cols_mask=0b10111, preds=preds) as st, \
                    ri.scan(cols_mask=0b10111, preds=ipreds) as si:
                st.stage(0)
                si.stage(0)
                # every value lives in a surviving chunk group here, so the
                # scan's dictionary is the table's and ranks line up
                assert st.text_dict(2) == d
                a, b = st.select(cols=[0, 1, 2, 4]), si.select(cols=[0, 1, 2, 4])
                assert a["n_rows"] == b["n_rows"]
                assert np.array_equal(a["row_numbers"], b["row_numbers"])
                for c in (0, 1, 2, 4):
                    assert a["values"][c].dtype == b["values"][c].dtype
                    assert np.array_equal(a["values"][c], b["values"][c]), (preds, c)
                    assert np.array_equal(a["nulls"][c], b["nulls"][c]), (preds, c)
                a, b = st.agg_hashed(AGGS, [2, 4], 256), si.agg_hashed(AGGS, [2, 4], 256)
                assert a["n_groups"] == b["n_groups"]
                for k in range(2):
                    assert np.array_equal(a["keys"][k], b["keys"][k])
                    assert np.array_equal(a["key_nulls"][k], b["key_nulls"][k])
                assert a["partials"].tobytes() == b["partials"].tobytes()


def test_pruned_scan_dictionary_covers_selected_chunks(tab, tmp_path):
    order = sorted(range(N), key=lambda i: (tab.t[i] is None, tab.t[i] or b"", i))
    t = [tab.t[i] for i in order]
    p = str(tmp_path / "sorted.cs")
    ca.write_table(p, DEFS, [tab.ids, tab.val[order], t, [tab.u[i] for i in order], tab.m],
                   nulls=[None, tab.val_null[order], None, None, None],
                   chunk_group_row_limit=CHUNK, stripe_row_limit=STRIPE,
                   compression=ca.COMP_LZ4)
    bounds = []
    for lo in range(0, N, CHUNK):
        present = [v for v in t[lo:lo + CHUNK] if v is not None]
        bounds.append((vtutil.prefix_key(min(present)), vtutil.prefix_key(max(present)))
                      if present else None)
    mid = t[2 * CHUNK + CHUNK // 2]
    assert mid is not None

    def survivors(preds):
        return [k for k, b in enumerate(bounds)
                if b is None or not any(vtutil.refuted(op, c, *b) for _, op, c in preds)]

    def rows_where(keep, fn):
        return np.array([i for k in keep for i in range(k * CHUNK, (k + 1) * CHUNK)
                         if t[i] is not None and fn(t[i])], dtype=np.int64)

    with ca.Reader(p) as r:
        preds = [(2, ca.PRED_EQ, mid)]
        keep = survivors(preds)
        assert 0 < len(keep) < 5
        with r.scan(cols_mask=1, preds=preds) as s:
            assert s.chunk_groups_filtered == 5 - len(keep)
            s.stage(0)
            sel = sorted({v for k in keep for v in t[k * CHUNK:(k + 1) * CHUNK] if v is not None})
            assert s.text_dict(2) == sel and len(sel) < len(tab.dict_t)
            rows = s.select(cols=[0], want_nulls=False)
            assert np.array_equal(rows["row_numbers"], rows_where(keep, lambda v: v == mid))
            assert rows["n_rows"] == tab.t.count(mid)
        # a constant living only in pruned chunks behaves as absent
        gone = t[0]
        preds = [(2, ca.PRED_GE, mid), (2, ca.PRED_NE, gone)]
        keep = survivors(preds[:1])
        assert 0 not in keep
        with r.scan(cols_mask=1, preds=preds) as s:
            assert s.chunk_groups_filtered == 5 - len(keep)
            s.stage(0)
            assert gone not in s.text_dict(2)
            rows = s.select(cols=[0], want_nulls=False)
            assert np.array_equal(rows["row_numbers"], rows_where(keep, lambda v: v >= mid))
        with r.scan(cols_mask=1, preds=[(2, ca.PRED_GE, mid), (2, ca.PRED_EQ, gone)]) as s:
            s.stage(0)
            assert s.select_count() == 0


def test_distinct_capacity(tab, none_path, monkeypatch):
    with ca.Reader(none_path) as r:
        monkeypatch.setenv("CSTRIPE_VARTEXT_MAX_DISTINCT", "64")
        with r.scan(cols_mask=0b1001) as s:
            with pytest.raises(ca.CStripeError, match=r"rc=-5.*column 3 .*\b64\b"):
                s.stage(0)
            with pytest.raises(ca.CStripeError, match="rc=-4"):      # left unstaged
                s.agg([(ca.AGG_COUNT_STAR, -1)])
        with r.scan(cols_mask=0b0110) as s:                          # 40 distinct fit
            s.stage(0)
            assert s.text_dict(2) == tab.dict_t
            check_partials(s.agg(AGGS), expect_aggs(tab, list(range(N))))
        # exactly full: 5000 distinct values under a limit of 5000
        monkeypatch.setenv("CSTRIPE_VARTEXT_MAX_DISTINCT", "5000")
        with r.scan(cols_mask=0b1001) as s:
            s.stage(0)
            assert s.text_dict(3) == sorted(tab.u)
            rows = s.select(cols=[3], decode_text=True)
            assert list(rows["text"][3]) == tab.u
        monkeypatch.setenv("CSTRIPE_VARTEXT_MAX_DISTINCT", "4999")
        with r.scan(cols_mask=0b1001) as s:
            with pytest.raises(ca.CStripeError, match=r"rc=-5.*column 3 .*\b4999\b"):
                s.stage(0)


def test_reinvocation_is_stable(tab, path):
    preds = [(2, ca.PRED_GT, b"FOB"), (2, ca.PRED_NE, ONLY)]
    want = [int(i) for i in np.flatnonzero(mask_of(tab, preds))]
    with ca.Reader(path) as r, r.scan(cols_mask=0b10111, preds=preds) as s:
        s.stage(0)
        first = None
        for _ in range(2):
            a = [(p.i128, p.count, p.is_null) for p in s.agg(AGGS)]
            rows = s.select(cols=[0, 2])
            h = s.agg_hashed(AGGS, [2], 64)
            got = (a, rows["row_numbers"].tobytes(), rows["values"][2].tobytes(),
                   h["keys"][0].tobytes(), h["partials"].tobytes())
            if first is None:
                first = got
                check_partials(s.agg(AGGS), expect_aggs(tab, want))
                assert list(rows["row_numbers"]) == want
            assert got == first
        ms = s.last_text_ms()
        assert len(ms) == 4 and all(math.isfinite(x) and x >= 0 for x in ms)
        s.stage(0)                                                  # restage rebuilds
        assert [(p.i128, p.count, p.is_null) for p in s.agg(AGGS)] == first[0]


def test_errors(tab, none_path, tmp_path):
    with ca.Reader(none_path) as r, r.scan(cols_mask=0b10111) as s:
        s.stage(0)
        for kind in (ca.AGG_SUM_I64, ca.AGG_MIN_I64, ca.AGG_MAX_I64, ca.AGG_SUM_F64):
            with pytest.raises(ca.CStripeError, match="rc=-5.*VARTEXT"):
                s.agg([(kind, 2)])
        with pytest.raises(ca.CStripeError, match="rc=-5.*VARTEXT"):
            s.agg([(ca.AGG_SUM_PROD_I64, 1, 2)])
        with pytest.raises(ca.CStripeError, match="rc=-5.*VARTEXT"):
            s.agg_hashed([(ca.AGG_SUM_I64, 2)], [4], 8)
        with pytest.raises(ca.CStripeError, match="rc=-5"):
            s.agg_grouped([(ca.AGG_COUNT_STAR, -1)], [2])
        ids = np.zeros(CHUNK, dtype=np.int64)
        txt = np.zeros(CHUNK, dtype=np.int32)
        with pytest.raises(ca.CStripeError, match="rc=-5.*VARTEXT"):
            s.next_batch({0: ids, 2: txt})
        s.rewind()
        got = []
        while True:
            nb = s.next_batch({0: ids})
            if nb is None:
                break
            got.extend(ids[:nb[0]].tolist())
        assert got == list(range(N))
        row = s.read_row(1234)                      # the other columns still read
        assert row[0] == 1234 and 2 not in row and row[4] == 1234 % 3
        vp = (ca.C.c_void_p * 5)()
        vp[2] = txt.ctypes.data
        assert ca._read_row(s._h, 0, vp, None) == ca.ERR_ARG
    with pytest.raises(ca.CStripeError, match="rc=-5.*VARTEXT"):
        ca.write_table_device(str(tmp_path / "dev.cs"), DEFS, [0] * 5, 10)


def test_two_shard_directory(tab, tmp_path):
    d = tmp_path / "shards"
    d.mkdir()
    tab.write(str(d / "shard00.cs"), ca.COMP_LZ4, slice(0, 3000))
    tab.write(str(d / "shard01.cs"), ca.COMP_ZSTD, slice(3000, N))
    preds = [(2, ca.PRED_GE, b"SHIP")]
    want = np.flatnonzero(mask_of(tab, preds))
    with ca.Reader(str(d)) as r:
        with r.scan(cols_mask=0b01111) as s:
            s.stage(0)
            assert s.text_dict(2) == tab.dict_t          # spans both files
            assert s.text_dict(3) == sorted(tab.u)
            rows = s.select(cols=[0, 2], decode_text=True)
            assert list(rows["text"][2]) == tab.t
            assert np.array_equal(rows["values"][0], tab.ids)
            res = s.agg_hashed(AGGS, [2], 64, decode_text=True)
            check_groups(res, expect_groups(tab, range(N), False), False)
        with r.scan(cols_mask=0b0111, preds=preds) as s:
            s.stage(0)
            rows = s.select(cols=[0], want_nulls=False)
            assert np.array_equal(rows["row_numbers"], want)
            check_partials(s.agg(AGGS), expect_aggs(tab, [int(i) for i in want]))


def test_malformed_stream_is_a_format_error(tab, none_path, tmp_path):
    """the last datum of one chunk claims 8 bytes more than the stream holds:
    the walk is bounded by decompressed_size, so stage reports it"""
    bad = str(tmp_path / "bad.cs")
    shutil.copy(none_path, bad)
    # chunk 0 or 1 of stripe 0, whichever ends in a datum whose header can
    # claim 8 more bytes in the same header form
    k, last = next((k, v) for k in (1, 0)
                   for v in [next(v for v in reversed(tab.t[k * CHUNK:(k + 1) * CHUNK])
                                  if v is not None)]
                   if not 118 <= len(v) <= 126)
    node = futil.read_footer(bad)["stripes"][0]["nodes"][2][k]
    datum = vtutil.ser_datum(last)
    pos = node["file_offset"] + node["value_off"] + node["value_len"] - len(datum)
    with open(bad, "r+b") as f:
        f.seek(pos)
        hdr = f.read(4)
        assert hdr == datum[:4]
        f.seek(pos)
        if hdr[0] & 1:
            total = (hdr[0] >> 1) + 8
            assert total <= 127
            f.write(bytes([(total << 1) | 1]))
        else:
            f.write((((int.from_bytes(hdr, "little") >> 2) + 8) << 2).to_bytes(4, "little"))
    with ca.Reader(bad) as r, r.scan(cols_mask=0b100) as s:
        with pytest.raises(ca.CStripeError, match="rc=-3"):
            s.stage(0)
    with ca.Reader(bad) as r, r.scan(cols_mask=0b001) as s:         # other columns are fine
        s.stage(0)
        assert s.agg([(ca.AGG_COUNT_STAR, -1)])[0].count == N
