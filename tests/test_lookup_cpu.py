"""
Lookups (cstripe_scan_begin_lookups, include/cstripe.h) — everything that
needs no GPU: the exported symbols and the C layout of cstripe_lookup, the
begin-time argument errors, and host chunk refutation. Expected removal
counts are computed here from the chunk bounds of the arrays the test wrote.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import citus_amd as ca

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------ symbols / layout
def test_symbols_and_constants():
    lib = C.CDLL(os.path.join(REPO, "citus_amd", "libcstripe.so"))
    for name in ("cstripe_scan_begin_lookups", "cstripe_scan_column_count",
                 "cstripe_scan_last_lookup_ms", "cstripe_scan_lookup_form"):
        assert hasattr(lib, name), name
    assert (ca.MAX_LOOKUPS, ca.MAX_LOOKUP_PAYLOADS, ca.LOOKUP_INNER) == (2, 4, 1)
    assert (ca.LOOKUP_FORM_NONE, ca.LOOKUP_FORM_HASH, ca.LOOKUP_FORM_DIRECT) == (0, 1, 2)
    for name in ("column_count", "derived", "last_lookup_ms", "lookup_form"):
        assert hasattr(ca.Scan, name), name
    lib.cstripe_abi_version.restype = C.c_uint32
    assert lib.cstripe_abi_version() == 2        # additive: the version stays


def test_lookup_struct_matches_c_layout(tmp_path):
    assert C.sizeof(ca.LookupIn) == 64
    src = tmp_path / "sz.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "cstripe.h"\n'
        'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d %u\\n",\n'
        '  sizeof(cstripe_lookup), offsetof(cstripe_lookup, key_column),\n'
        '  offsetof(cstripe_lookup, n_payloads), offsetof(cstripe_lookup, keys),\n'
        '  offsetof(cstripe_lookup, payloads), offsetof(cstripe_lookup, n),\n'
        '  offsetof(cstripe_lookup, on_device), offsetof(cstripe_lookup, flags),\n'
        '  (int)CSTRIPE_MAX_LOOKUPS, (int)CSTRIPE_MAX_LOOKUP_PAYLOADS,\n'
        '  (unsigned)CSTRIPE_LOOKUP_INNER);\n'
        '  return 0; }\n')
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c11", str(src),
                           "-I" + os.path.join(REPO, "include"), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    L = ca.LookupIn
    assert got == [64, L.key_column.offset, L.n_payloads.offset, L.keys.offset,
                   L.payloads.offset, L.n.offset, L.on_device.offset, L.flags.offset,
                   2, 4, 1]


# ------------------------------------------------------------ begin-time errors
DEFS = [("a", ca.I64, 0), ("f", ca.F64, 0), ("t", ca.VARTEXT, 0), ("c", ca.TEXT, 0),
        ("g", ca.F32, 0), ("h", ca.I16, 0)]
N_TAB = len(DEFS)


@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("lookup") / "mixed.cs")
    ca.write_table(p, DEFS, [np.arange(4, dtype=np.int64),
                             np.arange(4, dtype=np.float64),
                             [b"a", b"b", b"c", b"d"],
                             ca.text_slots(["A", "B", "C", "D"]).view(np.int32),
                             np.arange(4, dtype=np.float32),
                             np.arange(4, dtype=np.int16)],
                   compression=ca.COMP_NONE)
    return p


def raw_lookup(key_col, keys, payloads, n_payloads=None, flags=0, n=None):
    lk = ca.LookupIn()
    keep = []

    def ptr(v):
        if v is None:
            return None
        a = np.ascontiguousarray(v, dtype=np.int64)
        keep.append(a)
        return a.ctypes.data_as(C.c_void_p).value
    lk.key_column = key_col
    lk.n_payloads = len(payloads) if n_payloads is None else n_payloads
    lk.keys = ptr(keys)
    for i, p in enumerate(payloads[:4]):
        lk.payloads[i] = ptr(p)
    lk.n = (len(keys) if keys is not None else 0) if n is None else n
    lk.flags = flags
    lk._keep = keep
    return lk


def begin(r, preds, lookups, sets=()):
    arr = ca.make_preds(preds)
    la = (ca.LookupIn * max(1, len(lookups)))(*lookups)
    sa = (ca.ValueSet * max(1, len(sets)))(*sets)
    return ca._scan_begin_lookups(r._h, 0, arr, len(preds), None, 0,
                                  sa if sets else None, len(sets), la, len(lookups))


def test_begin_errors(mixed):
    K, P = [1, 2, 3], [10, 20, 30]
    with ca.Reader(mixed) as r:
        h = begin(r, [], [raw_lookup(0, K, [P])])
        assert h, ca.errmsg()
        lib_cc = ca._scan_column_count(h)
        assert lib_cc == N_TAB + 1
        ca._scan_end(h)
        # an I16 key, an empty map and a predicate on the derived column begin fine
        for preds, lks in (([], [raw_lookup(5, K, [P, P])]),
                           ([], [raw_lookup(0, [], [[]])]),
                           ([(N_TAB, ca.PRED_LT, 25)], [raw_lookup(0, K, [P])]),
                           ([(N_TAB + 2, ca.PRED_EQ, 10)],
                            [raw_lookup(0, K, [P, P]), raw_lookup(5, K, [P])])):
            h = begin(r, preds, lks)
            assert h, ca.errmsg()
            ca._scan_end(h)
        # more than CSTRIPE_MAX_LOOKUPS
        assert not begin(r, [], [raw_lookup(0, K, [P])] * 3)
        assert "3 lookups" in ca.errmsg()
        # n_payloads 0 or > 4
        assert not begin(r, [], [raw_lookup(0, K, [])])
        assert "lookup 0" in ca.errmsg() and "payloads" in ca.errmsg()
        assert not begin(r, [], [raw_lookup(0, K, [P]), raw_lookup(0, K, [P] * 4, n_payloads=5)])
        assert "lookup 1" in ca.errmsg() and "payloads" in ca.errmsg()
        # a NULL array with n > 0
        assert not begin(r, [], [raw_lookup(0, None, [P], n=3)])
        assert "lookup 0" in ca.errmsg() and "keys" in ca.errmsg()
        assert not begin(r, [], [raw_lookup(0, K, [P, None])])
        assert "lookup 0" in ca.errmsg() and "payload 1" in ca.errmsg()
        # n above the limit (rejected before the arrays are read)
        assert not begin(r, [], [raw_lookup(0, K, [P], n=(1 << 26) + 1)])
        assert "lookup 0" in ca.errmsg() and "max" in ca.errmsg()
        # key column out of range / of a wrong type
        assert not begin(r, [], [raw_lookup(N_TAB, K, [P])])
        assert "lookup 0" in ca.errmsg() and "key column" in ca.errmsg()
        for col in (1, 2, 3, 4):
            assert not begin(r, [], [raw_lookup(0, K, [P]), raw_lookup(col, K, [P])])
            assert "lookup 1" in ca.errmsg() and "key column %d" % col in ca.errmsg()
        # a predicate / set naming a derived id beyond the scan's column count
        assert not begin(r, [(N_TAB + 1, ca.PRED_EQ, 1)], [raw_lookup(0, K, [P])])
        assert "predicate 0" in ca.errmsg() and "column %d" % (N_TAB + 1) in ca.errmsg()
        vs = ca.ValueSet()
        assert not begin(r, [(0, ca.PRED_EQ, 1), (N_TAB + 1, ca.PRED_IN, 0)],
                         [raw_lookup(0, K, [P])], sets=[vs])
        assert "predicate 1" in ca.errmsg()
        # IN / NOT IN on a derived column
        for op in (ca.PRED_IN, ca.PRED_NOT_IN):
            assert not begin(r, [(N_TAB, op, 0)], [raw_lookup(0, K, [P])], sets=[vs])
            assert "predicate 0" in ca.errmsg() and "derived" in ca.errmsg()
        # the INNER atom counts against CSTRIPE_MAX_PREDS
        full = [(0, ca.PRED_GE, 0)] * 16
        h = begin(r, full, [raw_lookup(0, K, [P])])
        assert h, ca.errmsg()
        ca._scan_end(h)
        assert not begin(r, full, [raw_lookup(0, K, [P], flags=ca.LOOKUP_INNER)])
        assert "INNER" in ca.errmsg()
        # duplicate build keys in a host map: the message names the key
        assert not begin(r, [], [raw_lookup(0, [5, 7, -12345, 9, -12345], [[1, 2, 3, 4, 5]])])
        assert "lookup 0" in ca.errmsg() and "-12345" in ca.errmsg()
        assert not begin(r, [], [raw_lookup(0, K, [P]), raw_lookup(5, [8, 8], [[1, 2]])])
        assert "lookup 1" in ca.errmsg() and "key 8" in ca.errmsg()


def test_unknown_flags_and_the_64_column_limit(mixed, tmp_path):
    K, P = [1, 2, 3], [10, 20, 30]
    with ca.Reader(mixed) as r:
        assert not begin(r, [], [raw_lookup(0, K, [P]), raw_lookup(0, K, [P], flags=2)])
        assert "lookup 1" in ca.errmsg() and "flags" in ca.errmsg()
    # table plus derived columns must stay <= 64
    path = str(tmp_path / "wide62.cs")
    a = np.arange(4, dtype=np.int64)
    ca.write_table(path, [(f"c{j}", ca.I64, 0) for j in range(62)], [a] * 62,
                   compression=ca.COMP_NONE)
    with ca.Reader(path) as r:
        h = begin(r, [(63, ca.PRED_EQ, 10)], [raw_lookup(0, K, [P, P])])
        assert h, ca.errmsg()
        assert ca._scan_column_count(h) == 64
        ca._scan_end(h)
        assert not begin(r, [], [raw_lookup(0, K, [P, P, P])])
        assert "lookup 0" in ca.errmsg() and "64" in ca.errmsg()
        assert not begin(r, [], [raw_lookup(0, K, [P, P]), raw_lookup(1, K, [P])])
        assert "lookup 1" in ca.errmsg() and "64" in ca.errmsg()


def test_python_lookup_surface(mixed):
    with ca.Reader(mixed) as r:
        lks = [ca.Lookup(0, [1, 2], [[10, 20], [30, 40]]), ca.Lookup(5, [3], [[7]], inner=True)]
        with r.scan(lookups=lks) as s:
            assert s.column_count() == N_TAB + 3
            assert [s.derived(0, 0), s.derived(0, 1), s.derived(1, 0)] == \
                   [N_TAB, N_TAB + 1, N_TAB + 2]
            with pytest.raises(ca.CStripeError):
                s.derived(1, 1)
            assert s.lookup_form(0) == (ca.LOOKUP_FORM_NONE, 0)
            assert s.last_lookup_ms() == (0.0, 0.0)
            with pytest.raises(ca.CStripeError):
                s.lookup_form(2)
        with r.scan() as s:
            assert s.column_count() == N_TAB
        with pytest.raises(ca.CStripeError) as ei:
            r.scan(lookups=[ca.Lookup(0, [4, 4], [[1, 2]])])
        assert "duplicate" in str(ei.value) and "4" in str(ei.value)


# ------------------------------------------------------------ pruning
N_A, CHUNK = 4096, 256


@pytest.fixture(scope="module")
def sorted_key(tmp_path_factory):
    """a sorted I64 key in 4096 rows / chunk groups of 256: k = 3 * row"""
    p = str(tmp_path_factory.mktemp("lookup") / "sorted.cs")
    k = np.arange(N_A, dtype=np.int64) * 3
    ca.write_table(p, [("k", ca.I64, 0), ("b", ca.I64, 0)], [k, k + 1],
                   stripe_row_limit=1024, chunk_group_row_limit=CHUNK)
    bounds = [(int(k[i]), int(k[i + CHUNK - 1])) for i in range(0, N_A, CHUNK)]
    return p, bounds


def refuted_in(values, bounds):
    return sum(not any(mn <= v <= mx for v in values) for mn, mx in bounds)


def test_no_lookups_is_begin_sets(sorted_key):
    p, bounds = sorted_key
    S = [5, 1500, 9000]
    want = refuted_in(S, bounds)
    assert 0 < want < 16
    with ca.Reader(p) as r:
        arr, tc, n_tc, sa, n_sets = ca.make_preds_sets([(0, ca.PRED_IN, S)])
        a = ca._scan_begin_sets(r._h, 0, arr, 1, tc, n_tc, sa, n_sets)
        b = ca._scan_begin_lookups(r._h, 0, arr, 1, tc, n_tc, sa, n_sets, None, 0)
        assert a and b
        assert ca._filtered(a) == ca._filtered(b) == want
        assert ca._scan_column_count(b) == 2
        ca._scan_end(a)
        ca._scan_end(b)


def test_refutation_counts(sorted_key):
    p, bounds = sorted_key
    assert len(bounds) == 16
    # keys in chunks 0, 5 and 15, one between two chunks, two outside the table
    K = [4, 3 * 1300 + 1, 3 * 1400, 3 * 255 + 1, 3 * 4095, -9, 10 ** 9]
    P = [k * 7 for k in K]
    want = refuted_in(K, bounds)
    assert want == 13
    D = 2                                        # the derived column's id
    with ca.Reader(p) as r:
        # the INNER flag alone
        with r.scan(lookups=[ca.Lookup(0, K, [P], inner=True)]) as s:
            assert s.chunk_groups_filtered == want
        # a standalone EQ on the derived column refutes the same chunks
        with r.scan(preds=[(D, ca.PRED_EQ, 28)], lookups=[ca.Lookup(0, K, [P])]) as s:
            assert s.chunk_groups_filtered == want
        # an or_group of two atoms on derived columns of one lookup too
        with r.scan(preds=[(D, ca.PRED_EQ, 28, 5), (D + 1, ca.PRED_LT, 0, 5)],
                    lookups=[ca.Lookup(0, K, [P, P])]) as s:
            assert s.chunk_groups_filtered == want
        # inside an or_group with a table-column atom it never refutes
        # (b < 0 alone would refute every chunk)
        with r.scan(preds=[(D, ca.PRED_EQ, 28, 5), (1, ca.PRED_LT, 0, 5)],
                    lookups=[ca.Lookup(0, K, [P])]) as s:
            assert s.chunk_groups_filtered == 0
        with r.scan(preds=[(1, ca.PRED_LT, 0)], lookups=[ca.Lookup(0, K, [P])]) as s:
            assert s.chunk_groups_filtered == 16
        # nor in an or_group over derived columns of two lookups
        with r.scan(preds=[(D, ca.PRED_EQ, 28, 5), (D + 1, ca.PRED_EQ, 28, 5)],
                    lookups=[ca.Lookup(0, K, [P]), ca.Lookup(1, K, [P])]) as s:
            assert s.chunk_groups_filtered == 0
        # a non-INNER lookup with no derived predicate refutes none
        with r.scan(lookups=[ca.Lookup(0, K, [P])]) as s:
            assert s.chunk_groups_filtered == 0
        # n = 0 with INNER removes every chunk that has min/max
        with r.scan(lookups=[ca.Lookup(0, [], [[]], inner=True)]) as s:
            assert s.chunk_groups_filtered == 16
        # ANDed with a table predicate: a removed chunk is counted once
        want2 = sum(not any(mn <= v <= mx for v in K) or not mx >= 3 * 1300
                    for mn, mx in bounds)
        with r.scan(preds=[(0, ca.PRED_GE, 3 * 1300)],
                    lookups=[ca.Lookup(0, K, [P], inner=True)]) as s:
            assert s.chunk_groups_filtered == want2


def test_all_null_chunk_survives(tmp_path):
    p = str(tmp_path / "n.cs")
    a = np.arange(6, dtype=np.int64)
    nulls = np.array([0, 0, 1, 1, 0, 0], dtype=np.uint8)
    ca.write_table(p, [("a", ca.I64, 0)], [a], nulls=[nulls],
                   chunk_group_row_limit=2, stripe_row_limit=6, compression=ca.COMP_NONE)
    with ca.Reader(p) as r:
        with r.scan(lookups=[ca.Lookup(0, [100], [[1]], inner=True)]) as s:
            assert s.chunk_groups_filtered == 2          # the all-NULL chunk stays
        with r.scan(lookups=[ca.Lookup(0, [], [[]], inner=True)]) as s:
            assert s.chunk_groups_filtered == 2
