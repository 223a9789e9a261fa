"""
Set-membership predicates (CSTRIPE_PRED_IN / CSTRIPE_PRED_NOT_IN,
cstripe_scan_begin_sets, include/cstripe.h) — everything that needs no GPU:
the exported symbols and the C layout of cstripe_value_set, the begin-time
argument errors, and host chunk refutation. Expected removal counts are
computed here from the chunk bounds of the arrays the test wrote.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import citus_amd as ca
import vtutil

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------ symbols / layout
def test_symbols_and_constants():
    lib = C.CDLL(os.path.join(REPO, "citus_amd", "libcstripe.so"))
    for name in ("cstripe_scan_begin_sets", "cstripe_scan_last_set_ms",
                 "cstripe_scan_set_form"):
        assert hasattr(lib, name), name
    assert (ca.PRED_IN, ca.PRED_NOT_IN) == (6, 7)
    assert ca.MAX_SETS == 4 and ca.MAX_SET_VALUES == 1 << 26
    assert hasattr(ca.Scan, "last_set_ms") and hasattr(ca.Scan, "set_form")
    lib.cstripe_abi_version.restype = C.c_uint32
    assert lib.cstripe_abi_version() == 2        # additive: the version stays


def test_value_set_struct_matches_c_layout(tmp_path):
    assert C.sizeof(ca.ValueSet) == 32
    src = tmp_path / "sz.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "cstripe.h"\n'
        'int main(void) { printf("%zu %zu %zu %zu %zu %d %d %d %llu\\n",\n'
        '  sizeof(cstripe_value_set), offsetof(cstripe_value_set, values),\n'
        '  offsetof(cstripe_value_set, texts), offsetof(cstripe_value_set, n),\n'
        '  offsetof(cstripe_value_set, on_device), (int)CSTRIPE_PRED_IN,\n'
        '  (int)CSTRIPE_PRED_NOT_IN, (int)CSTRIPE_MAX_SETS,\n'
        '  (unsigned long long)CSTRIPE_MAX_SET_VALUES);\n'
        '  return 0; }\n')
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c11", str(src),
                           "-I" + os.path.join(REPO, "include"), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    assert got == [32, ca.ValueSet.values.offset, ca.ValueSet.texts.offset,
                   ca.ValueSet.n.offset, ca.ValueSet.on_device.offset,
                   6, 7, 4, 1 << 26]


# ------------------------------------------------------------ begin-time errors
DEFS = [("a", ca.I64, 0), ("f", ca.F64, 0), ("t", ca.VARTEXT, 0), ("c", ca.TEXT, 0),
        ("g", ca.F32, 0)]


@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("setpred") / "mixed.cs")
    ca.write_table(p, DEFS, [np.arange(4, dtype=np.int64),
                             np.arange(4, dtype=np.float64),
                             [b"a", b"b", b"c", b"d"],
                             ca.text_slots(["A", "B", "C", "D"]).view(np.int32),
                             np.arange(4, dtype=np.float32)],
                   compression=ca.COMP_NONE)
    return p


def int_set(vals):
    a = np.ascontiguousarray(vals, dtype=np.int64)
    vs = ca.ValueSet()
    vs.values = a.ctypes.data_as(C.c_void_p).value
    vs.n = len(a)
    vs._keep = a
    return vs


def text_set(strs):
    ta = (ca.TextConst * max(1, len(strs)))()
    for i, b in enumerate(strs):
        ta[i].data, ta[i].len = b, len(b)
    vs = ca.ValueSet()
    vs.texts = ta
    vs.n = len(strs)
    vs._keep = (ta, strs)
    return vs


def begin_sets(r, preds, sets):
    arr = ca.make_preds(preds)
    sa = (ca.ValueSet * max(1, len(sets)))(*sets)
    return ca._scan_begin_sets(r._h, 0, arr, len(preds), None, 0, sa, len(sets))


def test_begin_errors(mixed):
    with ca.Reader(mixed) as r:
        ok = begin_sets(r, [(0, ca.PRED_IN, 0)], [int_set([1, 2])])
        assert ok
        ca._scan_end(ok)
        # a set index >= n_sets (and a negative one)
        for idx in (1, 4, -1):
            assert not begin_sets(r, [(0, ca.PRED_IN, idx)], [int_set([1])])
            assert "cstripe_scan_begin_sets" in ca.errmsg()
        # more than CSTRIPE_MAX_SETS sets
        assert not begin_sets(r, [(0, ca.PRED_IN, 0)], [int_set([1])] * 5)
        assert "sets" in ca.errmsg()
        # n above CSTRIPE_MAX_SET_VALUES (rejected before the values are read)
        big = int_set([1])
        big.n = (1 << 26) + 1
        assert not begin_sets(r, [(0, ca.PRED_IN, 0)], [big])
        assert "max" in ca.errmsg()
        # texts on a non-VARTEXT column, values on a VARTEXT column
        assert not begin_sets(r, [(0, ca.PRED_IN, 0)], [text_set([b"a"])])
        assert "VARTEXT" in ca.errmsg()
        assert not begin_sets(r, [(3, ca.PRED_NOT_IN, 0)], [text_set([b"a"])])
        assert not begin_sets(r, [(2, ca.PRED_IN, 0)], [int_set([1])])
        assert "VARTEXT" in ca.errmsg()
        # float key columns
        for col in (1, 4):
            assert not begin_sets(r, [(col, ca.PRED_IN, 0)], [int_set([1])])
            assert "float" in ca.errmsg()
        # an op above 7
        assert not begin_sets(r, [(0, 8, 0)], [int_set([1])])
        assert "op" in ca.errmsg()
        # the right shapes on the text columns begin fine
        for preds, sets in (([(2, ca.PRED_IN, 0)], [text_set([b"a", b"zz"])]),
                            ([(3, ca.PRED_NOT_IN, 0)], [int_set(ca.text_slots(["A"]))]),
                            ([(2, ca.PRED_IN, 0), (0, ca.PRED_NOT_IN, 1)],
                             [text_set([]), int_set([])])):
            h = begin_sets(r, preds, sets)
            assert h, ca.errmsg()
            ca._scan_end(h)


def test_plain_begin_rejects_set_ops(mixed):
    with ca.Reader(mixed) as r:
        for op in (ca.PRED_IN, ca.PRED_NOT_IN):
            arr = ca.make_preds([(0, op, 0)])
            assert not ca._scan_begin(r._h, 0, arr, 1)
            assert "cstripe_scan_begin_sets" in ca.errmsg()
            assert not ca._scan_begin_ex(r._h, 0, arr, 1, None, 0)
            assert "cstripe_scan_begin_sets" in ca.errmsg()
        # with no sets the new entry is scan_begin_ex
        arr = ca.make_preds([(0, ca.PRED_GE, 2)])
        h = ca._scan_begin_sets(r._h, 0, arr, 1, None, 0, None, 0)
        assert h
        assert ca._filtered(h) == 0
        ca._scan_end(h)


def test_set_form_is_none_before_stage(mixed):
    with ca.Reader(mixed) as r, r.scan(preds=[(0, ca.PRED_IN, [1, 2, 3])]) as s:
        assert s.set_form(0) == (ca.SET_FORM_NONE, 0)
        assert s.last_set_ms() == (0.0, 0.0)
        with pytest.raises(ca.CStripeError):
            s.set_form(1)


# ------------------------------------------------------------ pruning
N_A, CHUNK = 20000, 1000


@pytest.fixture(scope="module")
def pushdown(tmp_path_factory):
    """the reference's pushdown_test shape: a = 1..20000, stripes of 2000
    rows in chunk groups of 1000"""
    p = str(tmp_path_factory.mktemp("setpred") / "push.cs")
    a = np.arange(1, N_A + 1, dtype=np.int64)
    ca.write_table(p, [("a", ca.I64, 0), ("b", ca.I64, 0)], [a, a * 2],
                   stripe_row_limit=2000, chunk_group_row_limit=CHUNK)
    bounds = [(int(a[i]), int(a[min(i + CHUNK, N_A) - 1])) for i in range(0, N_A, CHUNK)]
    return p, bounds


def refuted_in(values, bounds):
    return sum(not any(mn <= v <= mx for v in values) for mn, mx in bounds)


def test_in_prunes_by_elements(pushdown):
    p, bounds = pushdown
    assert len(bounds) == 20
    with ca.Reader(p) as r:
        S = [5, 1500, 19999]
        want = refuted_in(S, bounds)
        assert want == 17
        with r.scan(preds=[(0, ca.PRED_IN, S)]) as s:
            assert s.chunk_groups_filtered == want
        # 17 elements: more than an OR group of EQ atoms can hold. Unsorted,
        # with a duplicate and elements outside every chunk
        S17 = [15500, 3, 2001, 2001, 9999, 10000, 10001, -7, 30000, 4000, 4001,
               12345, 12346, 19000, 7, 8, 6500]
        assert len(S17) == 17
        want = refuted_in(S17, bounds)
        assert 0 < want < 20
        with r.scan(preds=[(0, ca.PRED_IN, np.array(S17))]) as s:
            assert s.chunk_groups_filtered == want
        # the empty set refutes every chunk that has min/max
        with r.scan(preds=[(0, ca.PRED_IN, [])]) as s:
            assert s.chunk_groups_filtered == 20
        # NOT IN never refutes, whatever the set
        for S in ([], [5], list(range(1, 1001))):
            with r.scan(preds=[(0, ca.PRED_NOT_IN, S)]) as s:
                assert s.chunk_groups_filtered == 0
        # in an OR group with a range atom a chunk goes only when both refute
        S = [5, 1500]
        g = 3
        want = sum(not any(mn <= v <= mx for v in S) and not mx > 18000
                   for mn, mx in bounds)
        assert want == 16
        with r.scan(preds=[(0, ca.PRED_IN, S, g), (0, ca.PRED_GT, 18000, g)]) as s:
            assert s.chunk_groups_filtered == want
        # ANDed with a second set predicate on another column: counted once
        T = [10, 3000, 39998]                       # b = 2a
        want = sum(not any(mn <= v <= mx for v in [5, 1500, 19999]) or
                   not any(2 * mn <= v <= 2 * mx for v in T) for mn, mx in bounds)
        with r.scan(preds=[(0, ca.PRED_IN, [5, 1500, 19999]), (1, ca.PRED_IN, T)]) as s:
            assert s.chunk_groups_filtered == want


def test_all_null_chunk_survives(tmp_path):
    p = str(tmp_path / "n.cs")
    a = np.arange(6, dtype=np.int64)
    nulls = np.array([0, 0, 1, 1, 0, 0], dtype=np.uint8)
    ca.write_table(p, [("a", ca.I64, 0)], [a], nulls=[nulls],
                   chunk_group_row_limit=2, stripe_row_limit=6, compression=ca.COMP_NONE)
    with ca.Reader(p) as r:
        with r.scan(preds=[(0, ca.PRED_IN, [100])]) as s:
            assert s.chunk_groups_filtered == 2          # the all-NULL chunk stays
        with r.scan(preds=[(0, ca.PRED_IN, [])]) as s:
            assert s.chunk_groups_filtered == 2


def test_text_reference_fixture(tmp_path):
    """the reference's own IN-list pushdown test
    (columnar_chunk_filtering.out:1085-1121): 8 rows in two-row chunk groups,
    country IN ('USA','BR','ZW') removes the groups {AL,AU} and {PK,PA} —
    the same count the OR group of three EQ atoms gives"""
    ids = np.arange(1, 9, dtype=np.int64)
    countries = ["AL", "AU", "BR", "BT", "PK", "PA", "USA", "ZW"]
    p = str(tmp_path / "push.cs")
    ca.write_table(p, [("id", ca.I64, 0), ("country", ca.TEXT, 0)],
                   [ids, ca.text_slots(countries).view(np.int32)],
                   compression=ca.COMP_LZ4, stripe_row_limit=2, chunk_group_row_limit=2)
    S = ["USA", "BR", "ZW"]
    eq = [(1, ca.PRED_EQ, int(ca.text_slot(c)), 42) for c in S]
    with ca.Reader(p) as r:
        with r.scan(cols_mask=0b11, preds=eq) as s:
            by_eq = s.chunk_groups_filtered
        with r.scan(cols_mask=0b11, preds=[(1, ca.PRED_IN, ca.text_slots(S))]) as s:
            assert s.chunk_groups_filtered == by_eq == 2
        with r.scan(cols_mask=0b11, preds=[(1, ca.PRED_NOT_IN, ca.text_slots(S))]) as s:
            assert s.chunk_groups_filtered == 0


SORTED = [b"", b"a", b"ab", b"abc",
          b"b", b"c", b"mmmmmmm", b"mmmmmmm1",
          b"mmmmmmm3", b"n", b"o", b"p",
          b"q", b"r", b"s", b"t"]


def test_vartext_prefix_keys_keep_boundary_chunks(tmp_path):
    """chunk 1 ends on "mmmmmmm1" and chunk 2 starts on "mmmmmmm3": an element
    sharing that 7-byte prefix keeps both, although neither holds it"""
    assert SORTED == sorted(SORTED)
    p = str(tmp_path / "v.cs")
    ca.write_table(p, [("id", ca.I64, 0), ("t", ca.VARTEXT, 0)],
                   [np.arange(16, dtype=np.int64), list(SORTED)],
                   chunk_group_row_limit=4, stripe_row_limit=8, compression=ca.COMP_NONE)
    bounds = [(vtutil.prefix_key(SORTED[i]), vtutil.prefix_key(SORTED[i + 3]))
              for i in range(0, 16, 4)]

    def want(S):
        keys = [vtutil.prefix_key(x) for x in S]
        return sum(not any(mn <= k <= mx for k in keys) for mn, mx in bounds)

    with ca.Reader(p) as r:
        for S in ([b"mmmmmmm2"], [b"mmmmmmm9", b"zzz"], [b"ab", b"t"], [b"bb"],
                  [b"zzz"], [b"a", "n", b"q"]):
            Sb = [x.encode() if isinstance(x, str) else x for x in S]
            with r.scan(preds=[(1, ca.PRED_IN, S)]) as s:
                assert s.chunk_groups_filtered == want(Sb), S
            with r.scan(preds=[(1, ca.PRED_NOT_IN, S)]) as s:
                assert s.chunk_groups_filtered == 0
        assert want([b"mmmmmmm2"]) == 2              # chunks 1 and 2 are kept
        with r.scan(preds=[(1, ca.PRED_IN, [])]) as s:
            assert s.chunk_groups_filtered == 4
