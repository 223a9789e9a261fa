"""
C-ABI boundary of the ORDER BY ... LIMIT entry points
(cstripe_scan_select_topn / cstripe_scan_last_topn_ms, include/cstripe.h)
and the host-side coordinator merge ca.merge_topn. No GPU needed: the
symbols are exported, the ctypes mirror of cstripe_order_key has the C
layout, an unstaged scan fails loudly before any argument is looked at, and
merge_topn is checked against hand-written expectations.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import citus_amd as ca

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_topn_symbols_exported():
    lib = C.CDLL(os.path.join(REPO, "citus_amd", "libcstripe.so"))
    for name in ("cstripe_scan_select_topn", "cstripe_scan_last_topn_ms"):
        assert hasattr(lib, name), name
    assert hasattr(ca.Scan, "select_topn") and hasattr(ca.Scan, "last_topn_ms")
    assert callable(ca.merge_topn)
    assert lib.cstripe_abi_version() == 2


def test_constants_match_header():
    hdr = open(os.path.join(REPO, "include", "cstripe.h")).read()
    assert "#define CSTRIPE_MAX_ORDER_COLS    4" in hdr
    assert "#define CSTRIPE_MAX_TOPN          (1u << 20)" in hdr
    assert (ca.MAX_ORDER_COLS, ca.MAX_TOPN) == (4, 1 << 20)
    assert (ca.ORDER_DESC, ca.ORDER_NULLS_FIRST) == (1, 2)


def test_order_key_struct_matches_c_layout(tmp_path):
    assert C.sizeof(ca.OrderKey) == 8
    src = tmp_path / "sz.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "cstripe.h"\n'
        'int main(void) { printf("%zu %zu %zu %u %u\\n", sizeof(cstripe_order_key),\n'
        '  offsetof(cstripe_order_key, column), offsetof(cstripe_order_key, flags),\n'
        '  CSTRIPE_ORDER_DESC, CSTRIPE_ORDER_NULLS_FIRST);\n'
        '  return 0; }\n')
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c11", str(src),
                           "-I" + os.path.join(REPO, "include"), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    assert got == [C.sizeof(ca.OrderKey), ca.OrderKey.column.offset,
                   ca.OrderKey.flags.offset, ca.ORDER_DESC, ca.ORDER_NULLS_FIRST]


def test_unstaged_scan_is_nogpu_before_any_argument(tmp_path):
    """never staged here (no stage() call), with or without a device: the
    staged check comes first, even with bad arguments"""
    path = str(tmp_path / "t.cs")
    ca.write_table(path, [("a", ca.I64, 0)], [np.arange(10, dtype=np.int64)])
    with ca.Reader(path) as r, r.scan(cols_mask=1) as s:
        with pytest.raises(ca.CStripeError, match=r"rc=-4"):
            s.select_topn([0], 3)
        with pytest.raises(ca.CStripeError, match=r"rc=-4"):
            s.select_topn([], 0)                        # n_order 0, limit 0
        with pytest.raises(ca.CStripeError, match=r"rc=-4"):
            s.select_topn([0, 0, 0, 0, 0], ca.MAX_TOPN + 1)
        rows = ca.Rows()
        assert ca._select_topn(s._h, None, 0, 0, C.byref(rows), 0) == ca.ERR_NOGPU
        assert ca._select_topn(s._h, None, 9, 0, None, 0) == ca.ERR_NOGPU
        assert s.last_topn_ms == (0.0, 0.0, 0.0)


def test_parse_order_defaults():
    assert ca.parse_order([3, (1, "asc"), (2, "desc"), (4, "asc", "first"),
                           (5, "DESC", "last")]) == \
        [(3, False, False), (1, False, False), (2, True, True),
         (4, False, True), (5, True, False)]
    with pytest.raises(ca.CStripeError):
        ca.parse_order([(1, "up")])
    with pytest.raises(ca.CStripeError):
        ca.parse_order([(1, "asc", "middle")])


# ---------------- merge_topn ----------------

def part(vals, rns, nulls=None, col=0, **extra):
    vals = np.asarray(vals)
    n = len(vals)
    nl = np.zeros(n, np.uint8) if nulls is None else np.asarray(nulls, np.uint8)
    res = {"n_rows": n, "row_numbers": np.asarray(rns, dtype=np.int64),
           "values": {col: vals}, "nulls": {col: nl}}
    res.update(extra)
    return res


def rows_of(m):
    return list(zip(m["part"].tolist(), m["row_numbers"].tolist()))


def test_merge_two_parts_interleaved():
    a = part(np.array([1, 4, 7], np.int64), [10, 11, 12])
    b = part(np.array([2, 3, 9], np.int64), [5, 6, 7])
    m = ca.merge_topn([a, b], [0], 4)
    assert m["n_rows"] == 4
    assert m["values"][0].tolist() == [1, 2, 3, 4]
    assert rows_of(m) == [(0, 10), (1, 5), (1, 6), (0, 11)]
    assert m["values"][0].dtype == np.int64


def test_merge_desc():
    a = part(np.array([7, 4, 1], np.int64), [12, 11, 10])
    b = part(np.array([9, 3, 2], np.int64), [7, 6, 5])
    m = ca.merge_topn([a, b], [(0, "desc")], 3)
    assert m["values"][0].tolist() == [9, 7, 4]
    assert rows_of(m) == [(1, 7), (0, 12), (0, 11)]
    # the most negative value does not wrap under DESC
    lo = np.iinfo(np.int64).min
    c = part(np.array([lo, 0, 5], np.int64), [0, 1, 2])
    assert ca.merge_topn([c], [(0, "desc")], 3)["values"][0].tolist() == [5, 0, lo]


def test_merge_nulls_first_and_last():
    a = part(np.array([0, 5, 1], np.int64), [0, 1, 2], nulls=[1, 0, 0])
    b = part(np.array([3, 0], np.int64), [0, 1], nulls=[0, 1])
    last = ca.merge_topn([a, b], [(0, "asc")], 10)            # PG default: last
    assert last["nulls"][0].tolist() == [0, 0, 0, 1, 1]
    assert last["values"][0].tolist() == [1, 3, 5, 0, 0]
    assert rows_of(last)[3:] == [(0, 0), (1, 1)]
    first = ca.merge_topn([a, b], [(0, "asc", "first")], 10)
    assert first["nulls"][0].tolist() == [1, 1, 0, 0, 0]
    assert first["values"][0].tolist() == [0, 0, 1, 3, 5]
    dflt = ca.merge_topn([a, b], [(0, "desc")], 10)           # PG default: first
    assert dflt["nulls"][0].tolist() == [1, 1, 0, 0, 0]
    assert dflt["values"][0].tolist() == [0, 0, 5, 3, 1]
    dlast = ca.merge_topn([a, b], [(0, "desc", "last")], 10)
    assert dlast["values"][0].tolist() == [5, 3, 1, 0, 0]
    assert dlast["nulls"][0].tolist() == [0, 0, 0, 1, 1]


def test_merge_nan_greatest_and_equal_to_itself():
    nan2 = np.frombuffer(np.uint64(0xFFF8000000000123).tobytes(), np.float64)[0]
    a = part(np.array([np.nan, 1.5, np.inf]), [0, 1, 2])
    b = part(np.array([nan2, -np.inf]), [0, 1])
    m = ca.merge_topn([a, b], [0], 10)
    v = m["values"][0]
    assert v[:3].tolist() == [-np.inf, 1.5, np.inf]
    assert np.isnan(v[3:]).all()
    # the two NaNs tie (different payloads, different signs): part, then row
    assert rows_of(m)[3:] == [(0, 0), (1, 0)]
    d = ca.merge_topn([a, b], [(0, "desc", "last")], 2)
    assert np.isnan(d["values"][0]).all() and rows_of(d) == [(0, 0), (1, 0)]


def test_merge_negative_zero_ties_with_zero():
    a = part(np.array([0.0, 1.0], np.float64), [3, 4])
    b = part(np.array([-0.0, -1.0], np.float64), [1, 2])
    m = ca.merge_topn([a, b], [0], 10)
    # -1 first; then the two zeros tie and part 0 comes first although its
    # zero is the positive one and its row number is larger
    assert rows_of(m) == [(1, 2), (0, 3), (1, 1), (0, 4)]
    assert np.signbit(m["values"][0]).tolist() == [True, False, True, False]
    f32 = ca.merge_topn([part(np.array([0.0], np.float32), [9]),
                         part(np.array([-0.0], np.float32), [0])], [0], 10)
    assert rows_of(f32) == [(0, 9), (1, 0)] and f32["values"][0].dtype == np.float32


def test_merge_tie_across_parts_part_then_row_number():
    a = part(np.array([5, 5], np.int64), [40, 41])
    b = part(np.array([5, 5, 1], np.int64), [7, 8, 9])
    m = ca.merge_topn([a, b], [0], 4)
    assert rows_of(m) == [(1, 9), (0, 40), (0, 41), (1, 7)]


def test_merge_offset_and_large_limit():
    a = part(np.array([1, 4, 7], np.int64), [0, 1, 2])
    b = part(np.array([2, 3, 9], np.int64), [0, 1, 2])
    m = ca.merge_topn([a, b], [0], 2, offset=3)
    assert m["values"][0].tolist() == [4, 7]
    big = ca.merge_topn([a, b], [0], 100)
    assert big["n_rows"] == 6 and big["values"][0].tolist() == [1, 2, 3, 4, 7, 9]
    assert ca.merge_topn([a, b], [0], 100, offset=6)["n_rows"] == 0
    assert ca.merge_topn([a, b], [0], 0)["n_rows"] == 0


def test_merge_two_columns_mixed_direction():
    def p2(k0, k1, rns):
        n = len(k0)
        return {"n_rows": n, "row_numbers": np.asarray(rns, np.int64),
                "values": {2: np.asarray(k0, np.int32), 5: np.asarray(k1, np.int16)},
                "nulls": {2: np.zeros(n, np.uint8), 5: np.zeros(n, np.uint8)}}
    a = p2([1, 1, 2], [9, 3, 0], [0, 1, 2])
    b = p2([1, 2], [5, 7], [0, 1])
    m = ca.merge_topn([a, b], [(2, "asc"), (5, "desc")], 10)
    assert list(zip(m["values"][2].tolist(), m["values"][5].tolist())) == \
        [(1, 9), (1, 5), (1, 3), (2, 7), (2, 0)]
    with pytest.raises(ca.CStripeError, match="not among"):
        ca.merge_topn([a, b], [3], 10)


def test_merge_vartext_by_bytes_and_error_without_text():
    def tp(strs, ranks, rns):
        t = np.empty(len(strs), dtype=object)
        t[:] = strs
        nl = np.array([1 if s is None else 0 for s in strs], np.uint8)
        return part(np.asarray(ranks, np.int32), rns, nulls=nl, col=1,
                    text_cols=[1], text={1: t})
    # ranks are per scan: rank 0 of part a ("pear") sorts after rank 1 of b
    a = tp([b"pear", b"zebra", None], [0, 1, 0], [0, 1, 2])
    b = tp([b"", b"apple", b"pea", b"\xc3\xa9"], [0, 1, 2, 3], [0, 1, 2, 3])
    m = ca.merge_topn([a, b], [1], 10, text=True)
    assert m["text"][1].tolist() == [b"", b"apple", b"pea", b"pear", b"zebra",
                                     b"\xc3\xa9", None]
    assert rows_of(m)[-1] == (0, 2) and m["nulls"][1].tolist()[-1] == 1
    d = ca.merge_topn([a, b], [(1, "desc", "last")], 2, text=True)
    assert d["text"][1].tolist() == [b"\xc3\xa9", b"zebra"]
    # the same parts as a worker returns them without decode_text
    for p_ in (a, b):
        del p_["text"]
    with pytest.raises(ca.CStripeError, match="(?i)text"):
        ca.merge_topn([a, b], [1], 10)
