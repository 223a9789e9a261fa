"""
CPU tests (no GPU) for GROUP BY ... HAVING ... ORDER BY ... LIMIT: the ABI
contract of cstripe_scan_agg_hashed_topn that holds without a device, and
merge_groups_topn — the coordinator side — against hand-written cases.

Expected values are written out here or computed in Python from the inputs
the test itself builds, never from the library.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import citus_amd as ca
from test_hashagg_cpu import (count_partial, f64_partial, make_part, null_partial,
                              result_keys, sum_partial)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AGGS = [(ca.AGG_SUM_I64, 0), (ca.AGG_COUNT_STAR, -1)]


def rows_of(inputs):
    """inputs: (key tuple, sum or None, count)"""
    return [(k, [null_partial() if s is None else sum_partial(s), count_partial(c)])
            for k, s, c in inputs]


def part(n_key_cols, inputs):
    return make_part(n_key_cols, rows_of(inputs))


def sums(res):
    return [None if p["is_null"] else ca.partial_i128(p) for p in res["partials"][:, 0]]


# ---------------- the ABI without a device ----------------

def test_symbols_are_exported_and_the_abi_version_is_2():
    lib = C.CDLL(os.path.join(REPO, "citus_amd", "libcstripe.so"))
    for name in ("cstripe_scan_agg_hashed_topn", "cstripe_scan_last_group_topn"):
        assert hasattr(lib, name), name
    lib.cstripe_abi_version.restype = C.c_uint32
    assert lib.cstripe_abi_version() == 2
    assert hasattr(ca.Scan, "agg_hashed_topn") and hasattr(ca.Scan, "last_group_topn")
    assert callable(ca.merge_groups_topn)


def test_struct_sizes_and_constants_match_the_header(tmp_path):
    assert C.sizeof(ca.GroupOrder) == 16
    assert C.sizeof(ca.Having) == 24
    assert (ca.MAX_GROUP_ORDER, ca.MAX_HAVING, ca.GORDER_AGG, ca.GORDER_KEY) == (4, 4, 0, 1)
    src = tmp_path / "sz.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "cstripe.h"\n'
        'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d %u %u %d\\n",\n'
        '  sizeof(cstripe_group_order), offsetof(cstripe_group_order, kind),\n'
        '  offsetof(cstripe_group_order, index), offsetof(cstripe_group_order, flags),\n'
        '  sizeof(cstripe_having), offsetof(cstripe_having, op),\n'
        '  offsetof(cstripe_having, ival), offsetof(cstripe_having, fval),\n'
        '  CSTRIPE_MAX_GROUP_ORDER, CSTRIPE_MAX_HAVING, CSTRIPE_GORDER_AGG,\n'
        '  CSTRIPE_GORDER_KEY, CSTRIPE_ABI_VERSION);\n'
        '  return 0; }\n')
    exe = str(tmp_path / "sz")
    # the header still compiles as C
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", str(src),
                           "-I" + os.path.join(REPO, "include"), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    assert got == [16, ca.GroupOrder.kind.offset, ca.GroupOrder.index.offset,
                   ca.GroupOrder.flags.offset, 24, ca.Having.op.offset,
                   ca.Having.ival.offset, ca.Having.fval.offset, 4, 4, 0, 1, 2]


def test_unstaged_scan_is_nogpu_before_any_argument_check(tmp_path):
    path = str(tmp_path / "t.cs")
    k = np.arange(100, dtype=np.int64) % 7
    ca.write_table(path, [("k", ca.I64, 0)], [k])
    with ca.Reader(path) as r, r.scan(cols_mask=1) as s:
        arr = ca.make_aggs([(ca.AGG_COUNT_STAR, -1)])
        kc = (C.c_uint32 * 1)(0)
        out = ca.HGroups()
        oarr, n_order = ca.make_group_order([("agg", 0, "desc")])
        assert ca._scan_agg_hashed_topn(s._h, arr, 1, kc, 1, 16, None, 0, oarr, n_order,
                                        5, C.byref(out)) == ca.ERR_NOGPU
        # even with arguments that would otherwise be ERR_ARG
        assert ca._scan_agg_hashed_topn(s._h, arr, 1, kc, 0, 0, None, 9, None, 9,
                                        0, C.byref(out)) == ca.ERR_NOGPU
        with pytest.raises(ca.CStripeError, match="not staged"):
            s.agg_hashed_topn([(ca.AGG_COUNT_STAR, -1)], [0], 16, [("agg", 0, "desc")], 3)
        assert s.last_group_topn == (0, 0, 0.0, 0.0, 0.0)


def test_group_order_parsing():
    assert ca.parse_group_order([("agg", 0, "desc"), ("key", 1),
                                 ("agg", 2, "asc", "nulls_first"),
                                 ("key", 0, "desc", "nulls_first")]) == [
        (ca.GORDER_AGG, 0, ca.ORDER_DESC), (ca.GORDER_KEY, 1, 0),
        (ca.GORDER_AGG, 2, ca.ORDER_NULLS_FIRST),
        (ca.GORDER_KEY, 0, ca.ORDER_DESC | ca.ORDER_NULLS_FIRST)]
    for bad in ([("col", 0)], [("agg",)], [("agg", 0, "down")]):
        with pytest.raises(ca.CStripeError):
            ca.parse_group_order(bad)


# ---------------- merge_groups_topn ----------------

def test_overlapping_parts_merge_before_the_order():
    """key 1 leads no part on its own and wins after the merge"""
    a = part(1, [((1,), 60, 1), ((2,), 100, 1), ((3,), 5, 1)])
    b = part(1, [((1,), 60, 1), ((4,), 90, 1)])
    res = ca.merge_groups_topn(AGGS, 1, [a, b], [("agg", 0, "desc")], 2)
    assert result_keys(res, 1) == [(1,), (2,)]
    assert sums(res) == [120, 100]
    assert res["partials"][0, 1]["count"] == 2


def test_disjoint_parts_per_shard_topn_is_exact():
    a_all = [((k,), 10 * k, 1) for k in (1, 3, 5, 7)]
    b_all = [((k,), 10 * k, 1) for k in (2, 4, 6, 8)]
    order = [("agg", 0, "desc")]
    whole = ca.merge_groups_topn(AGGS, 1, [part(1, a_all), part(1, b_all)], order, 3)
    a_top = ca.merge_groups_topn(AGGS, 1, [part(1, a_all)], order, 3)
    b_top = ca.merge_groups_topn(AGGS, 1, [part(1, b_all)], order, 3)
    res = ca.merge_groups_topn(AGGS, 1, [a_top, b_top], order, 3)
    assert result_keys(res, 1) == result_keys(whole, 1) == [(8,), (7,), (6,)]
    assert res["partials"].tobytes() == whole["partials"].tobytes()


def test_null_keys_last_in_ties_and_by_flag_in_key_terms():
    p = part(1, [((None,), 5, 1), ((2,), 5, 1), ((-1,), 5, 1), ((9,), 7, 1)])
    res = ca.merge_groups_topn(AGGS, 1, [p], [("agg", 0)], 10)
    assert result_keys(res, 1) == [(-1,), (2,), (None,), (9,)]
    assert res["keys"][0][2] == 0                  # NULL key comes back as 0
    res = ca.merge_groups_topn(AGGS, 1, [p], [("key", 0, "desc")], 10)
    assert result_keys(res, 1) == [(9,), (2,), (-1,), (None,)]
    res = ca.merge_groups_topn(AGGS, 1, [p], [("key", 0, "desc", "nulls_first")], 10)
    assert result_keys(res, 1) == [(None,), (9,), (2,), (-1,)]
    res = ca.merge_groups_topn(AGGS, 1, [p], [], 2)  # no terms: key order
    assert result_keys(res, 1) == [(-1,), (2,)]


def test_null_aggregates_sort_last_or_first():
    p = part(1, [((1,), None, 0), ((2,), -4, 1), ((3,), 8, 1)])
    assert result_keys(ca.merge_groups_topn(AGGS, 1, [p], [("agg", 0, "desc")], 3), 1) == \
        [(3,), (2,), (1,)]
    assert result_keys(ca.merge_groups_topn(
        AGGS, 1, [p], [("agg", 0, "desc", "nulls_first")], 3), 1) == [(1,), (3,), (2,)]
    assert result_keys(ca.merge_groups_topn(AGGS, 1, [p], [("agg", 0)], 2), 1) == \
        [(2,), (3,)]


def test_offset_and_limit_slice_the_total_order():
    p = part(1, [((k,), k * k, 1) for k in range(10)])
    order = [("agg", 0, "desc")]
    assert result_keys(ca.merge_groups_topn(AGGS, 1, [p], order, 3, offset=2), 1) == \
        [(7,), (6,), (5,)]
    assert result_keys(ca.merge_groups_topn(AGGS, 1, [p], order, 5, offset=8), 1) == \
        [(1,), (0,)]
    assert ca.merge_groups_topn(AGGS, 1, [p], order, 0)["n_groups"] == 0
    empty = ca.merge_groups_topn(AGGS, 1, [p], order, 5, offset=50)
    assert empty["n_groups"] == 0 and empty["partials"].shape == (0, 2)


def test_having_applies_after_the_merge():
    """each part's count is 1; only the merged count passes HAVING count > 1"""
    a = part(1, [((1,), 10, 1), ((2,), 50, 1)])
    b = part(1, [((1,), 10, 1), ((3,), 70, 1)])
    res = ca.merge_groups_topn(AGGS, 1, [a, b], [("agg", 0, "desc")], 5,
                               having=[(1, ca.PRED_GT, 1)])
    assert result_keys(res, 1) == [(1,)] and sums(res) == [20]
    # two atoms are ANDed; a NULL aggregate fails its atom
    c = part(1, [((4,), None, 3), ((5,), 2**70, 3), ((6,), 1, 3)])
    res = ca.merge_groups_topn(AGGS, 1, [c], [("key", 0)], 5,
                               having=[(0, ca.PRED_GE, 1), (1, ca.PRED_EQ, 3)])
    assert result_keys(res, 1) == [(5,), (6,)]
    res = ca.merge_groups_topn(AGGS, 1, [c], [("key", 0)], 5,
                               having=[(0, ca.PRED_GT, 2**63 - 1)])
    assert result_keys(res, 1) == [(5,)]           # int128 compares exactly


def test_ties_break_by_key_tuple_column_0_first():
    inputs = [((2, 1), 9, 1), ((1, None), 9, 1), ((1, 5), 9, 1), ((None, 0), 9, 1),
              ((1, -3), 9, 1), ((0, 0), 10, 1)]
    res = ca.merge_groups_topn(AGGS, 2, [part(2, inputs[:3]), part(2, inputs[3:])],
                               [("agg", 0, "desc")], 4)
    assert result_keys(res, 2) == [(0, 0), (1, -3), (1, 5), (1, None)]


def test_float_terms_follow_pg_order():
    aggs = [(ca.AGG_MAX_F64, 0)]
    vals = {1: 2.5, 2: float("nan"), 3: float("inf"), 4: -0.0, 5: 0.0, 6: float("-inf")}
    p = make_part(1, [((k,), [f64_partial(v)]) for k, v in vals.items()])
    res = ca.merge_groups_topn(aggs, 1, [p], [("agg", 0, "desc")], 6)
    assert result_keys(res, 1) == [(2,), (3,), (1,), (4,), (5,), (6,)]   # -0.0 ties 0.0
    res = ca.merge_groups_topn(aggs, 1, [p], [("key", 0)], 6,
                               having=[(0, ca.PRED_GE, float("inf"))])
    assert result_keys(res, 1) == [(2,), (3,)]


def test_bad_arguments_raise():
    p = part(1, [((1,), 1, 1)])
    with pytest.raises(ca.CStripeError):
        ca.merge_groups_topn(AGGS, 1, [p], [("agg", 2)], 1)
    with pytest.raises(ca.CStripeError):
        ca.merge_groups_topn(AGGS, 1, [p], [("key", 1)], 1)
    with pytest.raises(ca.CStripeError):
        ca.merge_groups_topn(AGGS, 1, [p], [("agg", 0)], -1)
