"""
Expressions (cstripe_scan_begin_exprs, include/cstripe.h) — everything that
needs no GPU: the exported symbols and C layouts, the begin-time argument
errors, column addressing, chunk refutation, the Python builder against
hand-written postfix, and the tests' own evaluator (exprutil) pinned on
hand-computed rows.
"""
import ctypes as C
import datetime
import os
import subprocess

import numpy as np
import pytest

import citus_amd as ca
import exprutil as X

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64_MIN, I64_MAX = X.I64_MIN, X.I64_MAX


# ------------------------------------------------------------ symbols / layout
def test_symbols_and_constants():
    lib = C.CDLL(os.path.join(REPO, "citus_amd", "libcstripe.so"))
    for name in ("cstripe_scan_begin_exprs", "cstripe_scan_expr_range",
                 "cstripe_scan_last_expr_ms"):
        assert hasattr(lib, name), name
    assert (ca.MAX_EXPRS, ca.MAX_EXPR_OPS, ca.MAX_EXPR_DEPTH) == (8, 48, 8)
    names = ("COL", "CONST", "NULL", "ADD", "SUB", "MUL", "DIV", "MOD", "NEG", "LT", "LE",
             "GT", "GE", "EQ", "NE", "AND", "OR", "NOT", "IS_NULL", "COALESCE", "SELECT", "YEAR")
    for i, n in enumerate(names):
        assert getattr(ca, "EX_" + n) == i == getattr(X, n)
    for name in ("computed", "expr_range", "last_expr_ms"):
        assert hasattr(ca.Scan, name), name
    lib.cstripe_abi_version.restype = C.c_uint32
    assert lib.cstripe_abi_version() == 2        # additive: the version stays


def test_structs_match_c_layout(tmp_path):
    assert C.sizeof(ca.ExprOp) == 16 and C.sizeof(ca.ExprIn) == 16
    src = tmp_path / "sz.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "cstripe.h"\n'
        'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d %d\\n",\n'
        '  sizeof(cstripe_expr_op), offsetof(cstripe_expr_op, op),\n'
        '  offsetof(cstripe_expr_op, column), offsetof(cstripe_expr_op, ival),\n'
        '  sizeof(cstripe_expr), offsetof(cstripe_expr, ops), offsetof(cstripe_expr, n_ops),\n'
        '  (int)CSTRIPE_MAX_EXPRS, (int)CSTRIPE_MAX_EXPR_OPS, (int)CSTRIPE_MAX_EXPR_DEPTH,\n'
        '  (int)CSTRIPE_EX_COL, (int)CSTRIPE_EX_SELECT, (int)CSTRIPE_EX_YEAR);\n'
        '  return 0; }\n')
    exe = str(tmp_path / "sz")
    subprocess.check_call(["gcc", "-std=c11", str(src),
                           "-I" + os.path.join(REPO, "include"), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    O, E = ca.ExprOp, ca.ExprIn
    assert got == [16, O.op.offset, O.column.offset, O.ival.offset,
                   16, E.ops.offset, E.n_ops.offset, 8, 48, 8, 0, 20, 21]


# ------------------------------------------------------------ begin-time errors
DEFS = [("a", ca.I64, 0), ("f", ca.F64, 0), ("t", ca.VARTEXT, 0), ("c", ca.TEXT, 0),
        ("g", ca.F32, 0), ("h", ca.I16, 0), ("b", ca.I8, 0), ("d", ca.I32, 0)]
N_TAB = len(DEFS)
A, H, B, D = 0, 5, 6, 7


@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("expr") / "mixed.cs")
    ca.write_table(p, DEFS, [np.arange(4, dtype=np.int64),
                             np.arange(4, dtype=np.float64),
                             [b"a", b"b", b"c", b"d"],
                             ca.text_slots(["A", "B", "C", "D"]).view(np.int32),
                             np.arange(4, dtype=np.float32),
                             np.arange(4, dtype=np.int16),
                             np.arange(4, dtype=np.int8),
                             np.arange(4, dtype=np.int32)],
                   compression=ca.COMP_NONE)
    return p


def raw_lookup(key_col, keys, payloads):
    lk = ca.LookupIn()
    keep = [np.ascontiguousarray(a, dtype=np.int64) for a in [keys] + list(payloads)]
    lk.key_column = key_col
    lk.n_payloads = len(payloads)
    lk.keys = keep[0].ctypes.data_as(C.c_void_p).value
    for i, p in enumerate(keep[1:]):
        lk.payloads[i] = p.ctypes.data_as(C.c_void_p).value
    lk.n = len(keys)
    lk._keep = keep
    return lk


def begin(r, preds, exprs, lookups=(), sets=(), n_exprs=None):
    arr = ca.make_preds(preds)
    la = (ca.LookupIn * max(1, len(lookups)))(*lookups)
    sa = (ca.ValueSet * max(1, len(sets)))(*sets)
    ea, n = ca.make_exprs(list(exprs))
    return ca._scan_begin_exprs(r._h, 0, arr, len(preds), None, 0,
                                sa if sets else None, len(sets),
                                la if lookups else None, len(lookups),
                                ea, n if n_exprs is None else n_exprs)


def col(i):
    return (X.COL, i, 0)


def const(v):
    return (X.CONST, 0, v)


def op(o):
    return (o, 0, 0)


K, P = [1, 2, 3], [10, 20, 30]


def refused(r, exprs, *words, **kw):
    assert not begin(r, [], exprs, **kw)
    msg = ca.errmsg()
    for w in words:
        assert w in msg, (w, msg)


def test_begin_errors(mixed):
    with ca.Reader(mixed) as r:
        good = [col(A), const(1), op(X.ADD)]
        h = begin(r, [], [good])
        assert h, ca.errmsg()
        assert ca._scan_column_count(h) == N_TAB + 1
        ca._scan_end(h)
        # every integer width and a lookup-derived column are legal inputs
        for c in (A, H, B, D):
            h = begin(r, [], [[col(c)]])
            assert h, ca.errmsg()
            ca._scan_end(h)
        h = begin(r, [], [[col(N_TAB), col(A), op(X.MUL)]], lookups=[raw_lookup(A, K, [P])])
        assert h, ca.errmsg()
        ca._scan_end(h)
        # more than CSTRIPE_MAX_EXPRS; a count without an array
        refused(r, [good] * 9, "9 expressions")
        assert not ca._scan_begin_exprs(r._h, 0, ca.make_preds([]), 0, None, 0, None, 0,
                                        None, 0, None, 2)
        assert "2 expressions" in ca.errmsg()
        # n_ops 0 or above the limit
        refused(r, [good, []], "expression 1", "0 ops")
        long = [const(1)] + [const(1), op(X.ADD)] * 24            # 49 ops, depth 2
        assert len(long) == 49
        refused(r, [long], "expression 0", "49 ops")
        h = begin(r, [], [long[:47]])                             # 47 ops is fine
        assert h, ca.errmsg()
        ca._scan_end(h)
        # an unknown op
        refused(r, [good, [col(A), (22, 0, 0)]], "expression 1", "op 1", "unknown op 22")
        # stack underflow: binary, unary and ternary
        refused(r, [[col(A), op(X.ADD)]], "expression 0", "op 1", "underflow")
        refused(r, [[op(X.NEG)]], "expression 0", "op 0", "underflow")
        refused(r, [good, good, [col(A), const(1), op(X.SELECT)]], "expression 2", "op 2",
                "underflow")
        # depth above CSTRIPE_MAX_EXPR_DEPTH: the ninth push
        deep = [const(1)] * 9 + [op(X.ADD)] * 8
        refused(r, [deep], "expression 0", "op 8", "depth 9")
        h = begin(r, [], [[const(1)] * 8 + [op(X.ADD)] * 7])
        assert h, ca.errmsg()
        ca._scan_end(h)
        # a final depth other than 1
        refused(r, [[col(A), const(1)]], "expression 0", "op 1", "2 values")
        # a bad or wrongly typed column
        refused(r, [[col(N_TAB + 1)]], "expression 0", "op 0", "column %d" % (N_TAB + 1),
                "out of range")
        refused(r, [[const(1), col(99), op(X.ADD)]], "expression 0", "op 1", "column 99")
        for c in (1, 2, 3, 4):
            refused(r, [good, [col(c)]], "expression 1", "op 0", "column %d" % c, "I8/I16/I32/I64")
        # another computed column, its own or an earlier one
        refused(r, [good, [col(N_TAB)]], "expression 1", "op 0", "computed")
        refused(r, [[col(N_TAB + 1)], good], "expression 0", "op 0", "computed",
                lookups=[raw_lookup(A, K, [P])])
        # a lookup key column must be a table column
        h = begin(r, [], [good], lookups=[raw_lookup(N_TAB, K, [P])])
        assert not h and "key column" in ca.errmsg()
        # a predicate beyond the scan's columns; IN / NOT IN on a computed column
        assert not begin(r, [(N_TAB + 1, ca.PRED_EQ, 1)], [good])
        assert "predicate 0" in ca.errmsg() and "column %d" % (N_TAB + 1) in ca.errmsg()
        vs = ca.ValueSet()
        for o in (ca.PRED_IN, ca.PRED_NOT_IN):
            assert not begin(r, [(N_TAB, o, 0)], [good], sets=[vs])
            assert "predicate 0" in ca.errmsg() and "computed" in ca.errmsg()
        h = begin(r, [(N_TAB, ca.PRED_EQ, 1)], [good])
        assert h, ca.errmsg()
        # the range is a stage-time measurement
        lo, hi, n = C.c_int64(), C.c_int64(), C.c_uint64()
        assert ca._expr_range(h, 0, C.byref(lo), C.byref(hi), C.byref(n)) == ca.ERR_NOGPU
        assert ca._expr_range(h, 1, C.byref(lo), C.byref(hi), C.byref(n)) == ca.ERR_ARG
        ms = C.c_double(-1)
        assert ca._last_expr_ms(h, C.byref(ms)) == ca.OK and ms.value == 0
        ca._scan_end(h)


def test_no_exprs_is_begin_lookups(tmp_path):
    path = str(tmp_path / "t.cs")
    v = np.arange(5000, dtype=np.int64)
    ca.write_table(path, [("a", ca.I64, 0), ("b", ca.I64, 0)], [v, v[::-1].copy()],
                   chunk_group_row_limit=1000)
    preds = [(0, ca.PRED_LT, 1500)]
    with ca.Reader(path) as r:
        arr = ca.make_preds(preds)
        la = (ca.LookupIn * 1)(raw_lookup(0, K, [P]))
        h0 = ca._scan_begin_lookups(r._h, 1, arr, 1, None, 0, None, 0, la, 1)
        h1 = ca._scan_begin_exprs(r._h, 1, arr, 1, None, 0, None, 0, la, 1, None, 0)
        assert h0 and h1, ca.errmsg()
        assert ca._filtered(h0) == ca._filtered(h1) == 3
        assert ca._scan_column_count(h0) == ca._scan_column_count(h1) == 3
        ca._scan_end(h0)
        ca._scan_end(h1)


def test_column_ids_after_the_lookups(mixed):
    e = [ca.col(A) + 1, ca.col(A) * 2]
    with ca.Reader(mixed) as r:
        for lks, n_derived in (([], 0), ([ca.Lookup(A, K, [P, P])], 2),
                               ([ca.Lookup(A, K, [P, P]), ca.Lookup(H, K, [P])], 3)):
            with r.scan(lookups=lks, exprs=e) as s:
                assert s.column_count() == N_TAB + n_derived + 2
                assert s.computed(0) == N_TAB + n_derived
                assert s.computed(1) == N_TAB + n_derived + 1
                with pytest.raises(ca.CStripeError):
                    s.computed(2)
        # an expression may read the derived columns in front of it
        with r.scan(lookups=[ca.Lookup(A, K, [P])], exprs=[ca.col(N_TAB) + ca.col(H)]) as s:
            assert s.computed(0) == N_TAB + 1


def test_the_64_column_limit(tmp_path):
    path = str(tmp_path / "wide60.cs")
    a = np.arange(4, dtype=np.int64)
    ca.write_table(path, [(f"c{j}", ca.I64, 0) for j in range(60)], [a] * 60,
                   compression=ca.COMP_NONE)
    one = [col(0)]
    with ca.Reader(path) as r:
        h = begin(r, [(63, ca.PRED_EQ, 1)], [one] * 2, lookups=[raw_lookup(0, K, [P, P])])
        assert h, ca.errmsg()
        assert ca._scan_column_count(h) == 64
        ca._scan_end(h)
        refused(r, [one] * 3, "64", lookups=[raw_lookup(0, K, [P, P])])
        refused(r, [one] * 5, "64")
        h = begin(r, [], [one] * 4)
        assert h, ca.errmsg()
        ca._scan_end(h)


def test_computed_predicates_never_refute(tmp_path):
    path = str(tmp_path / "t.cs")
    v = np.arange(5000, dtype=np.int64)
    ca.write_table(path, [("a", ca.I64, 0)], [v], chunk_group_row_limit=1000)
    e = [ca.col(0) + 1]
    with ca.Reader(path) as r:
        E0 = 1
        for preds, want in (([], 0),
                            ([(E0, ca.PRED_LT, -5)], 0),              # no row passes: still no pruning
                            ([(E0, ca.PRED_EQ, 10**12)], 0),
                            ([(0, ca.PRED_LT, 1500)], 3),             # the base column prunes
                            ([(0, ca.PRED_LT, 1500), (E0, ca.PRED_GT, 10**9)], 3),
                            ([(0, ca.PRED_LT, 1500, 7), (E0, ca.PRED_LT, -5, 7)], 0)):
            with r.scan(preds=preds, exprs=e) as s:
                assert s.chunk_groups_filtered == want, preds
        for env in ("0", "1"):                       # the device prune kernel is skipped
            os.environ["CSTRIPE_DEVICE_PRUNE"] = env
            try:
                with r.scan(preds=[(0, ca.PRED_LT, 1500), (E0, ca.PRED_GT, 10**9)], exprs=e) as s:
                    assert s.chunk_groups_filtered == 3
            finally:
                del os.environ["CSTRIPE_DEVICE_PRUNE"]


# ------------------------------------------------------------------ the builder
def test_builder_compiles_to_postfix():
    c, k, o = col, const, op
    cases = [
        (ca.col(2) * (100 - ca.col(3)),
         [c(2), k(100), c(3), o(X.SUB), o(X.MUL)]),
        (ca.col(5).lt(ca.col(6)) & ca.col(4).lt(ca.col(5)),
         [c(5), c(6), o(X.LT), c(4), c(5), o(X.LT), o(X.AND)]),
        (ca.col(5).year(), [c(5), o(X.YEAR)]),
        (ca.case(ca.col(1).ne(0), ca.col(0) // ca.col(1), 0),
         [c(1), k(0), o(X.NE), c(0), c(1), o(X.DIV), k(0), o(X.SELECT)]),
        (ca.case(ca.col(0).ge(10), ca.case(ca.col(0).ge(20), 2, 1)),
         [c(0), k(10), o(X.GE), c(0), k(20), o(X.GE), k(2), k(1), o(X.SELECT), o(X.NULL),
          o(X.SELECT)]),
        (ca.coalesce(-ca.col(0) % 7, ca.lit(I64_MIN)) | ~ca.col(1).is_null(),
         [c(0), o(X.NEG), k(7), o(X.MOD), k(I64_MIN), o(X.COALESCE), c(1), o(X.IS_NULL),
          o(X.NOT), o(X.OR)]),
        (1 + ca.col(0), [k(1), c(0), o(X.ADD)]),
        (ca.null().eq(ca.col(0)).le(3).gt(4), [o(X.NULL), c(0), o(X.EQ), k(3), o(X.LE), k(4), o(X.GT)]),
    ]
    for expr, want in cases:
        assert expr.ops == want
    with pytest.raises(ca.CStripeError):
        ca.lit(1 << 63)
    with pytest.raises(ca.CStripeError):
        ca.col(0) + 1.5
    # make_exprs takes builder objects, ints and raw tuples alike
    arr, n = ca.make_exprs([ca.col(2) + 1, 7, [c(2), k(1), o(X.ADD)]])
    assert n == 3 and arr[1].n_ops == 1 and arr[1].ops[0].ival == 7
    for i in (0, 2):
        assert [(arr[i].ops[j].op, arr[i].ops[j].column, arr[i].ops[j].ival)
                for j in range(arr[i].n_ops)] == [c(2), k(1), o(X.ADD)]


def test_differential_seed_classification():
    """the condition on the seed of the GPU differential, checked here too:
    the evaluator alone classifies the 200 programs; every one begins"""
    columns, programs = X.diff_columns(), X.diff_programs()
    assert len(programs) == 200 and all(X.stack_depth(p) <= 4 for p in programs)
    assert all(len(v) == 300 and 0 < int(nl.sum()) < 300 for v, nl in columns.values())
    kinds = [X.first_error(X.evaluate_rows(p, columns, X.DIFF_ROWS)) for p in programs]
    assert kinds.count(None) >= 60 and len(kinds) - kinds.count(None) >= 30
    assert {X.DIV0, X.RANGE, X.YEAR_RANGE} <= set(kinds)


# ------------------------------------------------------- the evaluator itself
def test_evaluator_year():
    epoch = datetime.date(1970, 1, 1).toordinal()
    for y in range(1, 10000):
        for d in (datetime.date(y, 1, 1), datetime.date(y, 12, 31), datetime.date(y, 3, 1)):
            assert X.year_of(d.toordinal() - epoch) == y
    feb29 = datetime.date(2000, 2, 29).toordinal() - epoch
    assert X.year_of(feb29) == 2000 and X.year_of(0) == 1970 and X.year_of(-1) == 1969
    days = [-1, -365, -366, -719162, -719163, -719528, -719529, -10**6, -(1 << 31),
            -146097 * 5, -146097 * 5 - 1, -800000, -2000000]
    for d in days:
        want = int(np.datetime64(d, "D").astype("datetime64[Y]").astype(np.int64)) + 1970
        assert X.year_of(d) == want, d
    assert X.year_of(-719528) == 0 and X.year_of(-719529) == -1    # year 0 exists
    ev = lambda v: X.evaluate([col(0), op(X.YEAR)], {0: v})
    assert ev(None) is None and ev(19000) == 2022
    assert ev((1 << 31) - 1) == X.year_of((1 << 31) - 1)
    assert ev(1 << 31).kind == X.YEAR_RANGE and ev(-(1 << 31) - 1).kind == X.YEAR_RANGE


def test_evaluator_arithmetic_and_logic():
    def ev2(o, a, b):
        return X.evaluate([col(0), col(1), op(o)], {0: a, 1: b})
    # DIV truncates toward zero, MOD takes the dividend's sign
    assert [ev2(X.DIV, a, b) for a, b in ((7, 2), (-7, 2), (7, -2), (-7, -2))] == [3, -3, -3, 3]
    assert [ev2(X.MOD, a, b) for a, b in ((7, 2), (-7, 2), (7, -2), (-7, -2))] == [1, -1, 1, -1]
    assert ev2(X.DIV, 5, 0).kind == X.DIV0 and ev2(X.MOD, 5, 0).kind == X.DIV0
    assert ev2(X.DIV, I64_MIN, -1).kind == X.RANGE and ev2(X.MOD, I64_MIN, -1) == 0
    assert ev2(X.DIV, I64_MIN, 1) == I64_MIN and ev2(X.DIV, I64_MAX, -1) == -I64_MAX
    assert ev2(X.DIV, None, 0) is None and ev2(X.MOD, 5, None) is None
    assert ev2(X.ADD, I64_MAX, 1).kind == X.RANGE and ev2(X.ADD, I64_MAX, 0) == I64_MAX
    assert ev2(X.SUB, I64_MIN, 1).kind == X.RANGE and ev2(X.SUB, -1, I64_MAX) == I64_MIN
    assert ev2(X.MUL, 1 << 32, 1 << 31).kind == X.RANGE and ev2(X.MUL, 1 << 31, 1 << 31) == 1 << 62
    assert ev2(X.MUL, I64_MIN, -1).kind == X.RANGE and ev2(X.ADD, None, I64_MAX) is None
    assert X.evaluate([col(0), op(X.NEG)], {0: I64_MIN}).kind == X.RANGE
    assert X.evaluate([col(0), op(X.NEG)], {0: I64_MAX}) == -I64_MAX
    assert [ev2(o, 3, 5) for o in (X.LT, X.LE, X.GT, X.GE, X.EQ, X.NE)] == [1, 1, 0, 0, 0, 1]
    assert [ev2(o, 5, 5) for o in (X.LT, X.LE, X.GT, X.GE, X.EQ, X.NE)] == [0, 1, 0, 1, 1, 0]
    assert ev2(X.EQ, None, None) is None
    # Kleene tables, rows a = 0, 1, NULL; columns b = 0, 1, NULL
    T = (0, 1, None)
    assert [[ev2(X.AND, a, b) for b in T] for a in T] == [[0, 0, 0], [0, 1, None], [0, None, None]]
    assert [[ev2(X.OR, a, b) for b in T] for a in T] == [[0, 1, None], [1, 1, 1], [None, 1, None]]
    assert ev2(X.AND, 5, -3) == 1 and ev2(X.OR, 0, 9) == 1          # truth = nonzero
    assert [X.evaluate([col(0), op(X.NOT)], {0: a}) for a in (0, 7, None)] == [1, 0, None]
    assert [X.evaluate([col(0), op(X.IS_NULL)], {0: a}) for a in (0, None)] == [0, 1]
    assert [ev2(X.COALESCE, a, b) for a, b in ((1, 2), (None, 2), (None, None), (0, None))] \
        == [1, 2, None, 0]
    sel = lambda c, a, b: X.evaluate([col(0), col(1), col(2), op(X.SELECT)], {0: c, 1: a, 2: b})
    assert [sel(c, 10, 20) for c in (1, -1, 0, None)] == [10, 10, 20, 20]
    # lazy errors: a / b guarded three ways, and unguarded
    div = [col(0), col(1), op(X.DIV)]
    guard = [col(1), const(0), op(X.NE)]
    r0 = {0: 5, 1: 0}
    assert X.evaluate(div, r0).kind == X.DIV0
    assert X.evaluate(guard + div + [const(0), op(X.SELECT)], r0) == 0
    assert X.evaluate(guard + div + [const(3), op(X.GT), op(X.AND)], r0) == 0
    assert X.evaluate([col(1), const(0), op(X.EQ)] + div + [const(3), op(X.GT), op(X.OR)], r0) == 1
    assert X.evaluate(div + [const(3), op(X.GT)] + guard + [op(X.AND)], r0).kind == X.DIV0   # left first
    assert X.evaluate([op(X.NULL)] + div + [op(X.AND)], r0).kind == X.DIV0    # NULL does not decide
    assert X.evaluate([const(1)] + div + [op(X.COALESCE)], r0) == 1
    assert X.evaluate([op(X.NULL)] + div + [op(X.COALESCE)], r0).kind == X.DIV0
    assert X.evaluate(div + [op(X.IS_NULL)], r0).kind == X.DIV0
    assert X.evaluate(div + [op(X.NULL), op(X.ADD)], r0).kind == X.DIV0       # the operand raised first
    assert X.evaluate(div + [const(1), const(2), op(X.SELECT)], r0).kind == X.DIV0
    # the left operand's error wins over the right one's
    both = [const(I64_MAX), const(1), op(X.ADD)] + div + [op(X.SUB)]
    assert X.evaluate(both, r0).kind == X.RANGE
    rows = X.evaluate_rows(div, {0: (np.array([4, 5, 6]), None),
                                 1: (np.array([2, 0, 0]), np.array([0, 0, 1]))}, 3)
    assert rows[0] == 2 and rows[1].kind == X.DIV0 and rows[2] is None
    assert X.first_error(rows) == X.DIV0 and X.first_error([1, None]) is None
