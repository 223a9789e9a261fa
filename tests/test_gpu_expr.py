"""
Expressions on the device (@pytest.mark.gpu): expr_eval_kernel at stage —
tile and word borders, every input stream shape, every op, the lazy errors —
and every query surface that then reads a computed column as an ordinary
sparse I64 column. Every expected value comes from the tests' own evaluator
(exprutil: Python ints, None for NULL, a sentinel for the errors) over the
arrays the test wrote and postfix programs written here, never from the
library or its builder; every comparison is exact.
"""
import os

import numpy as np
import pytest

import citus_amd as ca
import exprutil as X
import shapes
from exprutil import c, k, o
from shapes import Col, SHAPES

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = X.I64_MIN, X.I64_MAX
PATH_GENERAL = 2
NULLP = [(X.NULL, 0, 0)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module", autouse=True)
def require_gpu():
    assert ca.gpu_available(), "MI355X required for these tests"


def check_column(res, e, results, rows=None):
    """select() output of computed column e against the evaluator's results"""
    vals, nulls = X.to_arrays(results)
    rows = np.ones(len(vals), bool) if rows is None else rows
    assert res["n_rows"] == int(rows.sum())
    assert np.array_equal(res["row_numbers"], np.nonzero(rows)[0])
    assert np.array_equal(res["nulls"][e], nulls[rows])
    assert np.array_equal(res["values"][e], vals[rows])


def run_clean(path, programs, columns, n):
    """stage `programs` (at most 8) and check each against the evaluator"""
    want = [X.evaluate_rows(p, columns, n) for p in programs]
    for w in want:
        assert X.first_error(w) is None
    with ca.Reader(path) as r, r.scan(exprs=programs) as s:
        s.stage()
        assert s.last_expr_ms() > 0
        es = [s.computed(i) for i in range(len(programs))]
        res = s.select(cols=es)
        for e, w in zip(es, want):
            check_column(res, e, w)
        for i, w in enumerate(want):
            present = [v for v in w if v is not None]
            assert s.expr_range(i) == ((min(present), max(present), len(present))
                                       if present else (0, 0, 0))
    return want


def stage_raises(path, programs, kind, index=0, preds=()):
    with ca.Reader(path) as r, r.scan(preds=preds, exprs=programs) as s:
        with pytest.raises(ca.CStripeError, match=rf"rc=-5.*expression {index}: {kind}"):
            s.stage()
        # the scan is left unstaged
        with pytest.raises(ca.CStripeError, match=r"rc=-4"):
            s.agg([(ca.AGG_COUNT_STAR, -1)])
        with pytest.raises(ca.CStripeError, match=r"rc=-4"):
            s.expr_range(0)


# ------------------------------------------------- tile, word and group borders
@pytest.mark.parametrize("mask", ["none", "third", "all"])
@pytest.mark.parametrize("g", [1, 63, 64, 65, 255, 256, 257, 513])
def test_group_sizes(g, mask, tmp_path):
    """two full chunk groups of g rows and a partial third: the per-group
    reset of the running base, the partial last word, the tile border"""
    n = 2 * g + (g + 1) // 2
    i = np.arange(n, dtype=np.int64)
    a = (i * 2654435761) % 2003 - 1000
    b = (i * 40503) % 17 - 8
    nulls = {"none": None, "third": (i % 3 == 0).astype(np.uint8),
             "all": np.ones(n, np.uint8)}[mask]
    path = str(tmp_path / "g.cs")
    ca.write_table(path, [("a", ca.I64, 0), ("b", ca.I64, 0)], [a, b],
                   nulls=None if nulls is None else [nulls, None], chunk_group_row_limit=g)
    columns = {0: (a, nulls), 1: (b, None)}
    programs = [o(X.ADD, o(X.MUL, c(0), k(3)), c(1)),            # NULL where a is
                o(X.SELECT, o(X.EQ, o(X.MOD, c(1), k(4)), k(0)), NULLP, c(1)),   # NULLs of its own
                o(X.COALESCE, c(0), o(X.NEG, c(1))),             # never NULL
                o(X.IS_NULL, c(0))]
    want = run_clean(path, programs, columns, n)
    if mask == "all":
        assert all(v is None for v in want[0])


def test_result_all_null_in_one_group(tmp_path):
    n, g = 900, 300
    i = np.arange(n, dtype=np.int64)
    a = i * 7 - 3000
    nulls = ((i >= 300) & (i < 600)).astype(np.uint8)             # all of group 1
    path = str(tmp_path / "g1.cs")
    ca.write_table(path, [("a", ca.I64, 0)], [a], nulls=[nulls], chunk_group_row_limit=g)
    want = run_clean(path, [o(X.SUB, c(0), k(1)), o(X.SELECT, o(X.LT, c(0), k(-2000)), c(0), NULLP)],
                     {0: (a, nulls)}, n)
    assert all(v is None for v in want[0][300:600]) and want[0][0] is not None
    assert all(v is None for v in want[1][300:]) and want[1][0] is not None


# ------------------------------------------------------------ input stream shapes
INT_SHAPES = [n for n, sh in SHAPES.items() if sh.ctype in (ca.I8, ca.I32, ca.I64)]


@pytest.mark.parametrize("name", INT_SHAPES)
def test_input_stream_shapes(name, tmp_path):
    sh = SHAPES[name]
    path = str(tmp_path / "shape.cs")
    shapes.write_shape(path, sh)
    present = sh.values if sh.nulls is None else sh.values[sh.nulls == 0]
    pv = set(int(v) for v in present)
    const = 1 if I64_MAX not in pv else -1 if I64_MIN not in pv else 0     # never wraps
    want = run_clean(path, [o(X.ADD, c(0), k(const))], {0: (sh.values, sh.nulls)}, sh.n)
    got_back = [None if v is None else v - const for v in want[0]]
    assert got_back == [None if (sh.nulls is not None and sh.nulls[i]) else int(sh.values[i])
                        for i in range(sh.n)]


# ------------------------------------------------------------------------ every op
def op_table(path):
    vals = [0, 1, -1, 7, -7, 2, None]
    rows = [(a, b) for a in vals for b in vals]
    n = len(rows)
    third = [None, 0, 1, 5]
    cols, out = [], {}
    for ci in range(3):
        col = [r[ci] for r in rows] if ci < 2 else [third[i % 4] for i in range(n)]
        v = np.array([0 if x is None else x for x in col], dtype=np.int64)
        nl = np.array([x is None for x in col], dtype=np.uint8)
        cols.append((v, nl))
        out[ci] = (v, nl)
    ca.write_table(path, [("a", ca.I64, 0), ("b", ca.I64, 0), ("c", ca.I64, 0)],
                   [x[0] for x in cols], nulls=[x[1] for x in cols], chunk_group_row_limit=20)
    return out, n


def test_every_op(tmp_path):
    path = str(tmp_path / "ops.cs")
    columns, n = op_table(path)
    a, b, cc = c(0), c(1), c(2)
    b_ok = o(X.NE, b, k(0))
    programs = [
        o(X.ADD, a, b), o(X.SUB, a, b), o(X.MUL, a, b), o(X.NEG, a),
        o(X.SELECT, b_ok, o(X.DIV, a, b), k(0)),                  # CASE guards the zero divisor
        o(X.SELECT, b_ok, o(X.MOD, a, b), k(0)),
        o(X.DIV, a, o(X.SELECT, b_ok, b, NULLP)),                 # a NULL divisor raises nothing
        o(X.MOD, a, o(X.SELECT, b_ok, b, NULLP)),
        o(X.LT, a, b), o(X.LE, a, b), o(X.GT, a, b), o(X.GE, a, b), o(X.EQ, a, b), o(X.NE, a, b),
        o(X.AND, a, b), o(X.OR, a, b), o(X.NOT, a), o(X.IS_NULL, a),
        o(X.COALESCE, a, b), o(X.COALESCE, a, o(X.COALESCE, b, k(-99))),
        o(X.SELECT, cc, a, b),                                    # a NULL condition takes b
        o(X.SELECT, o(X.IS_NULL, cc), NULLP, o(X.ADD, cc, a)),
        o(X.YEAR, o(X.MUL, a, k(1000))), o(X.YEAR, o(X.SUB, o(X.MUL, b, k(100000)), k(719528))),
        o(X.AND, o(X.LT, a, b), o(X.OR, o(X.IS_NULL, cc), o(X.GT, cc, k(0)))),
        NULLP, k(I64_MIN), [(X.CONST, 0, 5), (X.CONST, 0, 0), (X.AND, 0, 0)],
    ]
    for at in range(0, len(programs), ca.MAX_EXPRS):
        run_clean(path, programs[at:at + ca.MAX_EXPRS], columns, n)
    # the Kleene tables really are in there: rows with a, b over {0, 1, NULL}^2
    av, an = columns[0]
    bv, bn = columns[1]
    seen = {(None if an[i] else int(av[i]), None if bn[i] else int(bv[i])) for i in range(n)}
    assert {(x, y) for x in (0, 1, None) for y in (0, 1, None)} <= seen


def test_int64_extremes(tmp_path):
    """INT64_MIN / INT64_MAX operands: what stays inside int64 is exact, what
    leaves it is the error, whichever side it leaves on"""
    n = 70
    x = np.arange(n, dtype=np.int64)
    path = str(tmp_path / "ext.cs")
    ca.write_table(path, [("x", ca.I64, 0)], [x], chunk_group_row_limit=64)
    columns = {0: (x, None)}
    MIN, MAX = k(I64_MIN), k(I64_MAX)
    clean = [o(X.ADD, MAX, k(0)), o(X.ADD, MIN, MAX), o(X.SUB, k(-1), MAX), o(X.SUB, MIN, k(0)),
             o(X.MUL, MIN, k(1)), o(X.MUL, MAX, k(-1)), o(X.MUL, k(1 << 31), k(1 << 31)),
             o(X.NEG, MAX), o(X.DIV, MIN, k(1)), o(X.DIV, MIN, k(2)), o(X.DIV, MAX, k(-1)),
             o(X.MOD, MIN, k(-1)), o(X.MOD, MIN, k(10)), o(X.MOD, MAX, MIN), o(X.DIV, MIN, MAX),
             o(X.LT, MIN, MAX), o(X.GE, MIN, MAX), o(X.EQ, MAX, MAX),
             o(X.SUB, o(X.ADD, MAX, o(X.NEG, c(0))), MAX),       # row-dependent, at the edge
             o(X.ADD, MIN, c(0)), o(X.YEAR, k((1 << 31) - 1)), o(X.YEAR, k(-(1 << 31)))]
    for at in range(0, len(clean), ca.MAX_EXPRS):
        run_clean(path, clean[at:at + ca.MAX_EXPRS], columns, n)
    for prog, kind in ((o(X.ADD, MAX, k(1)), X.RANGE), (o(X.SUB, MIN, k(1)), X.RANGE),
                       (o(X.MUL, MIN, k(-1)), X.RANGE), (o(X.MUL, k(1 << 32), k(1 << 31)), X.RANGE),
                       (o(X.NEG, MIN), X.RANGE), (o(X.DIV, MIN, k(-1)), X.RANGE),
                       (o(X.DIV, MAX, k(0)), X.DIV0), (o(X.MOD, MIN, k(0)), X.DIV0),
                       (o(X.YEAR, k(1 << 31)), X.YEAR_RANGE),
                       (o(X.YEAR, k(-(1 << 31) - 1)), X.YEAR_RANGE)):
        assert X.first_error(X.evaluate_rows(prog, columns, n)) == kind
        stage_raises(path, [prog], kind)
    # the erring expression is named: clean ones in front of it
    stage_raises(path, [o(X.ADD, c(0), k(1)), o(X.DIV, c(0), k(0))], X.DIV0, index=1)


# -------------------------------------------------------------------------- errors
ERR_N, ERR_G = 250, 100                                          # groups of 100, 100, 50


def error_case(kind, at):
    """columns a, b whose row `at` is the only one on which `bad` errs, the
    program `bad`, and the condition `ok` that is false exactly there"""
    i = np.arange(ERR_N, dtype=np.int64)
    a = i * 13 - 900
    b = i % 9 + 1
    if kind == X.DIV0:
        b[at] = 0
        bad, ok = o(X.DIV, c(0), c(1)), o(X.NE, c(1), k(0))
    elif kind == X.RANGE:
        a[at] = I64_MAX
        bad, ok = o(X.ADD, c(0), c(1)), o(X.LT, c(0), k(I64_MAX))
    else:
        a[at] = 1 << 31
        bad, ok = o(X.YEAR, c(0)), o(X.LT, c(0), k(1 << 31))
    return a, b, bad, ok


@pytest.mark.parametrize("at", [0, ERR_N - 1, 150])
@pytest.mark.parametrize("kind", [X.DIV0, X.RANGE, X.YEAR_RANGE])
def test_one_erring_row(kind, at, tmp_path):
    a, b, bad, ok = error_case(kind, at)
    grp = np.arange(ERR_N, dtype=np.int64) // ERR_G
    path = str(tmp_path / "err.cs")
    ca.write_table(path, [("a", ca.I64, 0), ("b", ca.I64, 0), ("g", ca.I64, 0)], [a, b, grp],
                   chunk_group_row_limit=ERR_G)
    columns = {0: (a, None), 1: (b, None)}
    res = X.evaluate_rows(bad, columns, ERR_N)
    assert [i for i, r in enumerate(res) if X.is_err(r)] == [at] and res[at].kind == kind
    stage_raises(path, [bad], kind)
    # the same row guarded: by SELECT, by AND / OR short-circuit, by a NULL operand
    field = c(1) if kind == X.DIV0 else c(0)
    nulled = o(X.SELECT, ok, field, NULLP)
    guarded = [o(X.SELECT, ok, bad, k(0)),
               o(X.AND, ok, o(X.GT, bad, k(3))),
               o(X.OR, o(X.NOT, ok), o(X.GT, bad, k(3))),
               o(X.DIV, c(0), nulled) if kind == X.DIV0 else
               o(X.ADD, nulled, c(1)) if kind == X.RANGE else o(X.YEAR, nulled)]
    want = run_clean(path, guarded, columns, ERR_N)
    assert want[0][at] == 0 and want[1][at] == 0 and want[2][at] == 1 and want[3][at] is None
    # an unguarded AND evaluates left to right: the error on the left is raised
    stage_raises(path, [o(X.AND, o(X.GT, bad, k(3)), ok)], kind)
    # a chunk group removed by min/max pruning is not evaluated
    gi = at // ERR_G
    pred = (2, ca.PRED_LT, gi) if gi else (2, ca.PRED_GT, 0)
    keep = (grp < gi) if gi else (grp > 0)
    with ca.Reader(path) as r, r.scan(preds=[pred], exprs=[bad]) as s:
        assert s.chunk_groups_filtered == 3 - len(set(grp[keep].tolist()))
        s.stage()
        check_column(s.select(cols=[s.computed(0)]), s.computed(0),
                     [0 if X.is_err(v) else v for v in res], keep)


# -------------------------------------------------------------- seeded differential
def test_seeded_differential(tmp_path):
    columns = X.diff_columns()
    programs = X.diff_programs()
    assert len(programs) == 200 and all(X.stack_depth(p) <= 4 for p in programs)
    path = str(tmp_path / "diff.cs")
    ca.write_table(path, [("a", ca.I64, 0), ("b", ca.I64, 0), ("c", ca.I64, 0)],
                   [columns[i][0] for i in range(3)], nulls=[columns[i][1] for i in range(3)],
                   chunk_group_row_limit=128)
    results = [X.evaluate_rows(p, columns, X.DIFF_ROWS) for p in programs]
    kinds = [X.first_error(r) for r in results]
    clean = [p for p, kd in zip(programs, kinds) if kd is None]
    erring = [(p, kd) for p, kd in zip(programs, kinds) if kd is not None]
    assert len(clean) >= 60 and len(erring) >= 30           # a condition on the seed
    assert {kd for _, kd in erring} == {X.DIV0, X.RANGE, X.YEAR_RANGE}
    for at in range(0, len(clean), ca.MAX_EXPRS):
        run_clean(path, clean[at:at + ca.MAX_EXPRS], columns, X.DIFF_ROWS)
    with ca.Reader(path) as r:
        for p, kd in erring:
            with r.scan(exprs=[p]) as s:
                with pytest.raises(ca.CStripeError, match=rf"expression 0: {kd}"):
                    s.stage()


# -------------------------------------------------------------------- every surface
SN, SG = 2900, 1000
KC, VC, DC, GC = 0, 1, 2, 3                # table columns
L0 = 4                                     # the lookup's derived column
E0, E1, E2, E3, E4 = 5, 6, 7, 8, 9         # computed columns


def surface():
    i = np.arange(SN, dtype=np.int64)
    kk = (i * 48271) % 997 - 300
    knulls = (i % 3 == 0).astype(np.uint8)
    v = (i * 31 + 7) % 5003 - 2500
    d = ((i * 37) % 3000 + 7000).astype(np.int32)             # 1989 .. 1997
    g = shapes.key_column(SN)
    keys = list(range(-300, 697, 3))
    pay = [x * x - 1000 for x in keys]
    lk = {x: p for x, p in zip(keys, pay)}
    lv = np.array([lk.get(int(x), 0) for x in kk], dtype=np.int64)
    ln = np.array([knulls[j] or int(kk[j]) not in lk for j in range(SN)], dtype=np.uint8)
    programs = [
        o(X.SUB, o(X.MUL, c(VC), k(3)), c(KC)),                # E0: negative values, NULLs
        o(X.LT, c(VC), c(KC)),                                 # E1: column versus column
        o(X.YEAR, c(DC)),                                      # E2
        o(X.ADD, c(L0), c(VC)),                                # E3: reads the derived column
        o(X.SELECT, o(X.EQ, o(X.MOD, c(VC), k(7)), k(0)), NULLP,
          o(X.SUB, o(X.MOD, c(VC), k(5)), k(2))),              # E4: a few keys, some negative
    ]
    columns = {KC: (kk, knulls), VC: (v, None), DC: (d, None), GC: (g, None), L0: (lv, ln)}
    return columns, programs, keys, pay


@pytest.fixture(scope="module")
def surf(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("exprsurf") / "surf.cs")
    columns, programs, keys, pay = surface()
    ca.write_table(path, [("k", ca.I64, 0), ("v", ca.I64, 0), ("d", ca.I32, 0), ("g", ca.I8, 0)],
                   [columns[j][0] for j in range(4)], nulls=[columns[KC][1], None, None, None],
                   chunk_group_row_limit=SG)
    cols = [Col(*columns[j]) for j in range(5)]
    results = []
    for p in programs:
        res = X.evaluate_rows(p, columns, SN)
        assert X.first_error(res) is None
        results.append(res)
        cols.append(Col(*X.to_arrays(res)))
    assert min(v for v in results[0] if v is not None) < 0
    assert min(v for v in results[4] if v is not None) < 0 and None in results[4]
    assert len({v for v in results[2]}) >= 8 and 0 < sum(v == 1 for v in results[1]) < SN
    return path, cols, programs, results, ca.Lookup(KC, keys, [pay])


def hashed_dict(res, n_keys):
    out = {}
    for gi in range(res["n_groups"]):
        key = tuple(None if res["key_nulls"][kx][gi] else int(res["keys"][kx][gi])
                    for kx in range(n_keys))
        out[key] = res["partials"][gi]
    assert len(out) == res["n_groups"]
    return out


def group_mask(cols, key_cols, key, rows):
    m = rows.copy()
    for col, kv in zip(key_cols, key):
        m &= ~cols[col].present if kv is None else (cols[col].present & (cols[col].wide == kv))
    return m


def check_group(ps, cols, aggs, m, what):
    for ai, a in enumerate(aggs):
        p = ps[ai]
        got = {"count": int(p["count"]), "is_null": bool(p["is_null"]),
               "i128": ca.partial_i128(p), "f64": float(p["f64"])}
        shapes.check_partial(got, shapes.expect_agg(cols, a, m), a[0], f"{what} {a}")


def check_hashed(res, key_cols, cols, aggs, rows, what):
    got = hashed_dict(res, len(key_cols))
    want_keys = {tuple(None if not cols[col].present[i] else int(cols[col].wide[i])
                       for col in key_cols) for i in np.nonzero(rows)[0]}
    assert set(got) == want_keys, what
    for key, ps in got.items():
        check_group(ps, cols, aggs, group_mask(cols, key_cols, key, rows), f"{what} {key}")


def test_surfaces_aggregates_and_keys(surf):
    path, cols, programs, results, lk = surf
    every = np.ones(SN, bool)
    aggs = shapes.with_one(cols, [
        (ca.AGG_COUNT_STAR, -1), (ca.AGG_SUM_I64, E0), (ca.AGG_MIN_I64, E0), (ca.AGG_MAX_I64, E0),
        (ca.AGG_COUNT_COL, E0), (ca.AGG_SUM_PROD_I64, E0, VC), (ca.AGG_SUM_PROD_I64, VC, E3),
        (ca.AGG_SUM_I64, E1), (ca.AGG_COUNT_COL, E4), (ca.AGG_SUM_I64, VC)])
    with ca.Reader(path) as r, r.scan(cols_mask=0b1111, lookups=[lk], exprs=programs) as s:
        assert s.column_count() == 10 and s.derived(0, 0) == L0
        assert [s.computed(i) for i in range(5)] == [E0, E1, E2, E3, E4]
        s.stage()
        assert s.last_expr_ms() > 0
        for i, res in enumerate(results):
            present = [v for v in res if v is not None]
            assert s.expr_range(i) == (min(present), max(present), len(present))
        parts = s.agg(aggs)
        assert s.last_agg_path == PATH_GENERAL
        for a, p in zip(aggs, parts):
            shapes.check_partial(p, shapes.expect_agg(cols, a, every), a[0], f"agg {a}")
        sel = s.select(cols=[E0, E1, E2, E3, E4, VC])
        for e, res in zip((E0, E1, E2, E3, E4), results):
            check_column(sel, e, res)
        assert np.array_equal(sel["values"][VC], cols[VC].values)
        # hashed GROUP BY year(d), and by a computed key with negative values and NULLs
        h_aggs = [aggs[0], aggs[1], aggs[9]]
        check_hashed(s.agg_hashed(h_aggs, [E2], 64), [E2], cols, h_aggs, every, "hashed year")
        res = s.agg_hashed(h_aggs, [E4], 64)
        check_hashed(res, [E4], cols, h_aggs, every, "hashed E4")
        assert any(bool(x) for x in res["key_nulls"][0])
        check_hashed(s.agg_hashed(h_aggs, [GC, E4], 256), [GC, E4], cols, h_aggs, every,
                     "hashed g,E4")
        # GROUP BY E4 ORDER BY E4 DESC LIMIT 4: NULLs last, as the flags say
        top = s.agg_hashed_topn(h_aggs, [E4], 64, [("key", 0, "desc")], 4)
        want = sorted({v for v in results[4] if v is not None}, reverse=True)[:4]
        assert top["n_groups"] == 4
        assert [int(x) for x in top["keys"][0][:4]] == want
        assert not any(bool(x) for x in top["key_nulls"][0][:4])
        for gi, kv in enumerate(want):
            check_group(top["partials"][gi], cols, h_aggs, group_mask(cols, [E4], (kv,), every),
                        f"topn group {kv}")
        # ORDER BY E0 DESC NULLS FIRST LIMIT 50
        t = s.select_topn([(E0, "desc", "first")], 50, cols=[E0, VC])
        idx = np.arange(SN)
        isnull = ~cols[E0].present
        order = idx[np.lexsort((idx, -cols[E0].wide, (~isnull).astype(np.int64)))][:50]
        assert np.array_equal(t["row_numbers"], order)
        assert np.array_equal(t["values"][E0], cols[E0].wide[order])
        assert np.array_equal(t["nulls"][E0], isnull[order].astype(np.uint8))
        # refused: grouped keys
        with pytest.raises(ca.CStripeError, match=r"rc=-5"):
            s.agg_grouped(aggs[:1], [E4])
        # a restage rebuilds everything: identical bytes
        s.stage()
        again = s.select(cols=[E0, E1, E2, E3, E4, VC])
        for e in (E0, E1, E2, E3, E4, VC):
            assert again["values"][e].tobytes() == sel["values"][e].tobytes()
            assert again["nulls"][e].tobytes() == sel["nulls"][e].tobytes()
        assert again["row_numbers"].tobytes() == sel["row_numbers"].tobytes()
        assert s.expr_range(0)[2] == int(cols[E0].present.sum())


def test_surfaces_predicates(surf):
    path, cols, programs, results, lk = surf
    aggs = shapes.with_one(cols, [(ca.AGG_COUNT_STAR, -1), (ca.AGG_SUM_I64, E0),
                                  (ca.AGG_SUM_I64, VC)])
    cases = [
        [(E1, ca.PRED_EQ, 1)],                                   # v < k, column versus column
        [(E1, ca.PRED_EQ, 0)],
        [(E0, ca.PRED_GT, 1000), (E2, ca.PRED_LE, 1993)],
        [(E1, ca.PRED_EQ, 1, 7), (VC, ca.PRED_LT, -2000, 7)],    # in an or_group with a table column
        [(E4, ca.PRED_LT, 0, 3), (E3, ca.PRED_GT, 50000, 3), (GC, ca.PRED_EQ, 2)],
    ]
    with ca.Reader(path) as r:
        for preds in cases:
            groups = {}
            for n_, p in enumerate(preds):
                groups.setdefault(p[3] if len(p) > 3 else -1 - n_, []).append(p)
            want = np.ones(SN, bool)
            for members in groups.values():
                m = np.zeros(SN, bool)
                for p in members:
                    m |= shapes.pred_mask(cols[p[0]], p[1], p[2])
                want &= m
            assert 0 < want.sum() < SN, preds
            with r.scan(cols_mask=0b1111, preds=preds, lookups=[lk], exprs=programs) as s:
                assert s.chunk_groups_filtered == 0
                s.stage()
                assert s.select_count() == int(want.sum())
                sel = s.select(cols=[E0, E1, VC])
                check_column(sel, E0, results[0], want)
                check_column(sel, E1, results[1], want)
                for a, p in zip(aggs, s.agg(aggs)):
                    shapes.check_partial(p, shapes.expect_agg(cols, a, want), a[0],
                                         f"{preds} {a}")
                assert s.last_agg_path == PATH_GENERAL


# --------------------------------------------------------------------- golden pins
QTY, EXT, DISC, TAX, SHIP, RF, LS = 1, 2, 3, 4, 5, 6, 7


@pytest.mark.parametrize("variant", ["none", "lz4", "zstd"])
def test_golden_q1_charge(variant, expected):
    path = os.path.join(GOLDEN, f"lineitem12k_{variant}.cs")
    q1 = expected["q1"]
    charge = o(X.MUL, o(X.MUL, c(EXT), o(X.SUB, k(100), c(DISC))), o(X.ADD, k(100), c(TAX)))
    with ca.Reader(path) as r, \
            r.scan(cols_mask=(1 << RF) | (1 << LS), preds=[(SHIP, ca.PRED_LE, q1["shipdate_le"])],
                   exprs=[charge]) as s:
        s.stage()
        E = s.computed(0)
        assert E == 8
        res = s.agg_hashed([(ca.AGG_SUM_I64, E), (ca.AGG_SUM_DISC_TAX_I64, EXT, DISC, TAX, 100),
                            (ca.AGG_COUNT_STAR, -1)], [RF, LS], 64)
        got = hashed_dict(res, 2)
    rf = expected["flag_codes"]["returnflag"]
    ls = expected["flag_codes"]["linestatus"]
    assert len(got) == len(q1["groups"])
    for key, vals in q1["groups"].items():
        a, b = key.split(",")
        ps = got[(rf[a], ls[b])]
        assert ca.partial_i128(ps[0]) == ca.partial_i128(ps[1]) == vals[3]
        assert int(ps[2]["count"]) == vals[4]


@pytest.mark.parametrize("variant", ["none", "lz4", "zstd"])
def test_golden_q6_revenue(variant, expected):
    path = os.path.join(GOLDEN, f"lineitem12k_{variant}.cs")
    q6 = expected["q6"]
    cond = o(X.AND, o(X.AND, o(X.AND, o(X.AND,
                                        o(X.GE, c(SHIP), k(q6["shipdate_ge"])),
                                        o(X.LT, c(SHIP), k(q6["shipdate_lt"]))),
                                o(X.GE, c(DISC), k(5))), o(X.LE, c(DISC), k(7))),
             o(X.LT, c(QTY), k(2400)))
    revenue = o(X.SELECT, cond, o(X.MUL, c(EXT), c(DISC)), k(0))
    with ca.Reader(path) as r, r.scan(exprs=[revenue]) as s:
        s.stage()
        p = s.agg([(ca.AGG_SUM_I64, s.computed(0)), (ca.AGG_COUNT_COL, s.computed(0))])
        assert p[0].i128 == q6["revenue_scale4"]
        assert p[1].count == expected["n_rows"]
