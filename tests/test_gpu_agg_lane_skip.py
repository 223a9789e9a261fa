"""multi_agg_kernel_ov: per-lane operand loads, 32-bit predicates, narrow sums.

Same conventions as test_gpu_agg_overlap.py, whose helpers are used here:
every test writes its own small table, reads the footer back to pin the
stream shapes on disk, asserts Scan.last_agg_path and compares with exact
Python-int results computed from the arrays that were written.

What the body does differently for these inputs:
  * the operand-only slots are loaded only by lanes that hold a passing row
    (a lane holds 8 consecutive rows of a chunk group, 4 in the unspecialised
    instance; the lane of rows 0.. also fetches the stream's first rows from
    their own offsets),
  * a predicate is reduced per chunk group to one unsigned 32-bit range test
    of the row's low word, or to a constant where the constant's high word
    differs from the chunk group's,
  * SUM_PROD of a specialised instance folds a row group in one u64 when
    both operands are their low words and their widths add to at most 61
    bits; every other sum, and the unspecialised instance, folds in 128 bits
    as before. The product cases below sit on both sides of that rule and on
    the sides of the wider one (non-negative factors, `one` included) that
    any narrow fold of SUM_DISC / SUM_DISC_TAX would have to respect.
"""
import numpy as np
import pytest

import citus_amd as ca
import futil
import test_gpu_agg_overlap as ovt

pytestmark = pytest.mark.gpu

PATH_NONE, PATH_OV = ovt.PATH_NONE, ovt.PATH_OV
LT, LE, GT, GE, EQ, NE = ovt.LT, ovt.LE, ovt.GT, ovt.GE, ovt.EQ, ovt.NE
ALL_OPS = (LT, LE, GT, GE, EQ, NE)
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
COMPS = [ca.COMP_LZ4, ca.COMP_ZSTD]


def p_modes(comp):
    """(P(L) base, CONST) stream modes of a codec"""
    if comp == ca.COMP_ZSTD:
        return futil.SEGMODE_ZRP_BASE, futil.SEGMODE_ZR_CONST
    return futil.SEGMODE_P_BASE, futil.SEGMODE_CONST


def assert_modes(path, col, comp, Ls=(1, 2, 3, 4), const=False):
    """every chunk group of the column is P(L), L in Ls, of this codec (or
    CONST): neither another codec's shape nor a fallback shape"""
    P, K = p_modes(comp)
    want = {K} if const else {P | L for L in Ls}
    got = set(ovt.col_modes(path, col))
    assert got and got <= want, f"col {col}: modes {got}, wanted within {want}"


# ------------------------------------------------- 1. single passing row

N1, CG1 = 8192, 4096
ROWS1 = [0, 1, 2, 7, 8, 9, 511, 512, 2047, 2048, 4095, CG1 + 0, CG1 + 1]
PAIRS1 = [(7, 16), (8, 15)]


def operand_column(kind, n):
    """a distinct value per row where the width allows it (L >= 2); for L = 1
    no two rows closer than 251 apart share a value; CONST is one value.
    L = 1 and 3 have no high bytes (the narrow fold of the Q6 instance),
    L = 2 and 4 do (its 128-bit fold)."""
    i = np.arange(n, dtype=np.int64)
    if kind == "const":
        return np.full(n, 123457, dtype=np.int64)
    L = int(kind)
    if L == 1:
        v = (i * 7) % 251 + 2
    elif L == 2:
        v = (i * 40503) % (1 << 16)                   # bijective in i
    else:
        v = i * 257 + 11
    # force exactly L in both chunk groups, on rows no case below selects
    v[3::CG1] = (1 << (8 * L)) - 1
    v[4::CG1] = 0
    return v + {1: 0, 2: 5 << 16, 3: 0, 4: 3 << 40}[L]


@pytest.mark.parametrize("kind", ["1", "2", "3", "4", "const"])
@pytest.mark.parametrize("comp", COMPS)
def test_single_passing_row(tmp_path, comp, kind):
    """exactly one row of two 4096-row chunk groups passes — in the lane of
    rows 0/1, at lane, wave and tile edges, in the second group — and then
    two rows whose lanes share a 128-B line with a lane that does not pass;
    through the Q6 instance, count(*) under one predicate and the
    unspecialised instance. A wrong row or a stale register gives a wrong
    sum: the operand differs from row to row."""
    n = N1
    rng = np.random.default_rng(17)
    i = np.arange(n, dtype=np.int64)
    # A selects rows by value; it is a permutation spread over both chunk
    # groups, so min/max pruning never removes a group and both are walked
    A = (1 << 20) + 2 * ((i * 4099) % n)
    A[5::CG1] = (1 << 20) - 2          # every selected value lies strictly
    A[6::CG1] = (1 << 20) + 2 * n      # inside both groups' [min, max]
    B = rng.integers(1, 200, n, dtype=np.int64)                 # L=1, predicate + operand
    C = 70000 + rng.integers(0, 60000, n, dtype=np.int64)       # L=2, predicate
    D = operand_column(kind, n)                                 # operand only
    cols = [A, B, C, D]
    path = ovt.write(tmp_path / "t.cs", cols, comp=comp, chunk_group_row_limit=CG1,
                     stripe_row_limit=4 * CG1)
    assert len(ovt.col_modes(path, 0)) == 2
    for c in (0, 1, 2):
        assert_modes(path, c, comp)
    if kind == "const":
        assert_modes(path, 3, comp, const=True)
    else:
        assert_modes(path, 3, comp, Ls=(int(kind),))
    assert ovt.eligible(path, [0, 1, 2, 3])

    for r in ROWS1:
        v = int(A[r])
        what = f"row {r}"
        p, a = ovt.q6_query(v, v + 1, -5, 1000, 1 << 40)
        assert ovt.check(path, cols, p, a, want_path=PATH_OV, what=what + " q6") == 0
        p, a = ovt.any_query(v, v + 1)
        ovt.check(path, cols, p, a, want_path=PATH_OV, what=what + " any")
        ovt.check(path, cols, [(0, EQ, v)], [(ca.AGG_COUNT_STAR, -1)],
                  want_path=PATH_OV, what=what + " count")
    for r0, r1 in PAIRS1:
        v0, v1 = int(A[r0]), int(A[r1])
        what = f"rows {r0}+{r1}"
        _, a = ovt.q6_query(0, 0, 0, 0, 0)
        p = [(0, EQ, v0, 1), (0, EQ, v1, 1), (1, GE, -5), (1, LE, 1000), (2, LT, 1 << 40)]
        ovt.check(path, cols, p, a, want_path=PATH_OV, what=what + " q6")
        _, a = ovt.any_query(0, 0)
        ovt.check(path, cols, [(0, EQ, v0, 1), (0, EQ, v1, 1)], a,
                  want_path=PATH_OV, what=what + " any")
        ovt.check(path, cols, [(0, EQ, v0, 1), (0, EQ, v1, 1)], [(ca.AGG_COUNT_STAR, -1)],
                  want_path=PATH_OV, what=what + " count")


# ------------------------------------------------- 2. selectivity sweep

# [lo, hi) over S = 2 * uniform[0, 4096): S is even, so 4097 is inside
# [min, max] of every chunk group (never pruned) and matches no row
SWEEP = {"0": (4097, 4098), "1/4096": (0, 0),        # one value that occurs, below
         "1/512": (2 * 800, 2 * 800 + 16), "2%": (0, 164),
         "50%": (0, 4096), "100%": (0, 8192)}


@pytest.fixture(scope="module")
def sweep_table(tmp_path_factory):
    """three chunk groups of 5003, 5003 and 1237 rows: 2048-row tiles end in
    one of 907 rows, and every group's last row group is shorter than 8"""
    cg, n = 5003, 2 * 5003 + 1237
    assert cg % 2048 and cg % 8 and (n % cg) % 8
    rng = np.random.default_rng(23)
    S = 2 * rng.integers(0, 4096, n, dtype=np.int64)            # L=2
    B = rng.integers(0, 11, n, dtype=np.int64)                  # L=1
    C = rng.integers(1, 51, n, dtype=np.int64) * 100            # L=2
    D = rng.integers(90000, 10500000, n, dtype=np.int64)        # L=3
    cols = [S, B, C, D]
    path = ovt.write(tmp_path_factory.mktemp("sweep") / "t.cs", cols,
                     chunk_group_row_limit=cg, stripe_row_limit=4 * cg)
    return path, cols


@pytest.mark.parametrize("frac", list(SWEEP))
def test_selectivity_sweep(sweep_table, frac):
    path, cols = sweep_table
    for c in range(4):
        assert_modes(path, c, ca.COMP_LZ4)
    assert ovt.eligible(path, [0, 1, 2, 3])
    assert len(ovt.col_modes(path, 0)) == 3
    lo, hi = SWEEP[frac]
    if frac == "1/4096":                       # a value that does occur
        lo = int(cols[0][100])
        hi = lo + 2
    got = int(((cols[0] >= lo) & (cols[0] < hi)).sum())
    n = len(cols[0])
    f = {"0": 0, "1/4096": 1 / 4096, "1/512": 1 / 512, "2%": 0.02, "50%": 0.5,
         "100%": 1}[frac]
    assert got == f * n if f in (0, 1) else 0 < got and f * n / 3 <= got <= 3 * f * n + 3
    p, a = ovt.q6_query(lo, hi, 0, 10, 1 << 30)
    assert ovt.check(path, cols, p, a, want_path=PATH_OV, what=f"{frac} q6") == 0
    p, a = ovt.any_query(lo, hi)
    assert ovt.check(path, cols, p, a, want_path=PATH_OV, what=f"{frac} any") == 0


# ------------------------------------------------- 3. predicate edges

RANGES = {
    "2^31": ((1 << 31) - 5, (1 << 31) + 5),
    "2^32-": ((1 << 32) - 300, (1 << 32) - 1),
    "2^32+": (1 << 32, (1 << 32) + 1000),
    "neg": (-1000, -1),
    "-2^31": (-(1 << 31) - 5, -(1 << 31) + 5),
    "2^62": ((1 << 62) + 7, (1 << 62) + (1 << 31) + 9),
    "min": (I64_MIN, I64_MIN + 70000),
    "max": (I64_MAX - 70000, I64_MAX),
    "u32": (0, (1 << 32) - 1),
    "const": (424242, 424242),
}
CG3 = 600                       # more than one wave of the R=8 instances


def range_values(rng, lo, hi, n):
    """uniform over [lo, hi] with both ends present"""
    v = lo + rng.integers(0, hi - lo + 1, n, dtype=np.int64)
    v[0], v[1 % n] = lo, hi
    return v


def refuted(op, ival, mn, mx):
    """min/max chunk-group pruning: no value in [mn, mx] passes"""
    return {LT: mn >= ival, LE: mn > ival, GT: mx <= ival, GE: mx < ival,
            EQ: ival < mn or ival > mx, NE: mn == mx == ival}[op]


def survivors(X, cg, op, ival):
    return sum(not refuted(op, ival, int(X[g:g + cg].min()), int(X[g:g + cg].max()))
               for g in range(0, len(X), cg))


def edge_ivals(X):
    """below the range, its minimum, an interior value, its maximum, above
    the range (clamped to int64), and the fixed constants"""
    mn, mx = int(X.min()), int(X.max())
    interior = int(np.sort(X)[len(X) // 2])
    return [max(mn - 1, I64_MIN), mn, interior, mx, min(mx + 1, I64_MAX),
            0, -1, 1 << 31, 1 << 32, I64_MIN, I64_MAX]


def edge_table(tmp_path, comp, names):
    """X holds one range per chunk group, in the order of names; K alternates
    0/1 (the live first member of the OR groups); B, C, D give the Q6 shape
    its other slots"""
    rng = np.random.default_rng(29)
    X = np.concatenate([range_values(rng, *RANGES[nm], CG3) for nm in names])
    n = len(X)
    K = np.arange(n, dtype=np.int64) % 2
    B = rng.integers(0, 11, n, dtype=np.int64)
    C = rng.integers(1, 51, n, dtype=np.int64) * 100
    D = rng.integers(90000, 10500000, n, dtype=np.int64)
    cols = [X, B, C, D, K]
    path = ovt.write(tmp_path / "t.cs", cols, comp=comp, chunk_group_row_limit=CG3,
                     stripe_row_limit=20 * CG3)
    P, Kc = p_modes(comp)
    modes = ovt.col_modes(path, 0)
    assert len(modes) == len(names)
    for nm, m in zip(names, modes):
        assert m == Kc if nm == "const" else m in {P | L for L in (2, 3, 4)}, (nm, hex(m))
    for c in (1, 2, 3, 4):
        assert_modes(path, c, comp)
    assert ovt.eligible(path, [0, 1, 2, 3, 4])
    return path, cols


def run_edges(path, cols):
    """every op x every constant, three ways: alone under count(*) (the count
    instance), as the second member of an OR group behind a predicate that
    holds on every other row (the unspecialised instance, values checked),
    and as the first predicate of the Q6 shape (the Q6 instance).

    last_agg_path is 4 wherever the kernel runs at all. A predicate that
    min/max pruning refutes in every chunk group (x < INT64_MIN, say) leaves
    nothing to launch and the scan reports path 0 by definition; the test
    derives which of the two it must be from the written values, so neither
    case is skipped and a fallback body cannot pass for either. Behind the OR
    member no chunk group is ever refuted: path 4 unconditionally."""
    X = cols[0]
    interior = edge_ivals(X)[2]
    n_ov = 0
    for op in ALL_OPS:
        for ival in edge_ivals(X):
            what = f"op {op} ival {ival}"
            alive = survivors(X, CG3, op, ival) > 0
            want = PATH_OV if alive else PATH_NONE
            n_ov += alive
            ovt.check(path, cols, [(0, op, ival)], [(ca.AGG_COUNT_STAR, -1)],
                      want_path=want, what=what + " solo")
            ovt.check(path, cols, [(4, EQ, 1, 1), (0, op, ival, 1)],
                      [(ca.AGG_SUM_I64, 0), (ca.AGG_COUNT_STAR, -1),
                       (ca.AGG_MIN_I64, 0), (ca.AGG_MAX_I64, 0)],
                      want_path=PATH_OV, what=what + " or")
            alive6 = any(not refuted(op, ival, int(X[g:g + CG3].min()), int(X[g:g + CG3].max()))
                         and not refuted(NE, interior, int(X[g:g + CG3].min()),
                                         int(X[g:g + CG3].max()))
                         for g in range(0, len(X), CG3))
            p = [(0, op, ival), (0, NE, interior), (1, GE, 0), (1, LE, 10), (2, LT, 1 << 30)]
            a = [(ca.AGG_SUM_PROD_I64, 3, 1), (ca.AGG_COUNT_STAR, -1)]
            ovt.check(path, cols, p, a, want_path=PATH_OV if alive6 else PATH_NONE,
                      what=what + " q6")
    # the solo form did reach the kernel for a good part of the constants
    assert n_ov >= 20


@pytest.mark.parametrize("name", list(RANGES))
@pytest.mark.parametrize("comp", COMPS)
def test_predicate_edges(tmp_path, comp, name):
    """one value range in every chunk group of the column"""
    path, cols = edge_table(tmp_path, comp, [name, name])
    run_edges(path, cols)


@pytest.mark.parametrize("comp", COMPS)
def test_predicate_edges_mixed(tmp_path, comp):
    """all ranges in one column, one per chunk group: hval, L and the
    constant/compare decision change from work item to work item"""
    path, cols = edge_table(tmp_path, comp, list(RANGES))
    run_edges(path, cols)


# ------------------------------------------------- 4. product edges

def product_table(tmp_path, B, D, C=None, comp=ca.COMP_LZ4, name="t.cs"):
    n = len(B)
    A = (1 << 20) + 2 * np.arange(n, dtype=np.int64)
    if C is None:
        C = np.random.default_rng(1).integers(0, 60000, n, dtype=np.int64)
    cols = [A, B, C, D]
    path = ovt.write(tmp_path / name, cols, comp=comp, chunk_group_row_limit=1000)
    for c in range(4):
        assert_modes(path, c, comp)
    assert ovt.eligible(path, [0, 1, 2, 3])
    return path, cols


def all_pass(cols):
    A = cols[0]
    return int(A[0]), int(A[-1]) + 1


def check_products(path, cols, one, what, preds=None):
    """every sum kind over (D, B[, C]) on the unspecialised instance, and
    sum(D*B) on the Q6 instance; every row passes unless preds are given"""
    lo, hi = all_pass(cols)
    aggs = [(ca.AGG_SUM_PROD_I64, 3, 1), (ca.AGG_SUM_DISC_I64, 3, 1, -1, one),
            (ca.AGG_SUM_DISC_TAX_I64, 3, 1, 2, one), (ca.AGG_SUM_I64, 3)]
    ovt.check(path, cols, preds or [(0, GE, lo), (0, LT, hi)], aggs,
              want_path=PATH_OV, what=what + " any")
    p, a = ovt.q6_query(lo, hi, I64_MIN, I64_MAX, I64_MAX)
    if preds:
        p = preds
    ovt.check(path, cols, p, a, want_path=PATH_OV, what=what + " q6")
    return ovt.expected(cols, preds or [(0, GE, lo), (0, LT, hi)], aggs)


N4 = 2_037


def test_product_wide_sum_exceeds_64_bits(tmp_path):
    """both operands in [2^32-300, 2^32-1], every row passing: eight products
    exceed 2^64, the 128-bit fold must be taken"""
    rng = np.random.default_rng(31)
    B = range_values(rng, (1 << 32) - 300, (1 << 32) - 1, N4)
    D = range_values(rng, (1 << 32) - 300, (1 << 32) - 1, N4)
    path, cols = product_table(tmp_path, B, D)
    exp = check_products(path, cols, 100, "2^32-")
    assert exp[0][0] > N4 * ((1 << 63) - (1 << 42))
    assert sum(int(x) * int(y) for x, y in zip(D[:8], B[:8])) > 1 << 64


def test_product_full_width_low_words(tmp_path):
    """L = 4 with hval 0 on both sides, most values near 2^32: the widths
    alone (32 + 32 > 61) must choose the 128-bit fold"""
    rng = np.random.default_rng(37)
    B = range_values(rng, (1 << 32) - 300, (1 << 32) - 1, N4)
    D = range_values(rng, (1 << 32) - 300, (1 << 32) - 1, N4)
    B[5::97] = rng.integers(0, 1 << 20, len(B[5::97]))
    D[7::89] = rng.integers(0, 1 << 20, len(D[7::89]))
    B[0] = D[0] = 0
    B[-1], D[-1] = 3, 5                        # L = 4 in the short last group too
    path, cols = product_table(tmp_path, B, D)
    P, _ = p_modes(ca.COMP_LZ4)
    assert set(ovt.col_modes(path, 1)) == set(ovt.col_modes(path, 3)) == {P | 4}
    exp = check_products(path, cols, (1 << 31) + 12345, "L4xL4")
    assert exp[0][0] > 1 << 72


def test_product_hval_nonzero(tmp_path):
    """one operand in [2^32, 2^32+1000]: its low word is not its value"""
    rng = np.random.default_rng(41)
    B = rng.integers(0, 200, N4, dtype=np.int64)
    D = range_values(rng, 1 << 32, (1 << 32) + 1000, N4)
    path, cols = product_table(tmp_path, B, D)
    check_products(path, cols, 1000, "hval D")
    path, cols = product_table(tmp_path, D, B, name="u.cs")
    check_products(path, cols, (1 << 32) + 2000, "hval B")


def test_product_negative_operand(tmp_path):
    rng = np.random.default_rng(43)
    B = rng.integers(0, 200, N4, dtype=np.int64)
    D = range_values(rng, -70000, -1, N4)
    path, cols = product_table(tmp_path, B, D)
    exp = check_products(path, cols, 1000, "neg D")
    assert exp[0][0] < 0
    path, cols = product_table(tmp_path, D, B, name="u.cs")
    check_products(path, cols, 1000, "neg B")


def test_sum_disc_negative_factor(tmp_path):
    """b > one on most rows, and on all of them: one - b < 0. one = 255 is
    the smallest for which no b of an L = 1 column exceeds it"""
    rng = np.random.default_rng(47)
    B = rng.integers(0, 256, N4, dtype=np.int64)
    D = rng.integers(90000, 10500000, N4, dtype=np.int64)
    path, cols = product_table(tmp_path, B, D)
    for one in (100, 0, 254, 255, -3):
        exp = check_products(path, cols, one, f"one={one}")
        assert exp[1][0] < 0 or one >= 254


def test_sum_disc_tax_widths_over_61_bits(tmp_path):
    """32 + 21 + 21 bits: each product fits 64 bits only just, eight do not
    provably; and the same operands with a small `one`, 32 + 9 + 17 bits"""
    rng = np.random.default_rng(53)
    B = rng.integers(0, 200, N4, dtype=np.int64)                       # L=1
    C = rng.integers(0, 60000, N4, dtype=np.int64)                     # L=2
    D = range_values(rng, 0, (1 << 32) - 1, N4)                        # L=4
    D[2::3] = (1 << 32) - 1 - rng.integers(0, 9, len(D[2::3]))
    path, cols = product_table(tmp_path, B, D, C)
    P, _ = p_modes(ca.COMP_LZ4)
    assert set(ovt.col_modes(path, 3)) == {P | 4}
    exp = check_products(path, cols, 1 << 20, "one=2^20")
    assert exp[2][0] > 1 << 72
    check_products(path, cols, 300, "one=300")


def test_sum_disc_narrow_bound(tmp_path):
    """SUM_DISC around 61 bits of factor width: a 32-bit operand, all rows at
    its maximum, times `one` of 29 bits (61 in all: the largest row-group sum
    a u64 could still hold) and of 30 bits (62)"""
    B = np.zeros(N4, dtype=np.int64)
    B[1::2] = 1
    D = np.full(N4, (1 << 32) - 1, dtype=np.int64)
    D[0::250], D[9::250] = 0, 77               # L = 4 in every chunk group
    path, cols = product_table(tmp_path, B, D)
    P, _ = p_modes(ca.COMP_LZ4)
    assert set(ovt.col_modes(path, 3)) == {P | 4}
    for one in ((1 << 29) - 1, 1 << 29, (1 << 30) - 1):
        exp = check_products(path, cols, one, f"one={one}")
        assert exp[1][0] > (N4 - 40) * ((1 << 32) - 1) * (one - 1)


@pytest.mark.parametrize("comp", COMPS)
def test_q6_widths_narrow(tmp_path, comp):
    """the Q6 widths, L=3 x L=1 with both hval 0, all rows and ~2 % passing"""
    rng = np.random.default_rng(59)
    n = 6_037
    A = 8000 + rng.integers(0, 2500, n, dtype=np.int64)
    B = rng.integers(0, 11, n, dtype=np.int64)
    C = rng.integers(1, 51, n, dtype=np.int64) * 100
    D = rng.integers(90000, 10500000, n, dtype=np.int64)
    D[:64] = (1 << 24) - 1                                 # the widest products
    B[:64] = 255
    cols = [A, B, C, D]
    path = ovt.write(tmp_path / "t.cs", cols, comp=comp, chunk_group_row_limit=1000)
    P, _ = p_modes(comp)
    assert set(ovt.col_modes(path, 3)) == {P | 3} and set(ovt.col_modes(path, 1)) == {P | 1}
    assert ovt.eligible(path, [0, 1, 2, 3])
    ovt.check(path, cols, *ovt.Q6ISH, want_path=PATH_OV, what="q6 2%")
    ovt.check(path, cols, *ovt.q6_query(0, 1 << 20, 0, 255, 1 << 20),
              want_path=PATH_OV, what="q6 all")
    aggs = [(ca.AGG_SUM_PROD_I64, 3, 1), (ca.AGG_SUM_DISC_I64, 3, 1, -1, 255),
            (ca.AGG_SUM_DISC_TAX_I64, 3, 1, 2, 10000), (ca.AGG_SUM_I64, 3)]
    ovt.check(path, cols, [(0, GE, 8766), (0, LT, 9131)], aggs, want_path=PATH_OV, what="any")
