"""multi_agg_kernel_ov: lane-contiguous rows, one dword per row.

Same conventions as test_gpu_agg_overlap.py, whose helpers are used here:
every test writes its own small table (at most 16 384 rows), reads the footer
back to pin the stream shapes on disk, asserts Scan.last_agg_path and
compares with exact Python-int results computed from the arrays written.

The layout under test: a work item is a (chunk group, R*256-row tile); lane t
of the block holds rows t, t+256, ..., t+(R-1)*256 of the tile (R = 8 in the
Q6 and count instances: a wave covers rows 64w..64w+63 of each of eight
256-row bands, a tile 2048 rows; R = 4 in the unspecialised instance: 1024).
Each row is the unaligned dword at its closed-form stream position; only row
0 of a stream sits elsewhere; rows past the group's row count, and rows of an
operand-only column that did not pass, are not loaded at all. Every case
runs through the Q6 instance, count(*) under one predicate and the
unspecialised instance, on lz4 and zstd. Scans over zstd streams keep the
per-lane window form of the body (it measured faster there); the same cases
and exact results hold for it.
"""
import numpy as np
import pytest

import citus_amd as ca
import futil
import test_gpu_agg_overlap as ovt

pytestmark = pytest.mark.gpu

PATH_NONE, PATH_OV = ovt.PATH_NONE, ovt.PATH_OV
LT, LE, GT, GE, EQ, NE = ovt.LT, ovt.LE, ovt.GT, ovt.GE, ovt.EQ, ovt.NE
COMPS = [ca.COMP_LZ4, ca.COMP_ZSTD]
COUNT = [(ca.AGG_COUNT_STAR, -1)]
Q6_AGGS = ovt.q6_query(0, 0, 0, 0, 0)[1]
ANY_AGGS = ovt.any_query(0, 0)[1]
Q6_REST = [(1, GE, -5), (1, LE, 1000), (2, LT, 1 << 40)]     # pass every row


def p_modes(comp):
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


def three(path, cols, on_a, count_pred, what, want_path=PATH_OV):
    """one selection through the three instances. on_a: the predicates on
    column 0 (two of them, so that the Q6 shape holds); count_pred: the same
    selection as ONE predicate for the count instance, or None"""
    assert len(on_a) == 2
    ovt.check(path, cols, list(on_a) + Q6_REST, Q6_AGGS, want_path=want_path, what=what + " q6")
    ovt.check(path, cols, list(on_a), ANY_AGGS, want_path=want_path, what=what + " any")
    ovt.check(path, cols, list(on_a) if count_pred is None else [count_pred], COUNT,
              want_path=want_path, what=what + " count")


def only(v):
    return [(0, GE, v), (0, LT, v + 1)], (0, EQ, v)


def all_but(v):
    return [(0, LT, v, 1), (0, GT, v, 1)], (0, NE, v)


# ------------------------------------------------- 1. exactly one passing row

N1, CG1 = 8192, 4096
# edges of lane, wave, k and tile (R = 8: 256 / 2048; R = 4: 1024 is 4*256),
# and rows 0/1 of the second group's streams
ROWS1 = [0, 1, 2, 63, 64, 255, 256, 257, 511, 512, 1791, 1792, 2047, 2048, 2049,
         4095, 4096, 4097]
# one lane at two k; two adjacent lanes at one k
PAIRS1 = [(10, 10 + 256), (522, 523)]


def one_row_table(n, cg, rng):
    i = np.arange(n, dtype=np.int64)
    # A selects rows by value: a permutation spread over both chunk groups,
    # so min/max pruning never removes a group and both are walked
    A = (1 << 20) + 2 * ((i * 4099) % n)
    A[5::cg] = (1 << 20) - 2           # every selected value lies strictly
    A[6::cg] = (1 << 20) + 2 * n       # inside both groups' [min, max]
    B = rng.integers(1, 200, n, dtype=np.int64)                 # L=1, predicate + operand
    C = 70000 + rng.integers(0, 60000, n, dtype=np.int64)       # L=2, predicate
    D = i * 257 + 11                                            # L=3, differs on every row
    return [A, B, C, D]


@pytest.fixture(scope="module", params=COMPS, ids=["lz4", "zstd"])
def one_row(request, tmp_path_factory):
    comp = request.param
    cols = one_row_table(N1, CG1, np.random.default_rng(17))
    path = ovt.write(tmp_path_factory.mktemp("one") / "t.cs", cols, comp=comp,
                     chunk_group_row_limit=CG1, stripe_row_limit=4 * CG1)
    assert len(ovt.col_modes(path, 0)) == 2
    for c in (0, 1, 2):
        assert_modes(path, c, comp)
    assert_modes(path, 3, comp, Ls=(3,))
    assert ovt.eligible(path, [0, 1, 2, 3])
    return path, cols


def test_single_passing_row(one_row):
    """one row of two 4096-row chunk groups passes: a wrong row, or a stale
    register, changes the sum, the operand being different on every row"""
    path, cols = one_row
    A = cols[0]
    for r in ROWS1:
        sel, cnt = only(int(A[r]))
        three(path, cols, sel, cnt, f"row {r}")


def test_two_passing_rows(one_row):
    path, cols = one_row
    A = cols[0]
    for r0, r1 in PAIRS1:
        sel = [(0, EQ, int(A[r0]), 1), (0, EQ, int(A[r1]), 1)]
        three(path, cols, sel, None, f"rows {r0}+{r1}")


def test_selectivity_extremes(one_row):
    """every row passes (every predicated operand load active); no row
    passes although no group can be pruned (A is even, the bounds are odd
    and inside every group's [min, max])"""
    path, cols = one_row
    A = cols[0]
    lo, hi = int(A.min()), int(A.max())
    three(path, cols, [(0, GE, lo), (0, LE, hi)], (0, GE, lo), "all")
    v = (1 << 20) + 4097
    assert lo < v < hi and v not in A
    sel, cnt = only(v)
    three(path, cols, sel, cnt, "none")
    assert ovt.run(path, sel + Q6_REST, Q6_AGGS)[2] == 0       # nothing pruned


# ------------------------------------------------- 2. length of the last group

CG2 = 5000
LENGTHS = [1, 2, 3, 8, 9, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4096 + 1]


@pytest.mark.parametrize("comp", COMPS, ids=["lz4", "zstd"])
@pytest.mark.parametrize("length", LENGTHS)
def test_last_group_length(tmp_path, comp, length):
    """a full first group, then a last group of `length` rows: every row
    passing, and only the last row passing. A row past row_count that was
    read would pass `A != absent` and change count(*).

    The writer does not store a group of fewer than 8 rows as a canonical
    stream in every case (lz4: 1 and 2 rows, zstd: 1 to 3), and one such
    group makes the whole scan ineligible. From 8 rows on every stream must
    be canonical and the body must be PATH_OV; below that the body asserted
    is the one that follows from the shapes on disk, and the exact results
    are asserted all the same. Lengths 8 and 9 are the shortest tails that
    do run the dense body: a last tile with rows in lanes 0..8 only."""
    n = CG2 + length
    rng = np.random.default_rng(length)
    A = (1 << 20) + 2 * np.arange(n, dtype=np.int64)
    B = rng.integers(1, 200, n, dtype=np.int64)
    C = 70000 + rng.integers(0, 60000, n, dtype=np.int64)
    D = np.arange(n, dtype=np.int64) * 257 + 11
    cols = [A, B, C, D]
    path = ovt.write(tmp_path / "t.cs", cols, comp=comp, chunk_group_row_limit=CG2,
                     stripe_row_limit=4 * CG2)
    assert len(ovt.col_modes(path, 0)) == 2
    want = PATH_OV
    if length >= 8 or ovt.eligible(path, [0, 1, 2, 3]):
        for c in range(4):
            assert_modes(path, c, comp)
    else:
        want = None                    # ovt.check: the body the shapes imply
    first, last = int(A[0]), int(A[-1])
    three(path, cols, [(0, GE, first), (0, NE, first - 1)], (0, NE, first - 1), "all", want)
    # the last row alone
    three(path, cols, [(0, GE, last), (0, NE, first - 1)], (0, GE, last), "last", want)


# ------------------------------------------------- 3. stream shapes

N3, CG3 = 4096 + 700, 4096
HIGH = {1: 0, 2: 5 << 16, 3: 0, 4: 3 << 40}


def shape_column(kind, n, cg):
    """exactly P(L) in both chunk groups (forced on rows 3 and 4, which no
    case selects); rows 0 and 1 of each group hold values no other row has"""
    if kind == "const":
        return np.full(n, 123457, dtype=np.int64)
    L = int(kind)
    W = 1 << (8 * L)
    i = np.arange(n, dtype=np.int64)
    v = 2 + (i * (7 if L == 1 else 40503)) % (W - 8)            # <= W - 7
    v[3::cg] = W - 1
    v[4::cg] = 0
    v[0], v[1], v[cg], v[cg + 1] = W - 6, W - 5, W - 4, W - 3
    return v + HIGH[L]


@pytest.mark.parametrize("comp", COMPS, ids=["lz4", "zstd"])
@pytest.mark.parametrize("kind", ["1", "2", "3", "4", "const"])
@pytest.mark.parametrize("where", ["predicate", "operand"])
def test_stream_shapes(tmp_path, comp, kind, where):
    """every P(L) and CONST once in a predicate slot and once in the
    operand-only slot; rows 0 and 1 of both groups' streams pass alone and
    fail alone"""
    n, cg = N3, CG3
    A, B, C, D = one_row_table(n, cg, np.random.default_rng(23))
    X = shape_column(kind, n, cg)
    cols = [X, B, C, D] if where == "predicate" else [A, B, C, X]
    xcol = 0 if where == "predicate" else 3
    path = ovt.write(tmp_path / "t.cs", cols, comp=comp, chunk_group_row_limit=cg,
                     stripe_row_limit=4 * cg)
    assert len(ovt.col_modes(path, 0)) == 2
    for c in range(4):
        if c == xcol:
            assert_modes(path, c, comp, Ls=() if kind == "const" else (int(kind),),
                         const=kind == "const")
        else:
            assert_modes(path, c, comp)
    if kind == "const" and where == "predicate":
        # a predicate that is false on a constant is refuted by min/max
        v = int(X[0])
        three(path, cols, [(0, GE, v), (0, LE, v)], (0, EQ, v), "const all")
        return
    sel_col = cols[0]
    for r in (0, 1, cg, cg + 1):
        v = int(sel_col[r])
        assert int((sel_col == v).sum()) == 1
        sel, cnt = only(v)
        three(path, cols, sel, cnt, f"only row {r}")
        sel, cnt = all_but(v)
        three(path, cols, sel, cnt, f"all but row {r}")


# ------------------------------------------------- 4. operators

@pytest.mark.parametrize("comp", COMPS, ids=["lz4", "zstd"])
def test_operators_at_k7(tmp_path, comp):
    """all six operators on an L = 2 slot, the constant at, just below and
    just above the value of a row held at k = 7 (R = 8) / k = 3 (R = 4) of
    the first tile's second lane band"""
    n, cg = 4096 + 404, 4096
    rng = np.random.default_rng(29)
    i = np.arange(n, dtype=np.int64)
    A = (5 << 16) + (i * 40503) % (1 << 16)                     # L=2, distinct
    B = rng.integers(1, 200, n, dtype=np.int64)
    C = 70000 + rng.integers(0, 60000, n, dtype=np.int64)
    D = i * 257 + 11
    cols = [A, B, C, D]
    path = ovt.write(tmp_path / "t.cs", cols, comp=comp, chunk_group_row_limit=cg,
                     stripe_row_limit=4 * cg)
    assert_modes(path, 0, comp, Ls=(2,))
    for c in (1, 2, 3):
        assert_modes(path, c, comp)
    absent = 1 << 40
    for r in (7 * 256 + 37, 3 * 256 + 37):
        for c in (int(A[r]) - 1, int(A[r]), int(A[r]) + 1):
            for op in (LT, LE, GT, GE, EQ, NE):
                three(path, cols, [(0, op, c), (0, NE, absent)], (0, op, c),
                      f"row {r} op {op} c {c}")
