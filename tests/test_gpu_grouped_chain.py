"""
The grouped scan_agg fallback chain (@pytest.mark.gpu), pinned to exact
results from numpy and Python ints.

An all-dense scan runs multi_grouped_kernel first; each of its waves owns a
16-slot key table and reads 512 consecutive rows. The keys here repeat with a
period of at most 65 rows, so every wave sees every key: 16 keys fit, 17 or
more are certain to raise device flag 8 and hand the query to
grouped_agg_kernel (64 slots per wave), and 65 overflow that one too. A scan
with a nullable column is not all-dense and starts at grouped_agg_kernel.

Bar: keys, counts, is_null and integer SUM/MIN/MAX exact, float MIN/MAX
exact, float SUM <= 1e-6 relative (the order of f64 additions differs).
"""
import numpy as np
import pytest

import citus_amd as ca

pytestmark = pytest.mark.gpu

K0, K1, V, F = range(4)
DEFS = [("k0", ca.I8, 0), ("k1", ca.I8, 0), ("v", ca.I64, 0), ("f", ca.F64, 0)]

INT_AGGS = [(ca.AGG_COUNT_STAR, -1), (ca.AGG_SUM_I64, V),
            (ca.AGG_MIN_I64, V), (ca.AGG_MAX_I64, V)]
FLOAT_AGGS = [(ca.AGG_SUM_F64, F), (ca.AGG_MIN_F64, F), (ca.AGG_MAX_F64, F),
              (ca.AGG_COUNT_COL, V)]
V_PRED = (V, ca.PRED_GT, 0)

WRITERS = {"lz4": dict(compression=ca.COMP_LZ4),
           "lz4_generic": dict(compression=ca.COMP_LZ4, canonical=0),
           "none": dict(compression=ca.COMP_NONE)}


@pytest.fixture(scope="module", autouse=True)
def require_gpu():
    assert ca.gpu_available(), "MI355X required for these tests"


def make_columns(a, b, n):
    """k0 = i % a, k1 = (i // a) % b: a*b distinct keys, period a*b rows.
    v spans +-2^62 so a group's sum needs the high word; f lies in [-1, 3),
    so a group's sum is well conditioned (sum|f| is about 1.25 |sum f|) and
    any summation order stays many orders inside the 1e-6 bound."""
    rng = np.random.default_rng(1000 * a + b)
    i = np.arange(n)
    k0 = (i % a).astype(np.int8)
    k1 = ((i // a) % b).astype(np.int8)
    v = rng.integers(-2**62, 2**62, n, dtype=np.int64)
    f = rng.random(n) * 4.0 - 1.0
    return k0, k1, v, f


def expected_groups(cols, aggs, v_null=None, pred=None):
    """{(k0, k1): [(count, is_null, value)]} per agg, from Python ints"""
    k0, k1, v, f = cols
    n = len(k0)
    v_ok = np.ones(n, bool) if v_null is None else v_null == 0
    keep = np.ones(n, bool)
    if pred is not None:                      # a NULL never passes
        assert pred == V_PRED
        keep = v_ok & (v > 0)
    exp = {}
    for key in sorted(set(zip(k0[keep].tolist(), k1[keep].tolist()))):
        rows = keep & (k0 == key[0]) & (k1 == key[1])
        ints = [int(x) for x in v[rows & v_ok]]
        flts = f[rows]
        out = []
        for kind, *_ in aggs:
            if kind == ca.AGG_COUNT_STAR:
                out.append((int(rows.sum()), 0, int(rows.sum())))
            elif kind == ca.AGG_COUNT_COL:
                out.append((len(ints), 0, len(ints)))
            elif kind == ca.AGG_SUM_I64:
                out.append((len(ints), int(not ints), sum(ints)))
            elif kind == ca.AGG_MIN_I64:
                out.append((len(ints), int(not ints), min(ints, default=0)))
            elif kind == ca.AGG_MAX_I64:
                out.append((len(ints), int(not ints), max(ints, default=0)))
            elif kind == ca.AGG_SUM_F64:
                out.append((len(flts), 0, float(np.sum(flts, dtype=np.longdouble))))
            elif kind == ca.AGG_MIN_F64:
                out.append((len(flts), 0, float(flts.min())))
            elif kind == ca.AGG_MAX_F64:
                out.append((len(flts), 0, float(flts.max())))
        exp[key] = out
    return exp


def run_grouped(path, aggs, preds, group_cols=(K0, K1)):
    mask = ca.agg_cols_mask(aggs)
    for c in group_cols:
        mask |= 1 << c
    for p in preds:
        mask |= 1 << p[0]
    with ca.Reader(path) as r, r.scan(cols_mask=mask, preds=preds) as s:
        s.stage()
        res = s.agg_grouped(aggs, group_cols)
        assert s.last_fused is False
    return res


def assert_groups(res, exp, aggs):
    assert set(res) == set(exp)
    for key, want in exp.items():
        for i, (kind, *_) in enumerate(aggs):
            got = res[key][i]
            count, is_null, value = want[i]
            assert got.count == count, (key, i)
            assert got.is_null == is_null, (key, i)
            if is_null:
                continue
            if kind == ca.AGG_SUM_F64:
                assert abs(got.f64 - value) <= 1e-6 * abs(value), (key, i)
            elif kind in (ca.AGG_MIN_F64, ca.AGG_MAX_F64):
                assert got.f64 == value, (key, i)
            else:
                assert got.i128 == value, (key, i)


def write(path, cols, n, writer, nulls=None):
    # n = 2000 is one chunk group; n = 5000 is two full ones and a 1000-row tail
    ca.write_table(path, DEFS, list(cols), nulls=nulls,
                   chunk_group_row_limit=2000 if n > 2000 else 10000,
                   **WRITERS[writer])


@pytest.mark.parametrize("writer", list(WRITERS))
@pytest.mark.parametrize("n", [2000, 5000])
@pytest.mark.parametrize("a,b", [(4, 4), (17, 1), (5, 5), (8, 8)])
def test_dense_key_counts_across_the_16_slot_cap(tmp_path, a, b, n, writer):
    """16 keys stay in multi_grouped_kernel; 17, 25 and 64 overflow its wave
    tables and must come back exact from the 64-slot kernel"""
    cols = make_columns(a, b, n)
    path = str(tmp_path / "g.cs")
    write(path, cols, n, writer)
    for aggs, preds in [(INT_AGGS, []), (INT_AGGS, [V_PRED]), (FLOAT_AGGS, [])]:
        exp = expected_groups(cols, aggs, pred=preds[0] if preds else None)
        if not preds:
            assert len(exp) == a * b
        assert_groups(run_grouped(path, aggs, preds), exp, aggs)


@pytest.mark.parametrize("n", [2000, 5000])
def test_sparse_scan_starts_at_the_64_slot_kernel(tmp_path, n):
    """25 keys with v 20 % NULL: not all-dense, so grouped_agg_kernel runs
    first and alone"""
    cols = make_columns(5, 5, n)
    v_null = (np.random.default_rng(55).random(n) < 0.2).astype(np.uint8)
    path = str(tmp_path / "s.cs")
    write(path, cols, n, "lz4", nulls=[None, None, v_null, None])
    for preds in ([], [V_PRED]):
        exp = expected_groups(cols, INT_AGGS, v_null=v_null,
                              pred=preds[0] if preds else None)
        assert_groups(run_grouped(path, INT_AGGS, preds), exp, INT_AGGS)


def test_65_keys_refused_then_scan_still_usable(tmp_path):
    """65 keys overflow the 64-slot tables too: the call is refused, and the
    same staged scan then answers a query it can hold"""
    n = 2000
    cols = make_columns(13, 5, n)
    path = str(tmp_path / "x.cs")
    write(path, cols, n, "lz4")
    mask = ca.agg_cols_mask(INT_AGGS) | 0b11
    with ca.Reader(path) as r, r.scan(cols_mask=mask) as s:
        s.stage()
        with pytest.raises(ca.CStripeError, match="too many distinct groups"):
            s.agg_grouped(INT_AGGS, (K0, K1))
        res = s.agg_grouped(INT_AGGS, (K1,))
        assert s.last_fused is False
    k0, k1, v, f = cols
    by_k1 = (k1, np.zeros(n, np.int8), v, f)       # absent key column reads 0
    assert_groups(res, expected_groups(by_k1, INT_AGGS), INT_AGGS)
