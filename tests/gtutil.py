"""
Shared helpers of the GROUP BY ... HAVING ... ORDER BY ... LIMIT tests
(test_hashagg_topn_cpu.py, test_gpu_hashagg_topn.py): a numpy / Python-int
reference that groups the arrays a test wrote, evaluates HAVING, applies the
documented total order and slices — never calling the library — and the
comparison of a library result against it.

Values compare as Python ints: counts and integer aggregates exactly (sums
are arbitrary-precision), floats through ford(), the PG float order (NaN
greatest and equal to itself, -0.0 = +0.0) as an integer code.
"""
import math
import struct

import numpy as np

import citus_amd as ca

COUNT_KINDS = (ca.AGG_COUNT_STAR, ca.AGG_COUNT_COL)
F64_KINDS = (ca.AGG_SUM_F64, ca.AGG_MIN_F64, ca.AGG_MAX_F64)
PROD_KINDS = (ca.AGG_SUM_PROD_I64, ca.AGG_SUM_DISC_I64, ca.AGG_SUM_DISC_TAX_I64)
ALL_KINDS = tuple(range(11))


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def ford(x):
    """integer code of a float whose order is PG's float order"""
    x = float(x)
    if math.isnan(x):
        return 0xFFF0000000000001
    u = f64_bits(x)
    if u == 1 << 63:
        u = 0
    return (~u & ((1 << 64) - 1)) if u >> 63 else (u | (1 << 63))


def full(agg):
    return (tuple(agg) + (-1, -1, -1, 0)[len(agg) - 1:])[:5]


def ref_agg(agg, idx, cols, nulls):
    """{"count", "null", "v"} of one aggregate over the rows idx; v is a
    Python int (integer kinds) or float (f64 kinds)"""
    kind, c_a, c_b, c_c, one = full(agg)
    if kind == ca.AGG_COUNT_STAR:
        return {"count": len(idx), "null": False, "v": len(idx)}

    def present(c):
        nl = nulls.get(c)
        return np.ones(len(idx), bool) if nl is None else nl[idx] == 0
    ok = present(c_a)
    if kind in PROD_KINDS:
        ok &= present(c_b)
    if kind == ca.AGG_SUM_DISC_TAX_I64:
        ok &= present(c_c)
    sel = idx[ok]
    cnt = len(sel)
    if kind == ca.AGG_COUNT_COL:
        return {"count": cnt, "null": False, "v": cnt}
    if cnt == 0:
        return {"count": 0, "null": True, "v": None}
    a = cols[c_a][sel]
    if kind == ca.AGG_SUM_I64:
        v = sum(a.tolist())
    elif kind == ca.AGG_MIN_I64:
        v = int(a.min())
    elif kind == ca.AGG_MAX_I64:
        v = int(a.max())
    elif kind == ca.AGG_SUM_F64:
        v = math.fsum(a.tolist())
    elif kind == ca.AGG_MIN_F64:            # PG order: NaN is the greatest float
        nn = a[~np.isnan(a)]
        v = float(nn.min()) if len(nn) else float("nan")
    elif kind == ca.AGG_MAX_F64:
        v = float("nan") if np.isnan(a).any() else float(a.max())
    elif kind == ca.AGG_SUM_PROD_I64:
        v = sum(x * y for x, y in zip(a.tolist(), cols[c_b][sel].tolist()))
    elif kind == ca.AGG_SUM_DISC_I64:
        v = sum(x * (one - y) for x, y in zip(a.tolist(), cols[c_b][sel].tolist()))
    else:
        v = sum(x * (one - y) * (one + z)
                for x, y, z in zip(a.tolist(), cols[c_b][sel].tolist(),
                                   cols[c_c][sel].tolist()))
    return {"count": cnt, "null": False, "v": v}


def ref_groups(key_cols, aggs, cols, nulls=None, mask=None):
    """{key tuple (None = NULL): [ref_agg per agg]} over the rows where mask"""
    nulls = nulls or {}
    n = len(cols[key_cols[0]])
    mask = np.ones(n, bool) if mask is None else mask
    kl = [(cols[c].tolist(), None if nulls.get(c) is None else nulls[c].tolist())
          for c in key_cols]
    groups = {}
    for i in np.flatnonzero(mask).tolist():
        t = tuple(None if (nl is not None and nl[i]) else v[i] for v, nl in kl)
        groups.setdefault(t, []).append(i)
    return {t: [ref_agg(a, np.array(ix), cols, nulls) for a in aggs]
            for t, ix in groups.items()}


def key_order(t):
    """ascending, signed, per column NULL last: the tie rule"""
    return tuple((1, 0) if v is None else (0, v) for v in t)


def cmp_value(kind, e):
    """the comparable int of a non-NULL reference aggregate"""
    return ford(e["v"]) if kind in F64_KINDS else e["v"]


def ref_having(groups, aggs, having):
    out = {}
    for t, es in groups.items():
        ok = True
        for a, op, value in having:
            kind, e = full(aggs[a])[0], es[a]
            if e["null"]:
                ok = False
                break
            v = cmp_value(kind, e)
            c = ford(value) if kind in F64_KINDS else value
            ok = ok and ((v < c), (v <= c), (v > c), (v >= c), (v == c), (v != c))[op]
        if ok:
            out[t] = es
    return out


def term_flags(term):
    opts = [str(o).lower() for o in term[2:]]
    return "desc" in opts, "nulls_first" in opts


def ref_topn(groups, aggs, order, limit, having=(), offset=0):
    """the key tuples of the expected result, in order"""
    kept = ref_having(groups, aggs, having)

    def sk(t):
        key = []
        for term in order:
            desc, first = term_flags(term)
            if term[0] == "agg":
                e = kept[t][term[1]]
                null = e["null"]
                v = None if null else cmp_value(full(aggs[term[1]])[0], e)
            else:
                v = t[term[1]]
                null = v is None
            key.append((0 if first else 2, 0) if null else (1, -v if desc else v))
        return tuple(key) + key_order(t)
    return sorted(kept, key=sk)[offset:offset + limit]


def result_keys(res):
    nk = len(res["keys"])
    return [tuple(None if res["key_nulls"][k][g] else int(res["keys"][k][g])
                  for k in range(nk)) for g in range(res["n_groups"])]


def check_topn(res, groups, want_keys, aggs, exact_f64_sum=True):
    """keys in the expected order, every partial equal to the reference"""
    assert result_keys(res) == list(want_keys)
    assert res["n_groups"] == len(want_keys)
    for k in range(len(res["keys"])):             # NULL keys carry value 0
        assert not res["keys"][k][res["key_nulls"][k] == 1].any()
    assert res["partials"].shape == (len(want_keys), len(aggs))
    for g, t in enumerate(want_keys):
        for a, agg in enumerate(aggs):
            p, e, kind = res["partials"][g, a], groups[t][a], full(agg)[0]
            where = (t, a)
            assert p["count"] == e["count"], where
            if kind in COUNT_KINDS:
                assert p["is_null"] == 0 and p["i128_lo"] == e["count"], where
                continue
            assert bool(p["is_null"]) == e["null"], where
            if e["null"]:
                continue
            if kind == ca.AGG_SUM_F64 and not exact_f64_sum:
                assert abs(p["f64"] - e["v"]) <= 1e-6 * abs(e["v"]), where
            elif kind in F64_KINDS:
                if math.isnan(e["v"]):
                    assert math.isnan(p["f64"]), where
                else:
                    assert f64_bits(p["f64"]) == f64_bits(e["v"]), where
            else:
                assert ca.partial_i128(p) == e["v"], where


def same_bytes(a, b):
    assert a["n_groups"] == b["n_groups"]
    for k in range(len(a["keys"])):
        assert a["keys"][k].tobytes() == b["keys"][k].tobytes()
        assert a["key_nulls"][k].tobytes() == b["key_nulls"][k].tobytes()
    assert a["partials"].tobytes() == b["partials"].tobytes()


def slice_of(res, idx):
    """the agg_hashed-shaped dict holding rows idx of res, in that order"""
    idx = np.array(list(idx), dtype=np.int64)
    return {"n_groups": len(idx),
            "keys": [a[idx] for a in res["keys"]],
            "key_nulls": [a[idx] for a in res["key_nulls"]],
            "partials": res["partials"][idx]}


def py_topn_of_hashed(res, aggs, order, limit, having=()):
    """Python sort and slice of an agg_hashed() result by the documented
    rules: HAVING, order terms, ties in the result's own (key) order"""
    kinds = [full(a)[0] for a in aggs]

    def value(g, a):
        p = res["partials"][g, a]
        if kinds[a] in COUNT_KINDS:
            return False, int(p["count"])
        if p["is_null"]:
            return True, None
        if kinds[a] in F64_KINDS:
            return False, ford(p["f64"])
        return False, ca.partial_i128(p)

    def keep(g):
        for a, op, c in having:
            null, v = value(g, a)
            if null:
                return False
            c = ford(c) if kinds[a] in F64_KINDS else c
            if not ((v < c), (v <= c), (v > c), (v >= c), (v == c), (v != c))[op]:
                return False
        return True

    def sk(g):
        key = []
        for term in order:
            desc, first = term_flags(term)
            if term[0] == "agg":
                null, v = value(g, term[1])
            else:
                null = bool(res["key_nulls"][term[1]][g])
                v = int(res["keys"][term[1]][g])
            key.append((0 if first else 2, 0) if null else (1, -v if desc else v))
        return tuple(key) + (g,)
    idx = sorted((g for g in range(res["n_groups"]) if keep(g)), key=sk)[:limit]
    return slice_of(res, idx)
