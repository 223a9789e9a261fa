"""
The expression tests' own evaluator: a pure-Python postfix interpreter over
Python ints, None for NULL and an Err sentinel for the three errors, written
from the semantics in include/cstripe.h (cstripe_scan_begin_exprs). Nothing
here calls the library or its builder; the opcode numbers are spelled out so
that the tests pin them too.
"""
import datetime

(COL, CONST, NULL, ADD, SUB, MUL, DIV, MOD, NEG, LT, LE, GT, GE, EQ, NE,
 AND, OR, NOT, IS_NULL, COALESCE, SELECT, YEAR) = range(22)

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
DIV0, RANGE, YEAR_RANGE = "division by zero", "bigint out of range", "year out of range"


class Err:
    """a value in error; kind is the message the stage must give"""

    def __init__(self, kind):
        self.kind = kind

    def __repr__(self):
        return f"Err({self.kind})"


def is_err(v):
    return isinstance(v, Err)


def year_of(days):
    """proleptic Gregorian (astronomical) year of a day count from
    1970-01-01: the Gregorian calendar repeats every 146097 days = 400 years,
    so the day is moved into datetime's years 1..400 and the cycles added"""
    cycles, rem = divmod(days + 719162, 146097)      # days since 0001-01-01
    return datetime.date.fromordinal(rem + 1).year + 400 * cycles


def _fit(v):
    return v if I64_MIN <= v <= I64_MAX else Err(RANGE)


def _div(a, b):
    if b == 0:
        return Err(DIV0)
    q = abs(a) // abs(b)
    return _fit(-q if (a < 0) != (b < 0) else q)      # toward zero


def _mod(a, b):
    if b == 0:
        return Err(DIV0)
    m = abs(a) % abs(b)
    return -m if a < 0 else m                          # the dividend's sign


def _year(a):
    if not -(1 << 31) <= a < (1 << 31):
        return Err(YEAR_RANGE)
    return year_of(a)


_BINARY = {
    ADD: lambda a, b: _fit(a + b), SUB: lambda a, b: _fit(a - b),
    MUL: lambda a, b: _fit(a * b), DIV: _div, MOD: _mod,
    LT: lambda a, b: int(a < b), LE: lambda a, b: int(a <= b),
    GT: lambda a, b: int(a > b), GE: lambda a, b: int(a >= b),
    EQ: lambda a, b: int(a == b), NE: lambda a, b: int(a != b),
}
_UNARY = {NEG: lambda a: _fit(-a), YEAR: _year, NOT: lambda a: int(a == 0)}


def _logic(a, b, decides):
    """Kleene AND (decides = 0) / OR (decides = 1), left to right"""
    if is_err(a):
        return a
    if a is not None and int(a != 0) == decides:
        return decides                                  # hides b, error or not
    if is_err(b):
        return b
    if b is not None and int(b != 0) == decides:
        return decides
    if a is None or b is None:
        return None
    return 1 - decides


def evaluate(ops, row):
    """the program's value for one row: an int, None, or an Err. `row` maps a
    column id to an int or None."""
    st = []
    for op, column, ival in ops:
        if op == COL:
            st.append(row[column])
        elif op == CONST:
            st.append(ival)
        elif op == NULL:
            st.append(None)
        elif op in _UNARY:
            a = st.pop()
            st.append(a if is_err(a) or a is None else _UNARY[op](a))
        elif op == IS_NULL:
            a = st.pop()
            st.append(a if is_err(a) else int(a is None))
        elif op in _BINARY:
            b, a = st.pop(), st.pop()
            if is_err(a):
                st.append(a)
            elif is_err(b):
                st.append(b)
            elif a is None or b is None:
                st.append(None)
            else:
                st.append(_BINARY[op](a, b))
        elif op in (AND, OR):
            b, a = st.pop(), st.pop()
            st.append(_logic(a, b, 0 if op == AND else 1))
        elif op == COALESCE:
            b, a = st.pop(), st.pop()
            st.append(a if is_err(a) or a is not None else b)
        elif op == SELECT:
            b, a, c = st.pop(), st.pop(), st.pop()
            if is_err(c):
                st.append(c)
            else:
                st.append(a if c is not None and c != 0 else b)
        else:
            raise AssertionError(f"unknown op {op}")
    assert len(st) == 1
    return st[0]


def evaluate_rows(ops, columns, n):
    """per row of `columns` ({column id: (values, nulls or None)}): the value"""
    out = []
    for i in range(n):
        row = {c: (None if nl is not None and nl[i] else int(v[i]))
               for c, (v, nl) in columns.items()}
        out.append(evaluate(ops, row))
    return out


def first_error(results):
    """the error kind the stage must report: that of the first row in scan
    order whose value is in error; None when every row is clean"""
    for r in results:
        if is_err(r):
            return r.kind
    return None


# ------------------------------------------------------------ writing programs
def c(i):
    return [(COL, i, 0)]


def k(v):
    return [(CONST, 0, v)]


def o(op, *operands):
    """the postfix of `op` applied to operand programs"""
    out = []
    for p in operands:
        out += p
    return out + [(op, 0, 0)]


def stack_depth(ops):
    pops = {COL: 0, CONST: 0, NULL: 0, NEG: 1, NOT: 1, IS_NULL: 1, YEAR: 1, SELECT: 3}
    d = m = 0
    for op, _, _ in ops:
        d += 1 - pops.get(op, 2)
        m = max(m, d)
    return m


def to_arrays(results):
    """(int64 values with 0 in NULL slots, uint8 null bytes) of clean results"""
    import numpy as np
    assert not any(is_err(r) for r in results)
    vals = np.array([0 if r is None else r for r in results], dtype=np.int64)
    nulls = np.array([r is None for r in results], dtype=np.uint8)
    return vals, nulls


# ------------------------------------------------- the seeded differential's input
DIFF_SEED = 20261021
DIFF_ROWS = 300
DIFF_PROGRAMS = 200
_POOL = (0, 1, -1, 2, 3, 7, -5, 100, I64_MIN, I64_MAX)


def diff_columns():
    """three I64 columns of 300 rows with NULLs: column 0 mixes small values
    with the int64 extremes, columns 1 and 2 are small (with zeros)"""
    import random
    import numpy as np
    rng = random.Random(DIFF_SEED)
    cols = {}
    for ci in range(3):
        pool = _POOL if ci == 0 else (0, 1, -1, 2, 3, 7, -5, 100, 12, -40)
        vals = np.array([rng.choice(pool) for _ in range(DIFF_ROWS)], dtype=np.int64)
        nulls = np.array([rng.random() < 0.15 for _ in range(DIFF_ROWS)], dtype=np.uint8)
        cols[ci] = (vals, nulls)
    return cols


def _gen(rng, height):
    if height <= 1 or rng.random() < 0.25:
        x = rng.random()
        if x < 0.55:
            return c(rng.randrange(3))
        if x < 0.93:
            return k(rng.choice(_POOL))
        return [(NULL, 0, 0)]
    op = rng.choice((ADD, SUB, MUL, DIV, MOD, NEG, LT, LE, GT, GE, EQ, NE, AND, OR, NOT,
                     IS_NULL, COALESCE, SELECT, SELECT, YEAR))
    arity = 1 if op in (NEG, NOT, IS_NULL, YEAR) else 3 if op == SELECT else 2
    return o(op, *[_gen(rng, height - 1) for _ in range(arity)])


def diff_programs():
    """200 random programs: tree height <= 4, stack depth <= 4"""
    import random
    rng = random.Random(DIFF_SEED + 1)
    out = []
    while len(out) < DIFF_PROGRAMS:
        p = _gen(rng, 4)
        if len(p) >= 3 and stack_depth(p) <= 4:
            out.append(p)
    return out
