"""Stream-shape catalogue shared by the stream-shape tests: one entry per
column whose value stream the writer lays out in one known way. Every entry
names the column type, the codec and writer options, the values (fixed
formulas, no randomness), an optional null mask, and — written out literally —
what the writer must have emitted for every chunk: (comp_type, segment mode,
n_segs). The CPU module pins those against the footer; the GPU module then
runs every device read path over the same entries.

Unless an entry says otherwise a table has N = 2100 rows in chunk groups of
1000: three chunks, the last one partial (100 rows), and more than one 8-row
window per lane."""
import numpy as np

import citus_amd as ca

LZ4, ZSTD, NONE = ca.COMP_LZ4, ca.COMP_ZSTD, ca.COMP_NONE
CODEC_NAME = {LZ4: "lz4", ZSTD: "zstd"}

N = 2100
CG = 1000
STARTS = (0, 1000, 2000)
ENDS = (999, 1999, 2099)          # last row of each chunk

HIGH = 0x0123456789ABCDEF         # the "arbitrary" high-byte pattern
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1

NP_DTYPE = {ca.I8: np.int8, ca.I32: np.int32, ca.I64: np.int64,
            ca.F32: np.float32, ca.F64: np.float64}
IS_FLOAT = {ca.I8: False, ca.I32: False, ca.I64: False,
            ca.F32: True, ca.F64: True}


class Shape:
    def __init__(self, name, ctype, codec, values, chunks, nulls=None,
                 canonical=1, cgrl=CG, helper=None):
        self.name = name
        self.ctype = ctype
        self.codec = codec
        self.canonical = canonical
        self.cgrl = cgrl
        self.values = np.ascontiguousarray(values, dtype=NP_DTYPE[ctype])
        self.nulls = None if nulls is None else \
            np.ascontiguousarray(nulls, dtype=np.uint8)
        self.chunks = list(chunks)       # [(comp_type, mode, n_segs)] per chunk
        self.helper = helper             # name of the I64 helper entry
        self.values.setflags(write=False)
        if self.nulls is not None:
            self.nulls.setflags(write=False)

    @property
    def n(self):
        return len(self.values)

    @property
    def is_float(self):
        return IS_FLOAT[self.ctype]

    @property
    def dense(self):
        return self.nulls is None

    def chunk_bounds(self):
        return [(s, min(s + self.cgrl, self.n))
                for s in range(0, self.n, self.cgrl)]

    def bits(self):
        """the values as unsigned bit patterns of the column's width"""
        w = self.values.dtype.itemsize
        return self.values.view({4: np.uint32, 8: np.uint64}[w])

    def __repr__(self):
        return f"Shape({self.name})"


SHAPES = {}


def _add(name, ctype, values, per_codec, **kw):
    """one entry per codec in per_codec: {codec: [chunk expectations]}"""
    for codec, chunks in per_codec.items():
        full = f"{name}_{CODEC_NAME[codec]}"
        assert full not in SHAPES, full
        SHAPES[full] = Shape(full, ctype, codec, values, chunks, **kw)


def _i64(u):
    return np.asarray(u, dtype=np.uint64).view(np.int64)


def lo_field(width_bytes, n=N, starts=STARTS):
    """low field of `width_bytes` bytes: a multiplicative scramble that, in
    every chunk, reaches 0 and the all-ones maximum at three adjacent rows
    each, so any null mask of the catalogue leaves both extremes present"""
    w = 1 << (8 * width_bytes)
    lo = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(w)
    for s in starts:
        if s + 10 <= n:
            lo[s + 4:s + 7] = 0
            lo[s + 7:s + 10] = w - 1
    return lo


def high_of(L):
    return HIGH & ~((1 << (8 * L)) - 1)


# ---------------------------------------------------------------- I64 P(L)
for _L in (1, 2, 3, 4):
    _lo = lo_field(_L)
    _exp = {LZ4: [(LZ4, 0x10 | _L, 1)] * 3, ZSTD: [(ZSTD, 0x60 | _L, 1)] * 3}
    _add(f"i64_p{_L}_zero", ca.I64, _i64(_lo), _exp)
    _add(f"i64_p{_L}_ones", ca.I64, _i64(~_lo), _exp)            # -1 - lo
    _add(f"i64_p{_L}_high", ca.I64, _i64(np.uint64(high_of(_L)) | _lo), _exp)

# the single value that forces L (byte L-1 differs) at row 0 / 1 / 2 / last
# of every chunk; all other rows vary only below byte L-1 (L = 1: constant)
for _L in (1, 2, 3, 4):
    for _pos in ("r0", "r1", "r2", "last"):
        _below = (np.arange(N, dtype=np.uint64) * np.uint64(40503)) \
            % np.uint64(1 << (8 * (_L - 1)))
        _v = np.uint64(high_of(_L)) | _below
        for _s, _e in zip(STARTS, ENDS):
            _row = {"r0": _s, "r1": _s + 1, "r2": _s + 2, "last": _e}[_pos]
            _v[_row] |= np.uint64(0xA5 << (8 * (_L - 1)))
        _add(f"i64_p{_L}_force_{_pos}", ca.I64, _i64(_v),
             {LZ4: [(LZ4, 0x10 | _L, 1)] * 3, ZSTD: [(ZSTD, 0x60 | _L, 1)] * 3})


# ------------------------------------------- I64 L = 5: generic, fusable
def l5_values(n, variant="a"):
    """byte 4 varies from row 1 on (no canonical parse applies) with a short
    period, so every 256 B segment still compresses"""
    i = np.arange(n, dtype=np.int64)
    if variant == "a":
        return ((i % 3) << 32) | (i % 5)
    return ((i % 5) << 32) | (i % 3)


# 1000 rows = 8000 B = 31 full 256 B segments + 64 B; 100 rows = 800 B = 4
for _var in ("a", "b"):
    _add(f"i64_l5{_var}", ca.I64, l5_values(N, _var),
         {LZ4: [(LZ4, 0x00, 32), (LZ4, 0x00, 32), (LZ4, 0x00, 4)],
          ZSTD: [(ZSTD, 0x50, 32), (ZSTD, 0x50, 32), (ZSTD, 0x50, 4)]})

# ---------------------------------------------------------------- I64 CONST
for _nm, _c in (("0", 0), ("m1", -1), ("min", I64_MIN), ("max", I64_MAX)):
    _add(f"i64_const_{_nm}", ca.I64, np.full(N, _c, dtype=np.int64),
         {LZ4: [(LZ4, 0x20, 1)] * 3, ZSTD: [(ZSTD, 0x70, 1)] * 3})

# CONST in one chunk group, P(2) in the next, another CONST in the last: the
# column location record (mode, L, high bytes) is per chunk group
_v = np.uint64(high_of(2)) | lo_field(2)
_v[:1000] = np.uint64(high_of(2) | 0x0007)
_v[2000:] = np.uint64(0xFEDCBA9876543210)
_add("i64_const_then_p2", ca.I64, _i64(_v),
     {LZ4: [(LZ4, 0x20, 1), (LZ4, 0x12, 1), (LZ4, 0x20, 1)],
      ZSTD: [(ZSTD, 0x70, 1), (ZSTD, 0x62, 1), (ZSTD, 0x70, 1)]})

# ---------------------------------------------------------------- F64
_add("f64_p2", ca.F64,
     (np.uint64(0x4059000000000000) | lo_field(2)).view(np.float64),
     {LZ4: [(LZ4, 0x12, 1)] * 3, ZSTD: [(ZSTD, 0x62, 1)] * 3})
_add("f64_p1_nan", ca.F64,
     (np.uint64(0x7FF8000000000000) | lo_field(1)).view(np.float64),
     {LZ4: [(LZ4, 0x11, 1)] * 3, ZSTD: [(ZSTD, 0x61, 1)] * 3})
for _nm, _b in (("0", 0x0000000000000000), ("neg0", 0x8000000000000000),
                ("nan", 0x7FF8000000000000)):
    _add(f"f64_const_{_nm}", ca.F64,
         np.full(N, _b, dtype=np.uint64).view(np.float64),
         {LZ4: [(LZ4, 0x20, 1)] * 3, ZSTD: [(ZSTD, 0x70, 1)] * 3})

# ---------------------------------------------------------------- tiny chunks
# width 8 needs >= 3 present values (24 B) for a canonical parse, and the
# parse must shrink the stream; everything else is generic or raw
_T1 = [0x00, 0xFF, 0x5A, 0x01]
_T4 = [0x00000000, 0xFFFFFFFF, 0x12345678, 0x80000000]
_TINY = {
    # (family, n): {codec: chunk}
    ("l1", 1): {LZ4: (NONE, 0x00, 1), ZSTD: (NONE, 0x00, 1)},
    ("l1", 2): {LZ4: (NONE, 0x00, 1), ZSTD: (NONE, 0x00, 1)},
    ("l1", 3): {LZ4: (LZ4, 0x11, 1), ZSTD: (NONE, 0x00, 1)},
    ("l1", 4): {LZ4: (LZ4, 0x11, 1), ZSTD: (ZSTD, 0x50, 1)},   # ZRP(1) does not shrink, one generic frame does
    ("l4", 1): {LZ4: (NONE, 0x00, 1), ZSTD: (NONE, 0x00, 1)},
    ("l4", 2): {LZ4: (NONE, 0x00, 1), ZSTD: (NONE, 0x00, 1)},
    ("l4", 3): {LZ4: (NONE, 0x00, 1), ZSTD: (NONE, 0x00, 1)},
    ("l4", 4): {LZ4: (LZ4, 0x14, 1), ZSTD: (NONE, 0x00, 1)},
    ("const", 1): {LZ4: (NONE, 0x00, 1), ZSTD: (NONE, 0x00, 1)},
    ("const", 2): {LZ4: (LZ4, 0x00, 1), ZSTD: (NONE, 0x00, 1)},
    ("const", 3): {LZ4: (LZ4, 0x20, 1), ZSTD: (ZSTD, 0x50, 1)},   # likewise ZR_CONST
    ("const", 4): {LZ4: (LZ4, 0x20, 1), ZSTD: (ZSTD, 0x70, 1)},
}
for (_fam, _n), _exp in _TINY.items():
    if _fam == "l1":
        _v = [high_of(1) | b for b in _T1[:_n]]
    elif _fam == "l4":
        _v = [high_of(4) | b for b in _T4[:_n]]
    else:
        _v = [(1 << 64) - 1] * _n       # -1: two of them still shrink under LZ4
    _add(f"tiny_{_fam}_n{_n}", ca.I64, _i64(np.array(_v, dtype=np.uint64)),
         {c: [e] for c, e in _exp.items()})

# ------------------------------------------------- the zstd 127 KiB boundary
# zstd canonical stops at 127 KiB of raw stream: 16255 I64 rows (130040 B)
# are one ZRP(1) frame, 16256 rows (130048 B) are 508 generic 256 B frames
for _nm, _mul in (("a", 1), ("b", 7)):
    for _rows, _chunk in ((16255, (ZSTD, 0x61, 1)), (16256, (ZSTD, 0x50, 508))):
        _add(f"i64_zr127k_{_rows}{_nm}", ca.I64,
             (np.arange(_rows, dtype=np.int64) * _mul) % 100,
             {ZSTD: [_chunk]}, cgrl=_rows)


# ------------------------------------------------------- width 4, zstd only
def byte_field(n=N, starts=STARTS):
    return lo_field(1, n, starts).astype(np.uint32)


def slots4(base, k, b):
    """u32 slots equal to `base` except byte k, which takes b"""
    return (np.uint32(base & ~(0xFF << (8 * k)) & 0xFFFFFFFF)
            | (b.astype(np.uint32) << np.uint32(8 * k)))


for _k in range(4):
    # k = 3: the varying byte is the sign byte, 0x00..0xFF
    _add(f"i32_zr4b{_k}", ca.I32,
         slots4(0x12345678, _k, byte_field()).view(np.int32),
         {ZSTD: [(ZSTD, 0x80 | _k, 1)] * 3})
_add("i32_zr4b0_neg", ca.I32,                       # -256 .. -1
     slots4(0xFFFFFF00, 0, byte_field()).view(np.int32),
     {ZSTD: [(ZSTD, 0x80, 1)] * 3})
for _k in range(3):
    _add(f"f32_zr4b{_k}", ca.F32,                   # around 100.0f, finite > 0
         slots4(0x42C80000, _k, byte_field()).view(np.float32),
         {ZSTD: [(ZSTD, 0x80 | _k, 1)] * 3})
# k = 3 over sign+exponent bytes 0x00..0x7F and 0xFF: finite values are all
# positive; 0x7F800000 / 0xFF800000 are +inf / -inf, 0x7FC00000 / 0xFFC00000
# are NaNs
_b3 = (np.arange(N, dtype=np.uint32) * np.uint32(37)) % np.uint32(129)
_b3[_b3 == 128] = 0xFF
_add("f32_zr4b3_inf", ca.F32, slots4(0x00800000, 3, _b3).view(np.float32),
     {ZSTD: [(ZSTD, 0x83, 1)] * 3})
_add("f32_zr4b3_nan", ca.F32, slots4(0x00C00000, 3, _b3).view(np.float32),
     {ZSTD: [(ZSTD, 0x83, 1)] * 3})
_add("i32_zr4_const", ca.I32, np.full(N, -5, dtype=np.int32),
     {ZSTD: [(ZSTD, 0x84, 1)] * 3})
_add("f32_zr4_const", ca.F32, np.full(N, 2.5, dtype=np.float32),
     {ZSTD: [(ZSTD, 0x84, 1)] * 3})
# width 4 needs >= 12 B (3 values) and must shrink
for _n, _ci, _cf in ((1, (NONE, 0x00, 1), (NONE, 0x00, 1)),
                     (2, (NONE, 0x00, 1), (NONE, 0x00, 1)),
                     (3, (NONE, 0x00, 1), (NONE, 0x00, 1))):
    _add(f"i32_tiny_n{_n}", ca.I32,
         np.array([-1, -2, -3][:_n], dtype=np.int32), {ZSTD: [_ci]})
    _add(f"f32_tiny_n{_n}", ca.F32,
         np.array([100.0, 100.5, 101.0][:_n], dtype=np.float32), {ZSTD: [_cf]})


# ---------------------------------------------------------------- sparse twins
def null_mask(kind, n=N):
    m = np.zeros(n, dtype=np.uint8)
    if kind == "first":
        m[0] = 1
    elif kind == "last":
        m[n - 1] = 1
    elif kind == "third":
        m[::3] = 1
    elif kind == "word64":
        m[64:128] = 1                    # one whole 64-row bitmap word
    elif kind == "but3":
        m[:] = 1
        m[[1, 1500, 2099]] = 0           # one present value per chunk: raw
    return m


MASKS = ("first", "last", "third", "word64", "but3")
_RAW3 = [(NONE, 0x00, 1)] * 3
_SPARSE_BASES = (
    ("i64_p2_high", {LZ4: [(LZ4, 0x12, 1)] * 3, ZSTD: [(ZSTD, 0x62, 1)] * 3}),
    ("i64_const_m1", {LZ4: [(LZ4, 0x20, 1)] * 3, ZSTD: [(ZSTD, 0x70, 1)] * 3}),
    ("f64_p2", {LZ4: [(LZ4, 0x12, 1)] * 3, ZSTD: [(ZSTD, 0x62, 1)] * 3}),
    ("i32_zr4b3", {ZSTD: [(ZSTD, 0x83, 1)] * 3}),
)
# ZR4B exists under zstd only. Under LZ4 the same slots are generic: a chunk
# whose slots repeat rarely does not shrink and stays raw, the 100-row tail
# (400 B, two segments) does
_ZR4B3_LZ4 = {
    "first": [(NONE, 0x00, 1), (NONE, 0x00, 1), (LZ4, 0x00, 2)],
    "last": [(NONE, 0x00, 1), (NONE, 0x00, 1), (LZ4, 0x00, 2)],
    "third": [(NONE, 0x00, 1), (NONE, 0x00, 1), (NONE, 0x00, 1)],
    "word64": [(NONE, 0x00, 1), (NONE, 0x00, 1), (LZ4, 0x00, 2)],
    "but3": [(NONE, 0x00, 1), (NONE, 0x00, 1), (NONE, 0x00, 1)],
}
for _base, _exp in _SPARSE_BASES:
    for _mk in MASKS:
        _src = SHAPES[_base + "_zstd"]
        _add(f"{_base}_null_{_mk}", _src.ctype, _src.values,
             {c: (_RAW3 if _mk == "but3" else e) for c, e in _exp.items()},
             nulls=null_mask(_mk))
for _mk in MASKS:
    _src = SHAPES["i32_zr4b3_zstd"]
    _add(f"i32_zr4b3_null_{_mk}", _src.ctype, _src.values,
         {LZ4: _ZR4B3_LZ4[_mk]}, nulls=null_mask(_mk))


# ---------------------------------------------------------------- helpers
# every table of the GPU matrix carries a dense I64 helper column from another
# entry of the same codec, row count and chunking, and of the same stream
# family, so the helper never changes which kernel path the entry takes
def _pick_helper(sh):
    c = CODEC_NAME[sh.codec]
    nm = sh.name
    if nm.startswith("tiny_") or "_tiny_n" in nm:
        n = sh.n
        fam = "l1" if nm.startswith("tiny_const") else "const"
        return f"tiny_{fam}_n{n}_{c}"
    if nm.startswith("i64_zr127k_"):
        rows = nm[len("i64_zr127k_"):-len("a_zstd")]
        other = "b" if nm.endswith("a_zstd") else "a"
        return f"i64_zr127k_{rows}{other}_{c}"
    if nm.startswith("i64_l5"):
        other = "b" if nm.startswith("i64_l5a") else "a"
        return f"i64_l5{other}_{c}"
    return f"i64_p3_zero_{c}" if nm.startswith("i64_p2_zero") else f"i64_p2_zero_{c}"


for _sh in SHAPES.values():
    _sh.helper = _pick_helper(_sh)
    _h = SHAPES[_sh.helper]
    assert _h is not _sh and _h.ctype == ca.I64 and _h.dense
    assert _h.codec == _sh.codec and _h.n == _sh.n and _h.cgrl == _sh.cgrl

ALL = list(SHAPES.values())
NAMES = list(SHAPES)


def is_canonical_mode(mode):
    return mode not in (0x00, 0x50)


def key_column(n):
    """the I8 group key of the GPU matrix: 0..4, out of phase with the
    chunking and with every value formula above"""
    return ((np.arange(n, dtype=np.int64) * 3 + (np.arange(n) // 7)) % 5).astype(np.int8)


def write_shape(path, sh, with_helpers=False):
    """write the entry's column (column 0); with_helpers adds the I64 helper
    (column 1) and the I8 key (column 2)"""
    defs = [("x", sh.ctype, 0)]
    cols = [sh.values.copy()]
    nulls = [None if sh.nulls is None else sh.nulls.copy()]
    if with_helpers:
        defs += [("h", ca.I64, 0), ("k", ca.I8, 0)]
        cols += [SHAPES[sh.helper].values.copy(), key_column(sh.n)]
        nulls += [None, None]
    ca.write_table(path, defs, cols,
                   nulls=None if all(x is None for x in nulls) else nulls,
                   compression=sh.codec, canonical=sh.canonical,
                   chunk_group_row_limit=sh.cgrl)


# ------------------------------------------------------------ expectations
# Everything below computes what a query must return from the arrays that
# were written, in numpy and Python ints: no library code is involved.
class Col:
    """one written column as the expectations see it"""

    def __init__(self, values, nulls=None):
        self.values = np.asarray(values)
        self.is_float = self.values.dtype.kind == "f"
        self.present = np.ones(len(self.values), dtype=bool) if nulls is None \
            else (np.asarray(nulls) == 0)
        if self.is_float:
            self.wide = self.values.astype(np.float64)      # exact widening
        else:
            self.wide = self.values.astype(np.int64)

    def present_values(self):
        """Python ints / floats of the non-null rows, in row order"""
        return self.wide[self.present].tolist()


def pg_sort_key(v):
    """PG float order: NaN is the greatest value and equal to itself"""
    return (1, 0.0) if isinstance(v, float) and v != v else (0, v)


def pred_mask(col, op, c):
    """rows on which `col op c` holds; a NULL operand fails the atom; floats
    compare in PG order (NaN greatest, NaN = NaN)"""
    v = col.wide
    if col.is_float:
        c = float(c)
        vn = np.isnan(v)
        cn = c != c
        with np.errstate(invalid="ignore"):
            lt = (v < c) | (~vn & cn)
            eq = (v == c) | (vn & cn)
    else:
        c = int(c)
        assert I64_MIN <= c <= I64_MAX
        lt = v < c
        eq = v == c
    gt = ~lt & ~eq
    m = {ca.PRED_LT: lt, ca.PRED_LE: lt | eq, ca.PRED_GT: gt,
         ca.PRED_GE: gt | eq, ca.PRED_EQ: eq, ca.PRED_NE: ~eq}[op]
    return m & col.present


def pass_mask(cols, preds):
    m = np.ones(len(cols[0].values), dtype=bool)
    for p in preds:
        m &= pred_mask(cols[p[0]], p[1], p[2])
    return m


def wrap128(x):
    x &= (1 << 128) - 1
    return x - (1 << 128) if x >> 127 else x


def float_sum(vals):
    """the exactly rounded sum, with IEEE's rules for the non-finite cases"""
    import math
    if any(v != v for v in vals):
        return float("nan")
    pinf = any(v == float("inf") for v in vals)
    ninf = any(v == float("-inf") for v in vals)
    if pinf and ninf:
        return float("nan")
    if pinf or ninf:
        return float("inf") if pinf else float("-inf")
    return math.fsum(vals)


INT_KINDS = (ca.AGG_SUM_I64, ca.AGG_MIN_I64, ca.AGG_MAX_I64,
             ca.AGG_SUM_PROD_I64, ca.AGG_SUM_DISC_I64, ca.AGG_SUM_DISC_TAX_I64)
FLOAT_KINDS = (ca.AGG_SUM_F64, ca.AGG_MIN_F64, ca.AGG_MAX_F64)
COUNT_KINDS = (ca.AGG_COUNT_STAR, ca.AGG_COUNT_COL)


def fits64(x):
    return I64_MIN <= x <= I64_MAX


def pick_one(cols, agg):
    """the fixed-point ONE of a disc / disc_tax spec: 100 (scale 2) unless
    ONE - b or ONE + c would leave int64 for some row, where 0 or -1 does not
    (the ABI computes those two factors in int64)"""
    kind = agg[0]
    if kind not in (ca.AGG_SUM_DISC_I64, ca.AGG_SUM_DISC_TAX_I64):
        return 0
    b = cols[agg[2]].present_values()
    c = cols[agg[3]].present_values() if kind == ca.AGG_SUM_DISC_TAX_I64 else []
    for one in (100, 0, -1):
        if all(fits64(one - x) for x in (min(b, default=0), max(b, default=0))) and \
           all(fits64(one + x) for x in (min(c, default=0), max(c, default=0))):
            return one
    raise AssertionError("no ONE keeps the factors inside int64")


def with_one(cols, aggs):
    """agg specs completed to (kind, a, b, c, one)"""
    out = []
    for a in aggs:
        a = tuple(a) + (-1, -1, -1)[len(a) - 1:]
        out.append(a[:4] + (pick_one(cols, a),))
    return out


def expect_agg(cols, agg, rows):
    """expected partial of one (kind, a, b, c, one) spec over the boolean row
    mask `rows`: {"count", "is_null", "i128" or "f64"}"""
    kind, a, b, c, one = agg
    if kind == ca.AGG_COUNT_STAR:
        n = int(rows.sum())
        return {"count": n, "is_null": False, "i128": n}
    m = rows & cols[a].present
    if kind in (ca.AGG_SUM_PROD_I64, ca.AGG_SUM_DISC_I64, ca.AGG_SUM_DISC_TAX_I64):
        m = m & cols[b].present
    if kind == ca.AGG_SUM_DISC_TAX_I64:
        m = m & cols[c].present
    n = int(m.sum())
    if kind == ca.AGG_COUNT_COL:
        return {"count": n, "is_null": False, "i128": n}
    if n == 0:
        return {"count": 0, "is_null": True}
    va = cols[a].wide[m].tolist()
    if kind in FLOAT_KINDS:
        assert cols[a].is_float
        if kind == ca.AGG_SUM_F64:
            f = float_sum(va)
        elif kind == ca.AGG_MIN_F64:
            f = min(va, key=pg_sort_key)
        else:
            f = max(va, key=pg_sort_key)
        return {"count": n, "is_null": False, "f64": f}
    assert not cols[a].is_float
    if kind == ca.AGG_SUM_I64:
        v = sum(va)
    elif kind == ca.AGG_MIN_I64:
        v = min(va)
    elif kind == ca.AGG_MAX_I64:
        v = max(va)
    else:
        vb = cols[b].wide[m].tolist()
        if kind == ca.AGG_SUM_PROD_I64:
            v = sum(x * y for x, y in zip(va, vb))
        elif kind == ca.AGG_SUM_DISC_I64:
            assert all(fits64(one - y) for y in vb)
            v = sum(x * (one - y) for x, y in zip(va, vb))
        else:
            vc = cols[c].wide[m].tolist()
            assert all(fits64(one - y) for y in vb)
            assert all(fits64(one + z) for z in vc)
            v = sum(x * (one - y) * (one + z) for x, y, z in zip(va, vb, vc))
    return {"count": n, "is_null": False, "i128": wrap128(v)}


def f64_bits(x):
    return int(np.array([x], dtype=np.float64).view(np.uint64)[0])


def check_partial(got, exp, kind, what):
    """got: anything with count / is_null / i128 / f64 (a Partial or a dict).
    Counts, is_null and integers exact; float MIN/MAX by bit pattern (NaN as
    NaN); SUM_F64 within 1e-6 relative of the exactly rounded sum (the
    project's bar, BASELINE.json), NaN and infinities exact."""
    if not isinstance(got, dict):
        got = got.as_dict()
    assert got["count"] == exp["count"], f"{what}: count {got['count']} != {exp['count']}"
    assert bool(got["is_null"]) == exp["is_null"], f"{what}: is_null {got['is_null']}"
    if exp["is_null"]:
        return
    if kind in FLOAT_KINDS:
        g, e = float(got["f64"]), exp["f64"]
        if e != e:
            assert g != g, f"{what}: {g!r} is not NaN"
        elif kind == ca.AGG_SUM_F64 and abs(e) != float("inf"):
            assert g == g and abs(g - e) <= 1e-6 * abs(e), f"{what}: sum {g!r} vs {e!r}"
        else:
            assert f64_bits(g) == f64_bits(e), f"{what}: {g!r} vs {e!r} (bit patterns)"
    else:
        assert got["i128"] == exp["i128"], f"{what}: {got['i128']} != {exp['i128']}"
