"""
citus_amd — MI355X-native implementation of Citus's columnar scan +
partial-aggregate hot path (chunk-group read -> LZ4 decode -> qual filter ->
partial aggregate -> combine), behind the reference's scan/combine surfaces
restated as a C ABI (include/cstripe.h).

This package is ctypes plumbing over libcstripe.so (hand-written HIP/CDNA4
kernels + host C++). The GPU path requires a visible MI355X and fails loudly
without one; the CPU reference restatement lives in oracle/ and is test
infrastructure only.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libcstripe.so")

if not os.path.exists(_LIB_PATH):
    raise ImportError(
        "libcstripe.so not built — run `make -C citus_amd/csrc` "
        "(or __graft_entry__.build())")

# Two HIP runtime instances in one process (torch's bundled copy + the
# system /opt/rocm one) break device enumeration for whichever initializes
# second — in either direction on some boxes. Both ship the same soname
# (libamdhip64.so.7), so preloading torch's copy globally makes
# libcstripe's NEEDED entry resolve to the SAME mapped runtime: one HIP
# instance shared by both stacks. Plain-C ABI consumers (no torch in the
# process) are unaffected and keep the system runtime.
try:
    import torch as _torch
    _torch_hip = os.path.join(os.path.dirname(_torch.__file__), "lib",
                              "libamdhip64.so")
    if os.path.exists(_torch_hip):
        C.CDLL(_torch_hip, mode=C.RTLD_GLOBAL)
except Exception:
    pass

_lib = C.CDLL(_LIB_PATH)

# ---- enums (include/cstripe.h) ----
I8, I16, I32, I64, F32, F64, TEXT = 1, 2, 3, 4, 5, 6, 7
VARTEXT = 8                      # general variable-length text (device dictionary)
VARTEXT_MAX_LEN = 65535
VARTEXT_MAX_DISTINCT = 1 << 20
COMP_NONE, COMP_PGLZ, COMP_LZ4, COMP_ZSTD = 0, 1, 2, 3
PRED_LT, PRED_LE, PRED_GT, PRED_GE, PRED_EQ, PRED_NE = range(6)
PRED_IN, PRED_NOT_IN = 6, 7      # value is a set (see make_preds_sets)
PRED_LIKE, PRED_NOT_LIKE = 8, 9  # value is the pattern (bytes / str), VARTEXT only
LIKE_MAX_PATTERN = 256
LIKE_FORM_NONE, LIKE_FORM_DICT, LIKE_FORM_STREAM = 0, 1, 2
MAX_SETS = 4
MAX_SET_VALUES = 1 << 26
SET_FORM_NONE, SET_FORM_HASH, SET_FORM_BITMAP = 0, 1, 2
(AGG_COUNT_STAR, AGG_COUNT_COL, AGG_SUM_I64, AGG_SUM_F64,
 AGG_MIN_I64, AGG_MAX_I64, AGG_MIN_F64, AGG_MAX_F64,
 AGG_SUM_PROD_I64, AGG_SUM_DISC_I64, AGG_SUM_DISC_TAX_I64) = range(11)

OK, ERR, ERR_IO, ERR_FORMAT, ERR_NOGPU, ERR_ARG, END = 0, -1, -2, -3, -4, -5, 1


class ColDef(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("type", C.c_uint8),
                ("scale", C.c_uint8), ("_pad", C.c_uint8 * 6)]


class Options(C.Structure):
    _fields_ = [("stripe_row_limit", C.c_uint64),
                ("chunk_group_row_limit", C.c_uint32),
                ("compression", C.c_uint8), ("compression_level", C.c_int8),
                ("lz4_seg_target_kb", C.c_uint16),
                ("lz4_seg_target_bytes", C.c_uint32),
                ("lz4_min_match", C.c_uint8), ("canonical", C.c_uint8),
                ("_pad2", C.c_uint8 * 6)]


class Pred(C.Structure):
    _fields_ = [("column", C.c_uint32), ("op", C.c_uint32),
                ("ival", C.c_int64), ("fval", C.c_double),
                ("or_group", C.c_uint32), ("_pad", C.c_uint32)]


class VarTextIn(C.Structure):
    _fields_ = [("offsets", C.c_void_p), ("bytes", C.c_void_p)]


class TextConst(C.Structure):
    _fields_ = [("data", C.c_char_p), ("len", C.c_uint32)]


class ValueSet(C.Structure):
    _fields_ = [("values", C.c_void_p), ("texts", C.POINTER(TextConst)),
                ("n", C.c_uint64), ("on_device", C.c_uint32), ("_pad", C.c_uint32)]


MAX_LOOKUPS = 2
MAX_LOOKUP_PAYLOADS = 4
LOOKUP_INNER = 1
LOOKUP_FORM_NONE, LOOKUP_FORM_HASH, LOOKUP_FORM_DIRECT = 0, 1, 2


class LookupIn(C.Structure):
    """cstripe_lookup"""
    _fields_ = [("key_column", C.c_uint32), ("n_payloads", C.c_uint32),
                ("keys", C.c_void_p),
                ("payloads", C.c_void_p * MAX_LOOKUP_PAYLOADS),
                ("n", C.c_uint64), ("on_device", C.c_uint32), ("flags", C.c_uint32)]


class Lookup:
    """The build side of an N:1 join for Reader.scan(lookups=[...]): the
    scanned table's `key_col` is looked up in `keys` (distinct, no NULLs) and
    every array of `payloads` (parallel to keys) becomes a derived int64
    column of the scan, NULL where the row has no match (a left join);
    inner=True drops those rows. keys and payloads are sequences / ndarrays
    of ints (copied at scan begin) or contiguous int64 torch tensors on the
    GPU, all of them, which are then read in place at every stage() and kept
    alive by the scan."""

    def __init__(self, key_col, keys, payloads, inner=False):
        self.key_col = key_col
        self.keys = keys
        self.payloads = list(payloads)
        self.inner = bool(inner)


def _is_torch(v):
    return type(v).__module__.split(".")[0] == "torch"


def make_lookups(lookups):
    """(LookupIn array or None, n) for cstripe_scan_begin_lookups; the array
    keeps every buffer it points at alive"""
    import numpy as np
    if not lookups:
        return None, 0
    arr = (LookupIn * len(lookups))()
    keep = []
    for i, lk in enumerate(lookups):
        arrays = [lk.keys] + lk.payloads
        dev = [_is_torch(a) for a in arrays]
        if any(dev) and not all(dev):
            raise CStripeError(f"lookup {i}: keys and payloads must all be host arrays "
                               "or all GPU tensors")
        arr[i].key_column = lk.key_col
        arr[i].n_payloads = len(lk.payloads)
        arr[i].flags = LOOKUP_INNER if lk.inner else 0
        n = len(lk.keys)
        arr[i].n = n
        ptrs = []
        if all(dev):
            import torch
            for a in arrays:
                if not a.is_cuda or str(a.dtype) != "torch.int64" or not a.is_contiguous() \
                        or a.dim() != 1 or a.numel() != n:
                    raise CStripeError(f"lookup {i}: a device map needs contiguous 1-d int64 "
                                       "GPU tensors of one length")
                ptrs.append(a.data_ptr() if n else None)
                keep.append(a)
            torch.cuda.synchronize(arrays[0].device)
            arr[i].on_device = 1
        else:
            for a in arrays:
                if len(a) != n:
                    raise CStripeError(f"lookup {i}: keys and payloads differ in length")
                h = np.ascontiguousarray(np.asarray(a).astype(np.int64, copy=False)
                                         if n else np.zeros(0, np.int64))
                ptrs.append(h.ctypes.data_as(C.c_void_p).value if n else None)
                keep.append(h)
        arr[i].keys = ptrs[0]
        for p_, q in enumerate(ptrs[1:MAX_LOOKUP_PAYLOADS + 1]):
            arr[i].payloads[p_] = q
    arr._keep = keep
    return arr, len(lookups)


MAX_EXPRS = 8
MAX_EXPR_OPS = 48
MAX_EXPR_DEPTH = 8
(EX_COL, EX_CONST, EX_NULL, EX_ADD, EX_SUB, EX_MUL, EX_DIV, EX_MOD, EX_NEG,
 EX_LT, EX_LE, EX_GT, EX_GE, EX_EQ, EX_NE, EX_AND, EX_OR, EX_NOT,
 EX_IS_NULL, EX_COALESCE, EX_SELECT, EX_YEAR) = range(22)


class ExprOp(C.Structure):
    """cstripe_expr_op"""
    _fields_ = [("op", C.c_uint32), ("column", C.c_uint32), ("ival", C.c_int64)]


class ExprIn(C.Structure):
    """cstripe_expr"""
    _fields_ = [("ops", C.POINTER(ExprOp)), ("n_ops", C.c_uint32), ("_pad", C.c_uint32)]


class Expr:
    """A row-level int64 expression for Reader.scan(exprs=[...]), built from
    col(i), lit(v) and null() with + - * // % and unary -, the comparisons
    .lt/.le/.gt/.ge/.eq/.ne (0 / 1), the three-valued & | ~, .is_null(),
    .year(), coalesce(a, b) and case(cond, then, else_). A Python int where
    an expression is expected is a literal. `ops` is the postfix program, a
    list of (op, column, ival) tuples; // and % follow PG int8 (truncation
    toward zero, the dividend's sign), not Python. See
    cstripe_scan_begin_exprs in include/cstripe.h for the value semantics."""

    def __init__(self, ops):
        self.ops = list(ops)

    def _bin(self, op, other, swap=False):
        a, b = (as_expr(other), self) if swap else (self, as_expr(other))
        return Expr(a.ops + b.ops + [(op, 0, 0)])

    def __add__(self, o): return self._bin(EX_ADD, o)
    def __radd__(self, o): return self._bin(EX_ADD, o, True)
    def __sub__(self, o): return self._bin(EX_SUB, o)
    def __rsub__(self, o): return self._bin(EX_SUB, o, True)
    def __mul__(self, o): return self._bin(EX_MUL, o)
    def __rmul__(self, o): return self._bin(EX_MUL, o, True)
    def __floordiv__(self, o): return self._bin(EX_DIV, o)
    def __rfloordiv__(self, o): return self._bin(EX_DIV, o, True)
    def __mod__(self, o): return self._bin(EX_MOD, o)
    def __rmod__(self, o): return self._bin(EX_MOD, o, True)
    def __and__(self, o): return self._bin(EX_AND, o)
    def __rand__(self, o): return self._bin(EX_AND, o, True)
    def __or__(self, o): return self._bin(EX_OR, o)
    def __ror__(self, o): return self._bin(EX_OR, o, True)
    def __neg__(self): return Expr(self.ops + [(EX_NEG, 0, 0)])
    def __invert__(self): return Expr(self.ops + [(EX_NOT, 0, 0)])
    def lt(self, o): return self._bin(EX_LT, o)
    def le(self, o): return self._bin(EX_LE, o)
    def gt(self, o): return self._bin(EX_GT, o)
    def ge(self, o): return self._bin(EX_GE, o)
    def eq(self, o): return self._bin(EX_EQ, o)
    def ne(self, o): return self._bin(EX_NE, o)
    def is_null(self): return Expr(self.ops + [(EX_IS_NULL, 0, 0)])
    def year(self): return Expr(self.ops + [(EX_YEAR, 0, 0)])


def as_expr(v):
    """an Expr as it is; a Python / numpy int as a literal"""
    if isinstance(v, Expr):
        return v
    if isinstance(v, bool) or not hasattr(v, "__index__"):
        raise CStripeError(f"expression operand {v!r} is neither an Expr nor an int")
    return lit(v)


def col(i):
    """the value of table or lookup-derived column i"""
    return Expr([(EX_COL, int(i), 0)])


def lit(v):
    """the int64 constant v"""
    v = int(v)
    if not -(1 << 63) <= v < (1 << 63):
        raise CStripeError(f"expression literal {v} is outside int64")
    return Expr([(EX_CONST, 0, v)])


def null():
    return Expr([(EX_NULL, 0, 0)])


def coalesce(a, b):
    """a unless it is NULL, then b"""
    return Expr(as_expr(a).ops + as_expr(b).ops + [(EX_COALESCE, 0, 0)])


def case(cond, then, else_=None):
    """CASE WHEN cond THEN then ELSE else_ END; else_ defaults to NULL"""
    e = null() if else_ is None else as_expr(else_)
    return Expr(as_expr(cond).ops + as_expr(then).ops + e.ops + [(EX_SELECT, 0, 0)])


def make_exprs(exprs):
    """(ExprIn array or None, n) for cstripe_scan_begin_exprs from Expr
    objects, ints, or raw lists of (op, column, ival) tuples; the array keeps
    the op arrays it points at alive"""
    if not exprs:
        return None, 0
    arr = (ExprIn * len(exprs))()
    keep = []
    for i, ex in enumerate(exprs):
        ops = list(ex) if isinstance(ex, (list, tuple)) else as_expr(ex).ops
        oa = (ExprOp * max(1, len(ops)))()
        for k, (op, column, ival) in enumerate(ops):
            oa[k].op, oa[k].column, oa[k].ival = int(op), int(column), int(ival)
        arr[i].ops = C.cast(oa, C.POINTER(ExprOp))
        arr[i].n_ops = len(ops)
        keep.append(oa)
    arr._keep = keep
    return arr, len(exprs)


class AggSpec(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("col_a", C.c_int32), ("col_b", C.c_int32),
                ("col_c", C.c_int32), ("one", C.c_int64)]


class Partial(C.Structure):
    _fields_ = [("i128_lo", C.c_int64), ("i128_hi", C.c_int64), ("f64", C.c_double),
                ("count", C.c_int64), ("is_null", C.c_uint8), ("_pad", C.c_uint8 * 7)]

    @property
    def i128(self):
        """signed 128-bit view (sums; min/max are sign-extended into hi)"""
        return (self.i128_hi << 64) | (self.i128_lo & ((1 << 64) - 1))

    def as_dict(self):
        return {"i128": self.i128, "f64": self.f64, "count": self.count,
                "is_null": bool(self.is_null)}


class Batch(C.Structure):
    _fields_ = [("n_rows", C.c_uint32), ("first_row_number", C.c_uint64),
                ("col_values", C.POINTER(C.c_void_p)),
                ("col_nulls", C.POINTER(C.POINTER(C.c_uint8)))]


class Rows(C.Structure):
    _fields_ = [("n_rows", C.c_uint64),
                ("col_values", C.POINTER(C.c_void_p)),
                ("col_nulls", C.POINTER(C.c_void_p)),
                ("row_numbers", C.c_void_p)]


MAX_ORDER_COLS = 4
MAX_TOPN = 1 << 20
ORDER_DESC = 1
ORDER_NULLS_FIRST = 2            # absent = NULLS LAST


class OrderKey(C.Structure):
    _fields_ = [("column", C.c_uint32), ("flags", C.c_uint32)]


MAX_HASH_KEY_COLS = 4
MAX_HASH_GROUPS = 1 << 24


class HGroups(C.Structure):
    _fields_ = [("n_groups", C.c_uint64),
                ("keys", C.c_void_p * MAX_HASH_KEY_COLS),
                ("key_nulls", C.c_void_p * MAX_HASH_KEY_COLS),
                ("partials", C.c_void_p)]


MAX_GROUP_ORDER = 4
MAX_HAVING = 4
GORDER_AGG = 0                   # index = position in aggs
GORDER_KEY = 1                   # index = position in key_cols


class GroupOrder(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("index", C.c_uint32), ("flags", C.c_uint32),
                ("_pad", C.c_uint32)]


class Having(C.Structure):
    _fields_ = [("agg", C.c_uint32), ("op", C.c_uint32), ("ival", C.c_int64),
                ("fval", C.c_double)]


def partial_dtype():
    """numpy structured dtype mirroring cstripe_partial (40 bytes)"""
    import numpy as np
    return np.dtype([("i128_lo", "<i8"), ("i128_hi", "<i8"), ("f64", "<f8"),
                     ("count", "<i8"), ("is_null", "u1"), ("_pad", "u1", (7,))])


def partial_i128(p):
    """signed 128-bit Python int of one structured-array partial"""
    return (int(p["i128_hi"]) << 64) | (int(p["i128_lo"]) & ((1 << 64) - 1))


class GroupResult(C.Structure):
    _fields_ = [("n_groups", C.c_uint32), ("keys", C.c_uint32 * 64)]


GROUP_KEY_NULL = 0x100          # 9-bit key encoding: bit 8 = NULL key


def decode_group_key(kv):
    """(k0, k1) from the packed 9-bit-per-column encoding; NULL keys (their
    own group, like the reference HashAggregate) decode to None."""
    e0 = kv & 0x1FF
    e1 = (kv >> 9) & 0x1FF
    return (None if e0 & GROUP_KEY_NULL else e0,
            None if e1 & GROUP_KEY_NULL else e1)


def encode_group_key(k):
    e0 = GROUP_KEY_NULL if k[0] is None else k[0]
    k1 = k[1] if len(k) > 1 else 0
    e1 = GROUP_KEY_NULL if k1 is None else k1
    return e0 | (e1 << 9)


def _sig(name, res, args):
    f = getattr(_lib, name)
    f.restype = res
    f.argtypes = args
    return f


_errmsg = _sig("cstripe_errmsg", C.c_char_p, [])
_default_options = _sig("cstripe_default_options", None, [C.POINTER(Options)])
_write_begin = _sig("cstripe_write_begin", C.c_void_p,
                    [C.c_char_p, C.POINTER(ColDef), C.c_uint32, C.POINTER(Options)])
_write_rows = _sig("cstripe_write_rows", C.c_int,
                   [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)])
_write_end = _sig("cstripe_write_end", C.c_int, [C.c_void_p])
_write_abort = _sig("cstripe_write_abort", None, [C.c_void_p])
_write_rows_device = _sig("cstripe_write_rows_device", C.c_int,
                          [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)])
_open = _sig("cstripe_open", C.c_void_p, [C.c_char_p])
_close = _sig("cstripe_close", None, [C.c_void_p])
_row_count = _sig("cstripe_row_count", C.c_uint64, [C.c_void_p])
_column_count = _sig("cstripe_column_count", C.c_uint32, [C.c_void_p])
_stripe_count = _sig("cstripe_stripe_count", C.c_uint32, [C.c_void_p])
_column_def = _sig("cstripe_column_def", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(ColDef)])
_scan_begin = _sig("cstripe_scan_begin", C.c_void_p,
                   [C.c_void_p, C.c_uint64, C.POINTER(Pred), C.c_uint32])
_scan_begin_ex = _sig("cstripe_scan_begin_ex", C.c_void_p,
                      [C.c_void_p, C.c_uint64, C.POINTER(Pred), C.c_uint32,
                       C.POINTER(TextConst), C.c_uint32])
_scan_begin_sets = _sig("cstripe_scan_begin_sets", C.c_void_p,
                        [C.c_void_p, C.c_uint64, C.POINTER(Pred), C.c_uint32,
                         C.POINTER(TextConst), C.c_uint32,
                         C.POINTER(ValueSet), C.c_uint32])
_scan_begin_lookups = _sig("cstripe_scan_begin_lookups", C.c_void_p,
                           [C.c_void_p, C.c_uint64, C.POINTER(Pred), C.c_uint32,
                            C.POINTER(TextConst), C.c_uint32,
                            C.POINTER(ValueSet), C.c_uint32,
                            C.POINTER(LookupIn), C.c_uint32])
_scan_begin_exprs = _sig("cstripe_scan_begin_exprs", C.c_void_p,
                         [C.c_void_p, C.c_uint64, C.POINTER(Pred), C.c_uint32,
                          C.POINTER(TextConst), C.c_uint32,
                          C.POINTER(ValueSet), C.c_uint32,
                          C.POINTER(LookupIn), C.c_uint32,
                          C.POINTER(ExprIn), C.c_uint32])
_expr_range = _sig("cstripe_scan_expr_range", C.c_int,
                   [C.c_void_p, C.c_uint32, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                    C.POINTER(C.c_uint64)])
_last_expr_ms = _sig("cstripe_scan_last_expr_ms", C.c_int,
                     [C.c_void_p, C.POINTER(C.c_double)])
_scan_column_count = _sig("cstripe_scan_column_count", C.c_uint32, [C.c_void_p])
_last_lookup_ms = _sig("cstripe_scan_last_lookup_ms", C.c_int,
                       [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)])
_lookup_form = _sig("cstripe_scan_lookup_form", C.c_int,
                    [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)])
_last_set_ms = _sig("cstripe_scan_last_set_ms", C.c_int,
                    [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)])
_set_form = _sig("cstripe_scan_set_form", C.c_int,
                 [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)])
_like_match = _sig("cstripe_like_match", C.c_int,
                   [C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32])
_last_like_ms = _sig("cstripe_scan_last_like_ms", C.c_int,
                     [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)])
_like_form = _sig("cstripe_scan_like_form", C.c_int, [C.c_void_p, C.c_uint32])
_vartext_validate = _sig("cstripe_vartext_validate", C.c_int,
                         [C.c_char_p, C.c_uint64, C.c_uint32])
_text_dict = _sig("cstripe_scan_text_dict", C.c_int,
                  [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32),
                   C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.POINTER(C.c_uint8))])
_last_text_ms = _sig("cstripe_scan_last_text_ms", C.c_int,
                     [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                      C.POINTER(C.c_double), C.POINTER(C.c_double)])
_scan_end = _sig("cstripe_scan_end", None, [C.c_void_p])
_filtered = _sig("cstripe_scan_chunk_groups_filtered", C.c_int64, [C.c_void_p])
_gpu_stage = _sig("cstripe_gpu_stage", C.c_int, [C.c_void_p, C.c_int])
_staged_bytes = _sig("cstripe_gpu_staged_bytes", C.c_uint64, [C.c_void_p])
_scan_agg = _sig("cstripe_scan_agg", C.c_int,
                 [C.c_void_p, C.POINTER(AggSpec), C.c_uint32, C.POINTER(Partial)])
_scan_agg_grouped = _sig("cstripe_scan_agg_grouped", C.c_int,
                         [C.c_void_p, C.POINTER(AggSpec), C.c_uint32,
                          C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(GroupResult),
                          C.POINTER(Partial)])
_next_batch = _sig("cstripe_scan_next_batch", C.c_int, [C.c_void_p, C.POINTER(Batch)])
_read_row = _sig("cstripe_read_row", C.c_int,
                 [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p),
                  C.POINTER(C.c_uint8)])
_select_count = _sig("cstripe_scan_select_count", C.c_int,
                     [C.c_void_p, C.POINTER(C.c_uint64)])
_select = _sig("cstripe_scan_select", C.c_int,
               [C.c_void_p, C.POINTER(Rows), C.c_uint64, C.c_int])
_last_select_ms = _sig("cstripe_scan_last_select_ms", C.c_int,
                       [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                        C.POINTER(C.c_double)])
_select_topn = _sig("cstripe_scan_select_topn", C.c_int,
                    [C.c_void_p, C.POINTER(OrderKey), C.c_uint32, C.c_uint64,
                     C.POINTER(Rows), C.c_int])
_last_topn_ms = _sig("cstripe_scan_last_topn_ms", C.c_int,
                     [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                      C.POINTER(C.c_double)])
_scan_agg_hashed = _sig("cstripe_scan_agg_hashed", C.c_int,
                        [C.c_void_p, C.POINTER(AggSpec), C.c_uint32,
                         C.POINTER(C.c_uint32), C.c_uint32, C.c_uint64,
                         C.POINTER(HGroups)])
_last_hash_ms = _sig("cstripe_scan_last_hash_ms", C.c_int,
                     [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                      C.POINTER(C.c_double)])
_scan_agg_hashed_topn = _sig("cstripe_scan_agg_hashed_topn", C.c_int,
                             [C.c_void_p, C.POINTER(AggSpec), C.c_uint32,
                              C.POINTER(C.c_uint32), C.c_uint32, C.c_uint64,
                              C.POINTER(Having), C.c_uint32,
                              C.POINTER(GroupOrder), C.c_uint32, C.c_uint64,
                              C.POINTER(HGroups)])
_last_group_topn = _sig("cstripe_scan_last_group_topn", C.c_int,
                        [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                         C.POINTER(C.c_double), C.POINTER(C.c_double),
                         C.POINTER(C.c_double)])
_combine_groups = _sig("cagg_combine_groups", C.c_int,
                       [C.POINTER(AggSpec), C.c_uint32, C.c_uint32,
                        C.POINTER(HGroups), C.c_uint32, C.POINTER(HGroups),
                        C.c_uint64])
_rewind = _sig("cstripe_scan_rewind", C.c_int, [C.c_void_p])
_last_fused = _sig("cstripe_scan_last_fused", C.c_int, [C.c_void_p])
_last_agg_path = _sig("cstripe_scan_last_agg_path", C.c_int, [C.c_void_p])
_last_kernel_ms = _sig("cstripe_scan_last_kernel_ms", C.c_double, [C.c_void_p])
_last_decode_ms = _sig("cstripe_scan_last_decode_kernel_ms", C.c_double, [C.c_void_p])
_last_agg_ms = _sig("cstripe_scan_last_agg_kernel_ms", C.c_double, [C.c_void_p])
_combine = _sig("cagg_combine", C.c_int,
                [C.POINTER(AggSpec), C.c_uint32, C.POINTER(Partial), C.c_uint32,
                 C.POINTER(Partial)])
_gpu_available = _sig("cstripe_gpu_available", C.c_int, [])
_comm_uid = _sig("cagg_comm_unique_id", C.c_int, [C.c_uint8 * 128])
_comm_init = _sig("cagg_comm_init", C.c_int,
                  [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_uint8 * 128, C.c_int])
_comm_destroy = _sig("cagg_comm_destroy", None, [C.c_void_p])
_comm_allgather = _sig("cagg_allgather", C.c_int,
                       [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p])
_combine_rccl = _sig("cagg_combine_rccl", C.c_int,
                     [C.c_void_p, C.POINTER(AggSpec), C.c_uint32,
                      C.POINTER(Partial), C.POINTER(Partial)])
_gen_lineitem = _sig("csbench_gen_lineitem", C.c_int,
                     [C.c_char_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int,
                      C.c_uint64, C.c_uint32])
_gen_lineitem2 = _sig("csbench_gen_lineitem2", C.c_int,
                      [C.c_char_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int,
                       C.c_uint64, C.c_uint32, C.c_int, C.c_int])
_gen_shards = _sig("csbench_gen_lineitem_shards", C.c_int,
                   [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, C.c_int,
                    C.c_int, C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_int])
_expected_q6 = _sig("csbench_expected_q6", C.c_int,
                    [C.c_uint64, C.c_uint64, C.POINTER(C.c_int64),
                     C.POINTER(C.c_int64), C.POINTER(C.c_int64)])
_expected_q1 = _sig("csbench_expected_q1", C.c_int,
                    [C.c_uint64, C.c_uint64, C.POINTER(C.c_int64),
                     C.POINTER(C.c_int64), C.POINTER(C.c_int64)])


def errmsg():
    return _errmsg().decode()


def gpu_available():
    return bool(_gpu_available())


class CStripeError(RuntimeError):
    pass


def _check(rc, what):
    if rc != OK:
        raise CStripeError(f"{what} failed (rc={rc}): {errmsg()}")


def default_options(**kw):
    o = Options()
    _default_options(C.byref(o))
    if "lz4_seg_target_kb" in kw and "lz4_seg_target_bytes" not in kw:
        kw["lz4_seg_target_bytes"] = 0   # the coarse knob overrides the default
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def text_slot(sval):
    """4-byte short-varlena slot (the reference's stored datum bytes) for a
    text value of <= 3 payload bytes: hdr = ((len+1)<<1)|1, payload, zero pad.
    Returns the slot as a little-endian u32 (use for TEXT predicates)."""
    b = sval.encode() if isinstance(sval, str) else bytes(sval)
    assert 1 <= len(b) <= 3
    slot = bytes([((len(b) + 1) << 1) | 1]) + b + b"\0" * (3 - len(b))
    return int.from_bytes(slot, "little")


def text_slots(values):
    """numpy uint32 array of varlena slots for a sequence of short strings"""
    import numpy as np
    return np.array([text_slot(v) for v in values], dtype=np.uint32)


def slot_text(slot):
    """decode a u32 varlena slot back to its string"""
    b = int(slot).to_bytes(4, "little")
    n = (b[0] >> 1) - 1
    return b[1:1 + n].decode()


def make_coldefs(defs):
    """defs: list of (name, type, scale)"""
    arr = (ColDef * len(defs))()
    for i, (name, typ, scale) in enumerate(defs):
        arr[i].name = name.encode()
        arr[i].type = typ
        arr[i].scale = scale
    return arr


def vartext_pack(values):
    """(offsets uint64[n+1], bytes uint8[], nulls uint8[n] or None) for a
    sequence of bytes / str / None — the cstripe_vartext_in form of a VARTEXT
    column. str values are stored as UTF-8."""
    import numpy as np
    enc = [b"" if v is None else (v.encode() if isinstance(v, str) else bytes(v))
           for v in values]
    offs = np.zeros(len(enc) + 1, dtype=np.uint64)
    if enc:
        offs[1:] = np.cumsum([len(b) for b in enc], dtype=np.uint64)
    data = np.frombuffer(b"".join(enc), dtype=np.uint8)
    nulls = None
    if any(v is None for v in values):
        nulls = np.array([1 if v is None else 0 for v in values], dtype=np.uint8)
    return offs, data, nulls


def like_match(pattern, value):
    """cstripe_like_match: whether `value` matches the LIKE `pattern` (bytes
    or str each) — PG LIKE, default escape, "C" collation, UTF-8 characters;
    the matcher source the device runs. Raises CStripeError for a pattern
    scan_begin would refuse."""
    p = pattern.encode() if isinstance(pattern, str) else bytes(pattern)
    v = value.encode() if isinstance(value, str) else bytes(value)
    rc = _like_match(p, len(p), v, len(v))
    if rc < 0:
        raise CStripeError(f"like_match failed (rc={rc}): {errmsg()}")
    return bool(rc)


def vartext_validate(stream, n_values):
    """cstripe_vartext_validate: OK when exactly n_values varlena datums tile
    the stream, ERR_FORMAT otherwise (host only)."""
    stream = bytes(stream)
    return _vartext_validate(stream, len(stream), n_values)


def write_table(path, defs, columns, nulls=None, **opt_kw):
    """Write numpy columns to a stripe file. columns: list of np arrays
    (dtype matching coldef types); nulls: optional list of uint8 arrays.
    A VARTEXT column is a list of bytes / str / None (None = NULL, merged
    with that column's nulls entry when both are given), or an
    (offsets uint64[n+1], bytes uint8[]) pair of numpy arrays."""
    import numpy as np
    opts = default_options(**opt_kw)
    cols = make_coldefs(defs)
    n = None
    vals = (C.c_void_p * len(defs))()
    keep = []
    text_nulls = {}
    for i, a in enumerate(columns):
        if defs[i][1] == VARTEXT:
            if isinstance(a, tuple):
                offs, data = a
            else:
                offs, data, tn = vartext_pack(a)
                if tn is not None:
                    text_nulls[i] = tn
            offs = np.ascontiguousarray(offs, dtype=np.uint64)
            data = np.ascontiguousarray(data, dtype=np.uint8)
            vt = VarTextIn(offs.ctypes.data, data.ctypes.data if data.size else None)
            keep += [offs, data, vt]
            vals[i] = C.addressof(vt)
            rows = len(offs) - 1
        else:
            a = np.ascontiguousarray(a)
            columns[i] = a
            vals[i] = a.ctypes.data_as(C.c_void_p).value
            rows = len(a)
        n = rows if n is None else n
        if rows != n:
            raise CStripeError(f"write_table: column {i} has {rows} rows, column 0 has {n}")
    nl = None
    if nulls is not None or text_nulls:
        nl = (C.c_void_p * len(defs))()
        for i in range(len(defs)):
            a = nulls[i] if nulls is not None else None
            if i in text_nulls:
                a = text_nulls[i] if a is None else \
                    (np.asarray(a, dtype=np.uint8) | text_nulls[i])
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.uint8)
                keep.append(a)
                nl[i] = a.ctypes.data_as(C.c_void_p).value
    w = _write_begin(path.encode(), cols, len(defs), C.byref(opts))
    if not w:
        raise CStripeError("write_begin: " + errmsg())
    rc = _write_rows(w, n, vals, nl)
    if rc != OK:
        msg = errmsg()
        _write_abort(w)
        raise CStripeError(f"write_rows failed (rc={rc}): {msg}")
    _check(_write_end(w), "write_end")


def write_table_device(path, defs, dev_ptrs, n_rows, **opt_kw):
    """Device-side write (cstripe_write_rows_device): dev_ptrs are raw HBM
    addresses of column arrays (e.g. torch tensor.data_ptr()); full chunks
    compress on the GPU, only compressed bytes cross PCIe."""
    opts = default_options(**opt_kw)
    cols = make_coldefs(defs)
    w = _write_begin(path.encode(), cols, len(defs), C.byref(opts))
    if not w:
        raise CStripeError("write_begin: " + errmsg())
    vals = (C.c_void_p * len(defs))(*[int(p) for p in dev_ptrs])
    rc = _write_rows_device(w, n_rows, vals)
    if rc != OK:
        _write_end(w)
        raise CStripeError(f"write_rows_device failed (rc={rc}): {errmsg()}")
    _check(_write_end(w), "write_end")


def gen_lineitem_shards(dirpath, total_rows, n_shards, base_seed=42,
                        compression=COMP_LZ4, level=3, seg_kb=0, stripe_rows=0,
                        chunk_rows=0, min_match=0, canonical=1, threads=0):
    """Parallel sharded generation: n_shards files shardNN.cs under dirpath
    (the config-3 shard-directory shape), seeds base_seed + i."""
    os.makedirs(dirpath, exist_ok=True)
    _check(_gen_shards(dirpath.encode(), total_rows, n_shards, base_seed,
                       compression, level, seg_kb, stripe_rows, chunk_rows,
                       min_match, canonical, threads), "gen_lineitem_shards")


def expected_q6(n_rows, seed=42):
    """Exact Q6 (revenue int128 at scale 4, count) recomputed from the
    generator streams on host CPU — the bench's in-run parity pin."""
    lo, hi, cnt = C.c_int64(), C.c_int64(), C.c_int64()
    _check(_expected_q6(n_rows, seed, C.byref(lo), C.byref(hi), C.byref(cnt)),
           "expected_q6")
    return (hi.value << 64) | (lo.value & ((1 << 64) - 1)), cnt.value


def expected_q1(n_rows, seed=42):
    """Exact Q1 per-(returnflag, linestatus) sums/counts from the generator.
    Returns {(rf, ls): [sum_qty, sum_price, sum_disc_price, sum_charge, count]}."""
    lo = (C.c_int64 * 24)()
    hi = (C.c_int64 * 24)()
    cnt = (C.c_int64 * 6)()
    _check(_expected_q1(n_rows, seed, lo, hi, cnt), "expected_q1")
    out = {}
    for rf in range(3):
        for ls in range(2):
            g = rf * 2 + ls
            sums = [(hi[g * 4 + k] << 64) | (lo[g * 4 + k] & ((1 << 64) - 1))
                    for k in range(4)]
            out[(rf, ls)] = sums + [cnt[g]]
    return out


def gen_lineitem(path, n_rows, seed=42, compression=COMP_LZ4, level=3, seg_kb=0,
                 stripe_rows=0, chunk_rows=0, seg_bytes=0, min_match=0,
                 canonical=1):
    if seg_bytes:
        seg_kb = -int(seg_bytes)      # negative seg_kb = bytes (csbench_gen_lineitem)
    _check(_gen_lineitem2(path.encode(), n_rows, seed, compression, level, seg_kb,
                          stripe_rows, chunk_rows, min_match, canonical),
           "gen_lineitem")


LINEITEM_COLS = {"l_orderkey": 0, "l_quantity": 1, "l_extendedprice": 2,
                 "l_discount": 3, "l_tax": 4, "l_shipdate": 5,
                 "l_returnflag": 6, "l_linestatus": 7}


class Reader:
    def __init__(self, path):
        self._h = _open(path.encode())
        if not self._h:
            raise CStripeError("open: " + errmsg())
        self.path = path

    def close(self):
        if self._h:
            _close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def row_count(self):
        return _row_count(self._h)

    @property
    def column_count(self):
        return _column_count(self._h)

    @property
    def stripe_count(self):
        return _stripe_count(self._h)

    def column_def(self, i):
        d = ColDef()
        _check(_column_def(self._h, i, C.byref(d)), "column_def")
        return d.name.decode(), d.type, d.scale

    def scan(self, cols_mask=0, preds=(), lookups=(), exprs=()):
        """lookups: a list of Lookup — each payload becomes a derived int64
        column with id column_count + ..., see Scan.derived(). exprs: a list
        of Expr (or raw postfix lists) — each becomes a computed int64 column
        after the derived ones, see Scan.computed()"""
        return Scan(self, cols_mask, preds, lookups, exprs)


def make_preds(preds):
    """preds: (column, op, value) or (column, op, value, or_group) tuples.
    A nonzero or_group groups predicates into a disjunction (CNF; see
    include/cstripe.h)."""
    return make_preds_ex(preds)[0]


def make_preds_ex(preds):
    """make_preds plus the string constants: a bytes / str value (a VARTEXT
    predicate) becomes an index into the returned cstripe_text_const array.
    Returns (Pred array, TextConst array or None, n_text_consts)."""
    arr = (Pred * max(1, len(preds)))()
    texts = []
    for i, p in enumerate(preds):
        arr[i].column = p[0]
        arr[i].op = p[1]
        v = p[2]
        if isinstance(v, (bytes, bytearray, str)):
            b = v.encode() if isinstance(v, str) else bytes(v)
            arr[i].ival = len(texts)
            arr[i].fval = 0.0
            texts.append(b)
        elif isinstance(v, float):
            arr[i].fval = v
            arr[i].ival = 0
        else:
            arr[i].ival = int(v)
            arr[i].fval = 0.0
        arr[i].or_group = p[3] if len(p) > 3 else 0
    if not texts:
        return arr, None, 0
    tc = (TextConst * len(texts))()
    for i, b in enumerate(texts):
        tc[i].data = b            # c_char_p keeps a reference to the bytes
        tc[i].len = len(b)
    tc._keep = texts
    return arr, tc, len(texts)


def _is_set_pred(p):
    return p[1] in (PRED_IN, PRED_NOT_IN)


def make_preds_sets(preds):
    """make_preds_ex plus the value sets of (col, PRED_IN | PRED_NOT_IN,
    values[, or_group]) predicates. `values` is a sequence / ndarray of ints
    (TEXT columns: text_slots() output), a list of bytes / str (a VARTEXT
    column), or a contiguous int64 torch tensor on the GPU, which becomes a
    device set read in place. The same `values` object given to several
    predicates is one set. Returns (Pred array, TextConst array or None,
    n_text_consts, ValueSet array or None, n_sets); the arrays keep every
    buffer they point at alive."""
    import numpy as np
    plain = [(p[0], p[1], 0) + tuple(p[3:4]) if _is_set_pred(p) else p for p in preds]
    arr, tc, n_tc = make_preds_ex(plain)
    sets, keep, index = [], [], {}
    for i, p in enumerate(preds):
        if not _is_set_pred(p):
            continue
        v = p[2]
        if id(v) in index:
            arr[i].ival = index[id(v)]
            continue
        vs = ValueSet()
        if type(v).__module__.split(".")[0] == "torch":
            if not v.is_cuda or str(v.dtype) != "torch.int64" or not v.is_contiguous():
                raise CStripeError("PRED_IN: a tensor set must be a contiguous int64 "
                                   "tensor on the GPU")
            import torch
            torch.cuda.synchronize(v.device)
            vs.values = v.data_ptr() if v.numel() else None
            vs.n = v.numel()
            vs.on_device = 1
            keep.append(v)
        elif (not isinstance(v, np.ndarray) and len(v) > 0 and
              all(isinstance(x, (bytes, bytearray, str)) for x in v)):
            bs = [x.encode() if isinstance(x, str) else bytes(x) for x in v]
            ta = (TextConst * len(bs))()
            for k, b in enumerate(bs):
                ta[k].data = b
                ta[k].len = len(b)
            vs.texts = ta
            vs.n = len(bs)
            keep.append((ta, bs))
        else:
            a = np.ascontiguousarray(np.asarray(v).astype(np.int64, copy=False)
                                     if len(v) else np.zeros(0, np.int64))
            vs.values = a.ctypes.data_as(C.c_void_p).value if len(a) else None
            vs.n = len(a)
            keep.append(a)
        index[id(v)] = len(sets)
        arr[i].ival = len(sets)
        sets.append(vs)
    if not sets:
        return arr, tc, n_tc, None, 0
    sa = (ValueSet * len(sets))(*sets)
    sa._keep = keep
    return arr, tc, n_tc, sa, len(sets)


def agg_cols_mask(aggs):
    """Projection bitmask covering every column the agg specs read — the
    caller-side analog of ColumnarAttrNeeded (columnar_customscan.c:1813-1851):
    projection is fixed at scan_begin, before aggs are bound."""
    m = 0
    for a in aggs:
        for c in a[1:4]:
            if isinstance(c, int) and c >= 0:
                m |= 1 << c
    return m


def make_aggs(aggs):
    """aggs: list of (kind, col_a[, col_b[, col_c[, one]]])"""
    arr = (AggSpec * len(aggs))()
    for i, a in enumerate(aggs):
        a = tuple(a) + (-1, -1, -1, 0)[len(a) - 1:]
        arr[i].kind, arr[i].col_a, arr[i].col_b, arr[i].col_c, arr[i].one = a[:5]
    return arr


def _alloc_hgroups(n_key_cols, n_aggs, capacity):
    """numpy destinations for `capacity` groups + the cstripe_hgroups
    pointing at them (the arrays must outlive the call)"""
    import numpy as np
    nk = min(n_key_cols, MAX_HASH_KEY_COLS)
    bufs = {"keys": [np.zeros(capacity, dtype=np.int64) for _ in range(nk)],
            "key_nulls": [np.zeros(capacity, dtype=np.uint8) for _ in range(nk)],
            "partials": np.zeros((capacity, n_aggs), dtype=partial_dtype())}
    hg = HGroups()
    for k in range(nk):
        hg.keys[k] = bufs["keys"][k].ctypes.data
        hg.key_nulls[k] = bufs["key_nulls"][k].ctypes.data
    hg.partials = bufs["partials"].ctypes.data
    return bufs, hg


def _hgroups_result(bufs, n):
    # copies, so a large capacity's buffers are not kept alive by the result
    return {"n_groups": n,
            "keys": [a[:n].copy() for a in bufs["keys"]],
            "key_nulls": [a[:n].copy() for a in bufs["key_nulls"]],
            "partials": bufs["partials"][:n].copy()}


def combine_groups(aggs, n_key_cols, results, capacity=None):
    """The coordinator merge per group (cagg_combine_groups): results is a
    list of agg_hashed()-shaped dicts (per shard/GPU, any order, duplicate
    keys allowed); returns one dict of the same shape, sorted. capacity
    defaults to the sum of the inputs' group counts, which always fits."""
    import numpy as np
    n_aggs = len(aggs)
    arr = make_aggs(aggs)
    parts = (HGroups * max(1, len(results)))()
    keep = []
    for i, res in enumerate(results):
        n = int(res["n_groups"])
        parts[i].n_groups = n
        pa = np.ascontiguousarray(res["partials"], dtype=partial_dtype())
        if pa.size != n * n_aggs:
            raise CStripeError("combine_groups: partials shape does not match "
                               f"n_groups={n}, n_aggs={n_aggs}")
        keep.append(pa)
        parts[i].partials = pa.ctypes.data
        for k in range(min(n_key_cols, MAX_HASH_KEY_COLS, len(res["keys"]))):
            ka = np.ascontiguousarray(res["keys"][k], dtype=np.int64)
            na = np.ascontiguousarray(res["key_nulls"][k], dtype=np.uint8)
            keep += [ka, na]
            parts[i].keys[k] = ka.ctypes.data
            parts[i].key_nulls[k] = na.ctypes.data
    cap = max(1, sum(int(r["n_groups"]) for r in results))
    if capacity is not None:
        cap = int(capacity)
    bufs, hg = _alloc_hgroups(n_key_cols, n_aggs, max(cap, 1))
    _check(_combine_groups(arr, n_aggs, n_key_cols, parts, len(results),
                           C.byref(hg), cap), "combine_groups")
    return _hgroups_result(bufs, hg.n_groups)


def parse_group_order(order):
    """[(kind, index, flags)] from items like ("agg", 0, "desc"), ("key", 1)
    or ("agg", 2, "desc", "nulls_first"). Direction defaults to ascending and
    NULLs to last; both flags are taken literally, as the C ABI takes them."""
    out = []
    for o in order:
        o = tuple(o)
        if len(o) < 2 or str(o[0]).lower() not in ("agg", "key"):
            raise CStripeError(f"group order entry {o!r}: want ('agg'|'key', index, ...)")
        flags = 0
        for opt in o[2:]:
            opt = str(opt).lower()
            if opt == "desc":
                flags |= ORDER_DESC
            elif opt == "nulls_first":
                flags |= ORDER_NULLS_FIRST
            elif opt not in ("asc", "nulls_last"):
                raise CStripeError(f"group order entry {o!r}: unknown option {opt!r}")
        out.append((GORDER_AGG if str(o[0]).lower() == "agg" else GORDER_KEY,
                    int(o[1]), flags))
    return out


def make_group_order(order):
    terms = parse_group_order(order)
    arr = (GroupOrder * max(1, len(terms)))()
    for i, (kind, index, flags) in enumerate(terms):
        arr[i].kind, arr[i].index, arr[i].flags = kind, index, flags
    return arr, len(terms)


def make_having(having):
    """having: list of (agg_index, PRED_LT..PRED_NE, value). The value goes
    into both constants: ival (COUNT and integer kinds) when it is integral,
    fval (f64 kinds) always."""
    import math
    arr = (Having * max(1, len(having)))()
    for i, (agg, op, value) in enumerate(having):
        arr[i].agg, arr[i].op = agg, op
        arr[i].fval = float(value)
        if not isinstance(value, float):
            arr[i].ival = int(value)
        elif math.isfinite(value) and value == int(value):
            arr[i].ival = int(value)
    return arr, len(having)


_F64_KINDS = (AGG_SUM_F64, AGG_MIN_F64, AGG_MAX_F64)
_COUNT_KINDS = (AGG_COUNT_STAR, AGG_COUNT_COL)


def _f64_ord(x):
    """order-preserving int of a float under PG order: NaN greatest and equal
    to itself, -0.0 = +0.0 (topn_f64_ord of the library)"""
    import struct
    x = float(x)
    if x != x:
        return 0xFFF0000000000001
    u = struct.unpack("<Q", struct.pack("<d", x))[0]
    if u == 1 << 63:
        u = 0
    return (~u & ((1 << 64) - 1)) if u >> 63 else (u | (1 << 63))


def _partial_value(kind, p):
    """(is_null, comparable Python int) of one aggregate's final value"""
    if kind in _COUNT_KINDS:
        return False, int(p["count"])
    if p["is_null"]:
        return True, 0
    if kind in _F64_KINDS:
        return False, _f64_ord(p["f64"])
    return False, partial_i128(p)


def merge_groups_topn(aggs, n_key_cols, results, order, limit, offset=0, having=()):
    """The coordinator side of GROUP BY ... HAVING ... ORDER BY ... LIMIT over
    per-shard agg_hashed() / agg_hashed_topn() results (host only):
    combine_groups, then HAVING on the merged values, then the total order of
    agg_hashed_topn (order terms, ties ascending by key tuple, NULL keys
    last), then rows [offset, offset + limit). Returns the agg_hashed dict.

    What the reference's planner says holds here too
    (multi_logical_optimizer.c:5039-5140, :2650-2682): a per-shard top-N with
    the exact limit + offset, and a per-shard HAVING, are exact only when the
    shards' groups are DISJOINT — the GROUP BY holds the partition column, so
    every group is complete on its shard. Otherwise a worker limit is an
    approximation (a group outside every shard's top-N may still win after
    the merge), and HAVING belongs after the merge: pass the shards' full
    agg_hashed() results and give `having` here."""
    if limit < 0 or offset < 0:
        raise CStripeError("merge_groups_topn: limit and offset must be >= 0")
    terms = parse_group_order(order)
    kinds = [tuple(a)[0] for a in aggs]
    for kind, index, _ in terms:
        if index < 0 or index >= (len(aggs) if kind == GORDER_AGG else n_key_cols):
            raise CStripeError(f"merge_groups_topn: order index {index} out of range")
    res = combine_groups(aggs, n_key_cols, list(results))
    n = int(res["n_groups"])
    parts = res["partials"]

    def survives(g):
        for agg, op, value in having:
            null, v = _partial_value(kinds[agg], parts[g, agg])
            if null:
                return False
            c = _f64_ord(value) if kinds[agg] in _F64_KINDS else value
            if not ((v < c), (v <= c), (v > c), (v >= c), (v == c), (v != c))[op]:
                return False
        return True

    def sort_key(g):
        key = []
        for kind, index, flags in terms:
            if kind == GORDER_AGG:
                null, v = _partial_value(kinds[index], parts[g, index])
            else:
                null, v = bool(res["key_nulls"][index][g]), int(res["keys"][index][g])
            if null:
                key.append((0 if flags & ORDER_NULLS_FIRST else 2, 0))
            else:
                key.append((1, -v if flags & ORDER_DESC else v))
        return tuple(key) + (g,)          # combine_groups' order breaks ties

    idx = sorted((g for g in range(n) if survives(g)), key=sort_key)
    import numpy as np
    idx = np.array(idx[offset:offset + limit], dtype=np.int64)
    return {"n_groups": len(idx),
            "keys": [a[idx] for a in res["keys"]],
            "key_nulls": [a[idx] for a in res["key_nulls"]],
            "partials": parts[idx]}


def parse_order(order):
    """[(col, desc, nulls_first)] from a list of col, (col, "asc"|"desc") or
    (col, dir, "first"|"last"); NULL placement defaults to PG's: ascending
    puts NULLs last, descending puts them first."""
    out = []
    for o in order:
        o = tuple(o) if isinstance(o, (tuple, list)) else (o,)
        if not 1 <= len(o) <= 3:
            raise CStripeError(f"order entry {o!r}: want col, (col, dir) or (col, dir, nulls)")
        d = str(o[1]).lower() if len(o) > 1 else "asc"
        if d not in ("asc", "desc"):
            raise CStripeError(f"order entry {o!r}: direction must be 'asc' or 'desc'")
        desc = d == "desc"
        first = desc
        if len(o) > 2:
            p = str(o[2]).lower()
            if p not in ("first", "last"):
                raise CStripeError(f"order entry {o!r}: nulls must be 'first' or 'last'")
            first = p == "first"
        out.append((int(o[0]), desc, first))
    return out


def _order_ranks(v):
    """dense ascending ranks (ties equal) of one order column under the
    library's comparison rules: integers signed; floats in PG order (NaN
    greatest and equal to itself, -0.0 = +0.0); bytes by memcmp"""
    import numpy as np
    if v.dtype == object:
        uniq = {b: i for i, b in enumerate(sorted(set(v.tolist())))}
        return np.array([uniq[b] for b in v], dtype=np.int64)
    if v.dtype.kind == "f":
        f = v.astype(np.float64)
        u = f.view(np.uint64).copy()
        u[f == 0] = 0                                   # -0.0 = +0.0
        u[np.isnan(f)] = 0x7FF0000000000001             # one above +inf
        neg = (u >> np.uint64(63)).astype(bool)
        v = np.where(neg, ~u, u | np.uint64(1 << 63))
    return np.unique(v, return_inverse=True)[1].astype(np.int64).reshape(-1)


def merge_topn(results, order, limit, offset=0, text=False):
    """The coordinator's Sort + Limit over per-shard select_topn() results
    (host numpy): concatenate, order by the rules of select_topn, break ties
    by (part index, row number), return rows [offset, offset + limit).
    The order columns must be among the returned values. A VARTEXT order
    column (listed in a part's "text_cols", or carrying decoded "text")
    compares the decoded bytes of results[i]["text"][col] — ranks are per
    scan — and raises CStripeError when a part has none. Returns {"n_rows",
    "part" (index into results per row), "row_numbers", "values", "nulls"};
    text=True adds "text" for the columns every part decoded. The merged
    "values" of a VARTEXT column stay per-scan ranks."""
    import numpy as np
    keys = parse_order(order)
    if limit < 0 or offset < 0:
        raise CStripeError("merge_topn: limit and offset must be >= 0")
    results = list(results)
    if not results:
        raise CStripeError("merge_topn: no results")
    for i, res in enumerate(results):
        if res.get("row_numbers") is None:
            raise CStripeError(f"merge_topn: part {i} has no row numbers")
    tcols = set()
    for res in results:
        tcols |= set(res.get("text_cols", ())) | set(res.get("text", {}))
    n_each = [int(res["n_rows"]) for res in results]
    part = np.repeat(np.arange(len(results), dtype=np.int64), n_each)
    rn = np.concatenate([np.asarray(res["row_numbers"], dtype=np.int64)[:n]
                         for res, n in zip(results, n_each)])
    cols = list(results[0]["values"])

    def cat(field, c, dtype=None):
        return np.concatenate([np.asarray(res[field][c], dtype=dtype)[:n]
                               for res, n in zip(results, n_each)])

    def cat_text(c):
        for i, res in enumerate(results):
            if c not in res.get("text", {}):
                raise CStripeError(
                    f"merge_topn: column {c} is VARTEXT and part {i} carries no decoded "
                    "text (select_topn(decode_text=True)); ranks of different scans "
                    "are not comparable")
        out = np.empty(len(part), dtype=object)
        out[:] = [b for res, n in zip(results, n_each)
                  for b in list(res["text"][c])[:n]]
        return out

    values = {c: cat("values", c) for c in cols}
    have_nulls = all(res.get("nulls") for res in results)
    nulls = {c: cat("nulls", c, np.uint8) for c in cols} if have_nulls else {}
    # np.lexsort: the LAST key is the most significant
    sort_keys = [rn, part]
    for c, desc, first in reversed(keys):
        if c not in values:
            raise CStripeError(f"merge_topn: order column {c} is not among the values")
        isnull = nulls[c].astype(bool) if have_nulls else np.zeros(len(part), bool)
        v = cat_text(c) if c in tcols else values[c]
        if v.dtype == object:
            v = v.copy()
            v[isnull] = b""
        rank = _order_ranks(v)
        if desc:
            rank = -rank
        rank[isnull] = 0
        sort_keys.append(rank)
        sort_keys.append(np.where(isnull, 0, 1) if first else isnull.astype(np.int64))
    idx = np.lexsort(sort_keys)[offset:offset + limit]
    res = {"n_rows": len(idx), "part": part[idx], "row_numbers": rn[idx],
           "values": {c: values[c][idx] for c in cols},
           "nulls": {c: nulls[c][idx] for c in nulls}}
    if text:
        res["text"] = {c: cat_text(c)[idx] for c in cols
                       if all(c in r_.get("text", {}) for r_ in results)}
    return res


class Scan:
    def __init__(self, reader, cols_mask, preds, lookups=(), exprs=()):
        self._sets = None
        self._lookups = None
        self._lookup_payloads = [len(lk.payloads) for lk in lookups]
        self._exprs = None
        self._n_exprs = len(exprs)
        if exprs:                                 # expressions: computed columns
            self._preds, self._texts, n_texts, self._sets, n_sets = make_preds_sets(preds)
            self._lookups, n_lk = make_lookups(list(lookups))
            self._exprs, n_ex = make_exprs(list(exprs))
            self._h = _scan_begin_exprs(reader._h, cols_mask, self._preds, len(preds),
                                        self._texts, n_texts, self._sets, n_sets,
                                        self._lookups, n_lk, self._exprs, n_ex)
        elif lookups:                             # N:1 joins: derived columns
            self._preds, self._texts, n_texts, self._sets, n_sets = make_preds_sets(preds)
            self._lookups, n_lk = make_lookups(list(lookups))
            self._h = _scan_begin_lookups(reader._h, cols_mask, self._preds, len(preds),
                                          self._texts, n_texts, self._sets, n_sets,
                                          self._lookups, n_lk)
        elif any(_is_set_pred(p) for p in preds):   # IN / NOT IN: value sets
            self._preds, self._texts, n_texts, self._sets, n_sets = make_preds_sets(preds)
            self._h = _scan_begin_sets(reader._h, cols_mask, self._preds, len(preds),
                                       self._texts, n_texts, self._sets, n_sets)
        else:
            self._preds, self._texts, n_texts = make_preds_ex(preds)
            if n_texts:     # string constants: VARTEXT predicates
                self._h = _scan_begin_ex(reader._h, cols_mask, self._preds, len(preds),
                                         self._texts, n_texts)
            else:
                self._h = _scan_begin(reader._h, cols_mask, self._preds, len(preds))
        if not self._h:
            raise CStripeError("scan_begin: " + errmsg())
        self.reader = reader
        self._reader = reader
        # pred columns are implicitly projected (scan_begin does the same)
        ntab = reader.column_count
        self._mask = cols_mask & ((1 << ntab) - 1)
        # (a column that is only pattern-matched has no values to read)
        for p in preds:
            if p[0] < ntab and p[1] not in (PRED_LIKE, PRED_NOT_LIKE):
                self._mask |= 1 << p[0]
        for lk in lookups:
            self._mask |= 1 << lk.key_col        # key columns are read too
        # and an expression's table inputs
        for i in range(self._n_exprs):
            for k in range(self._exprs[i].n_ops):
                op = self._exprs[i].ops[k]
                if op.op == EX_COL and op.column < ntab:
                    self._mask |= 1 << op.column
        if self._mask == 0:
            self._mask = 1
        # derived and computed columns are always projected
        for c in range(ntab, ntab + sum(self._lookup_payloads) + self._n_exprs):
            self._mask |= 1 << c
        self._device = -1

    def end(self):
        if self._h:
            _scan_end(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.end()

    @property
    def chunk_groups_filtered(self):
        return _filtered(self._h)

    @property
    def staged_bytes(self):
        return _staged_bytes(self._h)

    @property
    def last_fused(self):
        return bool(_last_fused(self._h))

    @property
    def last_agg_path(self):
        """body of the last agg(): 0 none/empty, 1 fused, 2 general,
        3 dense windowed, 4 dense overlapped"""
        return _last_agg_path(self._h)

    @property
    def last_kernel_ms(self):
        return _last_kernel_ms(self._h)

    @property
    def last_decode_ms(self):
        return _last_decode_ms(self._h)

    @property
    def last_agg_ms(self):
        return _last_agg_ms(self._h)

    def stage(self, device=-1):
        _check(_gpu_stage(self._h, device), "gpu_stage")
        self._device = device

    def text_dict(self, col):
        """The sorted per-scan dictionary of a projected VARTEXT column of a
        staged scan, as a list of bytes: rank i in select / agg_hashed
        results of this scan means entry i (memcmp order)."""
        import numpy as np
        n = C.c_uint32()
        offs = C.POINTER(C.c_uint64)()
        data = C.POINTER(C.c_uint8)()
        _check(_text_dict(self._h, col, C.byref(n), C.byref(offs), C.byref(data)),
               "scan_text_dict")
        o = np.ctypeslib.as_array(offs, shape=(n.value + 1,)).copy()
        total = int(o[-1])
        blob = C.string_at(data, total) if total else b""
        return [blob[int(o[i]):int(o[i + 1])] for i in range(n.value)]

    def last_text_ms(self):
        """(decode, walk, dict, remap) device ms of the last stage()'s
        VARTEXT dictionary build; zeros when no text column is projected"""
        d, w, t, m = C.c_double(), C.c_double(), C.c_double(), C.c_double()
        _check(_last_text_ms(self._h, C.byref(d), C.byref(w), C.byref(t), C.byref(m)),
               "scan_last_text_ms")
        return d.value, w.value, t.value, m.value

    def last_like_ms(self):
        """(match, apply) device ms of the last stage()'s LIKE / NOT LIKE
        work, all patterns together; zeros without one"""
        m, a = C.c_double(), C.c_double()
        _check(_last_like_ms(self._h, C.byref(m), C.byref(a)), "scan_last_like_ms")
        return m.value, a.value

    def like_form(self, col):
        """read form of a pattern-matched VARTEXT column at the last stage():
        None (unstaged, or no LIKE atom on it), "dict" or "stream" """
        return {LIKE_FORM_DICT: "dict", LIKE_FORM_STREAM: "stream"}.get(
            _like_form(self._h, col))

    def last_set_ms(self):
        """(build, probe) device ms of the last stage()'s set work (IN /
        NOT IN predicates), all sets together; zeros without one"""
        b, p = C.c_double(), C.c_double()
        _check(_last_set_ms(self._h, C.byref(b), C.byref(p)), "scan_last_set_ms")
        return b.value, p.value

    def set_form(self, i):
        """(form, size) of value set i at the last stage(): form is
        SET_FORM_NONE (unstaged), SET_FORM_HASH or SET_FORM_BITMAP, size the
        table's slots or bits"""
        size = C.c_uint64()
        rc = _set_form(self._h, i, C.byref(size))
        if rc < 0:
            raise CStripeError(f"scan_set_form failed (rc={rc}): {errmsg()}")
        return rc, size.value

    def column_count(self):
        """table + derived (lookup payload) + computed (expression) columns of this scan
        (cstripe_scan_column_count). A method, as the C entry is a call on
        the scan — unlike the Reader.column_count property, which it equals
        for a scan without lookups."""
        return _scan_column_count(self._h)

    def derived(self, l, p):
        """column id of payload p of lookup l"""
        if not (0 <= l < len(self._lookup_payloads) and 0 <= p < self._lookup_payloads[l]):
            raise CStripeError(f"derived: no payload {p} of lookup {l} in this scan")
        return self._reader.column_count + sum(self._lookup_payloads[:l]) + p

    def computed(self, e):
        """column id of expression e"""
        if not 0 <= e < self._n_exprs:
            raise CStripeError(f"computed: no expression {e} in this scan")
        return self._reader.column_count + sum(self._lookup_payloads) + e

    def expr_range(self, e):
        """(lo, hi, n_present) of computed column e over the selected chunk
        groups, measured by the last stage(); an all-NULL column gives
        (0, 0, 0)"""
        lo, hi, n = C.c_int64(), C.c_int64(), C.c_uint64()
        _check(_expr_range(self._h, e, C.byref(lo), C.byref(hi), C.byref(n)), "scan_expr_range")
        return lo.value, hi.value, n.value

    def last_expr_ms(self):
        """device ms of the last stage()'s expression evaluation launches,
        all expressions together; 0 without one"""
        ms = C.c_double()
        _check(_last_expr_ms(self._h, C.byref(ms)), "scan_last_expr_ms")
        return ms.value

    def last_lookup_ms(self):
        """(build, probe) device ms of the last stage()'s lookup work, all
        lookups together; zeros without one"""
        b, p = C.c_double(), C.c_double()
        _check(_last_lookup_ms(self._h, C.byref(b), C.byref(p)), "scan_last_lookup_ms")
        return b.value, p.value

    def lookup_form(self, i):
        """(form, size) of lookup i's table at the last stage(): form is
        LOOKUP_FORM_NONE (unstaged), LOOKUP_FORM_HASH or LOOKUP_FORM_DIRECT,
        size its slots or entries"""
        size = C.c_uint64()
        rc = _lookup_form(self._h, i, C.byref(size))
        if rc < 0:
            raise CStripeError(f"scan_lookup_form failed (rc={rc}): {errmsg()}")
        return rc, size.value

    def _col_type(self, c):
        """cstripe type of a table or derived / computed (I64) column id"""
        ntab = self._reader.column_count
        return I64 if c >= ntab else self._reader.column_def(c)[1]

    def _decode_ranks(self, col, ranks, nulls):
        """object array of bytes / None from a VARTEXT column's ranks"""
        import numpy as np
        d = self.text_dict(col)
        out = np.empty(len(ranks), dtype=object)
        for i in range(len(ranks)):
            out[i] = None if (nulls is not None and nulls[i]) else d[int(ranks[i])]
        return out

    def agg(self, aggs):
        """aggs: list of (kind, col_a[, col_b[, col_c[, one]]]) -> [Partial]"""
        arr = make_aggs(aggs)
        out = (Partial * len(aggs))()
        _check(_scan_agg(self._h, arr, len(aggs), out), "scan_agg")
        return list(out)

    def agg_grouped(self, aggs, group_cols):
        arr = make_aggs(aggs)
        gc = (C.c_uint32 * len(group_cols))(*group_cols)
        gr = GroupResult()
        out = (Partial * (64 * len(aggs)))()
        _check(_scan_agg_grouped(self._h, arr, len(aggs), gc, len(group_cols),
                                 C.byref(gr), out), "scan_agg_grouped")
        res = {}
        for g in range(gr.n_groups):
            key = decode_group_key(gr.keys[g])
            res[key] = [out[g * len(aggs) + a] for a in range(len(aggs))]
        return res

    def agg_hashed(self, aggs, key_cols, capacity, decode_text=False):
        """Hashed GROUP BY (cstripe_scan_agg_hashed) over 1..4 integer/TEXT
        key columns, at most `capacity` groups. Returns {"n_groups",
        "keys": [int64 array per key col], "key_nulls": [uint8 arrays],
        "partials": structured array (n_groups, n_aggs) of partial_dtype()},
        sorted ascending by key tuple, NULL keys last. A VARTEXT key comes
        back as its dictionary rank; decode_text=True adds "text_keys":
        {k: object array of bytes / None} for those key positions."""
        arr = make_aggs(aggs)
        kc = (C.c_uint32 * max(1, len(key_cols)))(*key_cols)
        bufs, hg = _alloc_hgroups(len(key_cols), len(aggs),
                                  min(max(int(capacity), 1), MAX_HASH_GROUPS))
        _check(_scan_agg_hashed(self._h, arr, len(aggs), kc, len(key_cols),
                                capacity, C.byref(hg)), "scan_agg_hashed")
        res = _hgroups_result(bufs, hg.n_groups)
        if decode_text:
            res["text_keys"] = {
                k: self._decode_ranks(c, res["keys"][k], res["key_nulls"][k])
                for k, c in enumerate(key_cols)
                if self._col_type(c) == VARTEXT}
        return res

    def agg_hashed_topn(self, aggs, key_cols, capacity, order, limit, having=(),
                        decode_text=False):
        """GROUP BY ... [HAVING] ORDER BY ... LIMIT on the device
        (cstripe_scan_agg_hashed_topn): the groups of agg_hashed(aggs,
        key_cols, capacity), filtered by `having` — items (agg_index,
        ca.PRED_GT, value), ANDed — ordered by `order` — items like
        ("agg", 0, "desc") and ("key", 1), with an optional "nulls_first";
        ties ascending by key tuple — and cut to `limit`. Only those groups
        are copied back. Returns the agg_hashed dict in the requested order."""
        arr = make_aggs(aggs)
        kc = (C.c_uint32 * max(1, len(key_cols)))(*key_cols)
        oarr, n_order = make_group_order(order)
        harr, n_having = make_having(having)
        bufs, hg = _alloc_hgroups(len(key_cols), len(aggs),
                                  min(max(int(limit), 1), MAX_TOPN))
        _check(_scan_agg_hashed_topn(self._h, arr, len(aggs), kc, len(key_cols),
                                     capacity, harr, n_having, oarr, n_order,
                                     limit, C.byref(hg)), "scan_agg_hashed_topn")
        res = _hgroups_result(bufs, hg.n_groups)
        if decode_text:
            res["text_keys"] = {
                k: self._decode_ranks(c, res["keys"][k], res["key_nulls"][k])
                for k, c in enumerate(key_cols)
                if self._col_type(c) == VARTEXT}
        return res

    @property
    def last_group_topn(self):
        """(groups before HAVING, groups kept, range ms, select ms, emit ms)
        of the last agg_hashed_topn call"""
        n, k = C.c_uint64(), C.c_uint64()
        r, s, e = C.c_double(), C.c_double(), C.c_double()
        _check(_last_group_topn(self._h, C.byref(n), C.byref(k), C.byref(r),
                                C.byref(s), C.byref(e)), "scan_last_group_topn")
        return n.value, k.value, r.value, s.value, e.value

    @property
    def last_hash_ms(self):
        """(init, scan, compact) device ms of the last agg_hashed call"""
        i, s, c = C.c_double(), C.c_double(), C.c_double()
        _check(_last_hash_ms(self._h, C.byref(i), C.byref(s), C.byref(c)),
               "scan_last_hash_ms")
        return i.value, s.value, c.value

    def next_batch(self, col_arrays, null_arrays=None):
        """col_arrays: dict col_index -> numpy array (capacity chunk rows).
        Returns (n_rows, first_row_number) or None at end."""
        ncols = self.reader.column_count
        b = Batch()
        vals = (C.c_void_p * ncols)()
        for ci, a in col_arrays.items():
            vals[ci] = a.ctypes.data_as(C.c_void_p).value
        b.col_values = vals
        if null_arrays:
            nl = (C.POINTER(C.c_uint8) * ncols)()
            for ci, a in null_arrays.items():
                nl[ci] = a.ctypes.data_as(C.POINTER(C.c_uint8))
            b.col_nulls = nl
        rc = _next_batch(self._h, C.byref(b))
        if rc == END:
            return None
        _check(rc, "next_batch")
        return b.n_rows, b.first_row_number

    def read_row(self, row_number):
        """Random access (ColumnarReadRowByRowNumber): {col: value-or-None}
        over the projected columns, or None when the row does not exist.
        Requires a predicate-free scan."""
        import numpy as np
        r = self._reader
        ncols = r.column_count
        DT = {1: np.int8, 2: np.int16, 3: np.int32, 4: np.int64,
              5: np.float32, 6: np.float64, 7: np.uint32}
        bufs, vp = {}, (C.c_void_p * ncols)()
        nulls = (C.c_uint8 * ncols)()
        for c in range(ncols):
            if not (self._mask >> c) & 1:
                continue
            if r.column_def(c)[1] == VARTEXT:
                continue        # no row access to variable-length text
            a = np.zeros(1, dtype=DT[r.column_def(c)[1]])
            bufs[c] = a
            vp[c] = a.ctypes.data_as(C.c_void_p).value
        rc = _read_row(self._h, row_number, vp, nulls)
        if rc == END:
            return None
        _check(rc, "read_row")
        return {c: (None if nulls[c] else bufs[c][0].item())
                for c in bufs}

    def _row_destinations(self, cols, types, cap, want_nulls, want_row_numbers,
                          device):
        """caller-owned destinations of `cap` rows for select / select_topn:
        (values, nulls, row_numbers, Rows) — numpy arrays, or torch tensors
        on the scan's device"""
        ncols = self.column_count()
        if device:
            import torch
            dev = torch.device("cuda", self._device if self._device >= 0
                               else torch.cuda.current_device())
            DT = {1: torch.int8, 2: torch.int16, 3: torch.int32,
                  4: torch.int64, 5: torch.float32, 6: torch.float64,
                  7: torch.int32, 8: torch.int32}

            def alloc(dt):
                return torch.empty(cap, dtype=dt, device=dev)

            def ptr(a):
                return a.data_ptr()
            null_dt, rn_dt = torch.uint8, torch.int64
            torch.cuda.synchronize(dev)
        else:
            import numpy as np
            DT = {1: np.int8, 2: np.int16, 3: np.int32, 4: np.int64,
                  5: np.float32, 6: np.float64, 7: np.uint32, 8: np.int32}

            def alloc(dt):
                return np.zeros(cap, dtype=dt)

            def ptr(a):
                return a.ctypes.data_as(C.c_void_p).value
            null_dt, rn_dt = np.uint8, np.int64
        vals = {c: alloc(DT[types[c]]) for c in cols}
        nulls = {c: alloc(null_dt) for c in cols} if want_nulls else {}
        rn = alloc(rn_dt) if want_row_numbers else None
        rows = Rows()
        vp = (C.c_void_p * ncols)()
        for c, a in vals.items():
            vp[c] = ptr(a)
        rows.col_values = vp
        if want_nulls:
            np_ = (C.c_void_p * ncols)()
            for c, a in nulls.items():
                np_[c] = ptr(a)
            rows.col_nulls = np_
        if rn is not None:
            rows.row_numbers = ptr(rn)
        return vals, nulls, rn, rows

    def select_count(self):
        """Rows select() returns: runs the device predicate pass and keeps
        the pass mask on the scan for a following select()."""
        n = C.c_uint64()
        _check(_select_count(self._h, C.byref(n)), "scan_select_count")
        return n.value

    @property
    def last_select_ms(self):
        """(mask, offsets, emit) device ms of the last select/select_count"""
        m, o, e = C.c_double(), C.c_double(), C.c_double()
        _check(_last_select_ms(self._h, C.byref(m), C.byref(o), C.byref(e)),
               "scan_last_select_ms")
        return m.value, o.value, e.value

    def select(self, cols=None, want_nulls=True, want_row_numbers=True,
               device=False, decode_text=False):
        """Filtered row materialisation (cstripe_scan_select): the rows that
        pass the scan's predicates, compacted on device, in scan order.
        cols: column indices to return (None = every projected column).
        Returns {"n_rows", "row_numbers", "values": {col: array},
        "nulls": {col: array}}; row_numbers / nulls are None / {} when not
        wanted. Host mode returns numpy arrays (read_row's dtype map);
        device=True returns torch tensors on the scan's device (ints and
        floats by width, TEXT as int32 bit patterns, row numbers int64)
        whose data_ptr() can go straight into write_table_device.
        A VARTEXT column comes back as int32 dictionary ranks (text_dict);
        decode_text=True (host mode, needs want_nulls) adds "text":
        {col: object array of bytes / None}."""
        ncols = self.column_count()
        if cols is None:
            cols = [c for c in range(ncols) if (self._mask >> c) & 1]
        cols = list(cols)
        for c in cols:
            if not 0 <= c < ncols:
                raise CStripeError(f"select: column {c} out of range")
        types = {c: self._col_type(c) for c in cols}
        n = self.select_count()
        m_ms, o_ms, _ = self.last_select_ms
        d_ms = self.last_decode_ms
        cap = max(n, 1)
        vals, nulls, rn, rows = self._row_destinations(
            cols, types, cap, want_nulls, want_row_numbers, device)
        _check(_select(self._h, C.byref(rows), cap, 1 if device else 0),
               "scan_select")
        k = rows.n_rows
        # device time of this call, both ABI calls together
        e_ms = self.last_select_ms[2]
        d_ms += self.last_decode_ms
        self.select_profile = {"decode_ms": d_ms, "mask_ms": m_ms,
                               "offsets_ms": o_ms, "emit_ms": e_ms,
                               "total_ms": d_ms + m_ms + o_ms + e_ms}
        res = {"n_rows": k,
               "row_numbers": None if rn is None else rn[:k],
               "values": {c: a[:k] for c, a in vals.items()},
               "nulls": {c: a[:k] for c, a in nulls.items()}}
        if decode_text:
            if device or not want_nulls:
                raise CStripeError("select: decode_text needs host mode and want_nulls")
            res["text"] = {c: self._decode_ranks(c, res["values"][c], res["nulls"][c])
                           for c in cols if types[c] == VARTEXT}
        return res

    @property
    def last_topn_ms(self):
        """(key build, selection, emit + permute) device ms of the last
        select_topn call"""
        k, s, e = C.c_double(), C.c_double(), C.c_double()
        _check(_last_topn_ms(self._h, C.byref(k), C.byref(s), C.byref(e)),
               "scan_last_topn_ms")
        return k.value, s.value, e.value

    def select_topn(self, order, limit, cols=None, want_nulls=True,
                    want_row_numbers=True, device=False, decode_text=False):
        """ORDER BY ... LIMIT over the scan (cstripe_scan_select_topn): the
        first `limit` passing rows in the given order, found on device by a
        radix select over packed keys — no full sort, no full materialisation.
        order: list of col, (col, "asc"|"desc") or (col, dir, "first"|"last");
        NULL placement defaults to PG's (asc -> last, desc -> first). Rows
        equal on every order column come out in ascending row number.
        Returns the dictionary of select() — "n_rows" = min(limit, passing
        rows), arrays of that length in final order — plus "topn_profile"
        (device ms per stage) and "text_cols" (the VARTEXT columns among
        "values", whose int32 ranks are per scan). cols, want_nulls,
        want_row_numbers, device and decode_text as in select()."""
        ncols = self.column_count()
        keys = parse_order(order)
        if cols is None:
            cols = [c for c in range(ncols) if (self._mask >> c) & 1]
        cols = list(cols)
        for c in cols:
            if not 0 <= c < ncols:
                raise CStripeError(f"select_topn: column {c} out of range")
        types = {c: self._col_type(c) for c in cols}
        # every destination holds `limit` entries; an out-of-range limit is
        # the library's error, so only the allocation is clamped
        cap = min(max(int(limit), 1), MAX_TOPN)
        vals, nulls, rn, rows = self._row_destinations(
            cols, types, cap, want_nulls, want_row_numbers, device)
        ok = (OrderKey * max(1, len(keys)))()
        for i, (c, desc, first) in enumerate(keys):
            ok[i].column = c
            ok[i].flags = (ORDER_DESC if desc else 0) | \
                          (ORDER_NULLS_FIRST if first else 0)
        _check(_select_topn(self._h, ok, len(keys), int(limit), C.byref(rows),
                            1 if device else 0), "scan_select_topn")
        k = rows.n_rows
        key_ms, sel_ms, emit_ms = self.last_topn_ms
        self.topn_profile = {"decode_ms": self.last_decode_ms, "key_ms": key_ms,
                             "select_ms": sel_ms, "emit_ms": emit_ms,
                             "total_ms": self.last_kernel_ms}
        res = {"n_rows": k,
               "row_numbers": None if rn is None else rn[:k],
               "values": {c: a[:k] for c, a in vals.items()},
               "nulls": {c: a[:k] for c, a in nulls.items()},
               "text_cols": [c for c in cols if types[c] == VARTEXT],
               "topn_profile": dict(self.topn_profile)}
        if decode_text:
            if device or not want_nulls:
                raise CStripeError("select_topn: decode_text needs host mode and want_nulls")
            res["text"] = {c: self._decode_ranks(c, res["values"][c], res["nulls"][c])
                           for c in cols if types[c] == VARTEXT}
        return res

    def rewind(self):
        _check(_rewind(self._h), "rewind")


class RcclComm:
    """C-ABI RCCL communicator (cagg_comm): the data-path collective of the
    combine step runs in host C over librccl; the launcher only distributes
    the 128-byte unique id (ncclCommInitRank's own bootstrap contract)."""

    def __init__(self, n_ranks, rank, uid_bytes, device=-1):
        uid = (C.c_uint8 * 128)(*uid_bytes)
        h = C.c_void_p()
        _check(_comm_init(C.byref(h), n_ranks, rank, uid, device), "cagg_comm_init")
        self._h = h
        self.rank = rank
        self.n_ranks = n_ranks

    @staticmethod
    def unique_id():
        uid = (C.c_uint8 * 128)()
        _check(_comm_uid(uid), "cagg_comm_unique_id")
        return bytes(uid)

    def close(self):
        if self._h:
            _comm_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def allgather_bytes(self, data):
        src = (C.c_uint8 * len(data)).from_buffer_copy(data)
        dst = (C.c_uint8 * (len(data) * self.n_ranks))()
        _check(_comm_allgather(self._h, src, len(data), dst), "cagg_allgather")
        return bytes(dst)

    def combine(self, aggs, parts):
        """cagg_combine_rccl: gather + strict merge, in C, over RCCL."""
        a = make_aggs(aggs)
        local = (Partial * len(parts))(*parts)
        out = (Partial * len(parts))()
        _check(_combine_rccl(self._h, a, len(aggs), local, out),
               "cagg_combine_rccl")
        return list(out)


def combine(aggs, parts_list):
    """parts_list: list (per shard/GPU) of lists of Partial -> [Partial].
    The coordinator-merge step (cagg_combine)."""
    n_aggs = len(aggs)
    arr = make_aggs(aggs)
    flat = (Partial * (n_aggs * len(parts_list)))()
    for p, parts in enumerate(parts_list):
        for a in range(n_aggs):
            flat[p * n_aggs + a] = parts[a]
    out = (Partial * n_aggs)()
    _check(_combine(arr, n_aggs, flat, len(parts_list), out), "combine")
    return list(out)
