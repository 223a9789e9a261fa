"""Python restatement of the VARTEXT on-disk rules, shared by the VARTEXT
tests: the reference's varlena serialisation (SerializeSingleDatum,
columnar_writer.c:555-585, typalign 'i'), the skip-node prefix key and the
prefix-key chunk refutation rule of include/cstripe.h."""
import citus_amd as ca

# payload lengths at every header / padding boundary: 126 is the last short
# header (total 127), 127 the first 4-byte header
EDGE_LENS = (0, 1, 2, 3, 4, 5, 126, 127, 128, 300)


def ser_datum(b):
    """one datum: header, payload, zero padding to a 4-byte boundary"""
    total = len(b) + 1
    if total <= 127:
        d = bytes([(total << 1) | 1]) + b
    else:
        d = ((len(b) + 4) << 2).to_bytes(4, "little") + b
    return d + b"\0" * (-len(d) % 4)


def ser_stream(values):
    """value stream of one chunk: present values only"""
    return b"".join(ser_datum(v) for v in values if v is not None)


def prefix_key(b):
    """first 7 payload bytes big-endian in bits 55..0, zero-padded"""
    return int.from_bytes(b[:7].ljust(7, b"\0"), "big")


def refuted(op, const, mn_key, mx_key):
    """chunk refutation on prefix keys (the table in include/cstripe.h)"""
    kc = prefix_key(const)
    if op in (ca.PRED_LT, ca.PRED_LE):
        return mn_key > kc
    if op in (ca.PRED_GT, ca.PRED_GE):
        return mx_key < kc
    if op == ca.PRED_EQ:
        return kc < mn_key or kc > mx_key
    return False


def py_pred(op, v, c):
    """row semantics: Python bytes comparison is memcmp order, shorter first
    on a prefix tie; a NULL operand fails the atom"""
    if v is None:
        return False
    return {ca.PRED_LT: v < c, ca.PRED_LE: v <= c, ca.PRED_GT: v > c,
            ca.PRED_GE: v >= c, ca.PRED_EQ: v == c, ca.PRED_NE: v != c}[op]
