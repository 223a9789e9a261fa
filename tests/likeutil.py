"""Python statement of the LIKE rules of include/cstripe.h, the row-level
yardstick of the LIKE tests: PG LIKE with the default escape under "C"
collation in a UTF-8 database, written as a direct recursion over the rules —
not a port of the library's loop.
  %   any run of characters, none included
  _   exactly one character
  \\x  the byte x literally
  any other byte matches itself
A character is one byte plus the continuation bytes ((b & 0xC0) == 0x80) that
follow it. The match is anchored at both ends. A NULL value fails LIKE and
NOT LIKE alike."""
import functools

import numpy as np

import vtutil

MAX_PATTERN = 256


class PatternError(ValueError):
    """a pattern scan_begin refuses"""


def tokens(pattern):
    """[('%',) | ('_',) | ('lit', byte)], or PatternError"""
    if len(pattern) > MAX_PATTERN:
        raise PatternError("too long")
    try:
        pattern.decode("utf-8")
    except UnicodeDecodeError:
        raise PatternError("not UTF-8")
    out, i = [], 0
    while i < len(pattern):
        b = pattern[i]
        if b == 0x5C:                       # backslash
            if i + 1 == len(pattern):
                raise PatternError("LIKE pattern must not end with escape character")
            out.append(("lit", pattern[i + 1]))
            i += 2
            continue
        out.append(("%",) if b == 0x25 else ("_",) if b == 0x5F else ("lit", b))
        i += 1
    return out


def next_char(v, i):
    """index after the character that starts at v[i]"""
    i += 1
    while i < len(v) and (v[i] & 0xC0) == 0x80:
        i += 1
    return i


def match(pattern, value):
    """whether value (bytes, not None) matches pattern (bytes)"""
    toks = tokens(pattern)

    @functools.lru_cache(maxsize=None)
    def m(ti, vi):
        if ti == len(toks):
            return vi == len(value)
        t = toks[ti]
        if t[0] == "%":
            if ti + 1 == len(toks):
                return True                 # the rest of the value, whatever it is
            pos = vi
            while True:
                if m(ti + 1, pos):
                    return True
                if pos == len(value):
                    return False
                pos = next_char(value, pos)
        if vi == len(value):
            return False
        if t[0] == "_":
            return m(ti + 1, next_char(value, vi))
        return value[vi] == t[1] and m(ti + 1, vi + 1)

    return m(0, 0)


def like_mask(values, pattern, negate=False):
    """bool array over rows: x LIKE p (negate: x NOT LIKE p); NULL fails both"""
    p = pattern.encode() if isinstance(pattern, str) else pattern
    memo = {}
    out = np.zeros(len(values), dtype=bool)
    for i, v in enumerate(values):
        if v is None:
            continue
        if v not in memo:
            memo[v] = match(p, v)
        out[i] = memo[v] != negate
    return out


def literal_prefix(pattern):
    """the literal bytes before the first unescaped % or _, escapes resolved"""
    pre = bytearray()
    for t in tokens(pattern):
        if t[0] != "lit":
            break
        pre.append(t[1])
    return bytes(pre)


def refuted(pattern, mn_key, mx_key, negate=False):
    """chunk refutation of LIKE on prefix keys (include/cstripe.h); NOT LIKE
    never refutes"""
    pre = literal_prefix(pattern)
    if negate or not pre:
        return False
    return (mx_key < vtutil.prefix_key(pre) or
            mn_key > vtutil.prefix_key(pre[:7].ljust(7, b"\xff")))
