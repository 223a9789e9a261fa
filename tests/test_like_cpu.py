"""CSTRIPE_PRED_LIKE / NOT_LIKE without a GPU: the symbols, the host matcher
(the source the device runs) against the recursive statement of the rules in
likeutil, the begin-time errors, and chunk pruning through the pattern's
literal prefix. Every comparison is exact."""
import random

import numpy as np
import pytest

import citus_amd as ca
import likeutil
import vtutil

DEFS = [("id", ca.I64, 0), ("t", ca.VARTEXT, 0), ("c", ca.TEXT, 0)]


def test_symbols_and_enum_values():
    assert (ca.PRED_LIKE, ca.PRED_NOT_LIKE) == (8, 9)
    assert ca.LIKE_MAX_PATTERN == 256
    assert (ca.LIKE_FORM_NONE, ca.LIKE_FORM_DICT, ca.LIKE_FORM_STREAM) == (0, 1, 2)
    for name in ("cstripe_like_match", "cstripe_scan_last_like_ms", "cstripe_scan_like_form"):
        assert hasattr(ca._lib, name)
    assert ca._lib.cstripe_abi_version() == 2           # not bumped
    assert callable(ca.Scan.last_like_ms) and callable(ca.Scan.like_form)


def agree(pat, val):
    try:
        want = likeutil.match(pat, val)
    except likeutil.PatternError:
        with pytest.raises(ca.CStripeError):
            ca.like_match(pat, val)
        return None
    got = ca.like_match(pat, val)
    assert got == want, (pat, val, got, want)
    return want


E2, E3, E4 = "é".encode(), "€".encode(), "😀".encode()
HAND = [
    # (pattern, value, expected; None = pattern error)
    (b"", b"", True), (b"", b"a", False),
    (b"%", b"", True), (b"%", b"abc", True),
    (b"_", b"", False), (b"_", b"a", True), (b"_", b"ab", False),
    (b"%%", b"", True), (b"%%", b"xyz", True),
    (b"_%_", b"a", False), (b"_%_", b"ab", True), (b"_%_", b"abcd", True),
    (b"\\%", b"%", True), (b"\\%", b"a", False), (b"a\\%", b"a%", True), (b"a\\%", b"ab", False),
    (b"\\_", b"_", True), (b"\\_", b"a", False),
    (b"\\\\", b"\\", True), (b"\\\\", b"\\\\", False), (b"\\a", b"a", True),
    (b"abc", b"abc", True), (b"abc", b"abcd", False), (b"abc", b"ab", False),
    (b"abc", b"xabc", False),
    (b"a\\", b"a", None), (b"\\", b"", None), (b"a\\\\\\", b"a\\", None),
    (b"PROMO%", b"PROMO BRUSHED TIN", True), (b"PROMO%", b"STANDARD PROMO", False),
    (b"%BRASS", b"SMALL PLATED BRASS", True), (b"%BRASS", b"BRASS PLATED", False),
    (b"%special%requests%", b"the special packages requests sleep", True),
    (b"%special%requests%", b"requests special", False),
    (b"%ab%ab", b"abab", True), (b"%ab%ab", b"ababa", False), (b"%ab%ab", b"ab", False),
    (b"%a_c%", b"xxabcxx", True), (b"a%b%c", b"abbbcbc", True), (b"a%b%c", b"acb", False),
    # multi-byte characters under _ and %
    (b"_", E2, True), (b"_", E3, True), (b"_", E4, True),
    (b"__", E2, False), (b"__", E2 + E4, True), (b"_", E2 + b"a", False),
    (b"%", E2 + E3 + E4, True), (b"%" + E3, E2 + E3, True), (b"%" + E3, E3 + E2, False),
    (b"_" + E3 + b"_", E4 + E3 + E2, True), (b"a_c", b"a" + E4 + b"c", True),
    (b"a_c", b"a" + E4 + E4 + b"c", False), (b"%_", E4, True), (b"%__", E4, False),
    (E2 + b"%", E2, True), (E2 + b"%", E3, False), (b"%" + E4 + b"%", b"x" + E4 + b"y", True),
    # the pattern length limit
    (b"a" * 256, b"a" * 256, True), (b"a" * 256, b"a" * 255, False),
    (b"%" * 255 + b"a", b"xxa", True),
    (b"a" * 257, b"a" * 257, None), (b"%" * 257, b"", None),
    # a pattern that is not valid UTF-8
    (b"\xff%", b"a", None), (b"a\xc3", b"a", None), (b"\x80", b"a", None),
]


def test_hand_cases():
    for pat, val, want in HAND:
        assert agree(pat, val) is want, (pat, val)
        if want is None:
            assert ca.errmsg()
    with pytest.raises(ca.CStripeError):
        ca.like_match(b"a\\", b"a")
    assert "LIKE pattern must not end with escape character" in ca.errmsg()
    # str arguments are encoded as UTF-8
    assert ca.like_match("_é%", "€é😀") is True


@pytest.mark.parametrize("alphabet", [
    [b"a", b"b", b"%", b"_", b"\\"],
    [b"a", E2, E3, E4, b"%", b"_"],
], ids=["ascii-escape", "utf8"])
def test_random_cases_agree(alphabet):
    rng = random.Random(20260518)
    valphabet = [a for a in alphabet if a not in (b"%", b"_", b"\\")] or [b"a"]
    # the escape alphabet's values also hold the wildcard bytes themselves
    if b"\\" in alphabet:
        valphabet = valphabet + [b"%", b"_", b"\\"]
    n_match = n_err = 0
    for _ in range(25_000):
        pat = b"".join(rng.choice(alphabet) for _ in range(rng.randint(0, 6)))
        val = b"".join(rng.choice(valphabet) for _ in range(rng.randint(0, 8)))
        got = agree(pat, val)
        n_match += got is True
        n_err += got is None
    assert n_match > 1000                   # the cases are not all trivial misses
    assert (n_err > 0) == (b"\\" in alphabet)


def write(path, vals, chunk=100, stripe=1000, **kw):
    n = len(vals)
    ca.write_table(path, DEFS, [np.arange(n, dtype=np.int64), list(vals),
                                ca.text_slots(["x"] * n)],
                   chunk_group_row_limit=chunk, stripe_row_limit=stripe, **kw)


def begin_ex(r, preds, consts, cols_mask=0):
    arr = ca.make_preds(preds)
    tc = (ca.TextConst * max(1, len(consts)))()
    for i, b in enumerate(consts):
        tc[i].data, tc[i].len = b, len(b)
    h = ca._scan_begin_ex(r._h, cols_mask, arr, len(preds), tc, len(consts))
    if h:
        ca._scan_end(h)
    return bool(h)


def test_begin_errors(tmp_path):
    p = str(tmp_path / "e.cs")
    write(p, [b"a", b"b", None], compression=ca.COMP_NONE)
    with ca.Reader(p) as r:
        for op, name in ((ca.PRED_LIKE, "LIKE"), (ca.PRED_NOT_LIKE, "NOT LIKE")):
            # the column is not VARTEXT: an integer column, a TEXT slot column
            for col in (0, 2):
                assert not begin_ex(r, [(0, ca.PRED_GE, 0), (col, op, 0)], [b"a%"])
                m = ca.errmsg()
                assert "predicate 1" in m and f"op {op}" in m and name in m and "VARTEXT" in m
            # the constant index is out of range
            for ival in (1, -1, 7):
                assert not begin_ex(r, [(1, op, ival)], [b"a%"])
                m = ca.errmsg()
                assert "predicate 0" in m and name in m and "text constants" in m
            # plain scan_begin has no constants
            arr = ca.make_preds([(1, op, 0)])
            assert not ca._scan_begin(r._h, 0, arr, 1)
            assert "predicate 0" in ca.errmsg()
            # longer than the limit; the limit itself begins
            assert not begin_ex(r, [(0, ca.PRED_GE, 0), (0, ca.PRED_LE, 9), (1, op, 0)],
                                [b"a" * 257])
            m = ca.errmsg()
            assert "predicate 2" in m and "257" in m and "CSTRIPE_LIKE_MAX_PATTERN" in m
            assert begin_ex(r, [(1, op, 0)], [b"a" * 256]), ca.errmsg()
            # ends in an unescaped backslash; an escaped one begins
            assert not begin_ex(r, [(1, op, 0)], [b"abc\\"])
            m = ca.errmsg()
            assert "predicate 0" in m
            assert "LIKE pattern must not end with escape character" in m
            assert begin_ex(r, [(1, op, 0)], [b"abc\\\\"]), ca.errmsg()
            # not valid UTF-8
            assert not begin_ex(r, [(1, op, 0)], [b"ab\xff%"])
            m = ca.errmsg()
            assert "predicate 0" in m and "UTF-8" in m
            assert begin_ex(r, [(1, op, 0)], ["é€😀%".encode()]), ca.errmsg()
        # a derived or computed column id
        lk = ca.Lookup(0, np.array([0, 1], np.int64), [np.array([5, 6], np.int64)])
        with pytest.raises(ca.CStripeError, match="op 8"):
            r.scan(preds=[(3, ca.PRED_LIKE, "a%")], lookups=[lk])
        # through the Python surface: an or_group works as for every atom
        with r.scan(preds=[(1, ca.PRED_LIKE, "a%", 1), (0, ca.PRED_EQ, 2, 1)]) as s:
            assert s.chunk_groups_filtered == 0
            assert s.like_form(1) is None                 # unstaged
            assert s.last_like_ms() == (0.0, 0.0)


# 1000 sorted values in 100-row chunk groups: the first letter changes every
# 40 rows, so a chunk spans two or three of them; some values hold the
# wildcard bytes themselves, some share a long prefix
def sorted_values():
    vals = []
    for i in range(1000):
        lead = bytes([97 + i // 40])
        if i % 40 < 4:
            vals.append(lead + b"%_" + b"%03d" % i)
        elif i % 40 < 8:
            vals.append(lead + b"longprefix" + b"%03d" % i)
        else:
            vals.append(lead + b"m%03d" % i)
    return sorted(vals)


PRUNE_PATTERNS = [
    # prefix patterns
    b"a%", b"c%", b"cm%", b"y%", b"z%", b"A%", b"\x7f%", b"cm1_5", b"k", b"",
    # an escaped prefix
    b"c\\%\\_%", b"c\\%%", b"\\d%", b"e\\_%",
    # a prefix longer than 7 bytes
    b"flongprefix%", b"flongprefix2%", b"flongprezzz%", b"flongpr\xc3\xa9%",
    # a leading wildcard
    b"%m1%", b"_m%", b"%",
]


def test_pruning_follows_literal_prefix_rule(tmp_path):
    vals = sorted_values()
    p = str(tmp_path / "sorted.cs")
    write(p, vals, compression=ca.COMP_NONE)
    bounds = [(vtutil.prefix_key(vals[i]), vtutil.prefix_key(vals[i + 99]))
              for i in range(0, 1000, 100)]

    def want(pat, negate=False):
        return sum(likeutil.refuted(pat, mn, mx, negate) for mn, mx in bounds)

    with ca.Reader(p) as r:
        some = 0
        for pat in PRUNE_PATTERNS:
            with r.scan(preds=[(1, ca.PRED_LIKE, pat)]) as s:
                assert s.chunk_groups_filtered == want(pat), pat
                some += 0 < want(pat) < 10
            # NOT LIKE never refutes
            with r.scan(preds=[(1, ca.PRED_NOT_LIKE, pat)]) as s:
                assert s.chunk_groups_filtered == 0, pat
        assert some >= 8
        # the rule never drops a chunk that holds a match
        for pat in PRUNE_PATTERNS:
            for k, (mn, mx) in enumerate(bounds):
                if likeutil.refuted(pat, mn, mx):
                    assert not likeutil.like_mask(vals[k * 100:(k + 1) * 100], pat).any()
        assert want(b"cm%") == 8 and want(b"%m1%") == 0 and want(b"z%") == 10
        # an or_group of two LIKEs: refuted only where both are
        for a, b in ((b"a%", b"y%"), (b"cm%", b"c\\%%"), (b"a%", b"%")):
            both = sum(likeutil.refuted(a, mn, mx) and likeutil.refuted(b, mn, mx)
                       for mn, mx in bounds)
            with r.scan(preds=[(1, ca.PRED_LIKE, a, 1), (1, ca.PRED_LIKE, b, 1)]) as s:
                assert s.chunk_groups_filtered == both, (a, b)
        # ... of a LIKE and a non-refuting atom: nothing is pruned
        for other in ((1, ca.PRED_NOT_LIKE, b"a%", 1), (1, ca.PRED_NE, b"a", 1),
                      (0, ca.PRED_GE, 0, 1)):
            with r.scan(preds=[(1, ca.PRED_LIKE, b"a%", 1), other]) as s:
                assert s.chunk_groups_filtered == 0
        # ANDed with an integer atom, a chunk is counted once
        with r.scan(preds=[(1, ca.PRED_LIKE, b"a%"), (0, ca.PRED_LT, 50)]) as s:
            assert s.chunk_groups_filtered == 9


def test_all_null_chunk_is_never_refuted(tmp_path):
    p = str(tmp_path / "n.cs")
    vals = [b"a", b"b", None, None, b"y", b"z"]
    write(p, vals, chunk=2, stripe=6, compression=ca.COMP_NONE)
    with ca.Reader(p) as r, r.scan(preds=[(1, ca.PRED_LIKE, b"zz%")]) as s:
        assert s.chunk_groups_filtered == 2
