"""CSTRIPE_VARTEXT without a GPU: on-disk byte layout (the reference's varlena
serialisation), standard-codec decodability, prefix-key skip nodes, the
header-walk validator, host-side chunk pruning through scan_begin_ex, and the
writer / scan_begin argument errors. Every comparison is exact."""
import ctypes as C
import itertools

import numpy as np
import pytest

import citus_amd as ca
import futil
import vtutil

DEFS = [("id", ca.I64, 0), ("t", ca.VARTEXT, 0)]
OPS = (ca.PRED_LT, ca.PRED_LE, ca.PRED_GT, ca.PRED_GE, ca.PRED_EQ, ca.PRED_NE)


def edge_values():
    """every EDGE_LENS length three times over, NULLs interleaved; 40 rows"""
    vals = []
    for rep in range(3):
        for n in vtutil.EDGE_LENS:
            vals.append(bytes((65 + (rep * 7 + i) % 26) for i in range(n)))
            if (len(vals) + rep) % 3 == 0:
                vals.append(None)
    return vals


def write(path, vals, chunk=16, stripe=32, **kw):
    ca.write_table(path, DEFS, [np.arange(len(vals), dtype=np.int64), list(vals)],
                   chunk_group_row_limit=chunk, stripe_row_limit=stripe, **kw)


def chunks_of(path, col):
    """[(node, python slice bounds)] of one column in scan order"""
    ft = futil.read_footer(path)
    out, row = [], 0
    for st in ft["stripes"]:
        for k, rows in enumerate(st["group_rows"]):
            out.append((st["nodes"][col][k], row, row + rows))
            row += rows
    return out


def test_abi_version_and_type():
    assert ca._lib.cstripe_abi_version() == 2
    assert ca.VARTEXT == 8


def test_byte_layout_matches_reference_serialisation(tmp_path):
    vals = edge_values()
    assert {len(v) for v in vals if v is not None} == set(vtutil.EDGE_LENS)
    p = str(tmp_path / "none.cs")
    write(p, vals, compression=ca.COMP_NONE)
    cks = chunks_of(p, 1)
    assert len(cks) == (len(vals) + 15) // 16 and len(cks) >= 3
    for node, lo, hi in cks:
        want = vtutil.ser_stream(vals[lo:hi])
        assert node["comp_type"] == ca.COMP_NONE
        assert node["n_present"] == sum(v is not None for v in vals[lo:hi])
        assert node["decompressed_size"] == len(want)
        assert futil.chunk_stream(p, node) == want
    # the two header forms at their boundary
    assert vtutil.ser_datum(b"x" * 126)[:1] == bytes([(127 << 1) | 1])
    assert vtutil.ser_datum(b"x" * 127)[:4] == (131 << 2).to_bytes(4, "little")


@pytest.mark.parametrize("codec", [ca.COMP_LZ4, ca.COMP_ZSTD])
def test_segments_decode_with_system_codec(tmp_path, codec):
    # compressible: the same edge values repeated, 200 rows per chunk
    vals = (edge_values() * 10)[:400]
    p = str(tmp_path / "c.cs")
    write(p, vals, chunk=200, stripe=400, compression=codec)
    lz4 = C.CDLL("liblz4.so.1")
    lz4.LZ4_decompress_safe.restype = C.c_int
    lz4.LZ4_decompress_safe.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    zstd = C.CDLL("libzstd.so.1")
    zstd.ZSTD_decompress.restype = C.c_size_t
    zstd.ZSTD_decompress.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    compressed = 0
    for node, lo, hi in chunks_of(p, 1):
        want = vtutil.ser_stream(vals[lo:hi])
        comp = futil.chunk_stream(p, node)
        if node["comp_type"] == ca.COMP_NONE:
            assert comp == want
            continue
        assert node["comp_type"] == codec
        compressed += 1
        got = bytearray()
        for sg in node["segs"]:
            # no canonical parse applies to a byte stream
            assert sg["mode"] in (futil.SEGMODE_GENERIC, futil.SEGMODE_ZR)
            assert sg["decomp_off"] == len(got)
            frame = comp[sg["comp_off"]:sg["comp_off"] + sg["comp_len"]]
            buf = C.create_string_buffer(max(sg["decomp_len"], 1))
            if codec == ca.COMP_LZ4:
                r = lz4.LZ4_decompress_safe(frame, buf, len(frame), sg["decomp_len"])
            else:
                r = zstd.ZSTD_decompress(buf, sg["decomp_len"], frame, len(frame))
            assert r == sg["decomp_len"]
            got += buf.raw[:sg["decomp_len"]]
        assert bytes(got) == want
    assert compressed > 0


def test_skip_nodes_hold_prefix_keys(tmp_path):
    vals = edge_values()[:32] + [None] * 16 + [b"abcdefgh", b"abcdefgz", b"", b"zz"]
    p = str(tmp_path / "s.cs")
    write(p, vals, compression=ca.COMP_NONE, stripe=64)
    seen_null_chunk = False
    for node, lo, hi in chunks_of(p, 1):
        present = [v for v in vals[lo:hi] if v is not None]
        if not present:
            assert node["has_min_max"] == 0
            assert node["n_present"] == 0 and node["decompressed_size"] == 0
            seen_null_chunk = True
            continue
        assert node["has_min_max"] == 1
        assert node["min_i"] == vtutil.prefix_key(min(present))
        assert node["max_i"] == vtutil.prefix_key(max(present))
        assert 0 <= node["min_i"] <= node["max_i"] < (1 << 56)
    assert seen_null_chunk
    # monotone, not injective
    assert vtutil.prefix_key(b"abcdefgh") == vtutil.prefix_key(b"abcdefgz")


def test_vartext_validate():
    vals = [v for v in edge_values() if v is not None]
    good = vtutil.ser_stream(vals)
    assert ca.vartext_validate(good, len(vals)) == ca.OK
    assert ca.vartext_validate(b"", 0) == ca.OK
    for v in (b"", b"a", b"x" * 126, b"x" * 127, b"x" * 65535):
        assert ca.vartext_validate(vtutil.ser_datum(v), 1) == ca.OK
    # truncated: the last datum (300 payload bytes) loses payload
    assert ca.vartext_validate(good[:-8], len(vals)) == ca.ERR_FORMAT
    assert ca.vartext_validate(good[:5], 2) == ca.ERR_FORMAT
    # count too small / too large
    assert ca.vartext_validate(good, len(vals) - 1) == ca.ERR_FORMAT
    assert ca.vartext_validate(good, len(vals) + 1) == ca.ERR_FORMAT
    # last datum overruns by 1 byte: short header and 4-byte header forms
    s = vtutil.ser_datum(b"ab") + vtutil.ser_datum(b"abc")       # total 4, no padding
    assert ca.vartext_validate(s, 2) == ca.OK
    bad = bytearray(s)
    bad[4] = ((4 + 1) << 1) | 1
    assert ca.vartext_validate(bytes(bad), 2) == ca.ERR_FORMAT
    long = vtutil.ser_datum(b"y" * 128)                           # total 132, no padding
    assert len(long) == 132 and ca.vartext_validate(long, 1) == ca.OK
    assert ca.vartext_validate((133 << 2).to_bytes(4, "little") + long[4:], 1) == ca.ERR_FORMAT
    # 4-byte header whose total is smaller than the header itself
    for total in (0, 1, 2, 3):
        assert ca.vartext_validate((total << 2).to_bytes(4, "little"), 1) == ca.ERR_FORMAT
    # header forms this format never writes: compressed (0b10) / external (0x01)
    assert ca.vartext_validate(b"\x02\0\0\0", 1) == ca.ERR_FORMAT
    assert ca.vartext_validate(b"\x01\0\0\0", 1) == ca.ERR_FORMAT
    assert "vartext" in ca.errmsg()


# 20 sorted values, 4 per chunk -> 5 chunks; chunk 1 ends and chunk 2 starts on
# values that share their first 7 bytes with each other and with two constants
SORTED = [b"", b"a", b"ab", b"abc",
          b"b", b"c", b"mmmmmmm", b"mmmmmmm1",
          b"mmmmmmm3", b"n", b"o", b"p",
          b"q" * 126, b"q" * 127, b"q" * 128, b"r",
          b"s", b"t", b"u" * 300, b"v"]
CONSTS = [b"c", b"ab", b"q" * 127,            # present
          b"bb", b"oo", b"r" * 5,             # between two values
          b"",                                # smallest possible (present)
          b"\x01",                            # below every non-empty value
          b"zzz", b"\xff" * 9,                # above all
          b"mmmmmmm2", b"mmmmmmm0", b"mmmmmmm9", b"mmmmmmmm"]   # share the boundary prefix


def test_pruning_follows_prefix_key_rule(tmp_path):
    assert SORTED == sorted(SORTED)
    p = str(tmp_path / "sorted.cs")
    ca.write_table(p, DEFS, [np.arange(20, dtype=np.int64), list(SORTED)],
                   chunk_group_row_limit=4, stripe_row_limit=12, compression=ca.COMP_NONE)
    bounds = [(vtutil.prefix_key(SORTED[i]), vtutil.prefix_key(SORTED[i + 3]))
              for i in range(0, 20, 4)]
    with ca.Reader(p) as r:
        for op, c in itertools.product(OPS, CONSTS):
            want = sum(vtutil.refuted(op, c, mn, mx) for mn, mx in bounds)
            with r.scan(preds=[(1, op, c)]) as s:
                assert s.chunk_groups_filtered == want, (op, c)
        # a constant sharing its 7-byte prefix with a chunk boundary value never
        # prunes that chunk, although the exact comparison would allow it
        with r.scan(preds=[(1, ca.PRED_GT, b"mmmmmmm2")]) as s:
            assert s.chunk_groups_filtered == 1       # only chunk 0; chunk 1 stays
        with r.scan(preds=[(1, ca.PRED_LT, b"mmmmmmm2")]) as s:
            assert s.chunk_groups_filtered == 2       # chunks 3, 4; chunk 2 stays
        with r.scan(preds=[(1, ca.PRED_EQ, b"mmmmmmm9")]) as s:
            assert s.chunk_groups_filtered == 3       # chunks 1 and 2 stay
        # OR group: pruned only where every member refutes
        with r.scan(preds=[(1, ca.PRED_EQ, b"a", 1), (1, ca.PRED_EQ, b"v", 1)]) as s:
            assert s.chunk_groups_filtered == 3
        # AND with an integer predicate, a chunk counted once
        with r.scan(preds=[(1, ca.PRED_GE, b"s"), (0, ca.PRED_LT, 18)]) as s:
            assert s.chunk_groups_filtered == 4


def test_all_null_chunk_is_never_refuted(tmp_path):
    p = str(tmp_path / "n.cs")
    vals = [b"a", b"b", None, None, b"y", b"z"]
    ca.write_table(p, DEFS, [np.arange(6, dtype=np.int64), vals],
                   chunk_group_row_limit=2, stripe_row_limit=6, compression=ca.COMP_NONE)
    with ca.Reader(p) as r, r.scan(preds=[(1, ca.PRED_EQ, b"zz")]) as s:
        assert s.chunk_groups_filtered == 2


def test_writer_rejects_bad_values(tmp_path):
    p = str(tmp_path / "bad.cs")
    ids = np.arange(2, dtype=np.int64)
    with pytest.raises(ca.CStripeError, match="rc=-5"):
        ca.write_table(p, DEFS, [ids, [b"ok", b"x" * 65536]])
    with pytest.raises(ca.CStripeError, match="NUL"):
        ca.write_table(p, DEFS, [ids, [b"ok", b"a\0b"]])
    # the limit itself, and a NULL row's bytes being ignored, are fine
    ca.write_table(p, DEFS, [ids, [b"x" * 65535, None]], compression=ca.COMP_NONE)
    node = chunks_of(p, 1)[0][0]
    assert futil.chunk_stream(p, node) == vtutil.ser_datum(b"x" * 65535)
    offs = np.array([0, 3, 6], dtype=np.uint64)
    data = np.frombuffer(b"abc\0\0\0", dtype=np.uint8)
    ca.write_table(p, DEFS, [ids, (offs, data)],
                   nulls=[None, np.array([0, 1], dtype=np.uint8)], compression=ca.COMP_NONE)
    node = chunks_of(p, 1)[0][0]
    assert futil.chunk_stream(p, node) == vtutil.ser_datum(b"abc")


def test_scan_begin_needs_a_string_constant(tmp_path):
    p = str(tmp_path / "t.cs")
    write(p, [b"a", b"b"], compression=ca.COMP_NONE)
    with ca.Reader(p) as r:
        # cstripe_scan_begin: no constant to compare against
        with pytest.raises(ca.CStripeError, match="VARTEXT"):
            r.scan(preds=[(1, ca.PRED_EQ, 0)])
        # scan_begin_ex: index past the constants
        preds = ca.make_preds([(1, ca.PRED_EQ, 1)])
        tc = (ca.TextConst * 1)()
        tc[0].data, tc[0].len = b"a", 1
        assert not ca._scan_begin_ex(r._h, 0, preds, 1, tc, 1)
        assert "VARTEXT" in ca.errmsg()
        preds[0].ival = -1
        assert not ca._scan_begin_ex(r._h, 0, preds, 1, tc, 1)
        preds[0].ival = 0
        h = ca._scan_begin_ex(r._h, 0, preds, 1, tc, 1)
        assert h
        ca._scan_end(h)
        # integer predicates are untouched by the extra arguments
        with r.scan(preds=[(0, ca.PRED_GE, 1), (1, ca.PRED_NE, "a")]) as s:
            assert s.chunk_groups_filtered == 0
