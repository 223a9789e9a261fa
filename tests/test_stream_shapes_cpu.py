"""
CPU pins for the stream-shape catalogue (tests/shapes.py): for every entry
the host writer must emit exactly the catalogued comp_type / n_segs / segment
mode per chunk, and the CPU oracle must read the written values back bit for
bit and aggregate them to the numpy expectation. This is the precondition
that makes the GPU matrix (test_gpu_stream_matrix.py) meaningful: an entry
that no longer takes its shape shows up here, without a GPU.
"""
import numpy as np
import pytest

import citus_amd as ca
import futil
import oracle
import shapes


def footer_chunks(path, col=0):
    """[(comp_type, mode, n_segs)] of one column, every chunk in file order;
    asserts that all segments of a chunk carry the same mode"""
    out = []
    for st in futil.read_footer(path)["stripes"]:
        for nd in st["nodes"][col]:
            modes = {s["mode"] for s in nd["segs"]}
            assert len(modes) == 1, f"mixed segment modes {modes}"
            assert len(nd["segs"]) == nd["n_segs"]
            out.append((nd["comp_type"], modes.pop(), nd["n_segs"]))
    return out


def test_catalogue_covers_every_shape():
    """every closed-form mode the writer can emit is in the catalogue"""
    seen = {(sh.codec, m) for sh in shapes.ALL for _, m, _ in sh.chunks}
    for m in (0x00, 0x11, 0x12, 0x13, 0x14, 0x20):
        assert (shapes.LZ4, m) in seen, hex(m)
    for m in (0x50, 0x61, 0x62, 0x63, 0x64, 0x70, 0x80, 0x81, 0x82, 0x83, 0x84):
        assert (shapes.ZSTD, m) in seen, hex(m)
    for sh in shapes.ALL:
        assert len(sh.chunks) == len(sh.chunk_bounds()), sh.name
        assert sh.n <= 2100 or sh.name.startswith("i64_zr127k_"), sh.name


@pytest.mark.parametrize("name", shapes.NAMES)
def test_shape_written_and_read_back(tmp_path, name):
    sh = shapes.SHAPES[name]
    path = str(tmp_path / "t.cs")
    shapes.write_shape(path, sh)

    # 1. the writer emitted the catalogued stream shape for every chunk
    ft = futil.read_footer(path)
    assert ft["total_rows"] == sh.n and len(ft["stripes"]) == 1
    assert footer_chunks(path) == sh.chunks

    # 2. the oracle reads every chunk back bit for bit, nulls included
    uint = sh.bits().dtype
    with oracle.OracleTable(path) as t:
        for k, (lo, hi) in enumerate(sh.chunk_bounds()):
            vals = np.zeros(sh.cgrl, dtype=sh.values.dtype)
            exists = np.zeros(sh.cgrl, dtype=np.uint8)
            t.read_chunk(0, k, 0, vals, exists)
            want_exists = np.ones(hi - lo, dtype=np.uint8) if sh.nulls is None \
                else 1 - sh.nulls[lo:hi]
            np.testing.assert_array_equal(exists[:hi - lo], want_exists)
            keep = want_exists.astype(bool)
            np.testing.assert_array_equal(vals[:hi - lo].view(uint)[keep],
                                          sh.bits()[lo:hi][keep])

        # 3. COUNT / SUM / MIN / MAX of the matching kind equal numpy's
        if sh.is_float:
            kinds = (ca.AGG_SUM_F64, ca.AGG_MIN_F64, ca.AGG_MAX_F64)
        else:
            kinds = (ca.AGG_SUM_I64, ca.AGG_MIN_I64, ca.AGG_MAX_I64)
        aggs = [(ca.AGG_COUNT_STAR, -1), (ca.AGG_COUNT_COL, 0)] + \
               [(k, 0) for k in kinds]
        cols = [shapes.Col(sh.values, sh.nulls)]
        parts, _ = t.scan_agg([], aggs)
        rows = np.ones(sh.n, dtype=bool)
        for p, a in zip(parts, shapes.with_one(cols, aggs)):
            shapes.check_partial(p, shapes.expect_agg(cols, a, rows), a[0],
                                 f"{name} agg kind {a[0]}")
