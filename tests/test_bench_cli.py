"""
bench.py surface that needs no GPU: the --full / --dump-outputs options exist,
and dump_outputs() writes the combined aggregates losslessly (float64 value +
exact 32-bit limbs of the int128) in a run-independent order.
"""
import os
import subprocess
import sys

import numpy as np

import citus_amd as ca

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _i128_from_limbs(row):
    u = 0
    for limb in row[1:5]:
        u = (u << 32) | int(limb)
    return u - (1 << 128) if u >> 127 else u


def test_bench_help_lists_full_and_dump_outputs():
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--help"],
                         capture_output=True, text=True)
    assert out.returncode == 0
    assert "--full" in out.stdout and "--dump-outputs" in out.stdout


def test_dump_outputs_ungrouped(tmp_path):
    import bench
    big = (1 << 100) + 12345            # not representable in a double
    parts = [ca.Partial(i128_lo=12345, i128_hi=1 << 36, count=7),
             ca.Partial(i128_lo=-3, i128_hi=-1, count=1),
             ca.Partial(f64=1.25, count=2, is_null=1)]
    d = str(tmp_path / "out")
    bench.dump_outputs(d, parts, None)
    assert sorted(os.listdir(d)) == ["aggregates.npy"]
    a = np.load(os.path.join(d, "aggregates.npy"))
    assert a.dtype == np.float64 and a.shape == (1, 3, 8)
    assert _i128_from_limbs(a[0, 0]) == parts[0].i128 == big
    assert a[0, 0, 0] == float(big) and a[0, 0, 5] == 7
    assert _i128_from_limbs(a[0, 1]) == -3 and a[0, 1, 0] == -3.0
    assert a[0, 2, 6] == 1.25 and a[0, 2, 7] == 1.0


def test_dump_outputs_grouped_sorted_keys(tmp_path):
    import bench
    res = {(82, 70): [ca.Partial(i128_lo=3, count=3)],
           (None, 79): [ca.Partial(i128_lo=9, count=1)],
           (65, 70): [ca.Partial(i128_lo=1, count=1)]}
    d = str(tmp_path / "out")
    bench.dump_outputs(d, res, (6, 7))
    keys = np.load(os.path.join(d, "group_keys.npy"))
    a = np.load(os.path.join(d, "aggregates.npy"))
    assert keys.dtype == np.float64 and keys.shape == (3, 2) and a.shape == (3, 1, 8)
    assert np.isnan(keys[0, 0]) and keys[0, 1] == 79          # NULL key sorts first
    assert keys[1:].tolist() == [[65.0, 70.0], [82.0, 70.0]]
    assert a[:, 0, 0].tolist() == [9.0, 1.0, 3.0]
