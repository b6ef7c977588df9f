"""Kernel RS's compile-time geometry (cleanrl_amd/csrc/convrs_geom.h, the layer-2 forward streamed by stride-parity class) checked on the host:
tests/host/convrs_geom_check.cpp is compiled with g++ against the header the device code includes and verifies that every one of the 243 rows of
a three-image group sits in exactly one lane slot, that the sixteen-lane sets of a fragment read hold sixteen distinct residues (no bank
conflicts), that (window origin) + (tap offset) is the record of pixel (2 gy + ty, 2 gx + tx) in the class (ty & 1, tx & 1) for all rows and taps,
that the visited k-steps are kernel R's layer-2 forward's (r_kstep<RConv2>) with phase g holding only class g, that every 16-byte unit of a
group's source belongs to exactly one (class, round, thread), and the LDS budget."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_kernel_rs_row_table_classes_and_units_hold_on_the_host(tmp_path):
    exe = str(tmp_path / "convrs_geom_check")
    subprocess.run(["g++", "-std=c++20", "-O1", "-I" + os.path.join(ROOT, "cleanrl_amd", "csrc"), os.path.join(ROOT, "tests", "host", "convrs_geom_check.cpp"),
                    "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip())
    assert (got["rows"], got["slots"], got["ksteps"], got["sets"]) == (243, 256, 32, 16)
    assert got["conflicts"] == 0 and got["lds_bytes"] == 120032 and got["lds_bytes"] <= 160 * 1024
    assert (got["class_units"], got["rounds_per_thread"]) == (2400, 5)
