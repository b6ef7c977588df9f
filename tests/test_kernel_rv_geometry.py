"""Kernel RV's compile-time geometry (cleanrl_amd/csrc/convrv_geom.h, the layer-3 data gradient by vertical border class, seven images per group)
checked on the host: tests/host/convrv_geom_check.cpp is compiled with g++ against the header the device code includes and verifies that every one of
the 567 rows of a group sits in exactly one lane slot of a tile of its own class, that a tile's active ring slots are its class's taps, that for every
row and every tap it multiplies the record read is the pixel of the row's OWN image or a zero record, that per (row tile, column tile) the visited
k-steps are exactly the valid-tap-row ones in ascending order on exactly one wave, that in every k-step the four SIMDs issue equal matrix
instructions (3,024 per group), that every source unit lands in its pixel's record, the LDS budget and the range of the ds_read immediates."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_kernel_rv_classes_schedule_and_records_hold_on_the_host(tmp_path):
    exe = str(tmp_path / "convrv_geom_check")
    subprocess.run(["g++", "-std=c++20", "-O1", "-I" + os.path.join(ROOT, "cleanrl_amd", "csrc"), os.path.join(ROOT, "tests", "host", "convrv_geom_check.cpp"),
                    "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip())
    assert (got["rows"], got["slots"], got["tiles"], got["ksteps"], got["sets"]) == (567, 576, 18, 36, 36)
    assert got["mfma_per_group"] == 3024 and got["mfma_per_simd_step"] == 21
    assert got["source_bytes"] == 120496 and got["lds_bytes"] == 155568 and got["lds_bytes"] <= 160 * 1024
    assert got["max_immediate"] < 65536 and got["rounds_per_thread"] == 11
    assert got["conflicts_c"] <= 8             # (the ten interior tiles: 20 sets; the border classes' 63 origins fall on 15 residues and cannot be dealt apart)
