"""Mint tests/golden/impala64_twin_digest.json: SHA-256 of y, saved, argmax and the 30 gradients of the 64x64x3 IMPALA trunk's
host twin at B = 3 (inputs: tests/impala84_cases.digest64).  Minted before the trunk kernels learned their second geometry;
tests/test_impala84_twins.py holds the twin to these bits, so the 64 family cannot move unnoticed.  Re-mint only when the 64
family's arithmetic contract (csrc/impala_rows.h) changes on purpose."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from cleanrl_amd import host_ops  # noqa: E402
import impala84_cases as C  # noqa: E402

if __name__ == "__main__":
    out = os.path.join(ROOT, "tests", "golden", "impala64_twin_digest.json")
    with open(out, "w") as f:
        json.dump(C.digest64(host_ops), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)
