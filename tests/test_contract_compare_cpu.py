"""The comparator of bin/gpu_contract_check (tests/native/contract_compare.hpp)
has teeth: fed arrays in which one value per family is wrong — one ulp off,
the wrong sign of zero, a NaN against a number and the reverse, one bit of a
64-bit state — it reports exactly those indices and nothing else (NaNs of
different payloads, equal zeros and infinities pass).  No GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import REPO


def test_contract_comparator_has_teeth(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "cmpchk")
    native = os.path.join(REPO, "tests", "native")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", native,
                    os.path.join(native, "contract_compare_check.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    fam = {m.group(1): (int(m.group(2)), int(m.group(3)))
           for m in re.finditer(r"^family (\w+) cases (\d+) mismatches (\d+)$", p.stdout, re.M)}
    assert fam == {"one_ulp": (10, 1), "zero_sign": (10, 1), "nan_for_number": (4, 1), "number_for_nan": (10, 1),
                   "state_bit": (4, 1), "all_equal": (3, 0)}, p.stdout
    missed = {(m.group(1), int(m.group(2))) for m in re.finditer(r"^  mismatch (\w+) index (\d+) ", p.stdout, re.M)}
    assert missed == {("one_ulp", 6), ("zero_sign", 1), ("nan_for_number", 2), ("number_for_nan", 4), ("state_bit", 3)}
    # the report names the values in hex: +0 was given for -0
    assert re.search(r"mismatch zero_sign index 1 .* got 0x0000000000000000 want 0x8000000000000000", p.stdout)
    assert "ulp_distance 1 1 0 1" in p.stdout
