"""Device check of the Tier-B contract's building blocks, each compared bit
for bit with the oracle's C code on inputs chosen for their branches, not
through 8-bit images: bin/gpu_contract_check (tests/native/gpu_contract_check.hip,
built in-tree by build()) evaluates on the GPU

  * csrc/rtw_libm.hpp's sin / cos / atan2 / acos (the gfx950 build) over the
    inputs of tests/native/libm_check.cpp plus the sphere-UV edges and every
    interval bound of atan / atan2 / acos (tests/native/libm_inputs.hpp);
  * rtw_math.hpp's sin_sign / checker_odd around every k * pi below 2^19 and in
    [2^19, 2^20 * pi/2), where the device answers with ocml's sin;
  * the f32 div_rn with y = RN(1/b) from the host and from the device, the
    device's own 1.0f / b and sqrt(float), against host IEEE arithmetic;
  * rtw_device.hpp's sm_mix, rnd_f64, rnd_f32, rnd3<double>, rnd3<float> and
    f64_long_lz on Tier-B states and on states CONSTRUCTED (the mixer's
    inverse) so that the rare long-leading-zero word is draw 1, 2 or 3,

and compares on the host with oracle/ro_libm.h and oracle/rtw_oracle.c, which
are compiled into the program.  sin / cos beyond 2^20 * pi/2 are outside the
contract: counted and printed, not asserted.  The comparator's own teeth:
tests/test_contract_compare_cpu.py."""
import json
import os
import re
import subprocess

import pytest

from conftest import GOLDEN, PKG_ROOT

pytestmark = pytest.mark.gpu

GAMMA, EXT, M64 = 0x9E3779B97F4A7C15, 0x5851F42D4C957F2D, (1 << 64) - 1
FAMILIES = ["libm_sin", "libm_cos", "libm_atan2", "libm_acos", "sin_sign", "checker_odd", "f32_div_rn_host_y",
            "f32_div_rn_device_y", "f32_device_rcp", "f32_device_sqrt", "rng_sm_mix", "rng_branch_taken", "rng_rnd_f64",
            "rng_rnd_f64_state", "rng_rnd_f32", "rng_rnd_f32_state", "rng_rnd3_f64", "rng_rnd3_f64_s2", "rng_rnd3_f32",
            "rng_rnd3_f32_s2", "rng_f64_long_lz_iterates", "rng_f64_long_lz"]


@pytest.fixture(scope="module")
def run():
    exe = os.path.join(PKG_ROOT, "bin", "gpu_contract_check")
    assert os.path.exists(exe), "bin/gpu_contract_check missing: run build() first"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    print(r.stderr)
    return r


def test_every_family_matches_the_oracle_bit_for_bit(run):
    fam = {m.group(1): (int(m.group(2)), int(m.group(3)))
           for m in re.finditer(r"^family (\w+) cases (\d+) mismatches (\d+)$", run.stdout, re.M)}
    assert sorted(fam) == sorted(FAMILIES), run.stdout + run.stderr
    for name in FAMILIES:
        cases, mismatches = fam[name]
        assert cases > 0 and mismatches == 0, (name, cases, mismatches, run.stdout)
    assert sum(c for c, _ in fam.values()) >= 3_000_000
    assert fam["libm_sin"][0] >= 250_000 and fam["libm_atan2"][0] >= 300_000 and fam["sin_sign"][0] >= 3 * 2 * 166_000 and fam["f32_device_sqrt"][0] == 1 << 20
    assert run.returncode == 0 and run.stdout.rstrip().endswith("ok")


def test_payne_hanek_range_is_counted_not_asserted(run):
    """|x| >= 2^20 * pi/2: the device returns ocml's sin / cos, the oracle
    glibc's.  The contract leaves it open; the line reports how
    many of the results differ and by how much."""
    m = re.search(r"^family payne_hanek cases (\d+) differing (\d+) max_ulp (\d+)", run.stdout, re.M)
    assert m, run.stdout
    print("Payne-Hanek range: cases", m.group(1), "differing", m.group(2), "largest ulp distance", m.group(3))
    assert int(m.group(1)) >= 400_000


def test_mixer_known_answers(run):
    with open(os.path.join(GOLDEN, "rng_kat.json")) as f:
        kat = json.load(f)
    got = {int(a): int(b) for a, b in re.findall(r"^sm_mix (\d+) -> (\d+)$", run.stdout, re.M)}
    assert got == dict(zip(kat["tb_mix_in"], kat["tb_mix_out"]))


def test_f64_long_lz_second_iteration(run):
    """f64_long_lz(d) with d = (unmix(0) - gamma) ^ kExt: the first extension
    word is zero, so the loop iterates — against ro_sm_f64's loop restated
    here with rtw_oracle_py.tb_mix."""
    import rtw_oracle_py as P

    def long_lz(d):
        ext, lz = d ^ EXT, 12
        while True:
            ext = (ext + GAMMA) & M64
            addl = 64 - P.tb_mix(ext).bit_length()
            lz += addl
            if addl != 64:
                return lz
            if lz >= 1022:
                return 1022

    rows = [(int(a, 16), int(b)) for a, b in re.findall(r"^f64_long_lz state 0x([0-9a-f]+) lz (\d+)$", run.stdout, re.M)]
    assert len(rows) == 4
    d0 = rows[0][0]
    assert P.tb_mix(((d0 ^ EXT) + GAMMA) & M64) == 0  # the first extension word
    assert rows[0][1] >= 12 + 64
    for d, lz in rows:
        assert lz == long_lz(d), (hex(d), lz)
