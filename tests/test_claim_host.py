"""The megakernel's guided claims on the unit queue (csrc/rtw_claim.hpp): the reserve, the guided K and the
same-tile test, as the kernel uses them, in a stand-alone host program (tests/native/claim_check.cpp) that
simulates waves against one counter in seeded random interleavings: every unit is taken exactly once, each
wave's units ascend, no wave overshoots the queue's end by more than kClaimMax x 64 units, and a beam pass is
reused only for its own tile.  The program is run once more against copies of the header with one line broken
each, and must report violations, and once built with the address and undefined-behaviour sanitizers."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import PKG_ROOT, REPO

CSRC = os.path.join(PKG_ROOT, "csrc")
SRC = os.path.join(REPO, "tests", "native", "claim_check.cpp")
FLAGS = ["-O2", "-std=c++17", "-Wall"]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def _build(out_dir, header_dir=CSRC, extra=()):
    exe = os.path.join(str(out_dir), "claim_check")
    return exe, subprocess.run(["g++", *FLAGS, *extra, "-I", str(header_dir), SRC, "-o", exe], capture_output=True, text=True)


def _run(exe):
    p = subprocess.run([exe], capture_output=True, text=True)
    m = re.search(r"sims (\d+) checks (\d+) violations (\d+)", p.stdout)
    assert m, p.stdout + p.stderr
    print(p.stdout.strip())
    return p.returncode, int(m.group(1)), int(m.group(2)), int(m.group(3)), p.stderr


def test_every_unit_once_ascending_bounded_overshoot(tmp_path):
    exe, r = _build(tmp_path)
    assert r.returncode == 0, r.stderr
    rc, sims, checks, viol, err = _run(exe)
    assert rc == 0 and viol == 0, err
    assert sims >= 5000 and checks >= 1000000, (sims, checks)  # the simulations did run


@pytest.mark.parametrize("kmax,div", [(2, 2), (2, 4), (4, 4), (8, 2), (8, 4)])
def test_other_claim_sizes(tmp_path, kmax, div):
    """The sizes of the A/B (profiles/r19/README.md), not only the one built."""
    exe, r = _build(tmp_path, extra=[f"-DRTW_CLAIM_MAX={kmax}", f"-DRTW_CLAIM_DIV={div}"])
    assert r.returncode == 0, r.stderr
    rc, _, _, viol, err = _run(exe)
    assert rc == 0 and viol == 0, err


# One line of the header broken per copy: (name, the line, its replacement).
BROKEN = [
    # K does not fall at the queue's end
    ("k_not_falling", "  const uint32_t left = head < total_units ? (total_units - head) / kClaimBatch : 0u;",
     "  const uint32_t left = 0xFFFFFFFFu / kClaimBatch; (void)head; (void)total_units;"),
    # the reserve handed out last-first
    ("reserve_last_first", "  return {base < total_units ? base + kClaimBatch : r.end, r.end};",
     "  return {base < total_units ? (base + kClaimBatch < r.end ? r.end - kClaimBatch : r.end) : r.end, r.end};"),
    # a batch past the end leaves the reserve as it is
    ("reserve_kept_past_the_end", "  return {base < total_units ? base + kClaimBatch : r.end, r.end};",
     "  return {base + kClaimBatch, r.end}; (void)total_units;"),
    # a claim of kClaimMax batches after one proven-empty batch
    ("run_not_counted", "RTWC_HD uint32_t run_after(uint32_t run, uint32_t empty) { return empty ? (run < kClaimMax ? run + 1u : run) : 0u; }",
     "RTWC_HD uint32_t run_after(uint32_t run, uint32_t empty) { return empty ? kClaimMax : (run & 0u); }"),
    # the proof reused across a tile change
    ("reuse_across_tiles", "RTWC_HD bool same_tile(uint32_t tile, uint32_t word) { return tile == (word & 0x7FFFFFFFu); }",
     "RTWC_HD bool same_tile(uint32_t tile, uint32_t word) { return word != kNoPass && tile / 2u == (word & 0x7FFFFFFFu) / 2u; }"),
]


@pytest.mark.parametrize("name,line,broken", BROKEN, ids=[b[0] for b in BROKEN])
def test_checks_have_teeth(tmp_path, name, line, broken):
    src = open(os.path.join(CSRC, "rtw_claim.hpp")).read()
    assert src.count(line) == 1, line
    (tmp_path / "rtw_claim.hpp").write_text(src.replace(line, broken))
    exe, r = _build(tmp_path, header_dir=tmp_path)
    assert r.returncode == 0, r.stderr
    rc, _, _, viol, err = _run(exe)
    assert rc == 1 and viol > 0, (name, err)


def test_clean_under_host_sanitizers(tmp_path):
    exe, r = _build(tmp_path, extra=["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", r.stderr):
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr
    rc, _, _, viol, err = _run(exe)
    assert rc == 0 and viol == 0 and "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err
