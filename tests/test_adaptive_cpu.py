"""Adaptive sampling on the CPU: the convergence criterion the
accumulator's kernels compile (csrc/rtw_adaptive.hpp) agrees case by case, se2
bit for bit, with the same formula in numpy f64; the library declares, exports
and binds the new entry points, and refuses null arguments.  No compute call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG_ROOT, REPO

ADAPTIVE_SYMBOLS = ["rtw_accum_set_mask", "rtw_accum_set_adaptive", "rtw_accum_active", "rtw_accum_read_counts",
                    "rtw_accum_load_counts"]


def criterion(sy, sy2, cnt, chunk, min_spp, thr):
    """(converged, se2) in numpy f64, one IEEE operation per operator, in the header's order."""
    sy, sy2, thr = np.float64(sy), np.float64(sy2), np.float64(thr)
    m = cnt // chunk
    if m < 2:
        return False, np.float64(0.0)
    fm, fc = np.float64(m), np.float64(chunk)
    var = np.maximum(np.float64(0.0), sy2 - sy * sy / fm)
    se2 = var / (fm * np.float64(m - 1) * fc * fc)
    return bool(cnt >= min_spp and se2 <= thr), se2


def stat_of(ys):
    sy = sy2 = np.float64(0.0)
    for y in ys:
        y = np.float64(y)
        sy = sy + y
        sy2 = sy2 + y * y
    return sy, sy2


def clamp_case():
    """Equal chunk luminances whose SY2 - SY*SY/m rounds below zero."""
    for k in range(1, 400):
        sy, sy2 = stat_of([np.float64(0.1) * k] * 3)
        if sy2 - sy * sy / np.float64(3.0) < 0:
            return sy, sy2
    raise AssertionError("no rounding case found")


def cases():
    out = []
    spread = [3.0, 5.5, 4.25]
    for m in (1, 2, 3):  # m < 2 never converges, whatever the budget
        sy, sy2 = stat_of(spread[:m])
        for thr in (1e-6, 1e-2, 1e3):
            out.append((sy, sy2, 20 * m, 20, 0, thr))
    sy, sy2 = stat_of(spread[:2])
    out.append((sy, sy2, 47, 20, 0, 1e3))  # cnt off the chunk grid: m = 2 full chunks
    out.append((sy, sy2, 14, 7, 0, 1e3))   # another chunk
    sy, sy2 = clamp_case()                 # the clamp: se2 = +0 <= any thr > 0
    out.append((sy, sy2, 60, 20, 0, 1e-300))
    sy, sy2 = stat_of(spread)              # se2 == thr exactly, one ulp below, one above
    _, se2 = criterion(sy, sy2, 60, 20, 0, 1.0)
    for thr in (se2, np.nextafter(se2, 0.0), np.nextafter(se2, 1.0)):
        out.append((sy, sy2, 60, 20, 0, thr))
    for min_spp in (40, 60, 61, 80):       # min_spp below, at and above cnt
        out.append((sy, sy2, 60, 20, min_spp, 1e3))
    return out


def bits(x):
    return "%016x" % int(np.float64(x).view(np.uint64))


def test_criterion_agrees_with_numpy_case_by_case(tmp_path):
    table = cases()
    want = [criterion(*c) for c in table]
    # the table covers what it claims to
    assert {c[2] // c[3] for c in table} >= {1, 2, 3}
    assert any(w[0] for w in want) and any(not w[0] for w in want)
    sy, sy2 = clamp_case()
    assert sy2 - sy * sy / np.float64(3.0) < 0 and criterion(sy, sy2, 60, 20, 0, 1e-300) == (True, 0.0)
    eq = [(c, w) for c, w in zip(table, want) if c[2] == 60 and c[4] == 0 and np.float64(c[5]) == w[1] and w[1] > 0]
    assert len(eq) == 1 and eq[0][1][0]  # se2 == thr converges ...
    below = [w for c, w in zip(table, want) if c[2] == 60 and c[4] == 0 and 0 < np.float64(c[5]) < w[1]]
    assert below and not any(w[0] for w in below)  # ... one ulp less does not
    assert [w[0] for c, w in zip(table, want) if c[4] in (40, 60, 61, 80) and c[4]] == [True, True, False, False]
    exe, tab = tmp_path / "adaptive_check", tmp_path / "cases.txt"
    src = os.path.join(REPO, "tests", "native", "adaptive_check.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-I", os.path.join(PKG_ROOT, "csrc"), src,
                    "-o", str(exe)], check=True)
    with open(tab, "w") as f:
        for c, w in zip(table, want):
            f.write(f"{bits(c[0])} {bits(c[1])} {c[2]} {c[3]} {c[4]} {bits(c[5])} {int(w[0])} {bits(w[1])}\n")
    r = subprocess.run([str(exe), str(tab)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and f"bad 0/{len(table)}" in r.stdout, r.stdout + r.stderr


def test_header_declares_library_exports_and_python_binds(rtw):
    syms = rtw.header_symbols()
    for s in ADAPTIVE_SYMBOLS:
        assert s in syms, s
        assert hasattr(rtw.lib(), s), s
        assert getattr(rtw.lib(), s).argtypes, s
    for m in ("set_mask", "set_adaptive", "active", "counts"):
        assert callable(getattr(rtw.Accumulator, m)), m
    assert rtw.abi_version() == 4


def test_null_arguments_are_refused(rtw):
    L = rtw.lib()
    E = rtw.RTW_EINVAL
    n, t = C.c_uint32(), C.c_uint32()
    buf = (C.c_uint8 * 16)()
    assert L.rtw_accum_set_mask(None, buf) == E
    assert L.rtw_accum_set_adaptive(None, 0.02, 0) == E
    assert L.rtw_accum_active(None, C.byref(n), C.byref(t)) == E
    assert L.rtw_accum_read_counts(None, buf) == E
    assert L.rtw_accum_load_counts(None, None, None, None, 0) == E
    assert L.rtw_last_error()
