"""The tile-beam bound (csrc/rtw_beam.hpp) is conservative: no sphere that a
camera ray of a tile can hit at a root >= tmin is left out of the tile's mask
(tests/native/beam_bound_check.cpp: frames 96x54 and 9x9, row splits (0, 1)
and (1, 3), the cover camera, aperture 2.0, focus distance 1 and a camera along
the ground plane; the cover scene and a scene whose glass sphere encloses the
camera).  The check has teeth: with the focus quad's half-diagonal halved it
finds violations.  Also pins the bound's tightness on the cover frame: a mean
mask of at most 8 of the 39 narrow spheres per tile (the megakernel's primary
phase tests the mask's spheres per lane)."""
import json
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "raytracinginoneweekend.zig_amd", "csrc")
SRC = os.path.join(REPO, "tests", "native", "beam_bound_check.cpp")
GOLDEN = os.path.join(REPO, "tests", "golden", "cover_scene_seed42.json")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def _cover():
    return [(s["c0"], s["c1"], s["radius"], s["t0"], s["t1"], s["moving"]) for s in json.load(open(GOLDEN))["spheres"]]


def _write(path, spheres):
    with open(path, "w") as f:
        f.write(f"{len(spheres)}\n")
        for c0, c1, r, t0, t1, mv in spheres:
            f.write(" ".join(repr(float(x)) for x in (*c0, *c1, r, t0, t1)) + f" {int(mv)}\n")
    return str(path)


def _build(tmp_path, header_dir, name="beamchk"):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-I", header_dir, SRC, "-o", exe], check=True)
    return exe


def _run(exe, *args):
    p = subprocess.run([exe, *args], capture_output=True, text=True)
    m = re.search(r"rays (\d+) hits (\d+) violations (\d+)", p.stdout)
    assert m, p.stdout + p.stderr
    return p, int(m.group(1)), int(m.group(2)), int(m.group(3))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("beam"), CSRC)


def test_cover_scene_masks_hold_every_sphere_a_camera_ray_hits(exe, tmp_path):
    p, rays, hits, viol = _run(exe, _write(tmp_path / "cover.txt", _cover()), "popcount")
    print(p.stdout)
    assert viol == 0 and p.returncode == 0, p.stderr
    assert rays > 1_000_000 and hits > rays // 2  # the rays do hit: the ground at least
    m = re.search(r"mean_popcount ([0-9.]+) of (\d+) narrow", p.stdout)
    assert m and int(m.group(2)) == 39
    assert float(m.group(1)) <= 8.0  # the primary phase's cost model (profiles/r11/README.md)


def test_camera_inside_a_sphere(exe, tmp_path):
    """Spheres that enclose the camera (a glass shell around the lens, a hollow
    one with a negative radius, a moving one) are hit from inside by every ray:
    they must be in every mask."""
    sph = _cover()
    sph.append(((13.2, 2.1, 3.0), (13.2, 2.1, 3.0), 1.5, 0.0, 0.0, 0))
    sph.append(((13.0, 2.0, 3.0), (13.0, 2.0, 3.0), -0.8, 0.0, 0.0, 0))
    sph.append(((13.0, 1.8, 3.0), (13.0, 2.4, 3.0), 2.5, -0.5, 1.5, 1))
    sph.append(((13.0, 0.3, 3.0), (13.0, 0.3, 3.0), 0.25, 0.0, 0.0, 0))  # around the ground-plane camera
    p, rays, hits, viol = _run(exe, _write(tmp_path / "inside.txt", sph))
    print(p.stdout)
    assert viol == 0 and p.returncode == 0, p.stderr
    assert hits > 3 * rays // 2


def test_check_detects_a_too_narrow_beam(tmp_path):
    weak = tmp_path / "weak"
    weak.mkdir()
    src = open(os.path.join(CSRC, "rtw_beam.hpp")).read()
    needle = "b.h = std::sqrt(std::fmax(p2, m2));"
    assert needle in src
    (weak / "rtw_beam.hpp").write_text(src.replace(needle, "b.h = 0.5 * std::sqrt(std::fmax(p2, m2));"))
    exe = _build(tmp_path, str(weak), "beamchk_weak")
    p, _, _, viol = _run(exe, _write(tmp_path / "cover.txt", _cover()))
    assert viol > 0 and p.returncode == 1
