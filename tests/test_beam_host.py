"""The tile-beam bound (csrc/rtw_beam.hpp) is conservative: no sphere that a
camera ray of a tile can hit at a root >= tmin is left out of the tile's mask
(tests/native/beam_bound_check.cpp: frames 96x54 and 9x9, row splits (0, 1)
and (1, 3), the cover camera, aperture 2.0, focus distance 1 and a camera along
the ground plane; the cover scene and a scene whose glass sphere encloses the
camera).  The check has teeth: with the focus quad's half-diagonal halved it
finds violations.  Also pins the bound's tightness on the cover frame: a mean
mask of at most 8 of the 39 narrow spheres per tile (the megakernel's primary
phase tests the mask's spheres per lane).

The same on generated cases (generated_cases: 320 seeded cameras and frames,
given to the checker as raw rtw_camera fields): cameras among, above and beside
the sphere field, looking anywhere in it or straight down, vfov 2-160 (a fifth
wider than the cone guard's ~45 degrees per tile), apertures 0-3, lens radii
above the focus distance, shutters inside [0, 1] down to zero length, frames of
2..40 x 2..32 pixels with row splits and short row counts — and half of them
sheared into structs Camera.init never makes (horizontal, vertical not
orthogonal; u, v not orthonormal), which rtw_plan.cpp accepts like any other.
The scene is the cover scene plus 40 spheres of radius 0.01 to 3 and -0.5, half
of them moving up to 3 units per axis over [-0.5, 1.5], some behind cameras and
some across a lens disk.  Besides the rays at the tile extremes the checker
aims rays at every sphere a mask excludes.  The counts are asserted so the run
cannot pass vacuously, and eight one-token mutants of rtw_beam.hpp (MUTANTS)
must each give a violation on these cases."""
import json
import math
import os
import re
import shutil
import subprocess
import time
import types

import numpy as np
import pytest

from helpers import build_beam_check, write_beam_cases, write_beam_scene

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "raytracinginoneweekend.zig_amd", "csrc")
GOLDEN = os.path.join(REPO, "tests", "golden", "cover_scene_seed42.json")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def _cover():
    return [(s["c0"], s["c1"], s["radius"], s["t0"], s["t1"], s["moving"]) for s in json.load(open(GOLDEN))["spheres"]]


_write = write_beam_scene


def _build(tmp_path, header_dir, name="beamchk"):
    return build_beam_check(tmp_path, header_dir, name)


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


# ------------------------------------------------------ generated cases ----
N_CASES = 320


def _unit(a):
    return a / np.linalg.norm(a)


def _camera_init(frm, at, vup, vfov, aspect, aperture, focus, t0, t1):
    """Camera.init (main.zig:60-89) as a namespace of the rtw_camera fields."""
    hh = math.tan(math.radians(vfov) / 2.0)
    vh, vw = 2.0 * hh, aspect * 2.0 * hh
    w = _unit(frm - at)
    u = _unit(np.cross(vup, w))
    v = np.cross(w, u)
    hor, ver = focus * vw * u, focus * vh * v
    return types.SimpleNamespace(origin=frm, horizontal=hor, vertical=ver, lower_left_corner=frm - hor / 2 - ver / 2 - focus * w,
                                 u=u, v=v, lens_radius=aperture / 2.0, time0=t0, time1=t1)


def generated_cases(seed=20240611, n=N_CASES):
    """(cases for write_beam_cases, spheres for write_beam_scene), from a fixed seed."""
    rng = np.random.default_rng(seed)
    U = rng.uniform
    cases = []
    for k in range(n):
        while True:
            where = k % 3  # among, above, beside the field
            if where == 0:
                frm = np.array([U(-11, 11), U(0.05, 1.5), U(-11, 11)])
            elif where == 1:
                frm = np.array([U(-11, 11), U(1.5, 12.0), U(-11, 11)])
            else:
                a = U(0, 2 * math.pi)
                frm = np.array([U(12, 22) * math.cos(a), U(0.05, 6.0), U(12, 22) * math.sin(a)])
            if k % 7 == 6:  # straight down
                at, vup = np.array([frm[0], 0.0, frm[2]]), np.array([0.0, 0.0, -1.0])
            else:
                at = np.array([U(-11, 11), U(0.0, 1.0), U(-11, 11)])
                tilt, az = math.radians(U(0, 15)), U(0, 2 * math.pi)
                vup = np.array([math.sin(tilt) * math.cos(az), math.cos(tilt), math.sin(tilt) * math.sin(az)])
            d = frm - at
            if np.linalg.norm(d) > 0.2 and np.linalg.norm(np.cross(vup, _unit(d))) > 0.1:  # vup never parallel to the view
                break
        vfov = U(100, 160) if k % 5 == 4 else U(2, 82)
        aperture = 0.0 if k % 4 == 3 else U(0.0, 3.0)
        focus = U(0.05, 1.0) if k % 3 == 2 else U(0.5, 30.0)
        t0 = U(0.0, 0.6)
        t1 = t0 if k % 6 == 5 else U(t0, 1.0)
        cam = _camera_init(frm, at, vup, vfov, U(0.4, 2.6), aperture, focus, t0, t1)
        if k % 2:  # a struct Camera.init never makes
            cam.horizontal = cam.horizontal + U(-0.6, 0.6) * cam.vertical
            cam.vertical = cam.vertical * U(0.3, 1.3)
            cam.lower_left_corner = cam.lower_left_corner + U(-0.3, 0.3) * cam.horizontal + U(-0.3, 0.3) * cam.vertical
            cam.u = cam.u + U(-0.7, 0.7) * cam.v
            cam.v = U(0.4, 1.6) * cam.v + U(-0.7, 0.7) * cam.u
        W, H = int(rng.integers(2, 41)), int(rng.integers(2, 33))
        rs = int(rng.integers(1, 4))
        rb = int(rng.integers(0, min(rs, H)))
        rc = (H - rb + rs - 1) // rs
        if k % 4 == 1 and rc > 1:
            rc = int(rng.integers(1, rc))
        cases.append((cam, (W, H, rb, rs, rc)))
    spheres = _cover()
    for i in range(40):
        r = (0.01, 0.2, 1.0, 3.0, -0.5)[i % 5]
        if i % 4 == 0:  # at a camera: across its lens disk, around it or just behind it
            cam = cases[int(rng.integers(0, n))][0]
            c0 = np.asarray(cam.origin) + _unit(rng.normal(size=3)) * U(0.0, 1.5) * max(abs(r), cam.lens_radius)
        elif i % 8 in (1, 2):  # all round the field, behind the cameras beside it
            c0 = np.array([U(-24, 24), U(-1.0, 9.0), U(-24, 24)])
        else:  # in the field, where the cameras look
            c0 = np.array([U(-12, 12), U(0.0, 3.0), U(-12, 12)])
        if i % 2:
            c1 = c0 + rng.choice([0.0, 0.5, 3.0], 3) * rng.choice([-1.0, 1.0], 3)
            spheres.append((tuple(c0), tuple(c1), r, -0.5, 1.5, 1))
        else:
            spheres.append((tuple(c0), tuple(c0), r, 0.0, 0.0, 0))
    return cases, spheres


@pytest.fixture(scope="module")
def case_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("beamcases")
    cases, spheres = generated_cases()
    assert len(cases) >= 300
    for cam, (W, H, rb, rs, rc) in cases:
        assert W >= 2 and H >= 2 and rb < rs and rb + (rc - 1) * rs < H
        assert all(np.isfinite(np.asarray(getattr(cam, f), float)).all() for f in vars(cam))
    return write_beam_scene(d / "scene.txt", spheres), write_beam_cases(d / "cases.txt", cases)


def test_generated_cameras_and_aimed_rays(exe, case_files):
    """No violation over the generated cases, extremes and aimed rays; and the
    run meets what it is for: most narrow (tile, sphere) pairs are excluded
    (only an excluded sphere can be a violation), a share of the tiles is
    answered by the wide-cone guard (a full mask), a share holds a sphere of
    negative radius, and the rays do hit narrow spheres."""
    t = time.time()
    p, rays, hits, viol = _run(exe, case_files[0], "cases", case_files[1])
    print(p.stdout, f"host run time {time.time() - t:.1f} s")
    assert viol == 0 and p.returncode == 0, p.stderr
    m = re.search(r"pairs (\d+) in_mask (\d+) tiles (\d+) full_tiles (\d+) neg_tiles (\d+) narrow_hits (\d+) aimed (\d+)", p.stdout)
    assert m, p.stdout
    pairs, in_mask, tiles, full, neg, narrow_hits, aimed = map(int, m.groups())
    print(f"excluded {1 - in_mask / pairs:.3f} of {pairs} pairs; full {full / tiles:.3f}, negative radius {neg / tiles:.3f} "
          f"of {tiles} tiles; {narrow_hits} narrow hits; {aimed} aimed rays")
    assert pairs - in_mask >= 0.5 * pairs
    assert full >= 0.05 * tiles
    assert neg >= 0.10 * tiles
    assert narrow_hits > 1_000_000
    assert aimed >= 17 * 3 * (pairs - in_mask) // 2  # (a singular aim is skipped; wide spheres add some)


# One-token mistakes in rtw_beam.hpp: (needle, replacement).  The p2 and fmin ones
# show only with the sheared camera structs.
MUTANTS = {
    "no_fabs": ("double r = std::fabs(radius);", "double r = radius;"),
    "no_cone_guard": ("if (!(b.DD - bw * bw > 1e-6 * (b.DD + bw * bw))) return true;", ""),
    "one_diagonal": ("b.h = std::sqrt(std::fmax(p2, m2));", "b.h = std::sqrt(p2);"),
    "lens_fmin": ("std::sqrt(std::fmax(uu, vv) + std::fabs(uv))", "std::sqrt(std::fmin(uu, vv))"),
    "no_jitter_s": ("s1 = ((double)px1 + 1.0) / w1", "s1 = (double)px1 / w1"),
    "no_jitter_t": ("t1 = ((double)H - (double)y0) / h1", "t1 = ((double)H - 1.0 - (double)y0) / h1"),
    "shutter_start": ("const double fm = 0.5 * (f0 + f1);", "const double fm = f0;"),
    "no_first_piece": ("if (beam_piece(E, b, r + b.R, b.h - b.R, 0.0, 1.0)) return true;", ""),
}


@pytest.mark.parametrize("name", MUTANTS)
def test_check_detects_mutant_on_generated_cases(name, tmp_path, case_files):
    needle, repl = MUTANTS[name]
    weak = tmp_path / "weak"
    weak.mkdir()
    src = open(os.path.join(CSRC, "rtw_beam.hpp")).read()
    assert needle in src
    (weak / "rtw_beam.hpp").write_text(src.replace(needle, repl))
    exe = build_beam_check(tmp_path, str(weak), "beamchk_" + name)
    p, _, _, viol = _run(exe, case_files[0], "cases", case_files[1], "quick")  # (stops at the first violating case)
    print(name, p.stdout, p.stderr)
    assert viol > 0 and p.returncode == 1
