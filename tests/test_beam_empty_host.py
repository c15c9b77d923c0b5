"""The megakernel finishes the units of a tile without tracing when csrc/rtw_beam.hpp's bound says
that no camera ray of the tile can hit ANY sphere, the wide ones included (rtw_trace.hip take_units,
TraceArgs::empty_on).  tests/native/beam_empty_check.cpp evaluates that rule on the host and, for
every tile it proves empty, solves rays exactly in f64 against every sphere — the tile's corners and
edge midpoints, 8 lens-rim points and the lens centre, both shutter ends, and 64 seeded random rays —
and must find no root >= 0.  The counts below keep the check from passing vacuously."""
import shutil

import numpy as np
import pytest

from sky_helpers import (COVER_CAM, GROUND, HOLLOW, MOVER, cam_init, cover_tuples, frame, host_empty, mover_at,
                         narrow)

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

ASPECT = 16 / 9


def test_cover_frames_prove_the_sky_and_nothing_else():
    cam = cam_init(aspect=ASPECT, **COVER_CAM)
    big, small, tiny = host_empty(cover_tuples(), [(cam, frame(1200, 675)), (cam, frame(128, 72)), (cam, frame(64, 36))])
    print({k: (len(r["empty"]), r["tiles"], r["rays"]) for k, r in (("1200x675", big), ("128x72", small), ("64x36", tiny))})
    assert big["tiles"] == 12750 and big["violations"] == small["violations"] == 0
    assert len(big["empty"]) >= 1900
    assert len(small["empty"]) == 9
    assert big["rays"] == len(big["empty"]) * (8 * 9 * 2 + 64)


def test_hollow_sphere_around_the_camera_proves_nothing():
    """Every camera ray hits the shell of radius -150 from inside."""
    cam = cam_init(aspect=ASPECT, **COVER_CAM)
    for scene in ([GROUND, HOLLOW], cover_tuples() + [HOLLOW]):
        for r in host_empty(scene, [(cam, frame(128, 72)), (cam, frame(100, 72, 1, 3))]):
            assert r["empty"] == [] and r["tiles"] > 0


def test_moving_sphere_is_bounded_over_its_travel():
    """The tiles proven empty with the radius-120 sphere moving during the shutter are empty with that sphere
    standing at either shutter end too, and the sphere does take tiles away from the sky."""
    cam = cam_init(aspect=ASPECT, **COVER_CAM)
    cases = [(cam, frame(128, 72)), (cam, frame(320, 180))]
    without = host_empty([GROUND], cases)
    moving = host_empty([GROUND, MOVER], cases)
    ends = [host_empty([GROUND, mover_at(f)], cases) for f in (0.0, 1.0)]
    for i in range(len(cases)):
        m = set(moving[i]["empty"])
        print(len(without[i]["empty"]), len(m), [len(e[i]["empty"]) for e in ends])
        assert moving[i]["violations"] == 0
        assert 0 < len(m) < len(without[i]["empty"])
        for e in ends:
            assert m <= set(e[i]["empty"])
        assert any(len(m) < len(e[i]["empty"]) for e in ends)  # the travel covers more than either end


def _fuzzed(n, seed):
    rng = np.random.default_rng(seed)
    cases = []
    for k in range(n):
        frm = (rng.uniform(-15, 15), rng.uniform(0.3, 12), rng.uniform(-15, 15))
        # half of them look above the horizon, so that tiles of sky exist
        at = (rng.uniform(-4, 4), rng.uniform(-1, 2) if k % 2 else frm[1] + rng.uniform(0, 8), rng.uniform(-4, 4))
        t0 = rng.uniform(0, 0.6)
        cam = cam_init(frm, at, (0, 1, 0), rng.uniform(8, 70), ASPECT, rng.uniform(0, 2) if k % 4 else 0.0,
                       rng.uniform(2, 15), t0, t0 + rng.uniform(0, 1 - t0))
        w, h = int(rng.integers(17, 130)), int(rng.integers(9, 80))
        rs = int(rng.integers(1, 4))
        cases.append((cam, frame(w, h, int(rng.integers(0, rs)), rs)))
    return cases


@pytest.mark.parametrize("name,scene", [
    ("ground and narrow", [GROUND] + narrow(30, 7)),
    ("cover", cover_tuples()),
    ("ground, mover, narrow", [GROUND, MOVER] + narrow(12, 8)),
    ("hollow", [GROUND, ((0, 2, 0), (0, 2, 0), -150.0, 0.0, 0.0, 0)] + narrow(6, 9)),
])
def test_fuzzed_cameras_no_ray_of_a_proven_tile_hits(name, scene):
    res = host_empty(scene, _fuzzed(60, 1234))
    tiles, empty, rays = (sum(r["tiles"] for r in res), sum(len(r["empty"]) for r in res), sum(r["rays"] for r in res))
    print(name, "tiles", tiles, "empty", empty, "rays", rays)
    assert sum(r["violations"] for r in res) == 0
    if name == "hollow":  # every fuzzed camera is inside the shell
        assert empty == 0
    else:
        assert empty > tiles // 20 and rays > 100_000
        assert sum(1 for r in res if r["empty"] and len(r["empty"]) < r["tiles"]) >= 10  # frames with a horizon
