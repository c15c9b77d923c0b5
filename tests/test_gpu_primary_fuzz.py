"""The primary-first loop's tile masks on the device, away from the cover camera
(tests/test_beam_host.py has the host side).  For every case:
the f64 megakernel render is bit-identical to oracle Tier B; the wavefront
engine, which has no primary phase, gives the same bytes (so a difference of
the megakernel alone points at the mask); the loop that ran is the one the host
rules predict (f64, the shutter inside every time group, 1..64 narrow spheres);
and primary_mask_popcount equals the host evaluation of csrc/rtw_beam.hpp for
the same camera, frame and scene (helpers.host_masks), which ties the device's
slot -> position table, group times, travel vectors, cvalid and the ballot's
bit order to the host's masks.

Frames of 17x9, 9x17 and 16x16 (partial tiles both ways) at 8 spp in chunks of
4: two batches per tile, so a wave holds units of a current and a new batch."""
import numpy as np
import pytest

from helpers import host_masks, to_oracle_scene
from test_gpu_primary import check, materials, scattered, spheres

pytestmark = pytest.mark.gpu

GROUND = ((0, -1000, 0), (0, -1000, 0), 1000.0, 0.0, 0.0, 0, 0)
FROM, AT = (13, 2, 3), (0, 0.3, 0)


def camera(rtw, w, h, frm=FROM, at=AT, vup=(0, 1, 0), vfov=30.0, aperture=0.1, focus=10.0, t0=0.0, t1=1.0):
    return rtw.camera_init(frm, at, vup, vfov, w / h, aperture, focus, t0, t1)


def field(rtw, n_narrow, seed, groups=((0.0, 1.0),), travel=(0.2, 0.6), neg=False, extra=(), ground=True):
    """`scattered`'s layout with two more knobs: movers that travel `travel` units, and (neg) a third of
    the narrow spheres hollow (radius -0.2 to -0.5, on the field, away from the camera), half of those glass."""
    rng = np.random.default_rng(seed)
    specs = [GROUND] * ground + list(extra)
    for k in range(n_narrow):
        x, z = -6 + 12 * rng.random(), -6 + 12 * rng.random()
        r, mat = 0.15 + 0.3 * rng.random(), 1 + k % 4
        if neg and k % 3 == 2:
            r, mat = -(0.2 + 0.3 * rng.random()), (3 if k % 2 else 1)
        c0 = (x, abs(r), z)
        if k % 4 == 0:
            specs.append((c0, c0, r, 0.0, 0.0, 0, mat))
            continue
        dv = [0.0, 0.0, 0.0]
        dv[k % 4 - 1] = travel[0] + (travel[1] - travel[0]) * rng.random()
        t0, t1 = groups[k % len(groups)]
        specs.append((c0, tuple(c + d for c, d in zip(c0, dv)), r, t0, t1, 1, mat))
    return spheres(rtw, specs)


def predicted_primary(sph, cam):
    """rtw_capi.hip launch_engine for an f64 megakernel frame: clusters_usable and one 64-slot block
    (ceil(narrow / 8) clusters of 8 slots)."""
    narrow = sum(1 for s in sph if not s.radius >= 100.0)
    groups = {(s.t0, s.t1) for s in sph if s.moving}
    return all(cam.time0 >= a and cam.time1 <= b for a, b in groups) and 1 <= narrow <= 64


def run(rtw, oracle, sph, cam, what, primary, **kw):
    """The four assertions; returns (image, stats, host masks)."""
    kw = dict(dict(spp=8, chunk=4), **kw)
    mats = materials(rtw)
    assert predicted_primary(sph, cam) == primary, what  # the case is what it says
    g, st = check(rtw, oracle, sph, mats, to_oracle_scene(oracle, sph, mats), cam, what, primary=primary, **kw)
    wf = rtw.render(cam, sph, mats, rtw.make_params(engine="wavefront", wf_paths=1024, **kw))
    assert np.array_equal(wf, g), what
    return g, st, host_masks(sph, cam, rtw.make_params(**kw))


def test_negative_radii(rtw, oracle):
    sph = field(rtw, 30, 101, neg=True)
    assert sum(s.radius < 0 for s in sph) == 10 and sum(s.radius < 0 and s.mat == 3 for s in sph) >= 3
    run(rtw, oracle, sph, camera(rtw, 17, 9), "negative radii", True, width=17, height=9)


def test_wide_cone_every_tile_guarded(rtw, oracle):
    """vfov 140 with a lens radius of 1 at focus distance 2: every tile's cone is wider than the
    guard's ~45 degrees, every mask is full (with a small lens the off-axis tiles of this frame,
    whose axes are long, stay just inside the guard)."""
    sph = scattered(rtw, 30, 102)
    cam = camera(rtw, 16, 16, vfov=140.0, aperture=2.0, focus=2.0)
    _, st, hm = run(rtw, oracle, sph, cam, "vfov 140", True, width=16, height=16)
    assert hm["guarded"] == hm["tiles"] == 4 and hm["narrow"] == 30
    assert st["primary_mask_popcount"] == 4 * 2 * 30


def test_cone_near_the_guard(rtw, oracle):
    """vfov 100 at 17x9: the two 8x8 tiles are guarded, the 1-pixel wide and high ones are not."""
    sph = scattered(rtw, 30, 103)
    _, _, hm = run(rtw, oracle, sph, camera(rtw, 17, 9, vfov=100.0), "vfov 100", True, width=17, height=9)
    assert hm["tiles"] == 6 and 0 < hm["guarded"] < 6


@pytest.mark.parametrize("t0,t1", [(0.25, 0.75), (0.5, 0.5)])
def test_shutter_inside_the_groups(rtw, oracle, t0, t1):
    sph = field(rtw, 28, 104, groups=((0.0, 1.0), (-0.5, 1.5)), travel=(3.0, 3.0))
    run(rtw, oracle, sph, camera(rtw, 17, 9, t0=t0, t1=t1), f"shutter [{t0}, {t1}]", True, width=17, height=9)


def test_group_without_the_shutter_falls_back(rtw, oracle):
    sph = field(rtw, 24, 105, groups=((0.0, 1.0), (0.3, 0.6)))
    run(rtw, oracle, sph, camera(rtw, 16, 16), "group (0.3, 0.6)", False, width=16, height=16)


def test_pinhole(rtw, oracle):
    run(rtw, oracle, scattered(rtw, 26, 106), camera(rtw, 17, 9, aperture=0.0), "aperture 0", True, width=17, height=9)


def test_lens_larger_than_focus_distance_among_the_spheres(rtw, oracle):
    cam = camera(rtw, 17, 9, frm=(2.0, 0.3, 2.5), at=(-3.0, 0.3, -1.0), vfov=50.0, aperture=4.0, focus=0.3)
    run(rtw, oracle, scattered(rtw, 34, 107), cam, "aperture 4 focus 0.3", True, width=17, height=9)


def test_straight_down(rtw, oracle):
    cam = camera(rtw, 16, 16, frm=(0.5, 6.0, 0.3), at=(0.5, 0.0, 0.3), vup=(0, 0, -1), vfov=60.0)
    run(rtw, oracle, scattered(rtw, 32, 108), cam, "straight down", True, width=16, height=16)


def test_rolled_portrait(rtw, oracle):
    cam = camera(rtw, 9, 17, vup=(0.6, 0.8, 0.3), vfov=40.0)
    run(rtw, oracle, scattered(rtw, 36, 109), cam, "rolled, 9x17", True, width=9, height=17)


def test_sheared_camera_struct(rtw, oracle):
    """A struct rtw_camera_init never makes: horizontal and vertical not orthogonal, u and v not
    orthonormal.  The oracle gets the same fields (helpers.to_oracle_camera)."""
    cam = camera(rtw, 17, 9, aperture=1.0)
    hor, ver, u, v = (np.array(list(x)) for x in (cam.horizontal, cam.vertical, cam.u, cam.v))
    hor = hor + 0.3 * ver
    ver = 0.8 * ver
    u = u + 0.4 * v
    v = 0.9 * v + 0.2 * u
    cam.horizontal[:], cam.vertical[:], cam.u[:], cam.v[:] = hor, ver, u, v
    assert abs(hor @ ver) > 0.1 and abs(u @ v) > 0.1 and abs(u @ u - 1) > 0.1
    run(rtw, oracle, scattered(rtw, 30, 110), cam, "sheared struct", True, width=17, height=9)


@pytest.mark.parametrize("n,primary", [(64, True), (65, False), (1, True)])
def test_slot_count(rtw, oracle, n, primary):
    _, _, hm = run(rtw, oracle, scattered(rtw, n, 111), camera(rtw, 16, 16), f"{n} narrow spheres", primary,
                   width=16, height=16)
    assert hm["narrow"] == n


def test_no_narrow_sphere_falls_back(rtw, oracle):
    sph = spheres(rtw, [GROUND, ((-170, 60, -340), (-170, 60, -340), 150.0, 0.0, 0.0, 0, 2)])
    run(rtw, oracle, sph, camera(rtw, 16, 16), "no narrow sphere", False, width=16, height=16)


@pytest.mark.parametrize("w,h,rows", [(17, 33, dict(row_begin=5, row_stride=4)),
                                      (9, 17, dict(row_begin=10, row_stride=1, row_count=5))])
def test_row_selection(rtw, oracle, w, h, rows):
    """17x33 rows 5::4: the one tile row's 7 rows span image rows 5..29, a tall beam; 9x17 rows
    10..14: row_count is not what the frame's height gives."""
    _, _, hm = run(rtw, oracle, scattered(rtw, 30, 112), camera(rtw, w, h), f"{w}x{h} {rows}", True, width=w, height=h,
                   **rows)
    assert hm["tiles"] == (w + 7) // 8


def test_spheres_at_the_lens(rtw, oracle):
    """Radius 0.04 centred 0.05 beside the origin with a lens radius of 0.1: the sphere cuts the lens
    disk and does not contain the origin; and one of radius 0.3 a unit behind the camera."""
    cam = camera(rtw, 17, 9, aperture=0.2)
    o, u, w = (np.array(list(x)) for x in (cam.origin, cam.u, cam.w))
    extra = [(tuple(o + 0.05 * u),) * 2 + (0.04, 0.0, 0.0, 0, 2), (tuple(o + 1.0 * w),) * 2 + (0.3, 0.0, 0.0, 0, 1)]
    run(rtw, oracle, scattered(rtw, 25, 113, extra=extra), cam, "spheres at the lens", True, width=17, height=9)


def test_enclosing_dome(rtw, oracle):
    """A narrow (radius 60) Lambertian sphere around camera and scene is in every mask: no camera ray
    ends in the primary phase, and no path reaches the background."""
    dome = ((0, 0, 0), (0, 0, 0), 60.0, 0.0, 0.0, 0, 1)
    g, st, hm = run(rtw, oracle, scattered(rtw, 20, 114, extra=[dome]), camera(rtw, 16, 16), "dome", True,
                    width=16, height=16, background=(3.0, 3.0, 3.0))
    assert st["primary_idle_lanes"] == 0 and hm["popcount"] >= hm["tiles"]
    assert (g == 0).all()


@pytest.mark.parametrize("depth", [1, 50])
@pytest.mark.parametrize("bg", [(0.0, 0.0, 0.0), (1.5, 0.25, 0.0)])
def test_background(rtw, oracle, bg, depth):
    """A camera ray that misses ends in the primary phase with the background."""
    g, st, _ = run(rtw, oracle, scattered(rtw, 22, 115), camera(rtw, 17, 9, vfov=40.0), f"background {bg} depth {depth}",
                   True, width=17, height=9, background=bg, max_depth=depth)
    assert st["primary_idle_lanes"] > 0
    if bg[0] > 0:
        assert (g[..., 0] == 255).any()  # the sky's red saturates where a camera ray misses
