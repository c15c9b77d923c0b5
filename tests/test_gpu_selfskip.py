"""The f64 megakernel's prefilter for the sphere a ray has just left (csrc/rtw_selfskip.hpp):
an exact test whose hb and cc satisfy rtws::leaves ends at the prefilter, where the older rule (cc > 0) let a
sphere under the ray's own origin go on to a square root and two divisions.  Every frame is bit-identical
(max|d| = 0) to oracle Tier B, with the oracle's samples and segments: the cover scene and a scene of
touching glass, hollow-glass, mirror, fuzzy-metal and moving spheres, at 8x8x8 (one wave), 24x16x8 and
48x27x20, max_depth 1, 2 and 50, with the tail dealing on (the product library) and off (a child process
with the development library and RTW_TRACE_TAIL=0).  The counting pass proves that the rule does something:
fewer lanes reach the root solve (cand_lanes) than in the same frame with the rule compiled out
(lib_ns/librtw_hip.so, -DRTW_NO_SELFSKIP, in a child process), every other per-lane count unchanged.  The
wavefront engine, which shares closest_hit without the rule, still gives the megakernel's bytes.

Not here: removing the sphere from the survivor loop altogether, with its self_skips counter, was built and
measured and did not pay (profiles/r25/README.md), so there is no such counter to assert.  t_min is 0.001 in
the C ABI and in the oracle (rayColor's constant), so no GPU frame can vary it: the range 1e-6 .. 1e-1 is
covered on the host, tests/test_selfskip_host.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import to_oracle_scene
from tail_helpers import check, spheres

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "raytracinginoneweekend.zig_amd")
MEASURE_LIB = os.path.join(PKG, "lib_m", "librtw_hip.so")
NOSKIP_LIB = os.path.join(PKG, "lib_ns", "librtw_hip.so")
CHILD = os.environ.get("RTW_SELFSKIP_CHILD")  # "tail_off": this process is test_tail_dealing_off's child

SIZES = [(8, 8, 8), (24, 16, 8), (48, 27, 20)]
DEPTHS = [1, 2, 50]
COUNT_KW = dict(width=48, height=27, spp=20)


def touching_scene(rtw):
    """The ground and spheres that touch it and each other: glass with a hollow (negative radius) glass
    sphere inside, touching the first's surface from inside at one point; a mirror and a fuzzy metal sphere
    that touch the glass; a diffuse sphere that moves through the mirror's tangent point over the shutter;
    a moving glass sphere; a small diffuse sphere resting in the gap.  Rays leave, enter, graze and are
    reflected between surfaces a rounding error apart."""
    mats = (rtw.Material * 6)()
    mats[0].kind = rtw.LAMBERT_CHECKER
    mats[0].albedo[:] = (0.9, 0.9, 0.9)
    mats[0].albedo_odd[:] = (0.2, 0.3, 0.1)
    mats[1].kind = rtw.LAMBERT_SOLID
    mats[1].albedo[:] = (0.7, 0.3, 0.2)
    mats[2].kind, mats[2].fuzz = rtw.METAL, 0.0
    mats[2].albedo[:] = (0.8, 0.8, 0.7)
    mats[3].kind, mats[3].ir = rtw.DIELECTRIC, 1.5
    mats[4].kind, mats[4].fuzz = rtw.METAL, 1.0
    mats[4].albedo[:] = (0.6, 0.7, 0.9)
    mats[5].kind = rtw.LAMBERT_SOLID
    mats[5].albedo[:] = (0.2, 0.4, 0.8)
    S = lambda c, r, m: (c, c, r, 0.0, 0.0, 0, m)
    specs = [
        S((0, -1000, 0), 1000.0, 0),
        S((0, 1, 0), 1.0, 3),             # glass, touching the ground
        S((0, 1.05, 0), -0.95, 3),        # hollow inside it, touching its top from inside
        S((2, 1, 0), 1.0, 2),             # mirror touching the glass and the ground
        S((-1.5, 0.5, 0), 0.5, 4),        # fuzz 1 touching the glass ((1.5)^2 + (0.5)^2 = 1.5^2 + .25: nearly)
        ((2, 1, 1.5), (2, 1.5, 1.5), 0.5, 0.0, 1.0, 1, 1),     # diffuse, touches the mirror at shutter start
        ((0.9, 0.4, 1.6), (0.9, 0.4, 1.9), 0.4, 0.0, 1.0, 1, 3),  # moving glass on the ground
        S((1, 0.2, 0.75), 0.2, 5),        # small diffuse sphere in the gap
        S((-0.6, 0.3, 1.4), 0.3, 1),
        S((-0.6, 0.9, 1.4), -0.25, 3),    # a hollow bubble resting on it (negative radius alone)
        S((0.4, 0.25, 2.2), 0.25, 2),
    ]
    return spheres(rtw, specs), mats


@pytest.fixture(scope="module")
def scenes(rtw, oracle):
    from rtw_amd.device import TorchRenderer
    sph, mats, _ = rtw.cover_scene(42)
    cover = (sph, mats, to_oracle_scene(oracle, sph, mats), TorchRenderer(sph, mats, 0), rtw.cover_camera(16 / 9))
    tsph, tmats = touching_scene(rtw)
    tcam = rtw.camera_init((5, 2.2, 6), (0.5, 0.8, 0), (0, 1, 0), 28.0, 16 / 9, 0.05, 8.0, 0.0, 1.0)
    touching = (tsph, tmats, to_oracle_scene(oracle, tsph, tmats), TorchRenderer(tsph, tmats, 0), tcam)
    return {"cover": cover, "touching": touching}


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("size", SIZES, ids=["%dx%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("name", ["cover", "touching"])
def test_frames_equal_the_oracle(rtw, oracle, scenes, name, size, depth):
    sph, mats, osc, rend, cam = scenes[name]
    w, h, spp = size
    g, st = check(rtw, oracle, rend, sph, mats, osc, cam, f"{name} {w}x{h}x{spp} depth {depth}", helped=None, width=w,
                  height=h, spp=spp, max_depth=depth)
    print({k: st[k] for k in ("cand_lanes", "disc_ge0_lanes", "cull_survivor_lanes")})
    assert st["cand_lanes"] <= st["disc_ge0_lanes"]


def test_fewer_lanes_reach_the_root_solve(rtw, scenes):
    """The cover scene at 48x27x20: the per-lane counts (the wave-level ones depend on which lanes share a
    wave).  With the rule, the lanes whose test passes disc >= 0 are the same and fewer of them are candidates
    for the root solve: at least the rays that leave a narrow sphere with cc <= 0, about a tenth here."""
    _, _, _, rend, cam = scenes["cover"]
    st = rend.stats(cam, rtw.make_params(**COUNT_KW))
    keys = ("samples", "segments", "disc_ge0_lanes", "cull_survivor_lanes", "cand_lanes")
    print({k: st[k] for k in keys})
    if CHILD:
        return
    assert os.path.exists(NOSKIP_LIB), "no -DRTW_NO_SELFSKIP library (make lib_ns/librtw_hip.so)"
    code = ("import json, sys; sys.path[:0] = %r; import rtw_amd as R; from rtw_amd.device import TorchRenderer; "
            "sph, mats, _ = R.cover_scene(42); rend = TorchRenderer(sph, mats, 0); "
            "st = rend.stats(R.cover_camera(16 / 9), R.make_params(**%r)); print('STATS ' + json.dumps(st))"
            % ([PKG], COUNT_KW))
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, RTW_LIB_PATH=NOSKIP_LIB), cwd=REPO,
                       capture_output=True, text=True, timeout=300)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("STATS ")]
    assert p.returncode == 0 and line, p.stdout[-2000:] + p.stderr[-2000:]
    ns = json.loads(line[0][6:])
    print("rule compiled out:", {k: ns[k] for k in keys})
    for k in ("samples", "segments", "disc_ge0_lanes", "cull_survivor_lanes"):
        assert ns[k] == st[k], (k, st, ns)
    assert st["cand_lanes"] < 0.95 * ns["cand_lanes"], (st, ns)


def test_wavefront_engine_gives_the_same_bytes(rtw, scenes):
    for name in ("cover", "touching"):
        sph, mats, _, _, cam = scenes[name]
        kw = dict(width=48, height=27, spp=8)
        a = rtw.render(cam, sph, mats, rtw.make_params(**kw), want_mean=True)
        b = rtw.render(cam, sph, mats, rtw.make_params(engine="wavefront", wf_paths=4096, **kw), want_mean=True)
        assert np.array_equal(a[0], b[0]), name
        assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), name


@pytest.mark.skipif(bool(CHILD), reason="this process is the child")
def test_tail_dealing_off():
    """The frames and counts above once more in a child process with the development library
    (lib_m/librtw_hip.so, -DRTW_MEASURE, which `make` builds) and RTW_TRACE_TAIL=0: the loop without the tail."""
    assert os.path.exists(MEASURE_LIB), "no development library (make lib_m/librtw_hip.so)"
    env = dict(os.environ, RTW_LIB_PATH=MEASURE_LIB, RTW_TRACE_TAIL="0", RTW_SELFSKIP_CHILD="tail_off")
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__)],
                       env=env, cwd=REPO, capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and " passed" in p.stdout and "failed" not in p.stdout, p.stdout[-3000:] + p.stderr[-2000:]
