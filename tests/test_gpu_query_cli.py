"""bin/rtw_render --pick and --focus-at (ray queries from the command line):
the printed hit is the oracle's hit of the pixel's feature ray, the pick's
primitive is the pixel's rtw_guide primitive, and --focus-at renders the image
of a camera focused at the hit's depth along the view axis."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from test_gpu_accum import _read_ppm

pytestmark = pytest.mark.gpu

W_, ASPECT = 60, 3 / 2          # scene 1's own aspect (main.zig:304): 60 x 40
LOOK_FROM, LOOK_AT = (13.0, 2.0, 3.0), (0.0, 0.0, 0.0)
HIT_PIXEL, SKY_PIXEL = (30, 20), (30, 0)


def _exe(rtw):
    return os.path.join(os.path.dirname(rtw.__file__), "..", "bin", "rtw_render")


@pytest.fixture(scope="module")
def scene1(rtw, oracle):
    from rtw_amd import world as W
    H = rtw.image_height(W_, ASPECT)
    cam = rtw.cover_camera(ASPECT)
    ow = oracle.OracleWorld(1, 42)

    def hit(x, y):
        r = rtw.pixel_ray(cam, W_, H, x, y)
        return ow.hit(list(r.origin), list(r.dir), r.time, r.t_min, r.t_max)
    built = W.BuiltScene(1, 42)
    return H, cam, hit, built


def test_pick_prints_the_oracles_hit(rtw, scene1):
    H, cam, hit, built = scene1
    x, y = HIT_PIXEL
    r = subprocess.run([_exe(rtw), "--scene", "1", "--width", str(W_), "--pick", f"{x},{y}"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    m = re.fullmatch(r"pick x=(\d+) y=(\d+) prim=(\d+) t=(\S+) p=([^, ]+),([^, ]+),([^, ]+) front=([01]) material=(\w+)\n",
                     r.stdout)
    assert m, r.stdout
    want = hit(x, y)
    assert want is not None
    assert (int(m.group(1)), int(m.group(2))) == (x, y)
    assert int(m.group(3)) == want["prim"] + 1
    assert float(m.group(4)) == want["t"]  # %.17g round-trips a double
    assert [float(m.group(k)) for k in (5, 6, 7)] == want["p"]
    assert int(m.group(8)) == int(want["front"])
    kind = built.desc.mats[built.desc.prims[want["prim"]].mat].kind
    assert m.group(9) == ("lambert", "metal", "dielectric", "light")[kind]
    # the same primitive as the pixel's guide
    sph, mats, _ = rtw.cover_scene(42)
    sc = rtw.DeviceScene(sph, mats)
    g = torch.zeros((H, W_, 32), dtype=torch.uint8, device="cuda")
    sc.guides(cam, rtw.make_params(W_, H, 1), g.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    guides = g.cpu().numpy().view(rtw.GUIDE_DTYPE).reshape(H, W_)
    assert int(guides[y, x]["prim"]) == int(m.group(3))
    sc.close()
    # a pixel of sky
    x, y = SKY_PIXEL
    assert hit(x, y) is None
    r = subprocess.run([_exe(rtw), "--scene", "1", "--width", str(W_), "--pick", f"{x},{y}"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and r.stdout == f"pick x={x} y={y} miss\n", r.stdout + r.stderr


def test_focus_at_renders_with_the_hits_depth(rtw, scene1, tmp_path):
    H, cam, hit, _ = scene1
    x, y = HIT_PIXEL
    out = tmp_path / "focus.ppm"
    r = subprocess.run([_exe(rtw), "--scene", "1", "--width", str(W_), "--spp", "20", "--focus-at", f"{x},{y}", "--out",
                        str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    m = re.search(r"^focus_dist=(\S+)$", r.stdout, re.M)
    assert m, r.stdout
    p = hit(x, y)["p"]
    a = [LOOK_AT[k] - LOOK_FROM[k] for k in range(3)]
    n = math.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])
    a = [v / n for v in a]
    f = (p[0] - LOOK_FROM[0]) * a[0] + (p[1] - LOOK_FROM[1]) * a[1] + (p[2] - LOOK_FROM[2]) * a[2]
    assert float(m.group(1)) == f
    sph, mats, _ = rtw.cover_scene(42)
    fcam = rtw.camera_init(LOOK_FROM, LOOK_AT, (0, 1, 0), 20.0, ASPECT, 0.1, f, 0.0, 1.0)
    want = rtw.render(fcam, sph, mats, rtw.make_params(W_, H, 20))
    assert np.array_equal(_read_ppm(str(out)), want)
    assert not np.array_equal(want, rtw.render(cam, sph, mats, rtw.make_params(W_, H, 20)))  # the focus matters


def test_focus_at_the_sky_is_an_error(rtw, tmp_path):
    x, y = SKY_PIXEL
    r = subprocess.run([_exe(rtw), "--scene", "1", "--width", str(W_), "--spp", "20", "--focus-at", f"{x},{y}", "--out",
                        str(tmp_path / "no.ppm")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "hits nothing" in r.stderr, r.stderr
    assert not (tmp_path / "no.ppm").exists()
