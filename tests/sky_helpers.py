"""Shared pieces of tests/test_beam_empty_host.py and tests/test_gpu_sky.py: the host evaluation of the
megakernel's "proven empty" rule for a tile (tests/native/beam_empty_check.cpp over csrc/rtw_beam.hpp:
no sphere of the scene, wide ones included, may be hit by a camera ray of the tile), cameras as plain
field sets, and the scenes of the cases."""
import json
import math
import os
import re
import subprocess
import tempfile
import types

from helpers import write_beam_cases, write_beam_scene

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "raytracinginoneweekend.zig_amd", "csrc")
GOLDEN = os.path.join(REPO, "tests", "golden", "cover_scene_seed42.json")

_exe = {}


def empty_check_exe(header_dir=None):
    """beam_empty_check built once per process and header directory (default: csrc)."""
    header_dir = header_dir or CSRC
    if header_dir not in _exe:
        import atexit
        import shutil
        d = tempfile.mkdtemp(prefix="beamempty")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, "beam_empty_check")
        subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-I", str(header_dir),
                        os.path.join(REPO, "tests", "native", "beam_empty_check.cpp"), "-o", exe], check=True)
        _exe[header_dir] = exe
    return _exe[header_dir]


def host_empty(spheres, cases, header_dir=None):
    """spheres: (c0, c1, radius, t0, t1, moving) tuples; cases: (camera, (W, H, row_begin, row_stride,
    row_count)) -> per case a dict of tiles, empty (a sorted list of tile indices), rays, violations."""
    with tempfile.TemporaryDirectory(prefix="emptycase") as d:
        sc = write_beam_scene(d + "/scene.txt", spheres)
        cs = write_beam_cases(d + "/cases.txt", cases)
        p = subprocess.run([empty_check_exe(header_dir), sc, cs, "list"], capture_output=True, text=True)
    assert p.returncode in (0, 1), p.stdout + p.stderr
    out = []
    for m in re.finditer(r"case (\d+) tiles (\d+) empty (\d+) rays (\d+) violations (\d+)\nempty \d+:([ \d]*)", p.stdout):
        lst = [int(x) for x in m.group(6).split()]
        assert len(lst) == int(m.group(3))
        out.append({"tiles": int(m.group(2)), "empty": lst, "rays": int(m.group(4)), "violations": int(m.group(5))})
    assert len(out) == len(cases), p.stdout + p.stderr
    return out


def frame(w, h, row_begin=0, row_stride=1, row_count=None):
    if row_count is None:
        row_count = (h - row_begin + row_stride - 1) // row_stride
    return (w, h, row_begin, row_stride, row_count)


def rtw_spheres_as_tuples(sph):
    return [(list(s.c0), list(s.c1), s.radius, s.t0, s.t1, int(s.moving)) for s in sph]


def host_empty_for(sph, cam, params):
    """The proven-empty tiles of one render (rtw Sphere array, Camera, Params)."""
    return host_empty(rtw_spheres_as_tuples(sph), [(cam, (params.width, params.height, params.row_begin,
                                                          params.row_stride, params.row_count))])[0]


def untraced(empty_tiles, w, row_count, spp, chunk):
    """(units, samples) the kernel must report for these tiles: per tile its pixels inside the frame (padding
    units are left out), times the chunks / the samples."""
    tiles_x = (w + 7) // 8
    px = 0
    for t in empty_tiles:
        ty, tx = divmod(t, tiles_x)
        px += min(8, w - 8 * tx) * min(8, row_count - 8 * ty)
    return px * -(-spp // chunk), px * spp


def cover_tuples():
    return [(s["c0"], s["c1"], s["radius"], s["t0"], s["t1"], s["moving"]) for s in json.load(open(GOLDEN))["spheres"]]


def cam_init(frm, at, vup, vfov, aspect, aperture, focus, t0=0.0, t1=1.0):
    """Camera.init (main.zig:60-89) as a namespace with the rtw_camera fields."""
    def unit(a):
        n = math.sqrt(sum(x * x for x in a))
        return [x / n for x in a]

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    hh = math.tan(math.radians(vfov) / 2.0)
    vh, vw = 2.0 * hh, aspect * 2.0 * hh
    w = unit([x - y for x, y in zip(frm, at)])
    u = unit(cross(vup, w))
    v = cross(w, u)
    hor, ver = [x * focus * vw for x in u], [x * focus * vh for x in v]
    llc = [o - 0.5 * a - 0.5 * b - focus * c for o, a, b, c in zip(frm, hor, ver, w)]
    return types.SimpleNamespace(origin=list(map(float, frm)), horizontal=hor, vertical=ver, lower_left_corner=llc, u=u, v=v,
                                 lens_radius=aperture / 2.0, time0=t0, time1=t1)


COVER_CAM = dict(frm=(13, 2, 3), at=(0, 0, 0), vup=(0, 1, 0), vfov=20.0, aperture=0.1, focus=10.0)

GROUND = ((0, -1000, 0), (0, -1000, 0), 1000.0, 0.0, 0.0, 0)
HOLLOW = ((13, 2, 3), (13, 2, 3), -150.0, 0.0, 0.0, 0)  # around the cover camera
# radius 120, far behind the scene: during the shutter it moves into the right part of the cover camera's sky
MOVER = ((-450.0, 100.0, -420.0), (-450.0, 100.0, -220.0), 120.0, 0.0, 1.0, 1)


def mover_at(f):
    """MOVER as a static sphere at fraction f of its travel."""
    c = tuple(a + (b - a) * f for a, b in zip(MOVER[0], MOVER[1]))
    return (c, c, MOVER[2], 0.0, 0.0, 0)


def narrow(n, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        x, z, r = -6 + 12 * rng.random(), -6 + 12 * rng.random(), 0.2 + 0.5 * rng.random()
        c0 = (x, r, z)
        if k % 3 == 0:
            out.append((c0, (x, r + 0.5 * rng.random(), z), r, 0.0, 1.0, 1))
        else:
            out.append((c0, c0, r, 0.0, 0.0, 0))
    return out


# ------------------------------------------------------------------ GPU ----
def gpu_check(rtw, oracle, rend, sph, osc, cam, what, **kw):
    """One f64 megakernel frame against oracle Tier B, bit for bit (max|d| == 0); the counting pass's
    samples, segments, static and moving tests are the oracle's own counts; and the units and samples
    finished without tracing are what the HOST rule gives for this camera, scene and frame (0 at depth 0
    and where the launch cannot take the shortcut).  Returns (image, stats, empty tiles of the host rule)."""
    import torch

    from helpers import diff_stats, to_oracle_camera
    params = rtw.make_params(**kw)
    g = rend.render(cam, params)
    torch.cuda.synchronize()
    g = g.cpu().numpy()
    okw = dict(kw)
    w, h, spp = okw.pop("width"), okw.pop("height"), okw.pop("spp")
    depth = okw.pop("max_depth", 50)
    if "background" in okw:
        okw["bg"] = okw.pop("background")
    o, ost = oracle.render_tier_b(osc, to_oracle_camera(oracle, cam), w, h, spp, depth=depth, **okw)
    d = diff_stats(g, o)
    st, cnt = rend.stats(cam, params), rend.counts(cam, params)
    host = host_empty_for(sph, cam, params)
    chunk = min(params.chunk or rtw.DEFAULT_CHUNK, spp)
    want = untraced(host["empty"], w, params.row_count, spp, chunk) if depth >= 1 else (0, 0)
    print(what, d, {k: st[k] for k in ("samples", "segments", "primary_rounds", "sphere_loop_wave_iters",
                                        "untraced_units", "untraced_samples")}, "host", len(host["empty"]), want)
    assert d["max"] == 0, (what, d)
    assert host["violations"] == 0
    for k in ("samples", "segments", "static_tests", "moving_tests"):
        assert cnt[k] == ost[k], (what, k, cnt, ost)
    assert st["samples"] == ost["samples"] and st["segments"] == ost["segments"], (what, st, ost)
    assert (st["untraced_units"], st["untraced_samples"]) == want, (what, st, want)
    return g, st, host["empty"]
