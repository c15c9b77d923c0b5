"""GPU parity of the general-world kernel (csrc/rtw_world.hip) against the
oracle's Tier B (oracle/rtw_world.c): every scene of the reference's main.zig
(1-6), the configs[4] globe + 10k spheres (7), a custom world exercising every
primitive / wrapper / material / texture under the LINEAR loop only (its 14
primitives get no BVH, as scenes 2-6), BVH == linear on the sphere worlds,
scene 1 == megakernel, and exactly-once sample counts.  The BVH counterpart
— rects, boxes, transform chains, lights and coincident primitives in worlds
of > 32 primitives, and the kernel's parameter edges — is
test_gpu_world_general.py.  Bar: as test_gpu_parity.py
(every channel within 1 LSB, >= 99.99 % bit-identical; observed: identical)."""
import numpy as np
import pytest

from helpers import _to_desc, diff_stats
from test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def W():
    from rtw_amd import world
    return world


@pytest.fixture(scope="module")
def earth(W):
    return W.earth_map()  # the reference's assets/sekaichizu.png


def built(W, scene, earth):
    return W.BuiltScene(scene, 42, image=earth if scene in (4, 7) else None)


def params(rtw, b, w, h, spp, **kw):
    return rtw.make_params(w, h, spp, 50, 42, background=b.background, **kw)


def oracle_world_from_desc(oracle, W, b, earth=None):
    t = b.table()
    imgs = [earth] if b.desc.n_images else []
    return oracle.TableWorld(t["prims"], t["xforms"], t["textures"], t["materials"], t["perlins"], imgs,
                             background=b.background)


@pytest.mark.parametrize("scene,w,spp,trav", [(1, 96, 4, "union"), (1, 96, 4, "lane"), (2, 96, 4, "union"),
                                              (3, 96, 4, "union"), (4, 96, 4, "union"), (5, 96, 8, "union"),
                                              (6, 64, 8, "union")])
def test_world_scene_parity(rtw, oracle, W, earth, scene, w, spp, trav):
    b = built(W, scene, earth)
    cam = b.camera()
    h = rtw.image_height(w, b.settings.aspect)
    g = W.render_world(cam, b.desc, params(rtw, b, w, h, spp, world_traversal=trav))
    o = oracle.OracleWorld(scene, 42, image=earth if scene in (4, 7) else None)
    ref, _ = o.render_tier_b(o.camera(), w, h, spp)
    assert_parity(g, ref, f"world scene {scene} {w}x{h}x{spp}")


def test_world_scene1_equals_megakernel(rtw, W, earth):
    b = built(W, 1, earth)
    cam = rtw.cover_camera(16 / 9)
    sph, mats, _ = rtw.cover_scene(42)
    p = rtw.make_params(200, 112, 12, chunk=5)
    mk, mkm = rtw.render(cam, sph, mats, p, want_mean=True)
    wd, wdm = W.render_world(cam, b.desc, p, want_mean=True)
    assert (mk == wd).all(), diff_stats(mk, wd)
    assert np.array_equal(mkm.view(np.uint32), wdm.view(np.uint32))


TRAVERSALS = ["union", "lane"]  # rtw_params.world_traversal: the wave's union walk / per-lane walks


@pytest.mark.parametrize("trav", TRAVERSALS)
def test_world_globe_parity(rtw, oracle, W, earth, trav):
    b = built(W, 7, earth)
    cam = b.camera()
    g = W.render_world(cam, b.desc, params(rtw, b, 64, 36, 2, world_traversal=trav))
    o = oracle.OracleWorld(7, 42, image=earth)
    ref, _ = o.render_tier_b(o.camera(), 64, 36, 2)
    assert_parity(g, ref, "globe 64x36x2")


@pytest.mark.parametrize("trav", TRAVERSALS)
def test_globe_config4_workload_equals_oracle(rtw, oracle, W, earth, trav):
    """BASELINE configs[4] at its bench workload: the globe + 10k-sphere frame
    at 1200x675x100 through the BVH (leaf pretest, outward-rounded f32 slabs:
    conservative bounds whose failure mode is a rare dropped hit).  16 rows
    spread over the frame (y = 7, 49, ..., 637; 1.92 M samples) equal the
    LINEAR oracle's Tier B (committed fixture, tests/golden/make_world_fixtures.py:
    ~15 CPU-minutes), and 2 more rows through the globe are rendered by the
    oracle live here (16 threads)."""
    import os
    import time

    from conftest import GOLDEN
    b = built(W, 7, earth)
    s = b.settings
    assert (s.width, s.height, s.spp) == (1200, 675, 100)
    cam = b.camera()
    t0 = time.time()
    g = W.render_world(cam, b.desc, params(rtw, b, s.width, s.height, s.spp, world_traversal=trav))
    t_gpu = time.time() - t0
    fx = np.load(os.path.join(GOLDEN, "globe_1200x675x100_rows7s42.npz"))
    rows = fx["rows"]
    assert len(rows) == 16 and int(fx["samples"]) == 16 * 1200 * 100
    d = diff_stats(g[rows], fx["rgb"])
    print(f"globe 1200x675x100 {trav} (GPU {t_gpu:.1f} s incl. upload + BVH build) vs fixture rows 7::42:", d)
    assert d["max"] == 0, d  # bit-identical
    o = oracle.OracleWorld(7, 42, image=earth)
    t0 = time.time()
    live, st = o.render_tier_b(o.camera(), 1200, 675, 100, row_begin=322, row_stride=42, row_count=2, threads=16)
    print(f"globe rows 322, 364 live oracle: {time.time() - t0:.1f} s, {st['segments']} segments")
    d2 = diff_stats(g[322:365:42], live)
    print("globe configs[4] rows 322, 364 (live oracle)", d2)
    assert d2["max"] == 0, d2


@pytest.mark.parametrize("scene,dims", [(3, (600, 400, 50)), (5, (600, 400, 400))])
def test_perlin_scenes_at_their_settings(rtw, oracle, W, earth, scene, dims):
    """The Perlin scenes at their own main.zig settings (scene 3 two Perlin
    spheres 600x400x50, scene 5 simple light 600x400x400; main.zig:304-308,
    :346), the WHOLE frame on the GPU (the Perlin worlds run their own
    feature-set instantiation at 2 waves/SIMD) against the oracle's world
    Tier B rendered live (16 threads; ~1-10 s)."""
    import time
    b = built(W, scene, earth)
    s = b.settings
    assert (s.width, s.height, s.spp) == dims
    g = W.render_world(b.camera(), b.desc, params(rtw, b, s.width, s.height, s.spp))
    o = oracle.OracleWorld(scene, 42)
    t0 = time.time()
    ref, st = o.render_tier_b(o.camera(), s.width, s.height, s.spp, threads=16)
    print(f"scene {scene} {s.width}x{s.height}x{s.spp} oracle: {time.time() - t0:.1f} s, {st['samples']} samples, "
          f"{st['segments']} segments")
    assert st["samples"] == s.width * s.height * s.spp
    d = diff_stats(g, ref)
    print(f"scene {scene} full frame", d)
    assert d["max"] == 0, d  # bit-identical
    assert g.std() > 5


def test_cornell_full_frame_equals_oracle(rtw, oracle, W, earth):
    """The reference's default scene (scene 6, main.zig:259-293, :352-362) at
    its own settings, 600x600x200 (72 M samples, ~6.6 segments each), the
    WHOLE frame against oracle world Tier B (16 threads)."""
    import time
    b = built(W, 6, earth)
    s = b.settings
    assert (s.width, s.height, s.spp) == (600, 600, 200)
    g = W.render_world(b.camera(), b.desc, params(rtw, b, s.width, s.height, s.spp))
    o = oracle.OracleWorld(6, 42)
    t0 = time.time()
    ref, st = o.render_tier_b(o.camera(), 600, 600, 200, threads=16)
    print(f"cornell 600x600x200 oracle: {time.time() - t0:.1f} s, {st['segments']} segments")
    assert st["samples"] == 600 * 600 * 200
    d = diff_stats(g, ref)
    print("cornell full frame 600x600x200", d)
    assert d["max"] == 0, d  # bit-identical
    assert g.std() > 5


def _render_dev(rtw, W, b, cam, p, linear):
    import torch
    dw = W.DeviceWorld(b.desc, linear=linear)
    need = dw.workspace_bytes(p)
    ws = torch.empty(need + 256, dtype=torch.uint8, device="cuda:0")
    ptr = (ws.data_ptr() + 255) & ~255
    rgb = torch.empty((p.row_count, p.width, 3), dtype=torch.uint8, device="cuda:0")
    mean = torch.empty((p.row_count, p.width, 3), dtype=torch.float32, device="cuda:0")
    dw.render_async(cam, p, ptr, need, rgb.data_ptr(), mean.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    counts = dw.counts(cam, p, ptr, need)
    info = dw.bvh_info()
    dw.close()
    return rgb.cpu().numpy(), mean.cpu().numpy(), counts, info


@pytest.mark.parametrize("trav", TRAVERSALS)
@pytest.mark.parametrize("scene,w,spp", [(7, 320, 4), (1, 160, 8)])
def test_world_bvh_equals_linear(rtw, W, earth, scene, w, spp, trav):
    b = built(W, scene, earth)
    cam = b.camera()
    h = rtw.image_height(w, b.settings.aspect)
    p = params(rtw, b, w, h, spp, world_traversal=trav)
    rb, mb, cb, info = _render_dev(rtw, W, b, cam, p, linear=False)
    rl, ml, cl, _ = _render_dev(rtw, W, b, cam, p, linear=True)
    assert (rb == rl).all() and np.array_equal(mb.view(np.uint32), ml.view(np.uint32)), diff_stats(rb, rl)
    assert cb["samples"] == cl["samples"] == w * h * spp
    assert cb["segments"] == cl["segments"]
    print(scene, trav, info, "prim tests bvh/linear", cb["prim_tests"], cl["prim_tests"],
          "node visits per segment", cb["node_visits"] / cb["segments"])
    assert info["nodes"] > 0  # worlds of > 32 primitives get a BVH
    if scene == 7:
        assert info["max_depth"] <= 32 and cb["prim_tests"] * 50 < cl["prim_tests"]
        assert cb["traversal"] == trav
        if trav == "lane":  # each lane's own walk (VERDICT r4 ask 2: <= 25 node visits per lane-segment)
            assert cb["lane_interior_iters"] > 0 and cb["node_visits"] <= 25 * cb["segments"]
            # its LDS (stack columns, walk rows, attenuation rows, tail rows, chunk sums: 40 KB per
            # 4-wave workgroup) still fits four workgroups per CU: 4 waves per SIMD
            dw = W.DeviceWorld(b.desc)
            li = dw.launch_info(p)
            dw.close()
            assert li["blocks_per_cu"] == 4 and li["waves"] == 4, li


@pytest.mark.parametrize("trav", ["lane", "auto"])
def test_lane_walk_on_a_deep_sphere_world(rtw, W, trav):
    """a 12k-sphere world whose unconstrained SAH tree is 24
    deep (helpers.deep_cluster_world; the 16-entry per-lane stack could not
    hold it, and the walk used to fall back to the union silently): the world
    is built with its depth capped at 16 (tests/test_world_cpu.py checks the
    build), the per-lane walk runs — forced, and chosen by AUTO — as
    rtw_world_launch_info and the walk's own iteration counts report, and the
    image equals the linear loop's bit for bit."""
    from helpers import deep_cluster_world
    prims, mats, tex = deep_cluster_world(W)
    d, keep = _to_desc(W, prims, [], tex, mats, [], [])
    b = type("B", (), {"desc": d})()
    cam = rtw.camera_init((0, 40, 90), (0, 0, 0), (0, 1, 0), 40.0, 16 / 9, 0.0, 10.0, 0.0, 1.0)
    p = rtw.make_params(320, 180, 4, 50, 42, background=(0.7, 0.8, 1.0), world_traversal=trav)
    dw = W.DeviceWorld(d)
    info, li = dw.bvh_info(), dw.launch_info(p)
    dw.close()
    assert info["nodes"] >= 10000 and info["max_depth"] <= 16 and info["max_leaf"] == 1, info
    assert li["traversal"] == "lane" and li["blocks_per_cu"] == 4, li
    rb, mb, cb, _ = _render_dev(rtw, W, b, cam, p, linear=False)
    rl, ml, cl, _ = _render_dev(rtw, W, b, cam, p, linear=True)
    print("deep world", info, li, "visits per lane-segment", cb["node_visits"] / cb["segments"])
    assert cb["traversal"] == "lane" and cb["lane_interior_iters"] > 0
    assert (rb == rl).all() and np.array_equal(mb.view(np.uint32), ml.view(np.uint32)), diff_stats(rb, rl)
    assert cb["samples"] == cl["samples"] == 320 * 180 * 4 and cb["segments"] == cl["segments"]
    assert rb.std() > 5


@pytest.mark.parametrize("scene,w,spp", [(7, 160, 2), (3, 96, 2), (6, 64, 4)])
def test_world_register_budgets_agree(rtw, W, earth, scene, w, spp, monkeypatch):
    # the kernel is instantiated per waves-per-SIMD target (1/3/4); the
    # register budget changes scheduling and spills, never results
    b = built(W, scene, earth)
    cam = b.camera()
    h = rtw.image_height(w, b.settings.aspect)
    p = params(rtw, b, w, h, spp)
    # and per feature set (params.world_features "all": the general kernel
    # instead of the one compiled for this world's features)
    outs = []
    for occ in (1, 3, 4):
        for feat in (0, 1):
            p.world_waves, p.world_features = occ, feat
            rgb, mean, _, _ = _render_dev(rtw, W, b, cam, p, linear=False)
            outs.append((rgb, mean))
    for rgb, mean in outs[1:]:
        assert (rgb == outs[0][0]).all() and np.array_equal(mean.view(np.uint32), outs[0][1].view(np.uint32))


def test_world_rings_in_caller_workspace(rtw, W, earth):
    """The tail dealing's per-lane rings live in the caller's workspace
    (rtw_world_workspace_bytes; ADVICE r3: they were one allocation per world,
    shared by every launch): two renders of ONE world issued on two streams,
    each with its own workspace, are independent and bit-identical; a
    workspace of only rtw_workspace_bytes(params) renders without tail
    dealing, the same image."""
    import torch
    b = built(W, 6, earth)
    cam = b.camera()
    p = params(rtw, b, 200, 200, 32)
    dw = W.DeviceWorld(b.desc)
    full, base = dw.workspace_bytes(p), rtw.workspace_bytes(p)
    assert full > base + 64 * 32 * 24  # at least one wave's rings
    outs = []
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    wss = [torch.empty(full + 256, dtype=torch.uint8, device="cuda:0") for _ in streams]
    rgbs = [torch.empty((p.row_count, p.width, 3), dtype=torch.uint8, device="cuda:0") for _ in streams]
    torch.cuda.synchronize()
    for rep in range(3):  # back to back on both streams: the launches overlap
        for s, ws, rgb in zip(streams, wss, rgbs):
            ptr = (ws.data_ptr() + 255) & ~255
            dw.render_async(cam, p, ptr, full, rgb.data_ptr(), None, s.cuda_stream)
    torch.cuda.synchronize()
    outs += [r.cpu().numpy() for r in rgbs]
    ws = torch.empty(base + 256, dtype=torch.uint8, device="cuda:0")
    ptr = (ws.data_ptr() + 255) & ~255
    dw.render_async(cam, p, ptr, base, rgbs[0].data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    outs.append(rgbs[0].cpu().numpy())
    dw.close()
    ref = W.render_world(cam, b.desc, p)
    for o in outs:
        assert (o == ref).all(), diff_stats(o, ref)


def test_small_worlds_run_linear(rtw, W, earth):
    for scene in (2, 3, 4, 5, 6):
        b = built(W, scene, earth)  # keep the built scene alive: desc points into it
        dw = W.DeviceWorld(b.desc)
        assert dw.bvh_info()["nodes"] == 0, scene
        dw.close()


def custom_world(W, earth):
    """Every primitive, wrapper, material and texture: a rotated+translated
    box and rect, a moving sphere inside a RotateY, an image-textured sphere
    and rect, Perlin noise, a light, metal, glass (hollow), checker ground."""
    import ctypes as C
    rng_world = W.BuiltScene(3, 7)  # borrow a Perlin table from scene 3
    perlin = rng_world.desc.perlins[0]
    tex = [dict(kind=W.TEX_CHECKER, odd=(0.2, 0.3, 0.1), even=(0.9, 0.9, 0.9)),
           dict(kind=W.TEX_NOISE, perlin=0, scale=4.0),
           dict(kind=W.TEX_IMAGE, image=0),
           dict(kind=W.TEX_SOLID, color=(6, 5, 4)),
           dict(kind=W.TEX_SOLID, color=(0.7, 0.3, 0.2))]
    mats = [dict(kind=W.WMAT_LAMBERT, tex=0), dict(kind=W.WMAT_LAMBERT, tex=1), dict(kind=W.WMAT_LAMBERT, tex=2),
            dict(kind=W.WMAT_LIGHT, tex=3), dict(kind=W.WMAT_METAL, albedo=(0.8, 0.8, 0.9), fuzz=0.1),
            dict(kind=W.WMAT_DIELECTRIC, ir=1.5), dict(kind=W.WMAT_LAMBERT, tex=4)]
    xf = [dict(n=2, op=[W.XF_TRANSLATE, W.XF_ROTATE_Y], v=[(1.5, 0, -1), (np.sin(0.4), np.cos(0.4), 0.4)]),
          dict(n=1, op=[W.XF_ROTATE_Y], v=[(np.sin(-0.7), np.cos(-0.7), -0.7)]),
          dict(n=2, op=[W.XF_ROTATE_Y, W.XF_TRANSLATE], v=[(np.sin(1.1), np.cos(1.1), 1.1), (-2, 0.5, 1)])]
    S, M, XY, XZ, YZ = W.PRIM_SPHERE, W.PRIM_MOVING_SPHERE, W.PRIM_XY_RECT, W.PRIM_XZ_RECT, W.PRIM_YZ_RECT
    prims = [dict(kind=S, mat=0, xform=-1, a=[0, -1000, 0, 0, -1000, 0, 1000, 0, 0]),
             dict(kind=S, mat=1, xform=-1, a=[0, 1, 0, 0, 1, 0, 1.0, 0, 0]),
             dict(kind=S, mat=2, xform=-1, a=[-2.2, 1, 0.5, -2.2, 1, 0.5, 1.0, 0, 0]),
             dict(kind=S, mat=5, xform=-1, a=[2.2, 0.8, 1.2, 2.2, 0.8, 1.2, 0.8, 0, 0]),
             dict(kind=S, mat=5, xform=-1, a=[2.2, 0.8, 1.2, 2.2, 0.8, 1.2, -0.7, 0, 0]),
             dict(kind=M, mat=4, xform=1, a=[0.5, 0.3, 2.5, 0.5, 0.6, 2.5, 0.3, 0.0, 1.0]),
             dict(kind=XZ, mat=3, xform=-1, a=[-1, 1, -1, 1, 4.0]),
             dict(kind=XY, mat=2, xform=2, a=[-1, 1, 0, 1.5, -2.0])]
    box = [(XY, [0, 1, 0, 1, 1]), (XY, [0, 1, 0, 1, 0]), (XZ, [0, 1, 0, 1, 1]), (XZ, [0, 1, 0, 1, 0]),
           (YZ, [0, 1, 0, 1, 1]), (YZ, [0, 1, 0, 1, 0])]
    prims += [dict(kind=k, mat=6, xform=0, a=a) for k, a in box]
    pv = {"ranvec": [list(perlin.ranvec[k]) for k in range(256)], "perm": [list(perlin.perm[a]) for a in range(3)]}
    return prims, xf, tex, mats, [pv], [earth]


@pytest.mark.parametrize("bg", [(0.7, 0.8, 1.0), (0.0, 0.0, 0.0)])
def test_world_custom_every_feature(rtw, oracle, W, earth, bg):
    prims, xf, tex, mats, perl, imgs = custom_world(W, earth)
    d, keep = _to_desc(W, prims, xf, tex, mats, perl, imgs)
    cam = rtw.camera_init((7, 3, 6), (0, 1, 0), (0, 1, 0), 35.0, 16 / 9, 0.05, 8.0, 0.0, 1.0)
    p = rtw.make_params(128, 72, 8, 50, 42, background=bg, chunk=3)
    g = W.render_world(cam, d, p)
    o = oracle.TableWorld(prims, xf, tex, mats, perl, imgs, background=bg)
    oc = oracle.Camera()
    for n in ("origin", "horizontal", "vertical", "lower_left_corner", "u", "v", "w"):
        getattr(oc, n)[:] = list(getattr(cam, n))
    oc.lens_radius, oc.time0, oc.time1 = cam.lens_radius, cam.time0, cam.time1
    ref, _ = o.render_tier_b(oc, 128, 72, 8, chunk=3, bg=bg)
    assert_parity(g, ref, f"custom world bg {bg}")
    assert g.std() > 5  # not a blank frame


def _write_png(path, rgba):
    import struct
    import zlib
    h, w, _ = rgba.shape
    raw = b"".join(b"\x00" + rgba[y].tobytes() for y in range(h))

    def chunk(t, body):
        return struct.pack(">I", len(body)) + t + body + struct.pack(">I", zlib.crc32(t + body))
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


def _read_ppm(path):
    data = open(path, "rb").read()
    parts = data.split(b"\n", 3)
    w, h = map(int, parts[1].split())
    return np.frombuffer(parts[3], np.uint8).reshape(h, w, 3)


@pytest.mark.parametrize("scene", [6, 4])
def test_cli_renders_reference_scenes(rtw, oracle, W, earth, scene, tmp_path):
    """bin/rtw_render (the reference's main() with the GPU loop): scene 6 is
    the reference's default; scene 4 reads its earth texture from a PNG
    through the CLI's own decoder.  Output equals oracle Tier B."""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(W.__file__), "..", "bin", "rtw_render")
    out = str(tmp_path / "out.ppm")
    args = [exe, "--scene", str(scene), "--width", "64", "--spp", "4", "--out", out]
    if scene == 4:
        png = str(tmp_path / "earth.png")
        _write_png(png, earth)
        args += ["--image", png]
    p = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    g = _read_ppm(out)
    o = oracle.OracleWorld(scene, 42, image=earth if scene == 4 else None)
    ref, _ = o.render_tier_b(o.camera(), g.shape[1], g.shape[0], 4)
    assert_parity(g, ref, f"cli scene {scene}")
