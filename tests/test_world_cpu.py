"""General worlds on the CPU: the product's scene builders (C++ host mirror of
main.zig:123-290) against the oracle's (rtw_world.c); the Tier-B libm
(product csrc/rtw_libm.hpp vs oracle ro_libm.h, bit for bit, and vs glibc);
Lemire intRangeLessThan and Perlin noise against independent Python
restatements; the PNG decoder; the world C-ABI validation (no GPU needed);
and Tier C consistency of the oracle's forward emission (Tier B) with the
reference's recursive rayColor (Tier A) on the emissive scenes."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

REF_PNG_DIGEST = os.path.join(REPO, "tests", "golden", "sekaichizu_png.json")


@pytest.fixture(scope="module")
def W():
    from rtw_amd import world
    return world


@pytest.fixture(scope="module")
def earth(W):
    return W.earth_map()


def resolved(t):
    """Materials with their textures (and perlins) inlined: the oracle shares
    one texture between materials where the Zig code copies a Texture value,
    the host emits one per material."""
    out = []
    for m in t["materials"]:
        d = {"kind": m["kind"]}
        if m["kind"] in (0, 3):
            tx = dict(t["textures"][m["tex"]])
            if tx["kind"] == 2:
                tx["perlin"] = t["perlins"][tx["perlin"]]
            d["tex"] = tx
        else:
            d.update(albedo=m["albedo"], fuzz=m["fuzz"], ir=m["ir"])
        out.append(d)
    return out


@pytest.mark.parametrize("scene", [1, 2, 3, 4, 5, 6, 7])
def test_scene_builders_equal_oracle(W, oracle, earth, scene):
    img = earth if scene in (4, 7) else None
    b = W.BuiltScene(scene, 42, image=img)
    o = oracle.OracleWorld(scene, 42, image=img)
    tb, to = b.table(), o.table()
    assert len(tb["prims"]) == len(to["prims"])
    for pb, po in zip(tb["prims"], to["prims"]):
        assert (pb["kind"], pb["xform"], pb["a"]) == (po["kind"], po["xform"], po["a"])
    assert tb["xforms"] == to["xforms"]
    rb, ro = resolved(tb), resolved(to)
    for pb, po in zip(tb["prims"], to["prims"]):
        assert rb[pb["mat"]] == ro[po["mat"]]
    assert b.rng_state == o.rng.state()  # the render continues the same stream
    s = b.settings
    st = to["settings"]
    assert list(s.look_from) == st["look_from"] and list(s.look_at) == st["look_at"]
    assert (s.vfov, s.aperture, s.aspect, s.width, s.height, s.spp) == \
        (st["vfov"], st["aperture"], st["aspect"], st["width"], st["height"], st["spp"])
    assert list(s.background) == st["background"]


def test_scene_sizes(W, earth):
    n = {i: W.BuiltScene(i, 42, image=earth if i in (4, 7) else None).desc.n_prims for i in range(1, 8)}
    assert n[1] == 40 and n[2] == 2 and n[3] == 2 and n[4] == 1 and n[5] == 3
    assert n[6] == 6 + 2 * 6  # five walls + light, two boxes of six rects
    assert 9900 <= n[7] <= 10002


def test_cornell_transforms(W):
    b = W.BuiltScene(6, 42)
    d = b.desc
    assert d.n_xforms == 2
    for i, (ang, off) in enumerate(((15.0, (265, 0, 295)), (-18.0, (130, 0, 65)))):
        x = d.xforms[i]
        assert x.n == 2 and list(x.op)[:2] == [W.XF_TRANSLATE, W.XF_ROTATE_Y]
        assert list(x.v[0]) == list(off)
        t = ang * math.pi / 180.0
        assert abs(x.v[1][0] - math.sin(t)) <= 1e-16 and abs(x.v[1][1] - math.cos(t)) <= 1e-16


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_tierb_libm_product_equals_oracle_and_glibc(tmp_path):
    exe = str(tmp_path / "libmchk")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-I", os.path.join(REPO, "oracle"), "-I",
                    os.path.join(REPO, "raytracinginoneweekend.zig_amd", "csrc"),
                    os.path.join(REPO, "tests", "native", "libm_check.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe, "1000000", "7"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "mismatch 0" in p.stdout


def _lemire(next_u64, at_least, less_than):
    """Zig 0.14 std.Random.uintLessThan (Lemire + pcg tweak), restated in Python."""
    lt = less_than - at_least
    m = next_u64() * lt
    lo = m & (2**64 - 1)
    if lo < lt:
        t = (2**64 - lt) % 2**64
        if t >= lt:
            t -= lt
            if t >= lt:
                t %= lt
        while lo < t:
            m = next_u64() * lt
            lo = m & (2**64 - 1)
    return at_least + (m >> 64)


def test_int_range_less_than_matches_python_restatement(oracle):
    oracle._world_lib()
    a, b = oracle.ZigRandom(42), oracle.ZigRandom(42)
    for bound in list(range(1, 300)) + [2**32 + 7, 2**63 + 5, 2**64 - 1]:
        x = oracle.lib().rw_int_range_less_than_u64(a.s, 0, bound)
        y = _lemire(b.next, 0, bound)
        assert x == y < bound
    assert a.state() == b.state()


def _perlin_py(pv, pt):
    """perlin.zig:49-124 restated in Python (independent of rtw_world.c)."""
    u, v, w = (c - math.floor(c) for c in pt)
    uu, vv, ww = (x * x * (3 - 2 * x) for x in (u, v, w))
    i, j, k = (int(math.floor(c)) for c in pt)
    acc = 0.0
    for di in range(2):
        for dj in range(2):
            for dk in range(2):
                c = pv["ranvec"][pv["perm"][0][(i + di) & 255] ^ pv["perm"][1][(j + dj) & 255] ^
                                  pv["perm"][2][(k + dk) & 255]]
                wt = (uu - di, vv - dj, ww - dk)
                acc += (di * uu + (1.0 - di) * (1.0 - uu)) * (dj * vv + (1.0 - dj) * (1.0 - vv)) * \
                    (dk * ww + (1.0 - dk) * (1.0 - ww)) * (c[0] * wt[0] + c[1] * wt[1] + c[2] * wt[2])
    return acc


def test_perlin_noise_matches_python_restatement(oracle):
    o = oracle.OracleWorld(3, 42)
    pv = o.table()["perlins"][0]
    assert sorted(pv["perm"][0]) == list(range(256)) and pv["perm"][0] != list(range(256))
    L = oracle._world_lib()
    rng = np.random.default_rng(3)
    for pt in rng.uniform(-300, 300, size=(2000, 3)):
        a = L.rw_perlin_noise(C.byref(o.w.perlins[0]), (C.c_double * 3)(*pt))
        assert a == _perlin_py(pv, pt)
        assert -1.5 < a < 1.5
    t = L.rw_perlin_turb(C.byref(o.w.perlins[0]), (C.c_double * 3)(1.5, -2.25, 3.0), 7)
    ref, wgt, q = 0.0, 1.0, [1.5, -2.25, 3.0]
    for _ in range(7):
        ref += wgt * _perlin_py(pv, q)
        wgt *= 0.5
        q = [c * 2.0 for c in q]
    assert t == abs(ref)


def test_load_png_reference_asset(W):
    img = W.earth_map()
    assert img.shape == (282, 500, 4) and img.dtype == np.uint8
    a = img[..., 3]
    assert (a == 0).any() and (a == 255).any()  # ocean (alpha 0) and land


def test_committed_asset_is_the_reference_file(W):
    """Byte for byte: the length and SHA-256 recorded from the reference's
    assets/sekaichizu.png (tests/golden/sekaichizu_png.json)."""
    import hashlib
    import json
    want = json.load(open(REF_PNG_DIGEST))
    data = open(W.EARTH_PNG, "rb").read()
    assert len(data) == want["bytes"] and hashlib.sha256(data).hexdigest() == want["sha256"]


def test_load_png_roundtrip(W, tmp_path):
    """Encode an RGBA image with all five scanline filters and decode it."""
    import struct
    import zlib
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, size=(9, 13, 4), dtype=np.uint8)
    raw = bytearray()
    prev = np.zeros(13 * 4, np.int32)
    for y in range(9):
        f = y % 5
        line = img[y].reshape(-1).astype(np.int32)
        enc = np.zeros_like(line)
        for x in range(len(line)):
            a = line[x - 4] if x >= 4 else 0
            b = prev[x]
            c = prev[x - 4] if x >= 4 else 0
            pred = [0, a, b, (a + b) >> 1, None][f]
            if f == 4:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            enc[x] = (line[x] - pred) & 255
        raw += bytes([f]) + enc.astype(np.uint8).tobytes()
        prev = line

    def chunk(t, body):
        return struct.pack(">I", len(body)) + t + body + struct.pack(">I", zlib.crc32(t + body))
    png = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", 13, 9, 8, 6, 0, 0, 0)) + \
        chunk(b"IDAT", zlib.compress(bytes(raw))) + chunk(b"IEND", b"")
    p = tmp_path / "t.png"
    p.write_bytes(png)
    assert (W.load_png(str(p)) == img).all()


def test_synthetic_world_map(W):
    m = W.synthetic_world_map()
    assert m.shape == (282, 500, 4) and m.dtype == np.uint8
    assert 0.2 < (m[..., 3] == 255).mean() < 0.8 and set(np.unique(m[..., 3])) == {0, 255}
    assert (W.synthetic_world_map() == m).all()


def test_world_create_validates_before_the_gpu(W, rtw):
    b = W.BuiltScene(6, 42)
    d = W.WorldDesc()
    C.memmove(C.byref(d), C.byref(b.desc), C.sizeof(d))
    prims = (W.Prim * d.n_prims)()
    C.memmove(prims, d.prims, C.sizeof(prims))
    prims[3].mat = 99
    d.prims = C.cast(prims, C.POINTER(W.Prim))
    with pytest.raises(rtw.RtwError) as e:
        W.DeviceWorld(d)
    assert e.value.status == rtw.RTW_EINVAL
    prims[3].mat = 0
    prims[3].xform = 7
    with pytest.raises(rtw.RtwError):
        W.DeviceWorld(d)


def test_world_create_rejects_empty_shutter(W, rtw):
    """A moving sphere with time1 <= time0 (NaN centre, hittable.zig:219-221)
    is refused: its box could not bound it, so BVH and linear would differ."""
    b = W.BuiltScene(1, 42)
    d = W.WorldDesc()
    C.memmove(C.byref(d), C.byref(b.desc), C.sizeof(d))
    prims = (W.Prim * d.n_prims)()
    C.memmove(prims, d.prims, C.sizeof(prims))
    k = next(i for i in range(d.n_prims) if prims[i].kind == W.PRIM_MOVING_SPHERE)
    d.prims = C.cast(prims, C.POINTER(W.Prim))
    for t0, t1 in ((0.5, 0.5), (1.0, 0.0)):
        prims[k].a[7], prims[k].a[8] = t0, t1
        with pytest.raises(rtw.RtwError) as e:
            W.DeviceWorld(d)
        assert e.value.status == rtw.RTW_EINVAL and "time1 > time0" in str(e.value)


def test_build_scene_rejects(W, rtw):
    with pytest.raises(rtw.RtwError):
        W.BuiltScene(9, 42)
    with pytest.raises(rtw.RtwError):
        W.BuiltScene(4, 42)  # earth needs its image


def test_world_oracle_scene1_equals_cover_oracle(oracle):
    """The general-world oracle reproduces the cover-scene oracle bit for bit
    (Tier A and Tier B) on scene 1."""
    sc, rng = oracle.cover_scene(42)
    cam = oracle.cover_camera(16 / 9)
    a, _, _ = oracle.render_tier_a(sc, cam, rng, 40, 22, 3)
    w = oracle.OracleWorld(1, 42)
    b, _ = w.render_tier_a(cam, 40, 22, 3)
    assert (a == b).all()
    tb, _ = oracle.render_tier_b(sc, cam, 48, 27, 5, chunk=2)
    wb, _ = w.render_tier_b(cam, 48, 27, 5, chunk=2)
    assert (tb == wb).all()


@pytest.mark.parametrize("scene", [5, 6])
def test_tier_c_emissive_forward_vs_recursive(oracle, scene):
    """Tier B evaluates rayColor forward (rad += T * emitted); Tier A is the
    reference's recursion.  Same scene, same spp: Tier A's image mean lies
    within the seed-to-seed spread of Tier B's (8 seeds; z <= 4 against the
    spread, which is ~0.45 LSB for scene 5's dim, light-lit image at 24 spp —
    one seed pair is too noisy an estimate of it)."""
    w = oracle.OracleWorld(scene, 42)
    W_, H_ = (48, 32) if scene == 5 else (40, 40)
    cam = w.camera()
    spp = 24
    a, _ = w.render_tier_a(cam, W_, H_, spp)
    mb = np.array([w.render_tier_b(cam, W_, H_, spp, seed=sd)[0].astype(float).mean((0, 1))
                   for sd in (42, 777, 1, 2, 3, 4, 5, 6)])
    sd_b = mb.std(0, ddof=1)
    z = np.abs(a.astype(float).mean((0, 1)) - mb.mean(0)) / (sd_b * np.sqrt(1 + 1 / len(mb)))
    assert z.max() <= 4.0, (z, mb.mean(0), sd_b)


def test_cornell_oracle_geometry(oracle):
    """Ray sanity on the Cornell box (hittable.zig rect/box/rotate/translate):
    a ray above both boxes meets the back wall (z = 555) from behind its +z
    normal (front_face false, normal flipped); the camera's centre ray is
    stopped by the tall box's rotated front face; a vertical ray down inside
    the tall box's footprint hits its top (y = 330) with an upward normal."""
    w = oracle.OracleWorld(6, 42)
    h = w.hit((100, 450, -800), (0, 0, 1))
    assert h is not None and abs(h["p"][2] - 555) < 1e-9 and h["normal"] == [0.0, 0.0, -1.0] and not h["front"]
    h = w.hit((278, 278, -800), (0, 0, 1))
    assert h is not None and 250 < h["p"][2] < 330 and abs(h["normal"][2]) > 0.9
    # tall box: Translate(265, 0, 295) of RotateY(15 deg) of [0,165]x[0,330]x[0,165]
    t = 15 * math.pi / 180
    cx, cz = 82.5, 82.5
    wx = math.cos(t) * cx + math.sin(t) * cz + 265
    wz = -math.sin(t) * cx + math.cos(t) * cz + 295
    h = w.hit((wx, 500, wz), (0, -1, 0))
    assert h is not None and abs(h["p"][1] - 330) < 1e-9 and abs(h["normal"][1] - 1) < 1e-12


def test_globe_bvh_isolates_the_ground_at_the_root():
    """configs[4]: the binned SAH puts the r=1000 ground sphere (box 2000 wide)
    in a leaf of its own at the root and the globe + 10k spheres in the other
    child (box ~100 x 4 x 100): the oversized primitive is already hoisted out
    of the traversal (one test per segment), the rest never descends under a
    scene-sized box.  (The builder runs before the device is needed.)"""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from rtw_amd import world as W\n"
            "b = W.BuiltScene(7, 42, image=W.earth_map())\n"
            "try:\n    W.DeviceWorld(b.desc, debug_bvh=True).close()\nexcept Exception:\n    pass\n") % os.path.join(REPO, "raytracinginoneweekend.zig_amd")
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    lines = [l for l in p.stderr.splitlines() if l.startswith("[rtw bvh] root child")]
    assert len(lines) == 2, p.stderr
    assert "leaf of 1, box x [-1000, 1000] y [-2000, 0] z [-1000, 1000]" in lines[0]
    assert "node" in lines[1] and "y [0, 4]" in lines[1]
    # the per-lane walk's refs packed into the lower bounds (rtw_world_capi.hip pack_refs): the
    # device's byte gather restated on the host recovers every ref, and no bound moved up
    # the globe's SAH tree fits the per-lane walk's stack as built (no depth-capped rebuild)
    dl = [l for l in p.stderr.splitlines() if l.startswith("[rtw bvh]") and "depth" in l]
    assert len(dl) == 1 and re.search(r"depth (\d+) \(unconstrained SAH: \1\)", dl[0]), dl
    packed = [l for l in p.stderr.splitlines() if l.startswith("[rtw bvh] packed refs:")]
    assert len(packed) == 1, p.stderr
    m = re.match(r"\[rtw bvh\] packed refs: (\d+) nodes, (\d+) mismatches, bounds moved down by <= (\d+) ulps", packed[0])
    assert m and int(m.group(1)) > 5000 and int(m.group(2)) == 0 and int(m.group(3)) < 512, packed[0]


def test_deep_sphere_world_bvh_capped_for_the_lane_walk():
    """the per-lane walk keeps its stack in 16 LDS entries per
    lane.  A >= 10k-sphere world whose binned-SAH tree is deeper than that
    (helpers.deep_cluster_world: depth 24) is rebuilt by rtw_world_create with
    SAH splits only while a median subtree still fits (rtw_world_capi.hip
    Builder depth_cap): depth <= 16, leaves of one, refs packed — the lane walk
    stays available (the GPU test renders it against the linear loop).  The
    globe's own SAH tree (depth 16) is kept as built (the globe test above)."""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from rtw_amd import world as W\n"
            "from helpers import deep_cluster_world\n"
            "from test_gpu_world import _to_desc\n"
            "prims, mats, tex = deep_cluster_world(W)\n"
            "d, keep = _to_desc(W, prims, [], tex, mats, [], [])\n"
            "try:\n    W.DeviceWorld(d, debug_bvh=True).close()\nexcept Exception:\n    pass\n") % (
        os.path.join(REPO, "raytracinginoneweekend.zig_amd"), os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    line = [l for l in p.stderr.splitlines() if l.startswith("[rtw bvh]") and "depth" in l]
    assert len(line) == 1, p.stderr
    m = re.match(r"\[rtw bvh\] (\d+) nodes, depth (\d+) \(unconstrained SAH: (\d+)\), max leaf (\d+)", line[0])
    assert m, line[0]
    nodes, depth, free_depth, leaf = (int(m.group(i)) for i in range(1, 5))
    assert nodes >= 10000 and free_depth > 16 and depth <= 16 and leaf == 1, line[0]
    packed = [l for l in p.stderr.splitlines() if l.startswith("[rtw bvh] packed refs:")]
    assert len(packed) == 1 and " 0 mismatches" in packed[0], p.stderr
