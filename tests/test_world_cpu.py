"""General worlds on the CPU: the product's scene builders (C++ host mirror of
main.zig:123-290) against the oracle's (rtw_world.c); the Tier-B libm
(product csrc/rtw_libm.hpp vs oracle ro_libm.h, bit for bit, and vs glibc);
Lemire intRangeLessThan and Perlin noise against independent Python
restatements; the PNG decoder; the world C-ABI validation (no GPU needed);
Tier C consistency of the oracle's forward emission (Tier B) with the
reference's recursive rayColor (Tier A) on the emissive scenes; and the
inputs of tests/test_gpu_world_general.py on the oracle alone — every class of
helpers.mixed_bvh_world is visible, the later of two coincident primitives is
the one seen, the BVHs have the leaf sizes those tests mean to walk — with
prim_box (csrc/rtw_world_box.hpp) against a long double restatement."""
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
    # the generator moved into libm_inputs.hpp (shared with the device check): no case was lost
    # (4,003,684 before the move), and the sphere-UV edges came on top
    assert int(re.search(r"cases (\d+)", p.stdout).group(1)) > 4003684


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
    # the per-lane walk's refs packed into the lower bounds (rtw_world_pack.cpp pack_refs): the
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
    SAH splits only while a median subtree still fits (rtw_world_pack.cpp
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


# ------------------------------------------------------------------------
# The mixed BVH worlds of tests/test_gpu_world_general.py, on the oracle alone
# (helpers.mixed_bvh_world): conditions on the INPUTS of the GPU tests, so that
# those cannot pass vacuously, and prim_box against an independent restatement.
def _mixed_oracle_camera(oracle, aspect=16 / 9, time0=0.0, time1=1.0):
    from helpers import MIXED_CAMERA as m
    cam = oracle.Camera()
    arr = C.c_double * 3
    oracle.lib().ro_camera_init(C.byref(cam), arr(*m["look_from"]), arr(*m["look_at"]), arr(0, 1, 0), m["vfov"],
                                aspect, m["aperture"], m["focus"], time0, time1)
    return cam


MIXED_BG = (0.7, 0.8, 1.0)
MIXED_SEED = 5  # the generator's seed in every test


@pytest.fixture(scope="module")
def mixed_renders(W, oracle, earth):
    """Oracle Tier B at 96x54x4 of the full mixed world, per size and pair order; rendered once."""
    from helpers import MIXED_SIZES, mixed_bvh_world
    cache = {}

    def get(size, swap=False, drop=()):
        key = (size, swap, tuple(drop))
        if key not in cache:
            t = mixed_bvh_world(W, earth, *MIXED_SIZES[size], MIXED_SEED, swap=swap, drop=drop)
            o = oracle.TableWorld(*t, background=MIXED_BG)
            cache[key] = (o.render_tier_b(_mixed_oracle_camera(oracle), 96, 54, 4, bg=MIXED_BG, threads=8)[0], t, o)
        return cache[key]
    return get


@pytest.mark.parametrize("size", ["small", "large"])
def test_mixed_world_every_class_is_visible(mixed_renders, size):
    """Removing any one class of the mixed world — free rects, transformed
    boxes, moving spheres with their own time range, the hollow sphere's
    negative inside, each coincident pair — changes >= 2 % of the pixels of the
    oracle's 96x54x4 frame (a condition on the generator's layout and camera,
    not a measurement: observed 4-22 %).  Tier B draws per-sample streams, so
    a pixel no path of which meets the class is unchanged."""
    from helpers import MIXED_CLASSES
    full, t, _ = mixed_renders(size)
    n = len(t[0])
    assert n >= 512 if size == "large" else 100 <= n <= 140, n
    assert full.std() > 5
    for cls in MIXED_CLASSES:
        assert any(p["cls"] == cls for p in t[0]), cls
        img, td, _ = mixed_renders(size, drop=(cls,))
        assert len(td[0]) < n
        frac = float((img != full).any(axis=2).mean())
        print(size, cls, "removed:", n - len(td[0]), "primitives, changed pixels", frac)
        assert frac >= 0.02, (size, cls, frac)


def test_mixed_world_contents(W, earth):
    """What the generator promises (helpers.mixed_bvh_world): chains of every
    length 1..4 in both op orders, one with near-cancelling translations of
    magnitude >= 1e3, boxes of six consecutive rects, every primitive kind,
    material and texture, and the pair members far apart in the list."""
    from helpers import MIXED_SIZES, PAIR_COLOURS, mixed_bvh_world
    for size in ("small", "large"):
        prims, xf, tex, mats, perl, imgs = mixed_bvh_world(W, earth, *MIXED_SIZES[size], MIXED_SEED)
        assert prims == mixed_bvh_world(W, earth, *MIXED_SIZES[size], MIXED_SEED)[0]  # deterministic
        box_chains = {p["xform"] for p in prims if p["cls"] == "xf_box"}
        assert {xf[i]["n"] for i in box_chains} == {1, 2, 3, 4}
        firsts = {(xf[i]["op"][0], xf[i]["op"][1]) for i in box_chains if xf[i]["n"] >= 2}
        assert (W.XF_TRANSLATE, W.XF_ROTATE_Y) in firsts and (W.XF_ROTATE_Y, W.XF_TRANSLATE) in firsts
        big = [x for x in xf for k in range(x["n"] - 1) if x["op"][k] == x["op"][k + 1] == W.XF_TRANSLATE and
               min(abs(c) for c in x["v"][k]) >= 1e3 and max(abs(a + b) for a, b in zip(x["v"][k], x["v"][k + 1])) <= 1.0]
        assert big
        assert any(p["cls"] == "base" and p["kind"] >= W.PRIM_XY_RECT and p["xform"] < 0 for p in prims[2:])  # chainless boxes
        assert {p["kind"] for p in prims} == {0, 1, 2, 3, 4}
        assert {p["kind"] for p in prims if p["cls"] == "free_rect" and p["xform"] < 0} == {2, 3, 4}
        assert {p["kind"] for p in prims if p["cls"] == "free_rect" and p["xform"] >= 0} == {2, 3, 4}
        assert any(p["a"][6] < 0 for p in prims if p["kind"] == 0)
        assert sum(1 for p in prims if p["kind"] == 0 and abs(p["a"][6]) >= 100) == 2
        assert {(p["a"][7], p["a"][8]) for p in prims if p["kind"] == 1} == {(0.0, 1.0), (-0.5, 1.5), (0.25, 0.75)}
        assert any(p["kind"] == 0 and p["xform"] >= 0 and xf[p["xform"]]["op"] == [W.XF_ROTATE_Y, W.XF_TRANSLATE] for p in prims)
        used = {mats[p["mat"]]["kind"] for p in prims}
        assert used == {W.WMAT_LAMBERT, W.WMAT_METAL, W.WMAT_DIELECTRIC, W.WMAT_LIGHT}
        assert {tex[mats[p["mat"]]["tex"]]["kind"] for p in prims if mats[p["mat"]]["kind"] == W.WMAT_LAMBERT} == {0, 1, 2, 3}
        assert {mats[p["mat"]]["fuzz"] > 0 for p in prims if mats[p["mat"]]["kind"] == W.WMAT_METAL} == {False, True}
        for name in PAIR_COLOURS:
            idx = [i for i, p in enumerate(prims) if p["cls"] == name and mats[p["mat"]]["kind"] == W.WMAT_LIGHT]
            assert len(idx) == 2 and idx[0] < 8 and idx[1] >= len(prims) - 8, (name, idx)
            a, b = prims[idx[0]], prims[idx[1]]
            assert (a["kind"], a["xform"], a["a"]) == (b["kind"], b["xform"], b["a"])  # identical geometry
        # boxes: six consecutive rects sharing one chain
        rects = [i for i, p in enumerate(prims) if p["cls"] == "xf_box"]
        assert len(rects) % 6 == 0 and all(prims[rects[k]]["xform"] == prims[rects[k - k % 6]]["xform"] and
                                           rects[k] == rects[k - k % 6] + k % 6 for k in range(len(rects)))


def test_mixed_world_bvh_shapes():
    """The BVHs rtw_world_create builds for the mixed worlds (the builder runs
    before the device is needed): ~120 primitives get leaves of up to 2; the
    >= 512 world gets leaves of 1, and its unconstrained SAH tree is deeper
    than the per-lane stack (17 > 16), so the depth-capped rebuild runs on a
    world that is not spheres only; every ref packs."""
    import sys
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from rtw_amd import world as W\n"
            "from helpers import MIXED_SIZES, _to_desc, mixed_bvh_world\n"
            "for size in ('small', 'large'):\n"
            "    d, keep = _to_desc(W, *mixed_bvh_world(W, W.earth_map(), *MIXED_SIZES[size], %d))\n"
            "    try:\n        W.DeviceWorld(d, debug_bvh=True).close()\n    except Exception:\n        pass\n") % (
        os.path.join(REPO, "raytracinginoneweekend.zig_amd"), os.path.dirname(os.path.abspath(__file__)), MIXED_SEED)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    lines = [l for l in p.stderr.splitlines() if l.startswith("[rtw bvh]") and "depth" in l]
    assert len(lines) == 2, p.stderr
    shape = [tuple(int(x) for x in re.match(
        r"\[rtw bvh\] (\d+) nodes, depth (\d+) \(unconstrained SAH: (\d+)\), max leaf (\d+)", l).groups()) for l in lines]
    (n_s, d_s, f_s, leaf_s), (n_l, d_l, f_l, leaf_l) = shape
    assert leaf_s == 2 and d_s == f_s <= 16 and n_s > 50, lines[0]
    assert leaf_l == 1 and n_l >= 511 and f_l > 16 >= d_l, lines[1]
    packed = [l for l in p.stderr.splitlines() if l.startswith("[rtw bvh] packed refs:")]
    assert len(packed) == 2 and all(" 0 mismatches" in l for l in packed), p.stderr


def _light_byte(oracle, colour, spp=4):
    return [int(oracle.lib().ro_quantize(c * spp, 1.0 / spp)) for c in colour]


@pytest.mark.parametrize("size", ["small", "large"])
def test_mixed_world_tie_rule_later_index_wins(oracle, mixed_renders, size):
    """Coincident primitives (identical geometry, two lights of different
    colours, list indices far apart): on t == closest_so_far the reference's
    sequential HittableList.hit takes the LATER primitive.  In the oracle's
    frame the pixels that cover each pair show the later member's colour and
    none shows the earlier one's; with the pair order swapped, the reverse.
    A ray aimed at each pair reports the later list index."""
    from helpers import MIXED_CAMERA, PAIR_COLOURS, chain_to_world
    imgs = {sw: mixed_renders(size, swap=sw) for sw in (False, True)}
    assert (imgs[False][0] != imgs[True][0]).any()
    for name, (ca, cb) in PAIR_COLOURS.items():
        ba, bb = _light_byte(oracle, ca), _light_byte(oracle, cb)
        assert max(abs(x - y) for x, y in zip(ba, bb)) > 100  # clearly different colours
        for sw in (False, True):
            img, t, o = imgs[sw]
            later, earlier = (ba, bb) if sw else (bb, ba)
            n_later = int((img == np.array(later, np.uint8)).all(axis=2).sum())
            n_earlier = int((img == np.array(earlier, np.uint8)).all(axis=2).sum())
            print(size, name, "swap", sw, "pixels of the later / earlier colour:", n_later, n_earlier)
            assert n_later >= 30 and n_earlier == 0, (name, sw, n_later, n_earlier)
            other = imgs[not sw][0]
            mask = (img == np.array(later, np.uint8)).all(axis=2)
            # the same pixels show the other colour in the other order (edge pixels aside: a sample
            # beside the pair can hide under one colour's clamp and not under the other's)
            assert (other[mask] == np.array(earlier, np.uint8)).all(axis=1).mean() >= 0.9
            prims, xf = t[0], t[1]
            idx = [i for i, p in enumerate(prims) if p["cls"] == name and o.w.mats[p["mat"]].kind == 3]
            p = prims[idx[1]]
            a = p["a"]
            if p["kind"] == 0:
                target = np.array(a[:3]) + np.array([0.0, 0.0, abs(a[6])])
            else:
                target = np.array([(a[0] + a[1]) / 2, (a[2] + a[3]) / 2, a[4]])
            if p["xform"] >= 0:
                target = chain_to_world(xf[p["xform"]], target)
            org = np.array(MIXED_CAMERA["look_from"])
            h = o.hit(tuple(org), tuple(target - org))
            assert h is not None and h["prim"] == idx[1], (name, sw, h, idx)
            assert abs(h["t"] - 1.0) < 1e-9


def test_prim_box_is_conservative(tmp_path):
    """csrc/rtw_world_box.hpp prim_box (the BVH builder's input): 1e5 random
    primitives of every kind with chains of 0-4 ops — moving spheres with their
    own time ranges, one radius in ten negative — and 12 surface points each at
    shutter times in [0, 1], carried to world space in long double by a
    restatement of hittable.zig's forward transforms: every point lies inside
    its box within 1e-12 * (1 + max |coordinate|), and rects are covered by
    their +-1e-4 padding (tests/native/prim_box_check.cpp)."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "primboxchk")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(REPO, "include"), "-I",
                    os.path.join(REPO, "raytracinginoneweekend.zig_amd", "csrc"),
                    os.path.join(REPO, "tests", "native", "prim_box_check.cpp"), "-o", exe], check=True)
    for seed in (1, 2):
        p = subprocess.run([exe, "100000", str(seed)], capture_output=True, text=True)
        print(p.stdout)
        m = re.search(r"violations (\d+)/(\d+)", p.stdout)
        assert m and p.returncode == 0, p.stdout + p.stderr
        assert int(m.group(1)) == 0 and int(m.group(2)) == 1_200_000


def test_prim_box_check_has_teeth(tmp_path):
    """The same program against two broken copies of the header finds
    violations: prim_box ignoring the RotateY op, and without the rect padding."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    src = open(os.path.join(REPO, "raytracinginoneweekend.zig_amd", "csrc", "rtw_world_box.hpp")).read()
    rot = "      } else {\n        const double sn = xf->v[i][0]"
    pad_lo, pad_hi = "p.a[4] - 0.0001", "p.a[4] + 0.0001"
    assert src.count(rot) == 1 and src.count(pad_lo) == 1 and src.count(pad_hi) == 1
    broken = {"norot": src.replace(rot, rot.replace("} else {", "} else if (false) {")),
              "nopad": src.replace(pad_lo, "p.a[4]").replace(pad_hi, "p.a[4]")}
    for name, text in broken.items():
        d = tmp_path / name
        d.mkdir()
        (d / "rtw_world_box.hpp").write_text(text)
        exe = str(d / "chk")
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(REPO, "include"), "-I", str(d),
                        os.path.join(REPO, "tests", "native", "prim_box_check.cpp"), "-o", exe], check=True)
        p = subprocess.run([exe, "20000", "1"], capture_output=True, text=True)
        m = re.search(r"violations (\d+)/(\d+)", p.stdout)
        assert m and int(m.group(1)) > 0 and p.returncode == 1, (name, p.stdout)


# ------------------------------------------------------------------------
# The textured world of tests/test_gpu_world_textures.py (helpers.textured_world),
# on the oracle alone: every image and every Perlin table is visible at its own
# index, the portrait image's row clamp bites and the alpha-0 colour is seen.
def _textured_oracle_camera(oracle, aspect=16 / 9):
    from helpers import TEXTURED_CAMERA as m
    cam = oracle.Camera()
    arr = C.c_double * 3
    oracle.lib().ro_camera_init(C.byref(cam), arr(*m["look_from"]), arr(*m["look_at"]), arr(0, 1, 0), m["vfov"],
                                aspect, m["aperture"], m["focus"], 0.0, 1.0)
    return cam


@pytest.fixture(scope="module")
def textured_render(W, oracle, earth):
    """Oracle Tier B at 96x54x8 (the GPU tests' frame) of a textured world -> rgb."""
    from helpers import TEXTURED_BG, TEXTURED_PERLIN_SEEDS, perlin_table, textured_images, textured_world
    base_imgs = textured_images(earth)
    base_perl = [perlin_table(W, s) for s in TEXTURED_PERLIN_SEEDS]

    def get(images=None, perlins=None, **kw):
        t = textured_world(W, earth, images=images or base_imgs, perlins=perlins or base_perl, **kw)
        o = oracle.TableWorld(*t, background=TEXTURED_BG)
        return o.render_tier_b(_textured_oracle_camera(oracle), 96, 54, 8, bg=TEXTURED_BG, threads=8)[0], t
    return get, base_imgs, base_perl


def _changed(a, b):
    return float((a != b).any(axis=2).mean())


def test_textured_world_every_table_is_visible(textured_render):
    """Exchanging any two images, or any two Perlin tables, changes >= 1 % of
    the pixels of the oracle's 96x54x8 frame: a kernel that read table 0 for
    every index, or strode the tables wrongly, cannot pass the GPU tests."""
    get, imgs, perl = textured_render
    full, t = get()
    assert len(t[0]) <= 32 and full.std() > 5
    assert [x["image"] for x in t[2] if x["kind"] == 3] == [0, 1, 2, 3, 1, 3]
    assert [(x["perlin"], x["scale"]) for x in t[2] if x["kind"] == 2] == [(0, 4.0), (1, 0.0), (2, -2.5)]
    assert imgs[1].shape == (9, 5, 4) and imgs[3].shape == (3, 7, 4) and imgs[0].shape == (1, 1, 4) and imgs[2].shape[1] == 500
    for a in range(4):
        for b in range(a + 1, 4):
            sw = list(imgs)
            sw[a], sw[b] = sw[b], sw[a]
            frac = _changed(get(images=sw)[0], full)
            print("images", a, b, "exchanged: changed pixels", frac)
            assert frac >= 0.01, (a, b, frac)
    for a in range(3):
        for b in range(a + 1, 3):
            sw = list(perl)
            sw[a], sw[b] = sw[b], sw[a]
            frac = _changed(get(perlins=sw)[0], full)
            print("perlin tables", a, b, "exchanged: changed pixels", frac)
            assert frac >= 0.01, (a, b, frac)


def test_textured_world_row_clamp_and_alpha_zero_are_visible(textured_render):
    """The portrait image (5 wide, 9 high): the reference clamps the ROW against
    width - 1 (texture.zig:130), so row 4 is shown wherever rows 4-8 would be
    and rows 5-8 never — repainting row 4 changes the frame, repainting rows
    5-8 does not (a kernel clamping against height - 1 would show them).  The
    alpha-0 texels of the 7x3 image are shown as (0, 0, 1): their rgb never
    shows, their alpha does."""
    get, imgs, _ = textured_render
    full, _ = get()

    def with_image(k, edit):
        sw = [i.copy() for i in imgs]
        edit(sw[k])
        return get(images=sw)[0]

    def row4(im):
        im[4, :, :3] = 255 - im[4, :, :3]

    def hidden_rows(im):
        im[5:, :, :3] = 255 - im[5:, :, :3]

    frac = _changed(with_image(1, row4), full)
    print("portrait row 4 repainted: changed pixels", frac)
    assert frac >= 0.01
    assert _changed(with_image(1, hidden_rows), full) == 0.0
    a0 = imgs[3][..., 3] == 0
    assert 5 <= a0.sum() <= 10

    def alpha0_rgb(im):
        im[a0, :3] = (0, 255, 0)

    def alpha0_opaque(im):
        im[a0, 3] = 255

    assert _changed(with_image(3, alpha0_rgb), full) == 0.0
    frac = _changed(with_image(3, alpha0_opaque), full)
    print("alpha-0 texels made opaque: changed pixels", frac)
    assert frac >= 0.01
    # the emitting rect shows the colour itself: (0, 0, 1) -> bytes (0, 0, 255) in pixels no other colour reaches
    assert ((full[..., 0] == 0) & (full[..., 1] == 0) & (full[..., 2] == 255)).sum() >= 10


def test_textured_world_variants(W, earth):
    from helpers import textured_world
    n = {v: textured_world(W, earth, variant=v) for v in (None, "noise", "image")}
    assert all(len(t[0]) <= 32 for t in n.values())
    assert not n["noise"][5] and len(n["noise"][4]) == 3 and max(x.get("perlin", 0) for x in n["noise"][2]) == 2
    assert not n["image"][4] and len(n["image"][5]) == 4 and max(x.get("image", 0) for x in n["image"][2]) == 3
    assert any(p["xform"] >= 0 and n[v][3][p["mat"]]["kind"] == W.WMAT_LAMBERT for v in n for p in n[v][0])
    big = textured_world(W, earth, filler=40)
    assert len(big[0]) > 32 and big[0][:len(n[None][0])] == n[None][0]
    # spheres only, no chains, every image (and both emitting ones): the world kernel's image-only feature set
    sp = textured_world(W, earth, variant="image_spheres", filler=40)
    assert all(p["kind"] == W.PRIM_SPHERE and p["xform"] < 0 for p in sp[0]) and not sp[1] and not sp[4]
    img = [(sp[3][p["mat"]]["kind"], sp[2][sp[3][p["mat"]]["tex"]]["image"]) for p in sp[0]
           if "tex" in sp[3][p["mat"]] and sp[2][sp[3][p["mat"]]["tex"]]["kind"] == W.TEX_IMAGE]
    assert {k for _, k in img} == {0, 1, 2, 3} and len(sp[0]) > 32
    assert sorted(k for m, k in img if m == W.WMAT_LIGHT) == [1, 3]
