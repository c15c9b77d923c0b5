"""Surface queries on the GPU (rtw_hip.h "surface queries"):
rtw_world_surface_device / rtw_scene_surface_device / rtw_world_surface held, bit for bit
(uint64 words), against
  - the oracle: rw_hit of every ray, the material table and rw_texture_value at that record's
    uv and p (tests/surface_helpers.py computes it once per frame on the CPU), and
  - rtw_world_guides_device / rtw_scene_guides_device: the guides read off the hits of a
    frame's feature rays are that kernel's buffer, byte for byte.
Frames: scenes 1-7 and the mixed world of tests/helpers.py; a census of the oracle's records
keeps each from passing vacuously.  Then one incoherent bounce, grid tails, misses and
out-of-range records, optional outputs, every refusal, a dynamic world after an update and a
rebuild, the scene path, and the torch wrappers on a non-default stream."""
import ctypes as C

import numpy as np
import pytest

from query_helpers import oracle_hits
from surface_helpers import (FRAMES, check_census, get_case, guides_of, oracle_surface, oracle_tex, texture_value, words)

pytestmark = pytest.mark.gpu

POISON = 0xA5
TAIL = 8  # guard records behind the last one


@pytest.fixture(scope="module")
def W():
    from rtw_amd import world
    return world


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def to_dev(a):
    import torch
    return torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).copy()).cuda()


def run_surface(rtw, target, d_hits, n, background, surf=True, guides=True):
    """n records through the pointer API into buffers pre-filled with POISON, TAIL guard records behind
    the last -> (surf (n + TAIL,) SURFACE_DTYPE or None, guides (n + TAIL,) GUIDE_DTYPE or None)."""
    import torch
    s = torch.full(((n + TAIL) * 64,), POISON, dtype=torch.uint8, device="cuda:0") if surf else None
    g = torch.full(((n + TAIL) * 32,), POISON, dtype=torch.uint8, device="cuda:0") if guides else None
    target.surface(d_hits.data_ptr(), n, s.data_ptr() if surf else None, g.data_ptr() if guides else None,
                   background if guides else None, _stream())
    torch.cuda.synchronize()
    return (s.cpu().numpy().view(rtw.SURFACE_DTYPE) if surf else None,
            g.cpu().numpy().view(rtw.GUIDE_DTYPE) if guides else None)


def assert_words(got, want, where):
    gw, ww = words(got), words(want)
    bad = np.nonzero((gw != ww).any(axis=1))[0]
    assert bad.size == 0, (where, bad.size, bad[:5], got[bad[:2]], want[bad[:2]])


def assert_poison(a, where):
    assert (np.ascontiguousarray(a).view(np.uint8) == POISON).all(), where


class Dev:
    """A case on the device: the world, the frame's feature rays and their closest hits."""

    def __init__(self, rtw, W, case, traversal="auto"):
        import torch
        self.dw = W.DeviceWorld(case.desc)
        self.rays = torch.empty((case.n, 9), dtype=torch.float64, device="cuda:0")
        self.hits = torch.empty((case.n, 10), dtype=torch.float64, device="cuda:0")
        rtw.pixel_rays_device(case.cam, case.w, case.h, self.rays.data_ptr(), _stream())
        self.dw.trace(self.rays.data_ptr(), case.n, self.hits.data_ptr(), rtw.query_opts(traversal), _stream())
        torch.cuda.synchronize()
        self.traversal = self.dw.query_info(rtw.query_opts(traversal))["traversal"]
        self.h_hits = self.hits.cpu().numpy().reshape(-1).view(rtw.HIT_DTYPE)


@pytest.fixture(scope="module")
def devs(rtw, oracle, W):
    made = {}

    def get(name, traversal="auto"):
        if (name, traversal) not in made:
            made[(name, traversal)] = Dev(rtw, W, get_case(rtw, oracle, W, name), traversal)
        return made[(name, traversal)]
    yield get
    for d in made.values():
        d.dw.close()


# ------------------------------------------------- 1. guides and oracle equality on the scenes --
@pytest.mark.parametrize("name,traversal", [(n, "auto") for n in FRAMES] + [("scene7", "union")])
def test_frame_equals_guides_kernel_and_oracle(rtw, oracle, W, devs, name, traversal):
    import torch
    case = get_case(rtw, oracle, W, name)
    c = check_census(oracle, W, case)
    dev = devs(name, traversal)
    if name == "scene7":
        assert case.desc.n_prims == 9982 and dev.traversal == ("lane" if traversal == "auto" else "union"), dev.traversal
    assert np.array_equal(dev.rays.cpu().numpy().reshape(-1).view(np.uint64), words(case.rays).reshape(-1))
    assert_words(dev.h_hits, case.ref_hits, (name, "hits"))
    surf, guides = run_surface(rtw, dev.dw, dev.hits, case.n, case.background)
    assert_poison(surf[case.n:], (name, "surface tail"))
    assert_poison(guides[case.n:], (name, "guide tail"))
    # the guides: rtw_world_guides_device's buffer, byte for byte
    p = rtw.make_params(case.w, case.h, 1, background=case.background)
    g = torch.full((case.n * 32,), POISON, dtype=torch.uint8, device="cuda:0")
    dev.dw.guides(case.cam, p, g.data_ptr(), _stream())
    torch.cuda.synchronize()
    kernel = g.cpu().numpy().view(rtw.GUIDE_DTYPE)
    assert_words(guides[:case.n], kernel, (name, "guides against rtw_world_guides_device"))
    # every field of the surface record: the oracle's
    assert_words(surf[:case.n], case.ref_surf, (name, "surface against the oracle"))
    assert_words(guides[:case.n], guides_of(rtw, case.ref_hits, case.ref_surf, case.background), (name, "guides against the oracle"))
    print(name, traversal, dev.traversal, {k: v for k, v in c.items() if v})


# ---------------------------------------------------------------- 2. incoherent records --
@pytest.mark.parametrize("name,need", [("scene1", ("inside", "metal", "glass", "checker", "miss")),
                                       ("scene6", ("back", "xy_front", "xy_back", "xz_back", "yz_back", "xform")),
                                       ("scene7", ("inside", "image", "metal", "glass", "checker", "miss"))])
def test_bounce_records_equal_the_oracle(rtw, oracle, W, devs, name, need):
    """One bounce built in torch from the frame's hits: the ray reflected about the normal, and the ray
    continued straight on (into the sphere it met), both from p.  The oracle is given the device's own ray
    bytes."""
    import torch
    case, dev = get_case(rtw, oracle, W, name), devs(name)
    hit = dev.hits.view(torch.int32)[:, 18] != 0
    d, nrm, p, time = dev.rays[hit, 3:6], dev.hits[hit, 4:7], dev.hits[hit, 1:4], dev.rays[hit, 6]
    refl = d - 2.0 * (d * nrm).sum(dim=1, keepdim=True) * nrm
    n = 2 * int(hit.sum())
    rays = torch.empty((n, 9), dtype=torch.float64, device="cuda:0")
    rays[:, 0:3], rays[:, 3:6], rays[:, 6] = torch.cat([p, p]), torch.cat([refl, d]), torch.cat([time, time])
    rays[:, 7], rays[:, 8] = 0.001, float("inf")
    hits = torch.empty((n, 10), dtype=torch.float64, device="cuda:0")
    dev.dw.trace(rays.data_ptr(), n, hits.data_ptr(), None, _stream())
    torch.cuda.synchronize()
    h_rays = rays.cpu().numpy().reshape(-1).view(rtw.RAY_DTYPE)
    ref_hits = oracle_hits(rtw, case.oracle, h_rays)
    ref_surf = oracle_surface(rtw, oracle, case.oracle, ref_hits, case.desc)
    c = check_census(oracle, W, case, ref_hits, ref_surf, need)
    if name != "scene6":  # off-centre u, v: the records' own, not a pixel grid's
        assert len(np.unique(ref_hits["u"][ref_surf["kind"] > 0])) > 50
    ok = ~np.isnan(ref_hits["t"])  # (a ray in a rect's plane: the reference's 0/0)
    assert ok.sum() >= n - 4
    got_hits = hits.cpu().numpy().reshape(-1).view(rtw.HIT_DTYPE)
    assert (got_hits["prim"] == ref_hits["prim"]).all()
    assert_words(got_hits[ok], ref_hits[ok], (name, "bounce hits"))
    surf, guides = run_surface(rtw, dev.dw, hits, n, case.background)
    assert_poison(surf[n:], (name, "surface tail"))
    assert_poison(guides[n:], (name, "guide tail"))
    assert_words(surf[:n][ok], ref_surf[ok], (name, "bounce surface against the oracle"))
    assert_words(guides[:n][ok], guides_of(rtw, ref_hits, ref_surf, case.background)[ok], (name, "bounce guides"))
    assert (surf[:n]["kind"] == ref_surf["kind"]).all() and (surf[:n]["mat"] == ref_surf["mat"]).all()
    print(name, n, {k: v for k, v in c.items() if v})


# ------------------------------------------------------------------------ 3. grid tails --
@pytest.mark.parametrize("n", [1, 63, 64, 257, 1296])
def test_grid_tails_keep_the_poison(rtw, oracle, W, devs, n):
    case, dev = get_case(rtw, oracle, W, "scene1"), devs("scene1")
    assert n <= case.n
    surf, guides = run_surface(rtw, dev.dw, dev.hits, n, case.background)
    assert_words(surf[:n], case.ref_surf[:n], ("tail", n))
    assert_words(guides[:n], guides_of(rtw, case.ref_hits, case.ref_surf, case.background)[:n], ("tail guides", n))
    assert_poison(surf[n:], ("surface records from n on", n))
    assert_poison(guides[n:], ("guide records from n on", n))


# -------------------------------------------------------------------- 4. misses and bounds --
@pytest.mark.parametrize("with_guides", [True, False])
def test_misses_mixed_among_hits(rtw, oracle, W, devs, with_guides):
    case, dev = get_case(rtw, oracle, W, "scene1"), devs("scene1")
    h = dev.h_hits.copy()
    n = len(h)
    miss = np.zeros(n, bool)
    for start, step, prim in ((3, 7, 0), (5, 11, case.desc.n_prims + 1), (9, 13, 0xFFFFFFFF)):
        h["prim"][start::step] = prim  # (the other fields stay: a record no trace produced)
        miss[start::step] = True
    assert (case.ref_surf["kind"][miss] > 0).sum() > 100 and (~miss).sum() > 1000
    surf, guides = run_surface(rtw, dev.dw, to_dev(h), n, case.background, guides=with_guides)
    want = case.ref_surf.copy()
    want[miss] = np.zeros(1, rtw.SURFACE_DTYPE)
    assert_words(surf[:n], want, "misses among hits")
    assert (words(surf[:n][miss]) == 0).all()
    assert_poison(surf[n:], "surface tail")
    if with_guides:
        hh = case.ref_hits.copy()
        hh["prim"][miss] = 0
        wg = guides_of(rtw, hh, want, case.background)
        assert_words(guides[:n], wg, "guides of misses among hits")
        g = guides[:n][miss]
        assert (g["normal"] == 0).all() and (g["depth"] == 0).all() and (g["prim"] == 0).all()
        assert (g["albedo"] == np.array(case.background, np.float64).astype(np.float32)).all()
        assert_poison(guides[n:], "guide tail")


@pytest.mark.parametrize("scale", [1.0, 1e3, 1e6])
@pytest.mark.parametrize("name,tex_kind", [("scene3", "noise"), ("scene4", "image")])
def test_out_of_range_uv_and_far_points(rtw, oracle, W, devs, name, tex_kind, scale):
    """Records no trace produced, on a noise and an image texture: u, v in {-3, 0, 1, 7} (and two values
    inside the image), |p| = 0.25-1 x `scale` (1, 1e3, 1e6) in directions uniform on the sphere — value is
    the oracle's for the same arguments and the neighbours keep their bytes; then NaN, infinite and 1e300
    u, v, p: the call returns and the neighbours keep their bytes.

    [scene3-noise-1000000.0]: the noise texture ends in sin(4 p.z + 10 |turb|), and for
    |x| >= 2^20 pi/2 = 1,647,099 — |p.z| above 4.1e5 here, 28 of the case's 72 records — the oracle's
    rol_sin leaves musl's path and calls glibc's sin (oracle/ro_libm.h: "never produced by the
    reference's scenes").  While the device called ocml's there, 1 of the 72 differed from
    rw_texture_value, by 2 ulp of value; the device's rtwl::sin_far is rounded to nearest
    (tests/test_sin_far_cpu.py) and so is glibc's in these 28, as in 99.86 % of arguments
    (DESIGN.md §19.3): 0 of 72 differ."""
    case, dev = get_case(rtw, oracle, W, name), devs(name)
    kind = {"noise": oracle.RW_TEX_NOISE, "image": oracle.RW_TEX_IMAGE}[tex_kind] + 1
    rows = np.nonzero(case.ref_surf["tex_kind"] == kind)[0]
    assert len(rows) >= 100
    rng = np.random.default_rng(19 + int(np.log10(scale)))
    edge = (-3.0, 0.0, 0.37, 0.61, 1.0, 7.0)  # the issue's four, and two inside the image
    uv = [(u, v) for u in edge for v in edge]
    crafted = []
    for j, (u, v) in enumerate(uv):
        for _ in range(2):  # |p| = 0.25-1 x scale, in a direction uniform on the sphere
            d = rng.normal(size=3)
            crafted.append((u, v, scale * rng.uniform(0.25, 1.0) * d / np.sqrt((d * d).sum())))
    wild = [(np.nan, 0.5, (1.0, 2.0, 3.0)), (0.5, np.nan, (1.0, 2.0, 3.0)), (np.inf, -np.inf, (1.0, 2.0, 3.0)),
            (0.5, 0.5, (np.nan, np.nan, np.nan)), (0.5, 0.5, (np.inf, -np.inf, np.inf)), (1e300, -1e300, (1e300, -1e300, 1e300)),
            (-0.0, -0.0, (-0.0, -0.0, -0.0)), (5e-324, 1.0 - 2.0 ** -53, (2.0 ** 31, -2.0 ** 31, 2.0 ** 52))]
    h = dev.h_hits.copy()
    n = len(h)
    assert 2 * (len(crafted) + len(wild)) < n
    at = 1 + 2 * np.arange(len(crafted) + len(wild))  # odd positions: every crafted record between two of the frame's
    tmpl = rows[np.arange(len(at)) % len(rows)]
    for i, t, (u, v, p) in zip(at, tmpl, crafted + wild):
        h[i] = dev.h_hits[t]
        h["u"][i], h["v"][i], h["p"][i] = u, v, p
    surf, guides = run_surface(rtw, dev.dw, to_dev(h), n, case.background)
    keep = np.ones(n, bool)
    keep[at] = False
    assert_words(surf[:n][keep], case.ref_surf[keep], (name, "neighbours"))
    assert_words(guides[:n][keep], guides_of(rtw, case.ref_hits, case.ref_surf, case.background)[keep], (name, "neighbour guides"))
    assert_poison(surf[n:], "surface tail")
    assert_poison(guides[n:], "guide tail")
    want = case.ref_surf[tmpl[:len(crafted)]].copy()
    for k, (t, (u, v, p)) in enumerate(zip(tmpl, crafted)):
        want["value"][k] = texture_value(oracle, case.oracle, oracle_tex(case.oracle, case.ref_hits["prim"][t]), u, v, p)
    got = surf[:n][at[:len(crafted)]]
    differ = (words(got["value"]) != words(want["value"])).any(axis=1)
    ulps = np.abs(words(got["value"]).astype(np.int64) - words(want["value"]).astype(np.int64)).max() if len(crafted) else 0
    beyond = sum(1 for _, _, p in crafted if abs(4.0 * p[2]) >= 2.0 ** 20 * np.pi / 2)
    print(f"{name} {tex_kind} scale {scale:g}: {int(differ.sum())} of {len(crafted)} crafted records differ from rw_texture_value "
          f"(largest distance {int(ulps)} ulp); {beyond} have |4 p.z| >= 2^20 pi/2")
    assert_words(got, want, (name, "crafted records against rw_texture_value"))
    moved =(words(got["value"]) != words(case.ref_surf["value"][tmpl[:len(crafted)]])).any(axis=1)
    assert moved.sum() > len(crafted) // 4, moved.sum()  # (the arguments did matter)
    for f in ("kind", "mat", "tex", "tex_kind"):  # the wild ones: the table fields are still the template's
        assert (surf[:n][at[len(crafted):]][f] == case.ref_surf[tmpl[len(crafted):]][f]).all(), f


# ------------------------------------------------------------------ 5. optional outputs --
@pytest.mark.parametrize("name", ["scene3", "mixed"])
def test_optional_outputs_agree(rtw, oracle, W, devs, name):
    case, dev = get_case(rtw, oracle, W, name), devs(name)
    both_s, both_g = run_surface(rtw, dev.dw, dev.hits, case.n, case.background)
    only_s, none_g = run_surface(rtw, dev.dw, dev.hits, case.n, case.background, guides=False)
    none_s, only_g = run_surface(rtw, dev.dw, dev.hits, case.n, case.background, surf=False)
    assert none_g is None and none_s is None
    assert both_s.tobytes() == only_s.tobytes() and both_g.tobytes() == only_g.tobytes()
    again_s, again_g = run_surface(rtw, dev.dw, dev.hits, case.n, case.background)
    assert both_s.tobytes() == again_s.tobytes() and both_g.tobytes() == again_g.tobytes()  # the same input, the same bytes


# ------------------------------------------------------------------------- 6. refusals --
def test_every_refusal(rtw, oracle, W, devs):
    import torch
    case, dev = get_case(rtw, oracle, W, "scene2"), devs("scene2")
    L = rtw.lib()
    n = case.n
    surf = torch.full(((n + TAIL) * 64,), POISON, dtype=torch.uint8, device="cuda:0")
    guides = torch.full(((n + TAIL) * 32,), POISON, dtype=torch.uint8, device="cuda:0")
    big = torch.zeros((n * 80 + n * 64,), dtype=torch.uint8, device="cuda:0")  # hits, then room for an overlapping output
    big[:n * 80] = dev.hits.view(torch.uint8).reshape(-1)
    bg = (C.c_double * 3)(*case.background)
    w, h, s, g = dev.dw.h, dev.hits.data_ptr(), surf.data_ptr(), guides.data_ptr()
    sph, mats, _ = rtw.cover_scene(42)
    sc = rtw.DeviceScene(sph, mats)
    V = C.c_void_p
    EINVAL, OK = rtw.RTW_EINVAL, rtw.RTW_OK

    def bad_bg(x):
        return (C.c_double * 3)(0.5, x, 0.5)
    for f, handle in ((L.rtw_world_surface_device, w), (L.rtw_scene_surface_device, sc.h)):
        cases = {
            "null handle": (None, V(h), n, bg, V(s), V(g)),
            "null d_hits": (handle, None, n, bg, V(s), V(g)),
            "both outputs null": (handle, V(h), n, bg, None, None),
            "guides without a background": (handle, V(h), n, None, V(s), V(g)),
            "nan background": (handle, V(h), n, bad_bg(float("nan")), V(s), V(g)),
            "inf background": (handle, V(h), n, bad_bg(float("inf")), None, V(g)),
            "d_hits not 8-byte aligned": (handle, V(h + 4), n - 1, bg, V(s), V(g)),
            "d_surf not 8-byte aligned": (handle, V(h), n, bg, V(s + 4), V(g)),
            "d_guides not 16-byte aligned": (handle, V(h), n, bg, V(s), V(g + 8)),
            "n > 2^31": (handle, V(h), (1 << 31) + 1, bg, V(s), V(g)),
            "d_surf on d_hits": (handle, V(big.data_ptr()), n, bg, V(big.data_ptr()), V(g)),
            "d_surf inside d_hits": (handle, V(big.data_ptr()), n, bg, V(big.data_ptr() + 80 * n - 8), V(g)),
            "d_hits inside d_guides": (handle, V(big.data_ptr() + 32), n, bg, V(s), V(big.data_ptr())),
            "d_guides overlaps d_surf": (handle, V(h), n, bg, V(big.data_ptr()), V(big.data_ptr() + 64 * n - 16)),
        }
        for what, args in cases.items():
            assert f(*args, None) == EINVAL, (f.__name__, what)
            assert rtw.lib().rtw_last_error(), what
        # in range, and what is NOT refused
        assert f(handle, None, 0, None, None, None, None) == OK                      # n == 0 with null buffers
        assert f(handle, V(h), n, None, V(s), None, None) == OK                      # no guides: no background needed
        assert f(handle, V(big.data_ptr()), n, bg, V(big.data_ptr() + 80 * n), None, None) == OK  # adjacent is not overlapping
        torch.cuda.synchronize()
    assert L.rtw_world_surface(None, V(h), n, V(s)) == EINVAL
    assert L.rtw_world_surface(w, None, n, V(s)) == EINVAL
    assert L.rtw_world_surface(w, V(h), n, None) == EINVAL
    assert L.rtw_world_surface(w, None, 0, None) == OK
    torch.cuda.synchronize()
    assert_poison(surf.cpu().numpy()[n * 64:], "surface guard after the refusals")
    assert_poison(guides.cpu().numpy(), "guides after the refusals")   # (no accepted call above wrote guides)
    if torch.cuda.device_count() > 1:  # a world that lives on another device
        with torch.cuda.device(1):
            assert L.rtw_world_surface_device(w, V(h), n, bg, V(s), V(g), None) == EINVAL
            assert L.rtw_scene_surface_device(sc.h, V(h), n, bg, V(s), V(g), None) == EINVAL
    sc.close()


def test_host_form_equals_the_device_form(rtw, oracle, W, devs):
    case, dev = get_case(rtw, oracle, W, "mixed"), devs("mixed")
    got = dev.dw.surface_host(dev.h_hits)
    assert_words(got, case.ref_surf, "rtw_world_surface")
    assert len(dev.dw.surface_host(dev.h_hits[:0])) == 0


# ------------------------------------------------ 7. a dynamic world after update and rebuild --
def test_dynamic_world_after_update_and_rebuild(rtw, W):
    """Half the spheres of the mixed sphere world move (an update), then move again (a rebuild): hits, surface
    records and guides equal those of a world freshly created from the same numbers."""
    import torch
    from helpers import MIXED_CAMERA, _to_desc, mixed_bvh_world
    from rtw_amd.device import rebuild_world, update_world
    from update_helpers import numbers, prims_with
    fw, fh = 48, 27
    n = fw * fh
    tables = mixed_bvh_world(W, W.earth_map(), 0, 600, 5, variant="spheres_image")
    desc, _keep = _to_desc(W, *tables)
    m = MIXED_CAMERA
    cam = rtw.camera_init(m["look_from"], m["look_at"], (0, 1, 0), m["vfov"], fw / fh, m["aperture"], m["focus"], 0.0, 1.0)
    a0, _ = numbers(tables)
    rng = np.random.default_rng(23)
    small = np.nonzero(np.abs(a0[:, 6]) < 5.0)[0]
    moved = small[::2]
    assert len(moved) >= 250

    def move(a, scale):
        b = a.copy()
        step = rng.uniform(-scale, scale, (len(moved), 3)) * np.array([1.0, 0.0, 1.0])
        b[moved, 0:3] += step
        b[moved, 3:6] += step
        return b
    a1 = move(a0, 3.0)
    a2 = move(a1, 3.0)
    bg = (0.7, 0.8, 1.0)

    def frame(dw):
        rays = torch.empty((n, 9), dtype=torch.float64, device="cuda:0")
        hits = torch.empty((n, 10), dtype=torch.float64, device="cuda:0")
        rtw.pixel_rays_device(cam, fw, fh, rays.data_ptr(), _stream())
        dw.trace(rays.data_ptr(), n, hits.data_ptr(), None, _stream())
        surf, guides = run_surface(rtw, dw, hits, n, bg)
        return hits.cpu().numpy().reshape(-1).view(rtw.HIT_DTYPE), surf[:n], guides[:n]

    def fresh(a):
        keep = prims_with(W, desc, a)
        d = W.WorldDesc()
        for f, _ in W.WorldDesc._fields_:
            setattr(d, f, getattr(desc, f))
        d.prims = C.cast(keep, C.POINTER(W.Prim))
        dw = W.DeviceWorld(d)
        try:
            return frame(dw)
        finally:
            dw.close()
    dyn = W.DeviceWorld(desc, dynamic=True)
    try:
        assert dyn.bvh_info()["max_leaf"] == 1 and desc.n_prims >= 512
        base = frame(dyn)
        update_world(dyn, torch.from_numpy(a1).cuda())
        upd = frame(dyn)
        rebuild_world(dyn, torch.from_numpy(a2).cuda())
        reb = frame(dyn)
    finally:
        dyn.close()
    assert (words(base[1]) != words(upd[1])).any(axis=1).sum() > 50 and (words(upd[1]) != words(reb[1])).any(axis=1).sum() > 50
    for got, a, what in ((upd, a1, "update"), (reb, a2, "rebuild")):
        want = fresh(a)
        kinds = set(np.unique(want[1]["tex_kind"])) | {10 + k for k in np.unique(want[1]["kind"])}
        assert kinds >= {0, 1, 4, 11, 12, 13}, kinds  # misses, solid and image textures; Lambert, metal and glass
        for g, w_, part in zip(got, want, ("hits", "surface", "guides")):
            assert_words(g, w_, (what, part))


# --------------------------------------------------------------------- 8. the scene path --
def test_scene_path(rtw):
    import torch
    w, h = 60, 33
    n = w * h
    sph, mats, _ = rtw.cover_scene(42)
    cam = rtw.cover_camera(w / h)
    sc = rtw.DeviceScene(sph, mats)
    try:
        rays = torch.empty((n, 9), dtype=torch.float64, device="cuda:0")
        hits = torch.empty((n, 10), dtype=torch.float64, device="cuda:0")
        rtw.pixel_rays_device(cam, w, h, rays.data_ptr(), _stream())
        sc.trace(rays.data_ptr(), n, hits.data_ptr(), _stream())
        surf, guides = run_surface(rtw, sc, hits, n, rtw.COVER_BACKGROUND)
        assert_poison(surf[n:], "surface tail")
        assert_poison(guides[n:], "guide tail")
        g = torch.full((n * 32,), POISON, dtype=torch.uint8, device="cuda:0")
        sc.guides(cam, rtw.make_params(w, h, 1), g.data_ptr(), _stream())
        torch.cuda.synchronize()
        kernel = g.cpu().numpy().view(rtw.GUIDE_DTYPE)
        assert_words(guides[:n], kernel, "guides against rtw_scene_guides_device")
        hh = hits.cpu().numpy().reshape(-1).view(rtw.HIT_DTYPE)
        assert_words(guides[:n], guides_of(rtw, hh, surf[:n], rtw.COVER_BACKGROUND), "guides against the surface records")
    finally:
        sc.close()
    s = surf[:n]
    seen = {"solid": 0, "even": 0, "odd": 0, "metal": 0, "glass": 0, "miss": 0}
    for i in range(n):
        k = int(hh[i]["prim"])
        if k == 0:
            assert words(s[i:i + 1]).any() == 0
            seen["miss"] += 1
            continue
        mi = int(sph[k - 1].mat)
        mt = mats[mi]
        assert s[i]["mat"] == mi + 1 and s[i]["tex"] == 0 and (s[i]["reserved"] == 0).all()
        val = tuple(s[i]["value"])
        if mt.kind == 0:    # RTW_LAMBERT_SOLID: Lambert over a solid texture
            assert (s[i]["kind"], s[i]["tex_kind"], s[i]["fuzz"], s[i]["ir"]) == (1, 1, 0.0, 0.0) and val == tuple(mt.albedo)
            seen["solid"] += 1
        elif mt.kind == 1:  # RTW_LAMBERT_CHECKER: the even or the odd colour
            assert (s[i]["kind"], s[i]["tex_kind"], s[i]["fuzz"], s[i]["ir"]) == (1, 2, 0.0, 0.0)
            assert tuple(mt.albedo) != tuple(mt.albedo_odd) and val in (tuple(mt.albedo), tuple(mt.albedo_odd))
            seen["even" if val == tuple(mt.albedo) else "odd"] += 1
        elif mt.kind == 2:  # RTW_METAL
            assert (s[i]["kind"], s[i]["tex_kind"], s[i]["fuzz"], s[i]["ir"]) == (2, 0, mt.fuzz, 0.0) and val == tuple(mt.albedo)
            seen["metal"] += 1
        else:               # RTW_DIELECTRIC
            assert (s[i]["kind"], s[i]["tex_kind"], s[i]["fuzz"], s[i]["ir"]) == (3, 0, 0.0, mt.ir) and val == (1.0, 1.0, 1.0)
            seen["glass"] += 1
    assert all(v >= 5 for v in seen.values()), seen


# ------------------------------------------------------------------------------ 9. torch --
def test_torch_wrappers_on_another_stream(rtw, oracle, W, devs):
    import torch
    from rtw_amd.device import TorchTracer
    case, dev = get_case(rtw, oracle, W, "scene4"), devs("scene4")
    want_s, want_g = run_surface(rtw, dev.dw, dev.hits, case.n, case.background)
    tr = TorchTracer(dev.dw, 0)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        hit = tr.trace(dev.rays[:, 0:3], dev.rays[:, 3:6], time=dev.rays[:, 6])
        out = tr.surface(hit, guides=True, background=case.background)
        plain = tr.surface(hit["records"])
        frame = tr.guides(case.cam, case.w, case.h, case.background)
        frame2 = tr.guides(case.cam, case.w, case.h, case.background)  # (the kept ray and hit tensors)
        empty = tr.surface(hit["records"][:0], guides=True, background=case.background)
    side.synchronize()
    assert hit["records"].cpu().numpy().tobytes() == dev.hits.cpu().numpy().tobytes()
    assert out["records"].cpu().numpy().tobytes() == want_s[:case.n].tobytes()
    assert plain["records"].cpu().numpy().tobytes() == want_s[:case.n].tobytes() and "guides" not in plain
    assert out["guides"].cpu().numpy().tobytes() == want_g[:case.n].tobytes()
    assert tuple(frame.shape) == (case.h, case.w, 32)
    assert frame.cpu().numpy().tobytes() == want_g[:case.n].tobytes() == frame2.cpu().numpy().tobytes()
    ref = case.ref_surf
    for f in ("kind", "mat", "tex", "tex_kind"):
        assert np.array_equal(out[f].cpu().numpy(), ref[f].astype(np.int64) - 1), f
    assert np.array_equal(out["value"].cpu().numpy(), ref["value"]) and np.array_equal(out["ir"].cpu().numpy(), ref["ir"])
    assert empty["records"].shape == (0, 8) and empty["guides"].shape == (0, 32)
    sph, mats, _ = rtw.cover_scene(42)  # the scene target through the same wrappers
    sc = rtw.DeviceScene(sph, mats)
    try:
        cam, p = rtw.cover_camera(16 / 9), rtw.make_params(32, 18, 1)
        with torch.cuda.stream(side):
            got = TorchTracer(sc, 0).guides(cam, 32, 18, rtw.COVER_BACKGROUND)
            g = torch.empty((18, 32, 32), dtype=torch.uint8, device="cuda:0")
            sc.guides(cam, p, g.data_ptr(), side.cuda_stream)
        side.synchronize()
        assert got.cpu().numpy().tobytes() == g.cpu().numpy().tobytes()
    finally:
        sc.close()
