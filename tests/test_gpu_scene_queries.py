"""The scene API on the GPU beyond cover_scene(42) (rtw_hip.h "ray queries", "surface queries";
DESIGN.md §14, §15, §19): scene_query_kernel<false / true>, scene_guides_kernel and
scene_surface_kernel against oracle.TableWorld on the scenes of tests/scene_query_helpers.py —
hollow glass, movers with ranges of their own, three and 64 time groups, coincident pairs whose
table order is not their list order, list index 4095 / material 4095 / time group 63, no sphere,
one sphere — with ray times inside and outside the ranges, interval ends on the roots, rays from
inside spheres and directions whose squared length overflows or underflows.

Everything is bit for bit (records as uint64 words); a record whose oracle root is NaN compares
prim and the NaN-ness of t (query_helpers._assert_records).  tests/test_scene_query_cpu.py holds
the census that keeps these from passing on an empty category."""
import numpy as np
import pytest

import query_helpers as Q
import scene_query_helpers as S
from query_helpers import _assert_records, _trace
from surface_helpers import guides_of, words

pytestmark = pytest.mark.gpu

import torch  # noqa: E402  (device buffers and streams)

POISON = 0xA5
GUARD = 256
SIZES = (1, 63, 64, 65)


class Dev:
    """A scene on the device and, per ray set, its rays there."""

    def __init__(self, rtw, sc):
        self.sc = sc
        self.dev = rtw.DeviceScene(sc.sph, sc.mats)
        self._rays = {}

    def rays(self, key):
        if key not in self._rays:
            self._rays[key] = Q.to_device(self.sc.sets()[key][0])
        return self._rays[key]


@pytest.fixture(scope="module")
def devs(rtw, oracle):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Dev(rtw, S.get_scene(rtw, oracle, name))
        return made[name]
    yield get
    for d in made.values():
        d.dev.close()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _check_set(rtw, d, key):
    """One ray set through rtw_scene_trace_device, rtw_scene_occluded_device and rtw_scene_trace: prefixes of
    1, 63, 64, 65 rays and the whole set, into poisoned buffers with a guard behind them."""
    rays, ref = d.sc.sets()[key]
    n_all = len(rays)
    if n_all == 0:
        return None
    where = (d.sc.name, key)
    full, guard = _trace(rtw, d.dev, d.rays(key), n_all, is_world=False)
    assert (guard == POISON).all(), where
    _assert_records(full, ref, where)
    occ_full, guard = _trace(rtw, d.dev, d.rays(key), n_all, occluded=True, is_world=False)
    assert (guard == POISON).all(), where
    bad = np.nonzero(occ_full != (ref["prim"] > 0))[0]
    assert bad.size == 0, (where, f"occlusion: {bad.size} of {n_all} rows differ", bad[:5])
    for n in SIZES:
        if n >= n_all:
            continue
        got, guard = _trace(rtw, d.dev, d.rays(key), n, is_world=False)
        assert (guard == POISON).all(), (where, n)
        assert words(got).tobytes() == words(full[:n]).tobytes(), (where, n)  # a prefix gives the full run's prefix
        occ, guard = _trace(rtw, d.dev, d.rays(key), n, occluded=True, is_world=False)
        assert (guard == POISON).all() and (occ == occ_full[:n]).all(), (where, n)
    assert words(d.dev.trace_host(rays)).tobytes() == words(full).tobytes(), where  # rtw_scene_trace: the device's bytes
    return full


# --------------------------------------------------------------- 1. trace and occlusion --
@pytest.mark.parametrize("name", S.SCENES)
def test_trace_and_occlusion_equal_the_oracle(rtw, devs, name):
    d = devs(name)
    for key in d.sc.sets():
        if key != "overflow":  # (test_overflow_rays_equal_the_oracle)
            _check_set(rtw, d, key)


@pytest.mark.parametrize("name", S.OVERFLOW_SCENES)
def test_overflow_rays_equal_the_oracle(rtw, devs, name):
    """|dir|^2 overflows: disc = inf - inf = NaN, which the reference does not reject, and after the first NaN
    closest it accepts every later sphere — the last list sphere wins with t = NaN, and the ray is occluded.
    Eight directions of length 2^-560: |dir|^2 and half_b^2 underflow to 0, the root is +-inf."""
    d = devs(name)
    rays, ref = d.sc.sets()["overflow"]
    assert np.isnan(ref["t"]).sum() >= 16 and np.isinf(ref["t"]).sum() >= 4
    got = _check_set(rtw, d, "overflow")
    nan = np.isnan(ref["t"])
    assert (got["prim"][nan] == d.sc.n).all() and np.isnan(got["t"][nan]).all()


# ------------------------------------------------------------------------- 2. guides --
def _device_guides(rtw, d, cam, rows):
    kw = {} if rows is None else dict(row_begin=rows[0], row_stride=rows[1], row_count=rows[2])
    p = rtw.make_params(S.FW, S.FH, 1, background=S.BACKGROUND, **kw)
    size = p.row_count * S.FW * 32
    g = torch.full((size + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    d.dev.guides(cam, p, g.data_ptr(), _stream())
    torch.cuda.synchronize()
    host = g.cpu().numpy()
    assert (host[size:] == POISON).all(), (d.sc.name, rows, "guard")
    image_rows = range(S.FH) if rows is None else [rows[0] + k * rows[1] for k in range(rows[2])]
    return host[:size].view(rtw.GUIDE_DTYPE), list(image_rows)


def _assert_words(got, want, where):
    gw, ww = words(got), words(want)
    bad = np.nonzero((gw != ww).any(axis=1))[0]
    assert bad.size == 0, (where, f"{bad.size} of {len(gw)} records differ", bad[:5], got[bad[:2]], want[bad[:2]])


@pytest.mark.parametrize("shutter", S.SHUTTERS, ids=["shutter0-1", "shutter0.25-2"])
@pytest.mark.parametrize("name", S.SCENES)
def test_guides_equal_the_oracle(rtw, devs, name, shutter):
    """rtw_scene_guides_device, word for word: guides_of the oracle's hits and surface values of the frame's
    feature rays (mid-shutter time 0.5, and 1.125 — outside the range [0, 1] of a mover)."""
    d = devs(name)
    cam, rays, hits, surf, want = d.sc.frame(shutter)
    assert (rays["time"] == 0.5 * (shutter[0] + shutter[1])).all()
    for rows in S.ROWS:
        got, image_rows = _device_guides(rtw, d, cam, rows)
        idx = np.concatenate([np.arange(y * S.FW, (y + 1) * S.FW) for y in image_rows])
        _assert_words(got, want[idx], (name, shutter, rows))


# ------------------------------------------------------------------------ 3. surface --
def _run_surface(rtw, d, d_hits, n):
    s = torch.full((n * 64 + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    g = torch.full((n * 32 + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    d.dev.surface(d_hits.data_ptr(), n, s.data_ptr(), g.data_ptr(), S.BACKGROUND, _stream())
    torch.cuda.synchronize()
    hs, hg = s.cpu().numpy(), g.cpu().numpy()
    assert (hs[n * 64:] == POISON).all() and (hg[n * 32:] == POISON).all(), (d.sc.name, "guard")
    return hs[:n * 64].view(rtw.SURFACE_DTYPE), hg[:n * 32].view(rtw.GUIDE_DTYPE)


def _device_hits(rtw, d, key):
    """The device's own hit records of ray set `key`: (device buffer, host records)."""
    n = len(d.sc.sets()[key][0])
    hits = torch.empty((n * 80,), dtype=torch.uint8, device="cuda")
    d.dev.trace(d.rays(key).data_ptr(), n, hits.data_ptr(), _stream())
    torch.cuda.synchronize()
    return hits, hits.cpu().numpy().view(rtw.HIT_DTYPE)


@pytest.mark.parametrize("name", S.SCENES)
def test_surface_records_equal_the_oracle(rtw, oracle, devs, name):
    """The device's own hits of the main set (feature, bounce, inward and shadow rays) and of the set at time 3
    through rtw_scene_surface_device: the records are the scene's material arrays and the oracle's checker value
    at the record's p, the guides guides_of those records."""
    d = devs(name)
    for key in ("main", "time3.0"):
        d_hits, hits = _device_hits(rtw, d, key)
        n = len(hits)
        surf, guides = _run_surface(rtw, d, d_hits, n)
        want = S.scene_surface(rtw, oracle, d.sc, hits)
        _assert_words(surf, want, (name, key, "surface"))
        _assert_words(guides, guides_of(rtw, hits, want, S.BACKGROUND), (name, key, "guides"))
        if d.sc.n:
            assert (want["kind"] > 0).sum() >= 100 and (want["kind"] == 0).sum() >= 100
            assert name == "one" or set(np.unique(want["kind"])) == {0, 1, 2, 3}
            assert (want["tex_kind"] == 2).sum() >= 50  # checker records


@pytest.mark.parametrize("name", ["custom", "clustered", "ties", "limits", "one"])
def test_far_checker_points(rtw, oracle, devs, name):
    """Checker records with p edited to magnitudes 6e4, 1e6 and -1e6 (|10 p| >= 2^19: sin_sign_libm) against
    the oracle's rw_texture_value at that p; the records between them keep their bytes."""
    d = devs(name)
    _, hits = _device_hits(rtw, d, "main")
    base = S.scene_surface(rtw, oracle, d.sc, hits)
    rows = np.nonzero(base["tex_kind"] == 2)[0][:96:2]  # every other one: an unedited record between two edited
    assert len(rows) >= 24
    rng = np.random.default_rng(66)
    h = hits.copy()
    for j, i in enumerate(rows):
        mag = (6e4, 1e6, -1e6)[j % 3]
        h["p"][i] = mag * rng.uniform(0.9, 1.0, 3) * np.where(rng.random(3) < 0.25, -1.0, 1.0)
    assert (np.abs(10.0 * h["p"][rows]) >= 2.0 ** 19).all()
    surf, guides = _run_surface(rtw, d, Q.to_device(h), len(h))
    want = S.scene_surface(rtw, oracle, d.sc, h)
    _assert_words(surf, want, (name, "far checker points"))
    _assert_words(guides, guides_of(rtw, h, want, S.BACKGROUND), (name, "far checker guides"))
    mats = [d.sc.mats[int(m) - 1] for m in want["mat"][rows]]
    odd = np.array([tuple(v) == tuple(m.albedo_odd) for v, m in zip(want["value"][rows], mats)])
    assert 4 <= odd.sum() <= len(rows) - 4, odd.sum()  # both colours


# --------------------------------------------------------------------------- 4. ties --
def test_ties_later_list_index_wins(rtw, oracle, devs):
    d = devs("ties")
    sc = d.sc
    d_hits, hits = _device_hits(rtw, d, "ties")
    surf, _ = _run_surface(rtw, d, d_hits, len(hits))
    ref = sc.sets()["ties"][1]
    for name, (i, j) in S.TIE_PAIRS.items():
        rows = sc.tie_rows[name]
        want = [int(ref["prim"][r]) - 1 for r in rows]
        in_pair = [r for r, p in zip(rows, want) if p in (i, j)]
        assert in_pair and all(int(ref["prim"][r]) - 1 == j for r in in_pair), (name, want)
        assert [int(hits["prim"][r]) - 1 for r in rows] == want, name
        for r in in_pair:  # the later list index, in prim and in the surface record's material
            assert hits["prim"][r] == j + 1 and surf["mat"][r] == sc.sph[j].mat + 1 != sc.sph[i].mat + 1, (name, r)
    earlier = [i for i, _ in S.TIE_PAIRS.values()]
    for key in sc.sets():  # no ray of any set may ever see the earlier entry of a pair
        if key != "overflow":
            _, got = _device_hits(rtw, d, key)
            assert not np.isin(got["prim"].astype(np.int64) - 1, earlier).any(), key


# ------------------------------------------------------------------------- 5. limits --
def test_limits_list_index_material_and_time_group_tops(rtw, oracle, devs):
    d = devs("limits")
    sc = d.sc
    rays, ref = sc.sets()["main"]
    mine = np.nonzero((sc.kinds == "a") & (ref["prim"] == S.LIMITS_LAST + 1))[0]
    assert len(mine) >= 5
    d_hits, hits = _device_hits(rtw, d, "main")
    surf, guides = _run_surface(rtw, d, d_hits, len(hits))
    assert (hits["prim"][mine] == 4096).all() and (surf["mat"][mine] == 4096).all() and (guides["prim"][mine] == 4096).all()
    m = sc.mats[4095]
    assert (surf["kind"][mine] == 3).all() and (surf["ir"][mine] == m.ir).all() and m.ir != sc.mats[2047].ir
    for t in (0.1, 3.0):  # outside group 63's range [0.3, 1.7]: the records are the oracle's only with that range
        key = f"time{t}"
        tref = sc.sets()[key][1]
        rows = np.nonzero(tref["prim"] == S.LIMITS_LAST + 1)[0]
        assert len(rows) >= 5
        _, got = _device_hits(rtw, d, key)
        _assert_records(got[rows], tref[rows], ("limits", key, "sphere 4095"))
        _assert_records(got, tref, ("limits", key))


# -------------------------------------------------------------------- 6. empty and one --
def test_empty_scene(rtw, devs):
    d = devs("empty")
    assert d.sc.n == 0
    rays, ref = d.sc.sets()["main"]
    n = len(rays)
    got, guard = _trace(rtw, d.dev, d.rays("main"), n, is_world=False)
    assert (guard == POISON).all() and not got.view(np.uint8).any()  # every record 80 zero bytes
    occ, guard = _trace(rtw, d.dev, d.rays("main"), n, occluded=True, is_world=False)
    assert (guard == POISON).all() and not occ.any()
    bg = np.array(S.BACKGROUND, np.float64).astype(np.float32)
    for shutter in S.SHUTTERS:
        for rows in S.ROWS:
            g, _ = _device_guides(rtw, d, d.sc.camera(shutter), rows)
            assert not g["normal"].any() and not g["depth"].any() and not g["prim"].any() and (g["albedo"] == bg).all()
            assert (words(g)[:, :2] == 0).all()  # (normal and depth: +0.0)
    d_hits, hits = _device_hits(rtw, d, "main")
    surf, guides = _run_surface(rtw, d, d_hits, n)
    assert not surf.view(np.uint8).any()  # every surface record 64 zero bytes
    assert not guides["normal"].any() and not guides["prim"].any() and (guides["albedo"] == bg).all()
    h = hits.copy()  # records no trace produced: prim beyond the (empty) list
    h["prim"], h["t"], h["p"] = 1, 2.5, (1.0, 2.0, 3.0)
    surf, guides = _run_surface(rtw, d, Q.to_device(h), n)
    assert not surf.view(np.uint8).any() and not guides["prim"].any() and (guides["albedo"] == bg).all()


def test_one_sphere(rtw, oracle, devs):
    d = devs("one")
    sc = d.sc
    assert sc.n == 1
    rays, ref = sc.sets()["main"]
    assert 100 <= (ref["prim"] == 1).sum() <= len(ref) - 100
    got = _check_set(rtw, d, "main")
    cam, _, fhits, fsurf, want = sc.frame(S.SHUTTERS[0])
    g, _ = _device_guides(rtw, d, cam, None)
    _assert_words(g, want, "one: guides")
    assert (want["prim"] == 1).sum() >= 100 and (want["prim"] == 0).sum() >= 100
    surf, guides = _run_surface(rtw, d, Q.to_device(got), len(got))
    _assert_words(surf, S.scene_surface(rtw, oracle, sc, ref), "one: surface")
    _assert_words(guides, guides_of(rtw, ref, S.scene_surface(rtw, oracle, sc, ref), S.BACKGROUND), "one: surface guides")
