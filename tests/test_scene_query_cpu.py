"""The scene API's scenes and ray sets (tests/scene_query_helpers.py), the part that needs no GPU:
the census of the ORACLE's records, so that tests/test_gpu_scene_queries.py cannot pass on an empty
category — hits on static, moving and negative-radius spheres, on every time group, on movers at
times outside their ranges, on every coincident pair, on list sphere 4095; NaN and infinite roots
among the overflow rays; interval rays accepted exactly at t_max == root — and the two scenes the
packer must refuse."""
import types

import numpy as np
import pytest

import scene_query_helpers as S


@pytest.fixture(scope="module")
def scenes(rtw, oracle):
    def get(name):
        return S.get_scene(rtw, oracle, name)
    return get


def _all_refs(sc):
    return np.concatenate([ref for _, ref in sc.sets().values()])


@pytest.mark.parametrize("name", ["custom", "clustered", "ties", "limits", "one"])
def test_hits_on_every_kind_of_sphere(scenes, name):
    sc = scenes(name)
    w = S.winners(_all_refs(sc))
    kinds = {"static": ~sc.moving, "moving": sc.moving, "negative radius": sc.radius < 0.0}
    for what, mask in kinds.items():
        if mask.any():  # the scene has one
            assert mask[w].sum() >= 20, (name, what, int(mask[w].sum()))
    assert kinds["negative radius"].any() == (name == "custom")
    assert kinds["moving"].any() == (name != "one")
    main_rays, main_ref = sc.sets()["main"]
    S.Q.check_conditions(main_rays, sc.kinds, main_ref)


def test_set_sizes_and_empty_scene(scenes):
    for name in S.SCENES:
        sets = scenes(name).sets()
        assert (scenes(name).kinds == "a").sum() == S.FW * S.FH
        for t in S.TIMES:
            assert (sets[f"time{t}"][0]["time"] == t).all()
        assert ("overflow" in sets) == (name in S.OVERFLOW_SCENES) and ("ties" in sets) == (name == "ties")
    e = scenes("empty")
    assert e.n == 0 and all((ref["prim"] == 0).all() for _, ref in e.sets().values())
    assert scenes("one").n == 1 and scenes("ties").n == 40 and scenes("custom").n == 8 and scenes("clustered").n == 102


def test_clustered_time_groups(scenes):
    sc = scenes("clustered")
    groups = sc.time_groups()
    assert len(groups) == 3
    w = S.winners(_all_refs(sc))
    for t0, t1 in groups:
        n = (sc.moving[w] & (sc.t0[w] == t0) & (sc.t1[w] == t1)).sum()
        assert n >= 10, ((t0, t1), int(n))
    mid = 0.5 * (S.SHUTTERS[1][0] + S.SHUTTERS[1][1])
    # the second camera: its shutter leaves two of the groups, its guides' mid time 1.125 leaves [0, 1]
    assert sum(1 for t0, t1 in groups if S.SHUTTERS[1][1] > t1) == 2 and sum(1 for t0, t1 in groups if not t0 <= mid <= t1) == 1


@pytest.mark.parametrize("time", S.TIMES)
def test_movers_hit_outside_their_ranges(scenes, time):
    """Per time value: records whose winner is a mover and whose ray time lies outside that mover's own range."""
    total = {}
    for name in ("custom", "clustered", "ties", "limits"):
        sc = scenes(name)
        w = S.winners(sc.sets()[f"time{time}"][1])
        total[name] = int((sc.moving[w] & ((time < sc.t0[w]) | (sc.t1[w] < time))).sum())
    assert sum(total.values()) >= 10, (time, total)
    if time != 0.5:  # (custom's ranges are [0, 1] and [0.25, 0.75]: 0.5 lies inside both)
        assert total["custom"] >= 10, (time, total)
    if time not in (0.1, 0.5):  # (clustered's ranges all hold [0, 1])
        assert total["clustered"] >= 10, (time, total)
    assert total["limits"] >= 10, (time, total)


def test_ties_pairs(scenes):
    sc = scenes("ties")
    pos = sc.table_position()
    reversed_pairs = []
    for name, (i, j) in S.TIE_PAIRS.items():
        a, b = sc.sph[i], sc.sph[j]
        assert i < j and list(a.c0) == list(b.c0) and a.radius == b.radius and a.mat != b.mat
        if a.moving and b.moving:
            assert (list(a.c1), a.t0, a.t1) == (list(b.c1), b.t0, b.t1) and list(a.c1) != list(a.c0)
        for s in (a, b):
            if s.moving != (a.moving and b.moving):  # the mover of a mixed pair stands still
                assert not s.moving or list(s.c0) == list(s.c1)
        if pos[j] < pos[i]:
            reversed_pairs.append(name)
        ref = sc.sets()["ties"][1]
        got = [int(ref["prim"][r]) - 1 for r in sc.tie_rows[name]]
        assert any(g in (i, j) for g in got), (name, got)  # a ray whose oracle winner belongs to the pair ...
        assert all(g == j for g in got if g in (i, j)), (name, got)  # ... and it is the later list index
    assert reversed_pairs == ["C"]  # listed (mover, static): the table holds the static one first
    assert any(i < k < j for k in range(sc.n) for i, j in [S.TIE_PAIRS["A"]])
    assert (sc.moving[S.TIE_PAIRS["C"][0]], sc.moving[S.TIE_PAIRS["C"][1]]) == (True, False)
    assert (sc.moving[S.TIE_PAIRS["D"][0]], sc.moving[S.TIE_PAIRS["D"][1]]) == (False, True)


def test_limits_tops(rtw, scenes):
    sc = scenes("limits")
    assert sc.n == 4096 and len(sc.mats) == 4096
    groups = sc.time_groups()
    last = sc.sph[S.LIMITS_LAST]
    assert len(groups) == 64 and groups[63] == S.LIMITS_LAST_RANGE == (last.t0, last.t1) and last.mat == 4095
    assert sum(1 for s in sc.sph if s.moving and (s.t0, s.t1) == S.LIMITS_LAST_RANGE) == 1
    main_rays, main_ref = sc.sets()["main"]
    a = sc.kinds == "a"
    assert (main_ref["prim"][a] == S.LIMITS_LAST + 1).sum() >= 5
    for t in (0.1, 3.0):  # group 63's own range decides where the sphere is
        assert (sc.sets()[f"time{t}"][1]["prim"] == S.LIMITS_LAST + 1).sum() >= 5, t
        assert not last.t0 <= t <= last.t1


def test_limits_refusals(rtw):
    import ctypes as C
    L = rtw.lib()
    for kw, what in ((dict(extra_range=True), b"time ranges"), (dict(n=4097), b"4097 spheres")):
        sph, mats = S.limits_scene(rtw, **kw)
        h = C.c_void_p()
        assert L.rtw_scene_create(sph, len(sph), mats, len(mats), C.byref(h)) == rtw.RTW_UNSUPPORTED, kw
        assert not h and what in (L.rtw_last_error() or b""), (kw, L.rtw_last_error())


@pytest.mark.parametrize("name", S.OVERFLOW_SCENES)
def test_overflow_rays(scenes, name):
    sc = scenes(name)
    rays, ref = sc.sets()["overflow"]
    length = np.sqrt((np.ldexp(rays["dir"], -500) ** 2).sum(axis=1))  # (scaled: the square must not overflow here)
    big = length > 2.0 ** 19
    assert big.sum() >= 32 and (length[big] >= 2.0 ** 19.9).all() and (length[big] <= 2.0 ** 500.1).all()
    assert (np.abs(rays["origin"]).max(axis=1) > 2.0 ** 519).sum() >= 8  # origins of that size too
    assert np.isfinite(rays["dir"]).all() and (rays["dir"] != 0.0).all() and np.isfinite(rays["origin"]).all()
    tiny = ~big
    assert tiny.sum() == 8 and (np.abs(rays["dir"][tiny]).max(axis=1) < 2.0 ** -559).all()
    assert np.isnan(ref["t"]).sum() >= 16 and np.isinf(ref["t"]).sum() >= 4, (np.isnan(ref["t"]).sum(), np.isinf(ref["t"]).sum())
    # the reference accepts a NaN root, and after it every sphere whose discriminant is not negative: the last one wins
    assert (ref["prim"][np.isnan(ref["t"])] == sc.n).all()
    assert (ref["prim"][tiny] == 0).sum() >= 2  # the two directed away miss


@pytest.mark.parametrize("name", ["custom", "clustered", "ties", "limits", "one"])
def test_interval_variants(scenes, name):
    sc = scenes(name)
    sets = sc.sets()
    v1_rays, v1_ref = sets["V1"]
    assert ((v1_ref["prim"] > 0) & (v1_ref["t"] == v1_rays["t_max"])).sum() >= 20
    assert (sets["V2"][1]["prim"] == 0).all()  # t_max one ulp below the root: nothing nearer exists
    base = S.Q.words(sets["main"][1][S.Q.finite_hits(types.SimpleNamespace(ref=sets["main"][1]))])
    for v in ("V1", "V3", "V5"):
        assert (S.Q.words(sets[v][1]) == base).all(), (name, v)
    assert not (S.Q.words(sets["V4"][1]) == base).all(axis=1).any()


def test_inside_rays(scenes):
    sc = scenes("custom")
    rays, ref = sc.sets()["inside"]
    w = ref["prim"].astype(int) - 1
    assert (w[:48] == 2).sum() >= 40 and (ref["front"][:48][w[:48] == 2] == 1).all()  # from inside the hollow: its front face
    assert (w[48:] == 0).sum() >= 40 and (ref["front"][48:][w[48:] == 0] == 0).all()  # from inside the ground sphere
    for name in ("clustered", "ties", "limits", "one"):
        _, ref = scenes(name).sets()["inside"]
        assert ((ref["prim"] > 0) & (ref["front"] == 0)).sum() >= 40, name


def test_frames_census(scenes):
    """The guides' frames: both cameras see every material kind and the sky; the far checker records exist."""
    for name in ("custom", "clustered", "ties", "limits"):
        for sh in S.SHUTTERS:
            _, _, hits, surf, _ = scenes(name).frame(sh)
            kinds, counts = np.unique(surf["kind"], return_counts=True)
            assert list(kinds) == [0, 1, 2, 3] and counts.min() >= 20, (name, sh, counts)
            assert (surf["tex_kind"] == 2).sum() >= 100, (name, sh)  # checker records
