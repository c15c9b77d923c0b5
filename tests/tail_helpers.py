"""Shared pieces of tests/test_gpu_tail.py: scenes of the `scattered` kind and the check of
one frame against oracle Tier B with the counting pass's tail words."""
import numpy as np

from helpers import diff_stats, to_oracle_camera, to_oracle_scene


def spheres(rtw, specs):
    sph = (rtw.Sphere * len(specs))()
    for s, (c0, c1, r, t0, t1, mv, m) in zip(sph, specs):
        s.c0[:], s.c1[:] = c0, c1
        s.radius, s.t0, s.t1, s.moving, s.mat = r, t0, t1, mv, m
    return sph


def materials(rtw):
    """Ground checker, a Lambertian, a mirror (Metal, fuzz 0) and glass: long and short paths."""
    mats = (rtw.Material * 4)()
    mats[0].kind = rtw.LAMBERT_CHECKER
    mats[0].albedo[:] = (0.9, 0.9, 0.9)
    mats[0].albedo_odd[:] = (0.2, 0.3, 0.1)
    mats[1].kind = rtw.LAMBERT_SOLID
    mats[1].albedo[:] = (0.6, 0.3, 0.2)
    mats[2].kind, mats[2].fuzz = rtw.METAL, 0.0
    mats[2].albedo[:] = (0.8, 0.8, 0.7)
    mats[3].kind, mats[3].ir = rtw.DIELECTRIC, 1.5
    return mats


def scattered(rtw, n_narrow=24, seed=5, groups=((0.0, 1.0), (-0.5, 1.5))):
    """The ground and n_narrow small spheres, every other one glass or mirror; three of four move,
    along x, y or z, over the time ranges `groups` (both contain the shutter 0..1)."""
    rng = np.random.default_rng(seed)
    specs = [((0, -1000, 0), (0, -1000, 0), 1000.0, 0.0, 0.0, 0, 0)]
    for k in range(n_narrow):
        x, z = -5 + 10 * rng.random(), -5 + 10 * rng.random()
        r = 0.3 + 0.4 * rng.random()
        c0 = (x, r, z)
        mat = (2 + (k // 2) % 2) if k % 2 else 1
        if k % 4 == 0:
            specs.append((c0, c0, r, 0.0, 0.0, 0, mat))
            continue
        dv = [0.0, 0.0, 0.0]
        dv[k % 4 - 1] = 0.2 + 0.4 * rng.random()
        t0, t1 = groups[k % len(groups)]
        specs.append((c0, tuple(c + d for c, d in zip(c0, dv)), r, t0, t1, 1, mat))
    return spheres(rtw, specs)


def oracle_frame(oracle, osc, cam, **kw):
    """(image, stats) of oracle Tier B for make_params-style keywords."""
    okw = dict(kw)
    w, h, spp = okw.pop("width"), okw.pop("height"), okw.pop("spp")
    depth = okw.pop("max_depth", 50)
    return oracle.render_tier_b(osc, to_oracle_camera(oracle, cam), w, h, spp, depth=depth, **okw)


def check(rtw, oracle, rend, sph, mats, osc, cam, what, helped=True, **kw):
    """The f64 megakernel's frame == oracle Tier B on every channel (max|d| == 0); the counting
    pass traced every sample once and the oracle's number of segments; and the tail handed samples
    out (helped=True), or had none to hand out (False; None: either).  Returns (image, stats)."""
    import torch
    g = rend.render(cam, rtw.make_params(**kw))
    torch.cuda.synchronize()
    g = g.cpu().numpy()
    o, ost = oracle_frame(oracle, osc, cam, **kw)
    d = diff_stats(g, o)
    st = rend.stats(cam, rtw.make_params(**kw))
    print(what, d, {k: st[k] for k in ("samples", "segments", "primary_rounds", "tail_helped_samples",
                                        "tail_wave_iters", "tail_idle_lane_iters")})
    assert d["max"] == 0, (what, d)
    assert st["samples"] == g.shape[0] * g.shape[1] * kw["spp"] == ost["samples"], (what, st, ost)
    assert st["segments"] == ost["segments"], (what, st, ost)
    if helped:
        assert st["tail_helped_samples"] > 0 and st["tail_wave_iters"] > 0, (what, st)
    elif helped is not None:
        assert st["tail_helped_samples"] == 0, (what, st)
    return g, st
