"""Ray sets for the ray-query tests (tests/test_gpu_query.py), built on the CPU
from the oracle alone: the 24x14 feature rays of a camera, each with its own
time, and from every hit a bounce, an inward ray and a shadow ray.  Records
are numpy arrays of rtw_amd.HIT_DTYPE holding the oracle's rw_hit answers
(prim = list index + 1, a miss all zero), compared with the device's bit for bit."""
import numpy as np

from denoise_helpers import feature_ray

QW, QH = 24, 14  # the primary rays' frame


def oracle_hits(rtw, ow, rays):
    """OracleWorld.hit of every ray -> (n,) HIT_DTYPE (a miss: all zero)."""
    out = np.zeros(len(rays), rtw.HIT_DTYPE)
    for i, r in enumerate(rays):
        h = ow.hit([float(x) for x in r["origin"]], [float(x) for x in r["dir"]], float(r["time"]), float(r["t_min"]),
                   float(r["t_max"]))
        if h is None:
            continue
        out[i]["t"], out[i]["p"], out[i]["normal"] = h["t"], h["p"], h["normal"]
        out[i]["u"], out[i]["v"] = h["uv"]
        out[i]["prim"], out[i]["front"] = h["prim"] + 1, int(h["front"])
    return out


def make_rays(rtw, rows):
    """rows of (origin, dir, time, t_min, t_max) -> (n,) RAY_DTYPE."""
    r = np.zeros(len(rows), rtw.RAY_DTYPE)
    for i, (o, d, time, t_min, t_max) in enumerate(rows):
        r[i]["origin"], r[i]["dir"], r[i]["time"], r[i]["t_min"], r[i]["t_max"] = o, d, time, t_min, t_max
    return r


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.sqrt((v * v).sum())


def ray_set(rtw, ow, cam, look_from, seed):
    """(rays, kinds): (a) the QW x QH feature rays of `cam` with random times in [0, 1); from every hit
    of (a): (b) a bounce normal + 0.999 unit, (c) an inward ray -normal + 0.5 unit, (d) a shadow ray
    towards 0.5 look_from + (0, 3, 0) with t_max = 1.  kinds[i] in "abcd"."""
    rng = np.random.default_rng(seed)
    rows = []
    for y in range(QH):
        for x in range(QW):
            o, d, _ = feature_ray(cam, QW, QH, x, y)
            rows.append((o, d, float(rng.random()), 0.001, np.inf))
    prim = make_rays(rtw, rows)
    hits = oracle_hits(rtw, ow, prim)
    kinds = ["a"] * len(rows)
    target = 0.5 * np.array(look_from, float) + np.array([0.0, 3.0, 0.0])
    for r, h in zip(prim, hits):
        if h["prim"] == 0:
            continue
        p, n, time = np.array(h["p"]), np.array(h["normal"]), float(r["time"])
        rows.append((p, n + 0.999 * _unit(rng), time, 0.001, np.inf))
        rows.append((p, -n + 0.5 * _unit(rng), time, 0.001, np.inf))
        rows.append((p, target - p, time, 0.001, 1.0))
        kinds += ["b", "c", "d"]
    return make_rays(rtw, rows), np.array(kinds)


def check_conditions(rays, kinds, ref, moving_prims=None):
    """The conditions a ray set must meet so that the device cannot pass vacuously, on the oracle's answers."""
    hit = ref["prim"] > 0
    assert 0.10 <= hit.mean() <= 0.90, hit.mean()
    assert ((ref["front"] == 0) & hit).any()
    d = kinds == "d"
    assert (hit & d).any() and (~hit & d).any()
    if moving_prims is not None:
        assert np.isin(ref["prim"][hit] - 1, list(moving_prims)).any()


def words(a):
    """A record array's bytes as uint64 words (one row per record)."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64).reshape(len(a), -1)
