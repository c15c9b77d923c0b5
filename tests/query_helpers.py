"""Ray sets for the ray-query tests (tests/test_gpu_query.py,
tests/test_gpu_query_edges.py, tests/test_query_cpu.py), built on the CPU from
the oracle alone: the 24x14 feature rays of a camera, each with its own time,
and from every hit a bounce, an inward ray and a shadow ray.  Records are numpy
arrays of rtw_amd.HIT_DTYPE holding the oracle's rw_hit answers (prim = list
index + 1, a miss all zero), compared with the device's bit for bit.

World: one world on both sides (the device's, lazily; the oracle's) with its
ray set and the oracle's records; get_world() builds each once per process.
The edge sets (derive()): index vectors of batches larger than the device,
times outside [0, 1], the ends of [t_min, t_max], far origins, scaled
directions, axis-aligned rays through every kind of surface and direction
components below box_dir's threshold; their conditions are
tests/test_query_cpu.py's."""
import numpy as np

from denoise_helpers import feature_ray
from helpers import MIXED_CAMERA, MIXED_SIZES, _to_desc, chain_to_world, mixed_bvh_world

QW, QH = 24, 14  # the primary rays' frame

SKY = (0.7, 0.8, 1.0)
GEN_SEED = 5  # mixed_bvh_world's seed (as tests/test_gpu_world_general.py)
MIXED = {"small": (*MIXED_SIZES["small"], None, False, 100), "small_swap": (*MIXED_SIZES["small"], None, True, 100),
         "spheres_image": (0, 520, "spheres_image", False, 101)}


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


def ray_set(rtw, ow, cam, look_from, seed, w=QW, h=QH):
    """(rays, kinds): (a) the w x h (QW x QH) feature rays of `cam` with random times in [0, 1); from every hit
    of (a): (b) a bounce normal + 0.999 unit, (c) an inward ray -normal + 0.5 unit, (d) a shadow ray
    towards 0.5 look_from + (0, 3, 0) with t_max = 1.  kinds[i] in "abcd"."""
    rng = np.random.default_rng(seed)
    rows = []
    for y in range(h):
        for x in range(w):
            o, d, _ = feature_ray(cam, w, h, x, y)
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


def _pair_rays(W, tables, look_from, rng):
    """For each coincident-pair class of a mixed world, rays aimed at the pair: from the camera origin and
    from one unit in front of its surface.  Returns (rows, [(class, later list index, [row indices])])."""
    prims, xf = tables[0], tables[1]
    rows, want = [], []
    for cls in ("pair_rect", "pair_sphere", "pair_face"):
        idx = [i for i, p in enumerate(prims) if p["cls"] == cls]
        if not idx:
            continue
        first = prims[idx[0]]
        same = [i for i in idx if (prims[i]["kind"], list(prims[i]["a"]), prims[i]["xform"]) ==
                (first["kind"], list(first["a"]), first["xform"])]
        assert len(same) >= 2, cls
        a = first["a"]
        if first["kind"] == W.PRIM_SPHERE:
            c, r = np.array(a[0:3]), a[6]
            to_cam = np.array(look_from) - c
            to_cam /= np.sqrt((to_cam * to_cam).sum())
            centre, front = c + r * to_cam, c + (r + 1.0) * to_cam
        else:  # an XY rect, facing +z in its object space
            mid = np.array([(a[0] + a[1]) / 2, (a[2] + a[3]) / 2, a[4]])
            centre, front = mid, mid + np.array([0.0, 0.0, 1.0])
            if first["xform"] >= 0:
                centre, front = chain_to_world(xf[first["xform"]], centre), chain_to_world(xf[first["xform"]], front)
        mine = []
        for o in (np.array(look_from, float), front):
            mine.append(len(rows))
            rows.append((o, centre - o, float(rng.random()), 0.001, np.inf))
        want.append((cls, max(same), mine))
    return rows, want


class World:
    """One world: the device's, the oracle's, the ray set and the oracle's records (computed once, read-only)."""

    def __init__(self, rtw, oracle, W, name):
        self.name = name
        self.pairs, extra = [], []
        if name.startswith("scene"):
            sid = int(name[5:])
            img = W.synthetic_world_map() if sid in (4, 7) else None
            self.built = W.BuiltScene(sid, 42, img)
            self.desc = self.built.desc
            self.oracle = oracle.OracleWorld(sid, 42, img)
            cam = self.built.camera(QW / QH)
            look_from, seed = tuple(self.built.settings.look_from), 1234 + sid
            self.moving = [i for i in range(self.desc.n_prims) if self.desc.prims[i].kind == W.PRIM_MOVING_SPHERE]
            if sid == 6:  # direction components exactly 0, from inside the box; then the ray in the back wall's plane
                rng = np.random.default_rng(99)
                for o in ((278.0, 278.0, 10.0), (100.0, 400.0, 300.0), (500.0, 50.0, 540.0)):
                    for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1)):
                        extra.append((o, tuple(float(x) for x in d), float(rng.random()), 0.001, np.inf))
                extra.append(((100.0, 100.0, 555.0), (1.0, 0.5, 0.0), 0.5, 0.001, np.inf))
        else:
            nb, ns, variant, swap, k = MIXED[name]
            self.tables = mixed_bvh_world(W, W.earth_map(), nb, ns, GEN_SEED, swap=swap, variant=variant)
            self.desc, self._keep = _to_desc(W, *self.tables)
            self.oracle = oracle.TableWorld(*self.tables, background=SKY)
            m = MIXED_CAMERA
            cam = rtw.camera_init(m["look_from"], m["look_at"], (0, 1, 0), m["vfov"], QW / QH, m["aperture"],
                                  m["focus"], 0.0, 1.0)
            look_from, seed = m["look_from"], 1234 + k
            self.moving = []
            extra, self.pairs = _pair_rays(W, self.tables, look_from, np.random.default_rng(7))
        rays, kinds = ray_set(rtw, self.oracle, cam, look_from, seed)
        self.n_main = len(rays)
        if extra:
            rays = np.concatenate([rays, make_rays(rtw, extra)])
            kinds = np.concatenate([kinds, np.array(["x"] * len(extra))])
        self.rays, self.kinds = rays, kinds
        self.ref = oracle_hits(rtw, self.oracle, rays)
        self.rays.setflags(write=False)
        self.ref.setflags(write=False)
        self._W, self._dev, self._d_rays = W, None, None
        self._rtw, self._sets = rtw, {}

    @property
    def dev(self):
        if self._dev is None:
            self._dev = self._W.DeviceWorld(self.desc)
        return self._dev

    @property
    def d_rays(self):
        if self._d_rays is None:
            self._d_rays = to_device(self.rays)
        return self._d_rays

    def derive(self, key, *args):
        """(rays, oracle records) of the edge set `key` (EDGE_SETS), built and answered once, read-only."""
        k = (key, *args)
        if k not in self._sets:
            rays = EDGE_SETS[key](self, *args)
            ref = oracle_hits(self._rtw, self.oracle, rays)
            rays.setflags(write=False)
            ref.setflags(write=False)
            self._sets[k] = (rays, ref)
        return self._sets[k]


_WORLDS = {}


def get_world(rtw, oracle, W, name):
    """The World `name`, built once per process (the test modules share it)."""
    if name not in _WORLDS:
        _WORLDS[name] = World(rtw, oracle, W, name)
    return _WORLDS[name]


def to_device(rays):
    """A record array's bytes as a uint8 tensor on the GPU."""
    import torch
    return torch.from_numpy(np.frombuffer(rays.tobytes(), np.uint8).copy()).cuda()


def _trace(rtw, target, d_rays, n, opts=None, occluded=False, is_world=True):
    """n rays through the pointer API into a buffer pre-filled with 0xA5, with a 256-byte guard behind
    the last record (or byte).  Returns (records or bytes, guard)."""
    import torch
    size = n * (1 if occluded else 80)
    buf = torch.full((size + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    f = target.occluded if occluded else target.trace
    if is_world:
        f(d_rays.data_ptr(), n, buf.data_ptr(), opts, stream)
    else:
        f(d_rays.data_ptr(), n, buf.data_ptr(), stream)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    out = host[:size].copy()
    return (out if occluded else out.view(rtw.HIT_DTYPE)), host[size:]


def _assert_records(got, ref, where):
    """Bit for bit, except a record whose oracle root is NaN (a ray in a rect's plane): prim, and t NaN on both sides."""
    nan = np.isnan(ref["t"])
    assert (got["prim"] == ref["prim"]).all(), where
    assert np.isnan(got["t"][nan]).all(), where
    gw, rw = words(got)[~nan], words(ref)[~nan]
    bad = np.nonzero((gw != rw).any(axis=1))[0]
    assert bad.size == 0, (where, bad[:5], got[~nan][bad[:2]], ref[~nan][bad[:2]])


# ---------------------------------------------------------------- edge sets --

def verified(w):
    """A world's verified set without the row whose oracle root is NaN (scene 6's ray in a rect's plane):
    (rays, records, kinds)."""
    ok = ~np.isnan(w.ref["t"])
    return w.rays[ok], w.ref[ok], w.kinds[ok]


def big_index(kinds, ref, n, order, seed):
    """The index vector of an n-ray batch drawn from a verified set.  "random": uniform draws.
    "stragglers": lane 0 of every 64-ray block a kind-b/c ray that hits, the other 63 lanes kind-d rays
    that miss (t_max = 1: short walks next to one long one)."""
    rng = np.random.default_rng(seed)
    if order == "random":
        return rng.integers(0, len(kinds), n)
    assert order == "stragglers"
    hit = ref["prim"] > 0
    long_ = np.nonzero(hit & ((kinds == "b") | (kinds == "c")))[0]
    short = np.nonzero(~hit & (kinds == "d"))[0]
    assert len(long_) >= 8 and len(short) >= 8, (len(long_), len(short))
    idx = short[rng.integers(0, len(short), n)]
    lane0 = np.arange(0, n, 64)
    idx[lane0] = long_[rng.integers(0, len(long_), len(lane0))]
    return idx


TIMES_OUTSIDE = (-0.75, 1.5, 3.0)


def _set_time(w, time):
    """w.rays at another time; "mixed": lanes alternate between their own time and 1.5."""
    r = w.rays.copy()
    if time == "mixed":
        r["time"][1::2] = 1.5
    else:
        r["time"] = time
    return r


def finite_hits(w):
    """Rows of the verified set whose oracle answer is a hit at a finite t."""
    return np.nonzero((w.ref["prim"] > 0) & np.isfinite(w.ref["t"]))[0]


def _interval(w, variant):
    """The rays that hit at a finite t, with an end of [t_min, t_max] moved onto the root t or next to it."""
    rows = finite_hits(w)
    r, t = w.rays[rows].copy(), w.ref["t"][rows]
    if variant == "V1":
        r["t_max"] = t
    elif variant == "V2":
        r["t_max"] = np.nextafter(t, 0.0)
    elif variant == "V3":
        r["t_min"] = t
    elif variant == "V4":
        r["t_min"] = np.nextafter(t, np.inf)
    else:
        assert variant == "V5"
        r["t_min"], r["t_max"] = t, t
    return r


def _plain_interval(w):
    """From the bounce and inward rays (they start on a surface): t_min = 0, the self-hit root; a negative
    t_min, surfaces behind the origin; t_max = 1e300."""
    rows = np.nonzero((w.kinds == "b") | (w.kinds == "c"))[0][:96]
    a, b, c = w.rays[rows].copy(), w.rays[rows].copy(), w.rays[rows].copy()
    a["t_min"] = 0.0
    b["t_min"] = -1.0
    c["t_max"] = 1e300
    return np.concatenate([a, b, c])


def _a_hits(w):
    """The kind-a hits: (rays, hit points, unit directions)."""
    rows = np.nonzero((w.kinds == "a") & (w.ref["prim"] > 0))[0]
    r = w.rays[rows]
    d = r["dir"]
    return r, w.ref["p"][rows], d / np.sqrt((d * d).sum(axis=1))[:, None]


FAR_D = (1e3, 1e5, 1e7)


def _far(w, D):
    """Towards each hit point from D away, the direction scaled by 2^k, k uniform in [-40, 40]."""
    rng = np.random.default_rng(4100 + int(np.log10(D)))
    r, p, u = _a_hits(w)
    r = r.copy()
    k = rng.integers(-40, 41, len(r))
    r["origin"] = p - D * u
    r["dir"] = u * np.ldexp(1.0, k)[:, None]
    return r


def far_hit_rows(w, D):
    """Rows of the far set whose oracle answer is a hit."""
    return np.nonzero(w.derive("far", D)[1]["prim"] > 0)[0]


def _far_ends(w, D):
    """The far rays that hit, with t_max on the root (even rows) or t_min = t_max on it (odd rows): the
    largest roots, so the largest f32 roundings of the closest, a box test can meet at an interval's end."""
    rays, ref = w.derive("far", D)
    rows = far_hit_rows(w, D)
    r, t = rays[rows].copy(), ref["t"][rows]
    r["t_max"] = t
    r["t_min"][1::2] = t[1::2]
    return r


def _scaled(w):
    """The world's own origins, the direction scaled by 2^k, k in +-[80, 100]; t_min scaled the other way
    (0.001 * 2^-k), so the interval holds the same points."""
    rng = np.random.default_rng(4200)
    r, _, u = _a_hits(w)
    r = r.copy()
    k = rng.integers(80, 101, len(r)) * np.where(np.arange(len(r)) % 2, -1, 1)
    r["dir"] = u * np.ldexp(1.0, k)[:, None]
    r["t_min"] = np.ldexp(0.001, -k)
    return r


AXIS_OFFSET = (0.0137, 0.0071, -0.0113)  # (keeps the rays out of a rect's plane: the reference's 0/0 case)


def _axis(w):
    """Six rays along +-x, +-y, +-z through a point next to each hit point, from 2.5 away; the other two
    components +0 or -0; lengths and t_max as test_gpu_query.py's _axis_rays."""
    r, p, _ = _a_hits(w)
    rows = []
    for j, (ray, q) in enumerate(zip(r, p + np.array(AXIS_OFFSET))):
        z = -0.0 if j % 2 else 0.0
        for axis in range(3):
            for s in (1.0, -1.0):
                o, d = q.copy(), np.array([z, z, z])
                o[axis] += s * 2.5
                d[axis] = -s * (1.0 + 0.25 * (j % 3))
                rows.append((o, d, float(ray["time"]), 0.001, np.inf if j % 4 else 3.0))
    return make_rays(w._rtw, rows)


def _tiny(w):
    """Through each hit point from one direction's length before it, one component (never the largest)
    replaced by +-max|d| * 2^-(61 + 100 j), j in 0..4: non-zero and below box_dir's threshold."""
    r, p, _ = _a_hits(w)
    out = []
    for j in range(5):
        q = r.copy()
        d = q["dir"]
        big = np.abs(d).max(axis=1)
        i = np.arange(len(q))
        comp = (np.abs(d).argmax(axis=1) + 1 + (i + j) % 2) % 3
        d[i, comp] = np.where(i % 4 < 2, 1.0, -1.0) * big * np.ldexp(1.0, -(61 + 100 * j))
        q["origin"] = p - d
        out.append(q)
    return np.concatenate(out)


EDGE_SETS = {"time": _set_time, "interval": _interval, "plain": _plain_interval, "far": _far, "far_ends": _far_ends,
             "scaled": _scaled, "axis": _axis, "tiny": _tiny}
