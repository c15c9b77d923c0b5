"""csrc/rtw_tri.hpp against exact rational arithmetic (tests/tri_exact.py), on the CPU.

tests/native/tri_exact_probe.cpp, built with g++ and no HIP, evaluates the header on (triangle, ray) pairs from a
file; tri_exact classifies every pair exactly: `in` must be accepted, `out` rejected, and an accepted pair's t,
point, u, v, front and normal must lie within DESIGN.md §22's bounds of the exact ones.  Ray sets: a ladder of
offsets 2^-20 .. 2^-54 of an edge length on both sides of edges and about vertices, rays exactly through vertices
and edge points and 1-3 ulps beside, over a tetrahedron, an icosahedron, a jittered level-2 icosphere, a 64-gon
bipyramid, a sliver strip of aspect 10^4 : 1, an icosahedron of size 2^-20 at offset ~1000 and the icosahedron at
scales 2^+-200; each ray against every triangle of its mesh it could touch (the whole fan of a vertex); and 2 x 10^4
random hits and misses.  The same rays go through rtw_world_trace_tri_host with each mesh under a chain of 1-4
ops.  The probe is rebuilt against the header with one line broken, five ways, and must be caught each time;
and runs once under the address and undefined-behaviour sanitizers."""
import math
import os
import re
import shutil
import subprocess
from collections import Counter

import numpy as np
import pytest

from conftest import PKG_ROOT, REPO
from helpers import _to_desc, chain_to_world
import tri_exact as X

CSRC = os.path.join(PKG_ROOT, "csrc")
SRC = os.path.join(REPO, "tests", "native", "tri_exact_probe.cpp")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off"]
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

LADDER_TRIS = {"tetrahedron": range(4), "icosahedron": range(0, 20, 2), "icosphere": range(0, 320, 16),
               "bipyramid": (0, 21, 64 + 40, 64 + 63), "sliver": range(8), "tiny": range(0, 20, 4),
               "icosahedron*2^200": range(0, 20, 5), "icosahedron*2^-200": range(0, 20, 5)}
DECIDED_RUNG = 36  # rungs k <= 36 must hold no band ray (the issue's condition on the ray sets)


def prims_of(v, f, xform=-1):
    return [dict(kind=5, mat=0, xform=xform, a=[float(x) for x in v[list(t)].reshape(9)]) for t in f]


class Case:
    """The pairs of the file: tris (nine doubles each), rays (tri, o, d) and their labels (mesh, rung, side)."""

    def __init__(self):
        self.tris, self.rays, self.labels, self.mesh_rays = [], [], [], {}
        M = dict(X.meshes())
        iv, if_, near = M["icosahedron"]
        M["icosahedron*2^200"], M["icosahedron*2^-200"] = (iv, if_, near), (iv, if_, near)
        self.meshes = {}
        for name, (v, f, near) in M.items():
            rows = []
            for i in LADDER_TRIS[name]:
                rows += X.ladder(v[f[i]], 100 + i, near)
                rows += X.exact_points(v[f[i]], 200 + i, near)
            o, d = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
            if "*" in name:  # (a power of two: every bit of the geometry is kept, only the exponents move)
                s = 2.0 ** (200 if name.endswith("^200") else -200)
                v, o, d = v * s, o * s, d * s
            world = X.World(prims_of(v, f), [])
            own = np.repeat(list(LADDER_TRIS[name]), len(rows) // len(LADDER_TRIS[name]))
            base = len(self.tris)
            self.tris += [t.a for t in world.tris]
            cand = world.candidates(o, d)
            self.mesh_rays[name] = (o, d, [r[2] for r in rows], [r[3] for r in rows], cand)
            self.meshes[name] = (v, f)
            for j, r in enumerate(rows):
                for k in sorted(set(cand[j]) | {int(own[j])}):
                    self.rays.append((base + k, o[j], d[j]))
                    self.labels.append((name, r[2], r[3] if k == own[j] else None))
        rng = np.random.default_rng(2024)  # 2 x 10^4 random hits and misses
        for _ in range(20000):
            tri = rng.uniform(-4, 4, (3, 3))
            b = rng.uniform(-0.5, 1.5, 2)
            tgt = tri[0] + b[0] * (tri[1] - tri[0]) + b[1] * (tri[2] - tri[0])
            o = tgt + rng.uniform(2, 30) * X._unit(rng.normal(size=3))
            self.rays.append((len(self.tris), o, (tgt - o) * float(rng.choice([1.0, 0.5, 3.0]))))
            self.labels.append(("random", None, None))
            self.tris.append(list(tri.reshape(9)))
        self.records = {}  # (built on first use, shared by the runs against the broken headers)
        self.exact = [X.classify(X.Tri(self.tris[i]), X.fr3(o), X.fr3(d)) for i, o, d in self.rays]

    def write(self, path):
        with open(path, "w") as f:
            for t in self.tris:
                f.write("T " + " ".join(float(x).hex() for x in t) + "\n")
            for i, o, d in self.rays:
                f.write(f"R {i} " + " ".join(float(x).hex() for x in (*o, *d)) + "\n")


@pytest.fixture(scope="module")
def case():
    return Case()


def _build(out_dir, inc=None, extra=()):
    exe = os.path.join(str(out_dir), "tri_exact_probe")
    incs = (["-I", str(inc)] if inc else []) + ["-I", CSRC]
    return exe, subprocess.run(["g++", *FLAGS, *extra, *incs, SRC, "-o", exe], capture_output=True, text=True)


def _run(exe, path):
    p = subprocess.run([exe, path], capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    rows = []
    for line in p.stdout.split("\n"):
        if line:
            w = line.split()
            rows.append(dict(ok=int(w[0]), inside=int(w[1]), hit=int(w[2]), t=float.fromhex(w[3]), u=float.fromhex(w[4]),
                             v=float.fromhex(w[5]), front=int(w[6]), normal=[float.fromhex(x) for x in w[7:10]]))
    return rows, p.stderr


def judge(case, rows, step=1):
    """The probe's lines against the exact classes and records: (violations, ratios, table); every step-th pair."""
    assert len(rows) == len(case.rays)
    bad, ratios, old, table = [], {}, {}, Counter()
    for j in range(0, len(rows), step):
        got, ex, lab = rows[j], case.exact[j], case.labels[j]
        if lab[2] is not None:
            table[(lab[0], lab[1], lab[2], ex.cls)] += 1
        table[(lab[0], "all", None, ex.cls)] += 1
        if not got["ok"]:
            bad.append((j, lab, "derive"))
        if ex.cls == "in" and not (got["inside"] and got["hit"]):
            bad.append((j, lab, "an exact inside ray is rejected"))
        if ex.cls == "out" and (got["inside"] or got["hit"]):
            bad.append((j, lab, "an out ray is accepted"))
        if got["hit"] and ex.t is not None:
            i, o, d = case.rays[j]
            got = dict(got, p=[float(o[c]) + float(d[c]) * got["t"] for c in range(3)])  # p = o + d t, as the kernels compute it
            key = lab[0] if "*" in lab[0] or lab[0] in ("tiny", "sliver") else "plain"
            r = ratios.setdefault(key, {})
            if j not in case.records:
                case.records[j] = X.Record(ex)
            for what in case.records[j].compare(got, r, old.setdefault(key, {})):
                bad.append((j, lab, what))
    return bad, ratios, old, table


def print_table(table, ratios, old):
    names = sorted({k[0] for k in table})
    print("per-rung classes, rays against their own triangle: mesh rung side in/out/band")
    for name in names:
        rungs = sorted({k[1] for k in table if k[0] == name and k[1] != "all" and k[1] is not None})
        for rung in rungs:
            cells = [f"{side:+d}:" + "/".join(str(table[(name, rung, side, c)]) for c in ("in", "out", "band"))
                     for side in (1, -1, 0) if any(table[(name, rung, side, c)] for c in ("in", "out", "band"))]
            print(f"  {name:22s} {rung:3d}  " + "  ".join(cells))
        print(f"  {name:22s} all pairs in/out/band " + "/".join(str(table[(name, 'all', None, c)]) for c in ("in", "out", "band")))
    for key in sorted(ratios):
        print("largest error / bound,", key, {k: float(f"{v:.3g}") for k, v in sorted(ratios[key].items())},
              "against §22's earlier p bound:", {k: float(f"{v:.3g}") for k, v in old.get(key, {}).items()})


@needs_gxx
def test_header_against_exact_rationals(case, tmp_path):
    path = str(tmp_path / "pairs.txt")
    case.write(path)
    exe, r = _build(tmp_path)
    assert r.returncode == 0, r.stderr
    rows, _ = _run(exe, path)
    bad, ratios, old, table = judge(case, rows)
    print_table(table, ratios, old)
    # the conditions on the sets: every class present, the rungs k <= 36 decided, exact aims exist
    for (name, rung, side, cls), n in table.items():
        if isinstance(rung, int) and rung >= 20 and side is not None and rung <= DECIDED_RUNG:
            assert cls != "band" or n == 0, (name, rung, side, n)
    assert sum(n for (m, r, s, c), n in table.items() if r == 0 and s == 0 and c == "in") >= 200  # exact aims, inside
    classes = Counter(e.cls for e in case.exact)
    assert classes["in"] > 20000 and classes["out"] > 20000 and classes["band"] > 500, classes
    assert len(case.rays) >= 60000
    assert not bad, (len(bad), bad[:8])
    assert all(v <= 1.0 for r in ratios.values() for v in r.values())


MUTANTS = [("0x1p-49", "0.0", "an exact inside ray is rejected"),
           ("0x1p-49", "0x1p-30", "an out ray is accepted"),
           ("bu = w1 / s, bv = w2 / s;", "bu = w2 / s, bv = w1 / s;", "u"),
           ("n[0] = Nx / s + 0.0, n[1] = Ny / s + 0.0, n[2] = Nz / s + 0.0;",
            "n[0] = Nx + 0.0, n[1] = Ny + 0.0, n[2] = Nz + 0.0;", "normal"),
           ("t = (h - (nx * ox + ny * oy + nz * oz)) / nd;", "t = ((nx * ox + ny * oy + nz * oz) - h) / nd;", "t")]


@needs_gxx
@pytest.mark.parametrize("old,new,what", MUTANTS)
def test_the_comparison_has_teeth(case, tmp_path, old, new, what):
    """One line of the header broken: tau 0 (a vertex ray that is inside in exact arithmetic is rejected), tau
    2^-30 (an `out` ray on a decided rung is accepted), u and v exchanged, the normal left unnormalised, the
    plane root's sign."""
    src = open(os.path.join(CSRC, "rtw_tri.hpp")).read()
    assert src.count(old) == 1
    d = tmp_path / "broken"
    d.mkdir()
    (d / "rtw_tri.hpp").write_text(src.replace(old, new))
    path = str(tmp_path / "pairs.txt")
    case.write(path)
    exe, r = _build(d, inc=d)
    assert r.returncode == 0, r.stderr
    rows, _ = _run(exe, path)
    bad, _, _, _ = judge(case, rows, step=3)  # (a third of the pairs is enough to catch each)
    found = [b for b in bad if (b[2] == what if isinstance(b[2], str) else b[2][0] == what)]
    assert found, (what, bad[:5])
    if new == "0.0":  # among them a ray about a vertex
        assert any(b[1][1] is not None and (b[1][1] >= 38 or b[1][1] <= 1) for b in found), found[:5]
    if new == "0x1p-30":  # among them a ladder ray of a decided rung
        assert any(b[1][1] is not None and 20 <= b[1][1] <= DECIDED_RUNG and b[1][2] == -1 for b in found), found[:5]


@needs_gxx
def test_probe_clean_under_host_sanitizers(case, tmp_path):
    exe, r = _build(tmp_path, extra=["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", r.stderr):
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr
    path = str(tmp_path / "pairs.txt")
    case.write(path)
    rows, err = _run(exe, path)
    assert len(rows) == len(case.rays) and "ERROR: AddressSanitizer" not in err and "runtime error" not in err, err


# ------------------------------------------------------------------ the library's host entry ----
CHAINS = {"tetrahedron": [(1, 0.7)], "icosahedron": [(0, (1.5, -0.25, 2.0)), (1, -0.4)],
          "icosphere": [(1, 0.9), (0, (-2.0, 0.5, 1.25)), (1, -1.1)],
          "bipyramid": [(0, (0.5, 1.0, -1.5)), (1, 0.35), (0, (2.0, 0.0, 0.75)), (1, 1.2)],
          "sliver": [(1, -0.6), (0, (1.0, 0.5, -0.5))], "tiny": [(0, (3.0, 0.5, -2.0))],
          "icosahedron*2^200": [(1, 0.5)], "icosahedron*2^-200": [(1, -0.8), (1, 0.3)]}


def make_chain(ops):
    """[(op, value)] -> the description's transform: an offset, or (sin, cos, angle)."""
    return dict(n=len(ops), op=[o for o, _ in ops],
                v=[tuple(float(x) for x in a) if o == 0 else (math.sin(a), math.cos(a), float(a)) for o, a in ops])


def check_world(rtw, W, ex_world, desc, rays, ratios, stats, label):
    """rtw_world_trace_tri_host over `rays` against the exact traces of ex_world."""
    got = W.trace_tri_host(desc, rays)
    bad = []
    for j, tr in enumerate(ex_world.trace(rays)):
        g = got[j]
        k = int(g["prim"]) - 1
        stats["rays"] += 1
        stats["decided"] += tr.decided
        if tr.decided:
            want = -1 if tr.hit is None else ex_world.rows[tr.hit]
            if k != want:
                bad.append((label, j, "prim", k, want))
                continue
        elif tr.must_hit and k < 0:
            bad.append((label, j, "a ray with an inside triangle in its interval misses"))
        if k >= 0:
            idx = ex_world.rows.index(k)
            if idx not in tr.allowed:
                bad.append((label, j, "an out triangle is returned", k))
                continue
            for what in tr.allowed[idx].compare(g, ratios):
                bad.append((label, j, what))
    return bad


RANDOM_CHAINS = [[(1, 2.4)], [(0, (-3.0, 1.0, 0.5)), (1, -0.9)], [(1, 0.2), (1, 1.3), (0, (0.25, -2.0, 4.0))],
                 [(1, -1.7), (0, (5.0, 0.0, -1.0)), (0, (-0.5, 2.5, 0.75)), (1, 0.6)]]
N_RANDOM_HOST = 4000  # of the file's 2 x 10^4 random pairs, twenty triangles to a world (the rest cost time, not coverage)


def test_host_entry_against_exact_rationals(rtw, case):
    """Every mesh of the file under its own chain (1-4 ops, Translate and RotateY mixed), its rays moved to
    world space with the chain; the 2^+-200 meshes under rotations only.  Then random triangles of the file, twenty
    to a world (they overlap: a ray meets several), the worlds under four more chains in turn."""
    from rtw_amd import world as W
    assert {len(c) for c in CHAINS.values()} == {1, 2, 3, 4} == {len(c) for c in RANDOM_CHAINS}  # up to RTW_MAX_XFORM_OPS
    ratios, stats, bad = {}, Counter(), []
    tex, mats = [dict(kind=W.TEX_SOLID, color=(0.5, 0.5, 0.5))], [dict(kind=W.WMAT_LAMBERT, tex=0)]

    def run(label, key, prims, xf, o, d):
        zero = dict(xf, v=[(0.0, 0.0, 0.0) if op == 0 else val for op, val in zip(xf["op"], xf["v"])])
        rays = np.zeros(len(o), rtw.RAY_DTYPE)
        for j in range(len(o)):
            rays[j]["origin"], rays[j]["dir"], rays[j]["t_max"] = chain_to_world(xf, o[j]), chain_to_world(zero, d[j]), np.inf
        desc, keep = _to_desc(W, prims, [xf], tex, mats, [], [])
        return check_world(rtw, W, X.World(prims, [xf]), desc, rays, ratios.setdefault(key, {}), stats, label)

    for name, (v, f) in case.meshes.items():
        o, d, rung, side, cand = case.mesh_rays[name]
        bad += run(name, "chained" if "*" not in name else name, prims_of(v, f, 0), make_chain(CHAINS[name]), o, d)
    rnd = [j for j, lab in enumerate(case.labels) if lab[0] == "random"][:N_RANDOM_HOST]
    for b in range(0, len(rnd), 20):
        js = rnd[b:b + 20]
        prims = [dict(kind=5, mat=0, xform=0, a=[float(x) for x in case.tris[case.rays[j][0]]]) for j in js]
        bad += run(("random", b), "random chained", prims, make_chain(RANDOM_CHAINS[(b // 20) % 4]),
                   [case.rays[j][1] for j in js], [case.rays[j][2] for j in js])
    print("host entry:", dict(stats), {k: {q: float(f"{x:.3g}") for q, x in sorted(v.items())} for k, v in ratios.items()})
    assert stats["decided"] >= 0.5 * stats["rays"]
    assert not bad, (len(bad), bad[:8])
