"""An exact reference for the triangle primitive (csrc/rtw_tri.hpp), in rational arithmetic.

Doubles are dyadic rationals, so every quantity of a ray / triangle intersection is a Fraction with no
rounding at all.  The arithmetic below uses Python integers and fractions.Fraction only: the numbers of one
(ray, triangle) pair are Fraction(float) values multiplied by one common power of two, which makes them
integers (the expressions are homogeneous, so the power cancels or is carried as `scale`).  numpy appears
only in World.candidates, a prefilter that discards triangles a ray misses by a margin more than 30 times
larger than anything the classification below could call close; it decides nothing else.

For the object-space ray (o, d) and the vertices v0, v1, v2:
  A, B, C = v_i - o (unrounded);  w0 = d.(BxC), w1 = d.(CxA), w2 = d.(AxB);
  T_i = 2^-49 sum_j |d_j| (|P_k Q_l| + |P_l Q_k|)            (the header's tau, on the unrounded terms)
  N = (v1 - v0) x (v2 - v0);  t = N.(v0 - o) / N.d;  u = w1 / S, v = w2 / S, S = w0 + w1 + w2.

Classification of one triangle (G_i = 0 without a chain):
  in    all w_i >= G_i or all w_i <= -G_i, and |N.d| > e_d |N|_1
  out   some w_a < -(2 T_a + G_a) and some w_b > 2 T_b + G_b
  band  anything else.
Why 2 T is enough.  The code computes w~_i from A~ = fl(v0 - o) etc.: one rounding per difference, so every
product P_k Q_l of the edge function is off by a factor (1 + e)^2, |e| <= u = 2^-53, and the edge function
by at most (2u + u^2) sum |d_j| (|P_k Q_l| + |P_l Q_k|) = (2u + u^2) 2^49 T < T / 8: this is the term the
rounding of v - o adds.  On the rounded differences the header's own count (seven roundings per term)
gives 7u 2^49 T = 7 T / 16.  So |w~_i - w_i| <= 9 T / 16 (1 + 2^-50), and the float tau~ is T (1 + e)^8.
An `in` triangle has w~_i >= -9 T / 16 > -tau~: accepted.  An `out` one has w~_a < -2 T + 9 T / 16 < -tau~
and w~_b > tau~: both clauses of the inside test fail.  Between them the code may go either way.

Chains.  to_object (rtw_tri_host.cpp, rtw_world_walk.hpp) runs the description's ops 0 .. n-1 on the ray in
doubles.  chain_ray maps the ray with the description's (sn, cs) and offsets exactly, and carries a bound
e_o (e_d) on the largest component error of the float origin (direction) against the exact one:
  Translate  o' = fl(o - v):                        e' = e + u (|o'|_inf + e)
  RotateY    o'_x = fl(fl(cs o_x) - fl(sn o_z)):    e' = (|cs| + |sn|) (e + 2.01 u (max(|o_x|, |o_z|) + e))
(two products and a difference: each product's rounding is u |cs o_x| and the difference's u |o'_x|, which
the two products bound; the input error passes through the row's absolute sum), and the same for d.
Both vertices of an edge move by the same origin error D, and (P - D) x (Q - D) = P x Q - D x (Q - P)
exactly, so with E = Q - P
  G = e_d |P x Q|_1 + e_o sum_j |d_j| (|E_k| + |E_l|) + 2 e_d e_o |E|_1
bounds the change of the edge function.  Both band edges move out by G.

Records.  With L = max |v_i - o|, M = max(|v_i|, |o|), E the longest edge, k = K / |N|_inf the shape factor
of the normal (below), all norms Euclidean and rounded up:
  t      |t - t_exact| |d| <= 16 u (M + k E) |d| / |n.d|.  The root is fl((h - fl(n.o)) / fl(n.d)) with h = fl(n.v0):
         the two dot products of absolute coordinates carry 3u |v0| and 3u |o|, the difference u L, the
         denominator 3u |d| and the division u, both relative to a t with |t d| <= L; with L <= 2 M that is
         16 u M |d| / |n.d|.  The stored normal is off the true one by at most 5u k across the plane (the part
         along n moves no root), which tilts the plane about v0: 5u k E |d| / |n.d| at a point of the triangle.
  p      |p - p_exact| <= the same + 3u M (the product d t and the sum o + d t).  DESIGN.md §22 stated
         16 u L |d| / |n.d| before this reference existed; that misses the coordinates' magnitude (a small
         triangle far from the origin) and is reported next to the bound as `p_old`.
  u, v   <= 126 u |d| L^2 / |S|
  normal the float N_j is off by at most 4u K_j, K_j = |e1_k e2_l| + |e1_l e2_k| (three roundings per
         product, one for the difference), its length by 4u K / |N| (K = K_x + K_y + K_z) relative plus 5u for
         the squares, the sums, the root and the division; so n_j = (s N_j + a_j) / |N| with s = +-1 the
         facing sign and |a_j| <= A_j = 4u K_j + |N_j| (4u K / |N|_inf + 5u).  Without a square root:
         |n_j^2 (N.N) - N_j^2| <= 2 |N_j| A_j + A_j^2,   |n.n - 1 - g| <= (2 sum |N_j| A_j + sum A_j^2) / N.N
         with g = 0; and n . (s N) > 0, and n_j has the sign of s N_j wherever |N_j| > A_j.
Chained triangles add: to t, dt = |N|_1 (e_o + |t| e_d) / (|N.d| - |N|_1 e_d); to the object-space point
e_o + |t| e_d + (|d|_inf + e_d) dt; then to_world's roundings by the recurrences above on the point, and on
the normal alpha' = (|cs| + |sn|) max(alpha_x, alpha_z) + 3 sqrt(3) u per RotateY; the reference point and normal are the
exact to_world of the exact object-space ones (the description's (sn, cs) need not lie on the unit circle:
g = N_world . N_world / N.N - 1 exactly); to u, v: (G_i + G_0 + G_1 + G_2) / (|S| - G_0 - G_1 - G_2).
"""
import math
from fractions import Fraction as Fr

import numpy as np

U = Fr(1, 2 ** 53)
SLACK = 1 + Fr(1, 2 ** 20)  # second-order terms of the first-order bounds above
XF_TRANSLATE, XF_ROTATE_Y = 0, 1


def fr3(x):
    return tuple(Fr(float(c)) for c in x)


def _den(fs):
    return max(f.denominator for f in fs)


def _ints(fs, D):
    return [f.numerator * (D // f.denominator) for f in fs]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def sqrt_up(x):
    """An upper bound on sqrt(x), x a non-negative Fraction or int, within 2^-100 relative."""
    x = Fr(x)
    if x == 0:
        return Fr(0)
    n, d = x.numerator, x.denominator
    s = max(0, 120 - (n * d).bit_length() // 2)
    return Fr(math.isqrt(n * d << (2 * s)) + 1, d << s)


# ------------------------------------------------------------------------------- chains ----
def chain_ray(xf, o, d):
    """The world ray (o, d) (Fractions) in the object space of the chain `xf` (dict n, op, v; None: no chain),
    exactly, with the bounds (e_o, e_d) on the float to_object's component errors."""
    e_o = e_d = Fr(0)
    if xf is None:
        return o, d, e_o, e_d
    for k in range(xf["n"]):
        v = fr3(xf["v"][k])
        if xf["op"][k] == XF_TRANSLATE:
            o = _sub(o, v)
            e_o = e_o + U * (max(abs(c) for c in o) + e_o)
        else:
            sn, cs = v[0], v[1]
            r = abs(cs) + abs(sn)
            e_o = r * (e_o + Fr(201, 100) * U * (max(abs(o[0]), abs(o[2])) + e_o))
            e_d = r * (e_d + Fr(201, 100) * U * (max(abs(d[0]), abs(d[2])) + e_d))
            o = (cs * o[0] - sn * o[2], o[1], sn * o[0] + cs * o[2])
            d = (cs * d[0] - sn * d[2], d[1], sn * d[0] + cs * d[2])
    return o, d, e_o, e_d


def chain_world(xf, p, n):
    """to_world, exactly: the object-space point p and normal n (Fractions) in world space."""
    for k in reversed(range(xf["n"])):
        v = fr3(xf["v"][k])
        if xf["op"][k] == XF_TRANSLATE:
            p = (p[0] + v[0], p[1] + v[1], p[2] + v[2])
        else:
            sn, cs = v[0], v[1]
            p = (cs * p[0] + sn * p[2], p[1], -sn * p[0] + cs * p[2])
            n = (cs * n[0] + sn * n[2], n[1], -sn * n[0] + cs * n[2])
    return p, n


def chain_world_bounds(xf, p, e_p, alpha):
    """The float to_world's error bounds: e_p (per component of the point, given the object-space bound) and
    alpha (of the unit normal's components), by the recurrences of the module's head; p is the object-space
    point in doubles (it enters through its magnitude only, and the bounds are rounded up by 1e-9)."""
    alpha, p = list(alpha), list(p)
    for k in reversed(range(xf["n"])):
        v = xf["v"][k]
        if xf["op"][k] == XF_TRANSLATE:
            p = [p[0] + v[0], p[1] + v[1], p[2] + v[2]]
            e_p = e_p + 2.0 ** -53 * (max(abs(c) for c in p) + e_p) * (1 + 1e-9)
        else:
            sn, cs = v[0], v[1]
            r = (abs(cs) + abs(sn)) * (1 + 1e-9)
            e_p = r * (e_p + 2.01 * 2.0 ** -53 * (max(abs(p[0]), abs(p[2])) + e_p))
            alpha[0] = alpha[2] = r * max(alpha[0], alpha[2]) + 3 * 2.0 ** -53 * 1.7321
            p = [cs * p[0] + sn * p[2], p[1], -sn * p[0] + cs * p[2]]
    return e_p, alpha


# ------------------------------------------------------------------------ one triangle ----
class Tri:
    """A triangle's vertices (nine doubles) as Fractions; xf its chain or None."""

    def __init__(self, a, xf=None):
        self.a = [float(x) for x in a]
        self.v = [Fr(x) for x in self.a]
        self.den = _den(self.v)
        self.xf = xf


class Pair:
    """One (ray, triangle) pair, classified.  cls in ("in", "out", "band"); t is None when N.d == 0."""
    __slots__ = ("tri", "o", "d", "e_o", "e_d", "cls", "t", "w", "T49", "G", "nd", "N", "D", "iv", "io", "id")


def _edge(P, Q, d, e_o, e_d, D):
    yz, zy, zx, xz, xy, yx = P[1] * Q[2], P[2] * Q[1], P[2] * Q[0], P[0] * Q[2], P[0] * Q[1], P[1] * Q[0]
    w = d[0] * (yz - zy) + d[1] * (zx - xz) + d[2] * (xy - yx)
    # 2^49 T, an integer at the pair's scale D^3
    T = abs(d[0]) * (abs(yz) + abs(zy)) + abs(d[1]) * (abs(zx) + abs(xz)) + abs(d[2]) * (abs(xy) + abs(yx))
    G = 0
    if e_o or e_d:
        E = (abs(Q[0] - P[0]), abs(Q[1] - P[1]), abs(Q[2] - P[2]))
        eo, ed = e_o * D, e_d * D  # (the bounds at the pair's scale)
        G = (ed * (abs(yz - zy) + abs(zx - xz) + abs(xy - yx)) +
             eo * (abs(d[0]) * (E[1] + E[2]) + abs(d[1]) * (E[2] + E[0]) + abs(d[2]) * (E[0] + E[1])) +
             2 * ed * eo * (E[0] + E[1] + E[2]))
    return w, T, G


def _beyond(w, T49, G):
    """-1: w < -(2 T + G); +1: w > 2 T + G; else 0.  T49 = 2^49 T."""
    return 0 if (abs(w) - G) * 2 ** 48 <= T49 else (1 if w > 0 else -1)


def classify(tri, o, d, e_o=Fr(0), e_d=Fr(0)):
    """The object-space ray (o, d) (Fractions, with the chain's error bounds) against `tri`."""
    D = max(tri.den, _den(o), _den(d))
    iv, io, id_ = _ints(tri.v, D), _ints(o, D), _ints(d, D)
    A, B, C = _sub(iv[0:3], io), _sub(iv[3:6], io), _sub(iv[6:9], io)
    w0, T0, G0 = _edge(B, C, id_, e_o, e_d, D)
    w1, T1, G1 = _edge(C, A, id_, e_o, e_d, D)
    w2, T2, G2 = _edge(A, B, id_, e_o, e_d, D)
    N = _cross(_sub(iv[3:6], iv[0:3]), _sub(iv[6:9], iv[0:3]))
    nd = _dot(N, id_)
    p = Pair()
    p.tri, p.o, p.d, p.e_o, p.e_d, p.D, p.iv, p.io, p.id = tri, o, d, e_o, e_d, D, iv, io, id_
    p.w, p.G, p.T49, p.N, p.nd = (w0, w1, w2), (G0, G1, G2), (T0, T1, T2), N, nd
    p.t = Fr(_dot(N, A), nd) if nd != 0 else None
    plane = abs(nd) > e_d * D * (abs(N[0]) + abs(N[1]) + abs(N[2]))
    if plane and ((w0 >= G0 and w1 >= G1 and w2 >= G2) or (w0 <= -G0 and w1 <= -G1 and w2 <= -G2)):
        p.cls = "in"
    else:
        side = (_beyond(w0, T0, G0), _beyond(w1, T1, G1), _beyond(w2, T2, G2))
        p.cls = "out" if -1 in side and 1 in side else "band"
    return p


def classify_world(tri, o, d):
    """As classify, for a world-space ray given as floats: through the triangle's chain first."""
    oo, dd, e_o, e_d = chain_ray(tri.xf, fr3(o), fr3(d))
    return classify(tri, oo, dd, e_o, e_d)


UF = 2.0 ** -53
UP = 1.0 + 1e-9  # the bounds are evaluated in doubles and rounded up by this; the errors are exact


def _len(x, scale):
    """sqrt(x / scale) of integers, as a double (correctly rounded quotient, then the root)."""
    return math.sqrt(x / scale)


class Record:
    """The exact record of a pair whose plane the ray crosses (t, p, u, v, front, the facing normal: Fractions)
    and the bounds a computed record must meet (doubles, rounded up)."""

    def __init__(self, p):
        tri, D, N, nd = p.tri, p.D, p.N, p.nd
        iv, io, id_ = p.iv, p.io, p.id
        D2 = D * D
        self.pair, self.t, self.front, self.p = p, p.t, nd < 0, None
        S = p.w[0] + p.w[1] + p.w[2]
        self.S = S
        tf = abs(float(p.t))
        rel = [_sub(iv[3 * i:3 * i + 3], io) for i in range(3)]
        L = _len(max(_dot(r, r) for r in rel), D2)
        M = _len(max([_dot(iv[3 * i:3 * i + 3], iv[3 * i:3 * i + 3]) for i in range(3)] + [_dot(io, io)]), D2)
        e1, e2 = _sub(iv[3:6], iv[0:3]), _sub(iv[6:9], iv[0:3])
        e3 = _sub(e2, e1)
        E = _len(max(_dot(e, e) for e in (e1, e2, e3)), D2)
        dn = _len(_dot(id_, id_), D2)
        NN = _dot(N, N)
        nlen = _len(NN, D2 * D2)
        K = [abs(e1[1] * e2[2]) + abs(e1[2] * e2[1]), abs(e1[2] * e2[0]) + abs(e1[0] * e2[2]),
             abs(e1[0] * e2[1]) + abs(e1[1] * e2[0])]
        n_inf, n_1 = max(abs(c) for c in N), abs(N[0]) + abs(N[1]) + abs(N[2])
        shape = sum(K) / n_inf
        ndt = abs(nd) / (D2 * D)  # |N . d|
        cos = ndt / nlen
        self.b_p_old = 16 * UF * L * dn / cos * UP
        self.b_t = 16 * UF * (M + shape * E) * dn / cos * UP
        self.b_p = self.b_t + 3 * UF * M * UP
        b_uv = 126 * UF * dn * L * L / (abs(S) / (D2 * D)) * UP if S != 0 else None
        self.b_uv = [b_uv, b_uv]
        alpha = [(4 * UF * (K[j] / D2) / nlen + (abs(N[j]) / D2) / nlen * (4 * UF * shape + 5 * UF)) * (1 + 1e-6) for j in range(3)]
        self.chained = tri.xf is not None
        self.dmax = float(max(abs(c) for c in p.d))
        self.dt, e_p = 0.0, 0.0
        if self.chained:
            e_o, e_d, n1t = float(p.e_o) * UP, float(p.e_d) * UP, n_1 / D2
            self.dt = n1t * (e_o + tf * e_d) / (ndt - n1t * e_d) * (1 + 1e-6)
            e_p = self.b_p + (e_o + tf * e_d + (self.dmax + e_d) * self.dt) * (1 + 1e-6)
            gs = sum(p.G)
            if S != 0 and abs(S) > gs:
                self.b_uv = [b_uv + float((g + gs) / (abs(S) - gs)) * (1 + 1e-6) for g in p.G[1:]]
        self.NN, self.nlen, self.e_p, self.alpha = NN, nlen, 0.0, alpha
        if self.chained:
            pf = [float(p.o[j]) + float(p.t) * float(p.d[j]) for j in range(3)]
            self.e_p, self.alpha = chain_world_bounds(tri.xf, pf, e_p, alpha)

    def _exact(self):
        """The exact record itself, on first use (a Record is also built for its t bound alone)."""
        p, t = self.pair, self.t
        S, N, D2 = self.S, p.N, p.D * p.D
        self.u, self.v = (Fr(p.w[1], S), Fr(p.w[2], S)) if S != 0 else (None, None)
        self.p = tuple(p.o[j] + t * p.d[j] for j in range(3))
        s = 1 if self.front else -1
        self.Nw, self.g = tuple(s * c for c in N), 0
        if self.chained:
            self.p, self.Nw = chain_world(p.tri.xf, self.p, tuple(Fr(c) for c in self.Nw))
            self.g = Fr(_dot(self.Nw, self.Nw), self.NN) - 1
        self.nu = [abs(float(Fr(c) / D2)) / self.nlen for c in self.Nw]

    def tol_t(self):
        """How far a computed t may lie from the exact one."""
        return Fr((self.e_p if self.chained else self.b_p) / self.dmax + self.dt) * SLACK

    def compare(self, got, ratios, old=None):
        """got: a mapping with t, p, normal, u, v, front.  Returns the list of failed checks; `ratios`
        (a dict) keeps the largest error / bound per quantity."""
        bad = []
        if self.p is None:
            self._exact()

        def note(key, err, bound):
            r = err / bound if bound else (0.0 if err == 0 else math.inf)
            if r > ratios.get(key, 0.0):
                ratios[key] = r
            if not err <= bound:
                bad.append((key, r))

        if bool(got["front"]) != self.front:
            bad.append(("front", None))
        gp = fr3(got["p"])
        dp = [float(abs(gp[j] - self.p[j])) for j in range(3)]
        dt = float(abs(Fr(float(got["t"])) - self.t)) * self.dmax
        if self.chained:
            note("p_chain", max(dp), self.e_p)
            note("t_chain", dt, (self.b_t + self.dt * self.dmax) * (1 + 1e-6))
        else:
            err = math.sqrt(dp[0] * dp[0] + dp[1] * dp[1] + dp[2] * dp[2])
            note("p", err, self.b_p)
            if old is not None:
                old["p_old"] = max(old.get("p_old", 0.0), err / self.b_p_old)
            note("t", dt, self.b_t)
        if self.u is not None:
            note("u", float(abs(Fr(float(got["u"])) - self.u)), self.b_uv[0])
            note("v", float(abs(Fr(float(got["v"])) - self.v)), self.b_uv[1])
        n = fr3(got["normal"])
        if not _dot(n, self.Nw) > 0:
            bad.append(("normal faces", None))
        rhs3 = 0.0
        for j in range(3):
            nu, al = self.nu[j], self.alpha[j]
            rhs = 2 * nu * al + al * al
            note("normal", float(abs(n[j] * n[j] - Fr(self.Nw[j] * self.Nw[j]) / self.NN)), rhs)
            rhs3 += rhs
            if nu > al and (n[j] > 0) != (self.Nw[j] > 0):
                bad.append(("normal sign", j))
        note("normal", float(abs(_dot(n, n) - 1 - self.g)), rhs3)
        return bad


# ------------------------------------------------------------------------------ worlds ----
class World:
    """The triangles of a primitive list (dicts: kind, xform, a) with the list's transforms."""

    def __init__(self, prims, xforms, tri_kind=5):
        self.rows = [i for i, q in enumerate(prims) if q["kind"] == tri_kind]
        self.tris = [Tri(prims[i]["a"], xforms[prims[i]["xform"]] if prims[i]["xform"] >= 0 else None) for i in self.rows]
        self.xforms = xforms
        self.xf_of = np.array([prims[i]["xform"] for i in self.rows])
        self.verts = np.array([t.a for t in self.tris]).reshape(-1, 3, 3)

    def candidates(self, o, d):
        """For rays (n, 3) origins and directions: per ray the indices (into self.tris) of the triangles that are
        not surely `out`.  Float edge functions; a triangle is dropped only when one is below -m and one above
        m with m = 2^-40 |d|_inf L_inf^2 plus 2^10 times the chain terms: 2 T <= 12 * 2^-49 |d|_inf L_inf^2 and the
        float functions' own error is below that, so m is more than 30 times either."""
        n = len(o)
        keep = [[] for _ in range(n)]
        for x in sorted(set(self.xf_of.tolist())):
            idx = np.nonzero(self.xf_of == x)[0]
            oo, dd = np.array(o, float), np.array(d, float)
            eo, ed = np.zeros(n), np.zeros(n)
            if x >= 0:
                xf, u = self.xforms[x], 2.0 ** -52
                for k in range(xf["n"]):
                    v = xf["v"][k]
                    if xf["op"][k] == XF_TRANSLATE:
                        oo = oo - np.array(v, float)
                        eo = eo + u * (np.abs(oo).max(axis=1) + eo)
                    else:
                        sn, cs = v[0], v[1]
                        eo = 1.5 * (eo + 3 * u * (np.abs(oo).max(axis=1) + eo))
                        ed = 1.5 * (ed + 3 * u * (np.abs(dd).max(axis=1) + ed))
                        oo = np.stack([cs * oo[:, 0] - sn * oo[:, 2], oo[:, 1], sn * oo[:, 0] + cs * oo[:, 2]], 1)
                        dd = np.stack([cs * dd[:, 0] - sn * dd[:, 2], dd[:, 1], sn * dd[:, 0] + cs * dd[:, 2]], 1)
            V = [[self.verts[idx, i, c][None, :] for c in range(3)] for i in range(3)]  # V[vertex][axis]: (1, tris)
            for lo in range(0, n, 512):
                sl = slice(lo, min(n, lo + 512))
                ox, dx = [oo[sl, c][:, None] for c in range(3)], [dd[sl, c][:, None] for c in range(3)]
                P = [[V[i][c] - ox[c] for c in range(3)] for i in range(3)]                # P[vertex][axis]: (rays, tris)
                w = []
                for a, b in ((1, 2), (2, 0), (0, 1)):
                    (px, py, pz), (qx, qy, qz) = P[a], P[b]
                    w.append(dx[0] * (py * qz - pz * qy) + dx[1] * (pz * qx - px * qz) + dx[2] * (px * qy - py * qx))
                lmax = np.abs(P[0][0])
                for i in range(3):
                    for c in range(3):
                        np.maximum(lmax, np.abs(P[i][c]), out=lmax)
                dmax = np.abs(dd[sl]).max(axis=1)[:, None]
                m = 2.0 ** -40 * dmax * lmax * lmax + 1024 * (ed[sl, None] * 6 * lmax * lmax + eo[sl, None] * 12 * dmax * lmax)
                wmin, wmax = np.minimum(np.minimum(w[0], w[1]), w[2]), np.maximum(np.maximum(w[0], w[1]), w[2])
                r, c = np.nonzero(~((wmin < -m) & (wmax > m)))
                for ri, ci in zip(r.tolist(), c.tolist()):
                    keep[lo + ri].append(int(idx[ci]))
        return keep

    def trace(self, rays, cand=None):
        """Per ray a Trace: the exact answer over the triangles and whether it is decided."""
        o, d = rays["origin"], rays["dir"]
        cand = self.candidates(o, d) if cand is None else cand
        out = []
        for i in range(len(rays)):
            fo, fd = fr3(o[i]), fr3(d[i])
            chains, pairs = {}, []
            for k in sorted(cand[i]):
                tri = self.tris[k]
                key = id(tri.xf)
                if key not in chains:
                    chains[key] = chain_ray(tri.xf, fo, fd)
                p = classify(tri, *chains[key])
                if p.cls != "out":
                    pairs.append((k, p))
            out.append(Trace(self, pairs, Fr(float(rays["t_min"][i])), float(rays["t_max"][i])))
        return out


class Trace:
    """One ray against a World.  hit: index into world.tris of the exact winner, or None; rec its Record;
    decided: no band triangle and no second `in` triangle can have changed the answer; must_hit: an `in`
    triangle lies inside [t_min, t_max] by more than its t bound; allowed: {index: Record} of every triangle a
    correct implementation may return."""

    def __init__(self, world, pairs, t_min, t_max):
        t_hi = Fr(t_max) if math.isfinite(t_max) else None
        recs = []
        for k, p in pairs:
            if p.t is None:
                continue
            r = Record(p)
            recs.append((k, p, r, r.tol_t()))
        self.allowed = {k: r for k, p, r, tol in recs
                        if p.t >= t_min - tol and (t_hi is None or p.t <= t_hi + tol)}
        self.edge = any(abs(p.t - t_min) <= tol or (t_hi is not None and abs(p.t - t_hi) <= tol) for k, p, r, tol in recs)
        ins = [(p.t, -k, k, r, tol) for k, p, r, tol in recs if p.cls == "in" and p.t >= t_min and (t_hi is None or p.t <= t_hi)]
        ins.sort(key=lambda x: (x[0], x[1]))
        self.hit, self.rec, self.tol = None, None, Fr(0)
        self.cls = {k: p.cls for k, p in pairs}  # (a triangle that is not here is `out`)
        self.tols = {k: tol for k, p, r, tol in recs}
        self.must_hit = any(t >= t_min + tol and (t_hi is None or t <= t_hi - tol) for t, _, k, r, tol in ins)
        self.any_band = any(p.cls == "band" for k, p in pairs)
        decided = not self.edge
        limit = None
        if ins:
            t, _, self.hit, self.rec, self.tol = ins[0]
            limit = t + self.tol
            if len(ins) > 1 and ins[1][0] <= limit + ins[1][4]:
                decided = False
        for k, p, r, tol in recs:
            if p.cls == "band" and k in self.allowed and (limit is None or p.t <= limit + tol):
                decided = False
        if any(p.cls == "band" and p.t is None for k, p in pairs):
            decided = False
        self.decided = decided
        if limit is not None:  # nothing behind the winner's reach may be returned
            tols = {k: tol for k, p, r, tol in recs}
            self.allowed = {k: r for k, r in self.allowed.items() if r.t <= limit + tols[k]}


# ------------------------------------------------------------------------------ meshes ----
def bipyramid(n=64, radius=1.0, height=0.8):
    """Two apexes of valence n over a regular n-gon (in the plane y = 0), outward winding."""
    a = 2.0 * np.pi * np.arange(n) / n
    v = np.concatenate([np.stack([radius * np.cos(a), np.zeros(n), radius * np.sin(a)], 1), [[0.0, height, 0.0], [0.0, -height, 0.0]]])
    f = [[n, (i + 1) % n, i] for i in range(n)] + [[n + 1, i, (i + 1) % n] for i in range(n)]
    return v, np.array(f)


def sliver_strip(quads=4, length=2.5, aspect=1.0e4, centred=False):
    """A planar strip of 2 * quads triangles, each `length` long and length / aspect wide, tilted so that no
    face is axis-aligned; from the origin, or centred on it."""
    wdt = length / aspect
    ax, up = np.array([0.8, 0.36, 0.48]), np.array([-0.6, 0.48, 0.64])  # orthonormal
    i0 = quads / 2.0 if centred else 0.0
    v = [(i - i0) * length * ax + j * wdt * up for i in range(quads + 1) for j in (0, 1)]
    f = []
    for i in range(quads):
        a, b, c, d = 2 * i, 2 * i + 1, 2 * i + 2, 2 * i + 3
        f += [[a, c, d], [a, d, b]]
    return np.array(v), np.array(f)


# -------------------------------------------------------------------------------- rays ----
RUNGS = tuple(range(20, 55, 2))
SCALES = (Fr(1), Fr(1, 2), Fr(3))


def _unit(x):
    x = np.array(x, float)
    return x / np.sqrt((x * x).sum())


def _aim(o, target, scale):
    """The direction scale * (target - o), from exact terms, rounded once per component."""
    fo = fr3(o)
    return tuple(float(scale * (target[j] - fo[j])) for j in range(3))


def ladder(tri_world, seed, near=8.0, rungs=RUNGS, exact=None):
    """Rays about one triangle (world-space vertices, (3, 3) floats): for each edge a point at s in 0.1 .. 0.9 and
    for each vertex the vertex itself, displaced in the triangle's plane by +-2^-k times an edge length (the edge's
    own; about a vertex the longer adjacent one, along the bisector), k in `rungs`; the direction scale cycles
    through 1, 0.5, 3.  The origin lies `near` times the triangle's shortest edge from the target, on alternating
    sides of the plane.  The targets are exact rationals; only the direction's components are rounded.
    Returns rows (origin, dir, rung, side) with side +1 towards the inside."""
    # (edges and normal below come from the double vertices: directions only, their rounding moves no target)
    rng = np.random.default_rng(seed)
    v = np.array(tri_world, float)
    fv = [fr3(x) for x in v] if exact is None else exact  # (exact: the vertices as Fractions, where doubles are too coarse)
    edges = [v[(k + 1) % 3] - v[k] for k in range(3)]
    elen = [float(np.sqrt((e * e).sum())) for e in edges]
    nrm = _unit(np.cross(edges[0], -edges[2]))
    rows, j = [], 0
    for k in range(3):
        # the edge k -> k + 1: inward is n x e
        s = Fr(int(rng.integers(1, 10)), 10)
        base = tuple(fv[k][c] + s * (fv[(k + 1) % 3][c] - fv[k][c]) for c in range(3))
        inward = _unit(np.cross(nrm, edges[k]))
        targets = [(base, inward, elen[k])]
        # the vertex k: the bisector of its two edges
        bis = _unit(_unit(edges[k]) - _unit(edges[(k + 2) % 3]))
        targets.append((fv[k], bis, max(elen[k], elen[(k + 2) % 3])))
        for base, m, scale_len in targets:
            for rung in rungs:
                for side in (1, -1):
                    j += 1
                    tilt = nrm * (1.0 if j % 2 else -1.0) + 0.3 * _unit(edges[k]) + 0.2 * m
                    o = np.array([float(c) for c in base]) + near * min(elen) * _unit(tilt)
                    step = Fr(side, 2 ** rung) * Fr(scale_len)
                    tgt = tuple(base[c] + step * Fr(float(m[c])) for c in range(3))
                    rows.append((tuple(float(c) for c in o), _aim(o, tgt, SCALES[j % 3]), rung, side))
    return rows


def _quant(x, q):
    return np.round(np.array(x, float) / q) * q


def exact_points(tri_world, seed, near=8.0):
    """Rays aimed at the three vertices and at a point of each edge (s = 1/4, 1/2, 3/4), and 1-3 ulps beside them
    (one direction component stepped).  The origin is the target plus an offset on a coarse dyadic grid, so that
    for vertices with short significands (the test meshes are rounded to float32) target - origin is exact and
    the ray passes through the point in exact arithmetic.  Rows (origin, dir, rung, side): rung 0 where the aim is
    exact, 1 where the direction had to be rounded, -ulps beside."""
    rng = np.random.default_rng(seed)
    v = np.array(tri_world, float)
    edges = [v[(k + 1) % 3] - v[k] for k in range(3)]
    elen = min(float(np.sqrt((e * e).sum())) for e in edges)
    q = 2.0 ** (math.floor(math.log2(elen)) - 20)
    nrm = _unit(np.cross(edges[0], -edges[2]))
    rows = []
    for k in range(3):
        for tgt in (v[k], v[k] + float(rng.choice([0.5, 0.25, 0.75])) * edges[k]):
            off = _quant(near * elen * _unit(nrm * float(rng.choice([-1.0, 1.0])) + 0.4 * rng.normal(size=3)), q)
            o = tgt + off
            sc = SCALES[int(rng.integers(0, 3))]
            want = [sc * (Fr(float(tgt[c])) - Fr(float(o[c]))) for c in range(3)]
            d = np.array([float(x) for x in want])
            exact = all(Fr(float(d[c])) == want[c] for c in range(3))
            rows.append((tuple(o), tuple(d), 0 if exact else 1, 0))
            for ulps in (1, 2, 3):
                d2 = d.copy()
                c = int(rng.integers(0, 3))
                for _ in range(ulps):
                    d2[c] = np.nextafter(d2[c], np.inf if rng.random() < 0.5 else -np.inf)
                rows.append((tuple(o), tuple(d2), -ulps, 0))
    return rows


def f32(v):
    """Vertices rounded to float32 values (held as doubles): short significands, so exact aims exist."""
    return np.array(v, np.float32).astype(np.float64)


def meshes(seed=11):
    """The test meshes, name -> (vertices, faces, near): a tetrahedron, an icosahedron, a jittered level-2
    icosphere, a 64-gon bipyramid, a sliver strip of aspect 10^4 : 1, and the icosahedron scaled by 2^-20 at an
    offset of about 1000.  near: the ladder origins' distance in shortest edges."""
    import tri_helpers as T
    rng = np.random.default_rng(seed)
    tv, tf = T.tetrahedron()
    iv, if_ = T.icosahedron()
    sv, sf = T.icosphere(2)
    sv = T.rot_y(sv * 1.5 * (1 + 0.06 * rng.uniform(-1, 1, sv.shape)), 0.41)
    bv, bf = bipyramid(64, 1.2, 0.9)
    bv = T.rot_y(bv, 0.3)[:, [1, 2, 0]] * np.array([1.0, 1.1, 0.9])  # (a cyclic axis change keeps the winding)
    lv, lf = sliver_strip()
    out = {"tetrahedron": (f32(tv * 1.3 + [0.11, 0.07, -0.05]), tf, 3.0),
           "icosahedron": (f32(T.rot_y(iv, 0.2) * 1.1), if_, 5.0),
           "icosphere": (f32(sv), sf, 8.0),
           "bipyramid": (f32(bv), bf, 8.0),
           "sliver": (f32(lv + [-5.0, 0.3, 0.2]), lf, 8.0),
           "tiny": (T.rot_y(iv, 0.7) * 2.0 ** -20 + np.array([1000.25, 1.5, -999.75]), if_, 8.0)}
    return out
