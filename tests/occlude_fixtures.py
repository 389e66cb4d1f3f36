"""Per-ray ranges and oracle references for the occlusion and ranged-cast tests (fr_ctx_occluded,
fr_ctx_cast with FR_CAST_TMAX): shared by tests/test_occlude_fixtures.py,
tests/test_occlude_host.py and tests/test_occlude.py; not a test module.

The rays are tests/cast_fixtures.py's batches. Ray i's t_max is entry i mod 12 of MODES, where t*
is the ray's unbounded closest root (1 for a miss): FLT_MAX, +inf, t*, the two neighbours of t*,
t* / 2, 2 t*, 0.001 (t_min), its upper neighbour, 0, -1 and NaN.

The expected answers are built from the oracle as it is. oracle_closest_hit on the one-primitive
list prims[i:i+1] gives primitive i's own accepted root t_i in (0.001, FLT_MAX). For a sphere, a
box, an oriented box or a triangle that root is the smallest root above t_min, so the primitive is
accepted under `closest` iff t_i < closest. A plane is gated on its denominator: it is accepted
iff the oracle accepts it and denom_i < closest, with denom_i = dot(orientation, d) restated in
f32 in the reference's order ((x + y) + z); its t is not compared. The closest-hit loop from
closest = t_max over those is the ranged winner and root; occlusion is "some primitive is accepted
at t_max itself". Normal, point and albedo of a winner are cast_fixtures.hits' of the list cut
down to the winner alone (a list cut only after it can lose the winner to an earlier plane that
the ranged loop's gate refused)."""
import ctypes as C

import numpy as np

from oracle import oracle_py as O
from oracle import scene_ref as S
from tests import cast_fixtures as CF

F = np.float32
MISS = CF.MISS
FLT_MAX = np.finfo(F).max
T_MIN = F(0.001)
MODES = ("flt_max", "inf", "t", "t_up", "t_down", "half", "twice", "t_min", "t_min_up", "zero", "minus_one", "nan")


def t_max_of(t_star):
    """[n] f32: the per-ray t_max of a batch whose unbounded roots (0 for a miss) are t_star."""
    t = np.where(t_star == 0, F(1.0), t_star).astype(F)
    with np.errstate(all="ignore"):
        cols = [np.full(len(t), FLT_MAX, F), np.full(len(t), np.inf, F), t, np.nextafter(t, F(np.inf)),
                np.nextafter(t, F(-np.inf)), (F(0.5) * t).astype(F), (F(2.0) * t).astype(F), np.full(len(t), T_MIN, F),
                np.full(len(t), np.nextafter(T_MIN, F(np.inf)), F), np.zeros(len(t), F), np.full(len(t), -1.0, F),
                np.full(len(t), np.nan, F)]
    assert len(cols) == len(MODES)
    out = np.stack(cols, axis=1)[np.arange(len(t)), np.arange(len(t)) % len(MODES)].astype(F)
    out.setflags(write=False)
    return out


def own_roots(prims, o, d):
    """(ok [n, m] bool, t [n, m] f32): whether the oracle accepts primitive j alone on ray i in
    (0.001, FLT_MAX), and its accepted root."""
    o, d = np.ascontiguousarray(o, F), np.ascontiguousarray(d, F)
    arr = O.prims_to_c(prims)
    hit = O.lib().oracle_closest_hit
    size = C.sizeof(O.OrPrim)
    one = [C.cast(C.byref(arr, j * size), C.POINTER(O.OrPrim)) for j in range(len(prims))]
    ok, t = np.zeros((len(o), len(prims)), bool), np.zeros((len(o), len(prims)), F)
    rec = (C.c_float * 7)()
    for i in range(len(o)):
        oo = (C.c_float * 3)(*[float(c) for c in o[i]])
        dd = (C.c_float * 3)(*[float(c) for c in d[i]])
        oki, ti = ok[i], t[i]
        for j, pj in enumerate(one):
            if hit(pj, 1, oo, dd, rec) == 0:
                oki[j] = True
                ti[j] = rec[0]
    return ok, t


def plane_denoms(prims, d):
    """[n, m] f32: dot(orientation_j, d_i), (x + y) + z with every operation rounded in f32; +inf
    in the columns of primitives that are not planes."""
    d = np.asarray(d, F)
    out = np.full((len(d), len(prims)), np.inf, F)
    with np.errstate(all="ignore"):
        for j, p in enumerate(prims):
            if p["kind"] == S.PLANE:
                n = np.asarray(p["g"][3:6], F)
                out[:, j] = (((n[0] * d[:, 0]).astype(F) + (n[1] * d[:, 1]).astype(F)).astype(F) + (n[2] * d[:, 2]).astype(F)).astype(F)
    return out


def ranged(prims, o, d, t_max):
    """{"occluded" [n] bool, "prim", "t", "normal", "position", "albedo": the ranged closest hit as
    cast_fixtures.hits' dict} of rays o, d with ranges t_max."""
    o, d = np.ascontiguousarray(o, F), np.ascontiguousarray(d, F)
    n = len(o)
    ok, t = own_roots(prims, o, d)
    den = plane_denoms(prims, d)
    is_plane = np.array([p["kind"] == S.PLANE for p in prims], bool)
    out = {"occluded": np.zeros(n, bool), "prim": np.full(n, MISS, np.uint32), "t": np.zeros(n, F),
           "normal": np.zeros((n, 3), F), "position": np.zeros((n, 3), F), "albedo": np.ones((n, 3), F)}
    for i in range(n):
        cand = np.nonzero(ok[i])[0]
        closest, best = F(t_max[i]), -1
        any_hit = False
        for j in cand:
            key = den[i, j] if is_plane[j] else t[i, j]
            any_hit |= bool(key < F(t_max[i]))  # the test against t_max itself
            if key < closest:                   # the list loop's test against closest
                closest, best = t[i, j], int(j)
        out["occluded"][i] = any_hit
        assert any_hit == (best >= 0)  # the equivalence the kernel relies on
        if best >= 0:
            h = CF.hits(prims[best:best + 1], o[i:i + 1], d[i:i + 1])
            assert h["prim"][0] == 0 and h["t"][0].view(np.uint32) == t[i, best].view(np.uint32)
            out["prim"][i], out["t"][i] = best, t[i, best]
            for name in ("normal", "position", "albedo"):
                out[name][i] = h[name][0]
    for a in out.values():
        a.setflags(write=False)
    return out


_cache = {}


def lattice(fr, kind):
    """(batch, t_max [n], ranged reference) of a lattice kind's batch, computed once."""
    key = ("lattice", kind)
    if key not in _cache:
        b = CF.batch(fr, kind)
        tm = t_max_of(CF.expected(fr, kind)["t"])
        _cache[key] = (b, tm, ranged(b["prims"], b["o"], b["d"], tm))
    return _cache[key]


def spheres(fr, count, w=24, h=16):
    """(prims, o, d, t_max, ranged reference) of cast_fixtures.gen_batch, computed once."""
    key = ("gen", count, w, h)
    if key not in _cache:
        prims, o, d, want = CF.gen_batch(fr, count, w, h)
        tm = t_max_of(want["t"])
        _cache[key] = (prims, o, d, tm, ranged(prims, o, d, tm))
    return _cache[key]


def truncated(want, t_max):
    """The unbounded hits `want` cut at t_max: a hit whose root is not below t_max becomes a miss.
    What a caller comparing t on the host would get; the ranged loop differs where a plane's gate
    decides."""
    with np.errstate(all="ignore"):
        keep = (want["prim"] != MISS) & (want["t"] < t_max)
    return np.where(keep, want["prim"], MISS).astype(np.uint32)
