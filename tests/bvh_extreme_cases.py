"""Scenes and rays shared by tests/test_bvh_extremes_cpu.py and tests/test_gpu_bvh_extremes.py: the BVH path (traversal padding,
16-bit grid, host and device builders) away from the near-origin, unit-scale scenes of the other BVH tests.  numpy only, every
scene and ray set deterministic from its seed.

A case is a FAMILY under a TRANSFORM p -> s p + off (radii scaled by s), computed in f64 and rounded once to f32; t_min and the
clipped intervals scale with s.  Families: cloud (random_scene's mix, the control), ratio (the cloud between a radius-1000
ground, a radius-5000 enclosure and 100 spheres far below one grid cell), flat / flat3 (17 x 17 quads in one plane y = const:
that grid axis has zero extent; flat3: 10 x 10 quads in each of the planes y, x, z = const), needles (aspect 1e5 triangles, huge boxes over
tiny areas, and small spheres) and stacked (coincident copies spread over the index range, concentric spheres).

Ray sets (ray_sets): random, silhouette, face (face-tangent), edge, stack, and for the flat families inplane.  A set exists
where the family has the primitives it aims at:
  * flat / flat3 hold no sphere, so no silhouette and no face set; their rays go to edge and inplane;
  * only stacked has a stack set.
Each grazing set records the object every ray was aimed at, so that the CPU test can ask the oracle about that object alone.

What was narrowed, and why:
  * edge targets are triangles whose f32-rounded vertices still span an area.  Under the offsets (ulp 4.9e-4 at 4096, 0.5 at
    2^22) a needle of width 2e-5 s rounds to a segment (never hit: its normal is 0) or to a sliver one ulp wide; the former
    cannot be grazed.  They stay in the scene.
  * in needles only spheres emit: a zero-area light has no finite sampling density.
  * a silhouette ray's aim is c + r' u with r' = r D / sqrt(D^2 - r^2), D = |c - o|: the perpendicular offset at which the LINE
    is tangent.  (At offset r itself every ray passes inside the sphere by r / 2 rho^2, thousands of eps.)
"""
import numpy as np

FAMILIES = ("cloud", "ratio", "flat", "flat3", "needles", "stacked")
TRANSFORMS = {
    "unit": (1.0, (0.0, 0.0, 0.0)),
    "small": (2.0 ** -10, (0.0, 0.0, 0.0)),
    "large": (2.0 ** 10, (0.0, 0.0, 0.0)),
    "offset": (1.0, (4096.0, -4096.0, 4096.0)),                       # ulp(grid_min) = 4.9e-4, cell ~ 4e-5 .. 2e-4
    "large_offset": (2.0 ** 10, (2.0 ** 22, 2.0 ** 22, -2.0 ** 22)),  # ulp(grid_min) = 0.25 .. 0.5, cell ~ 0.04 .. 0.2
}
CASES = [(f, t) for f in FAMILIES for t in TRANSFORMS]
INTERVALS = ((0.001, float("inf")), (0.001, 0.4), (0.3, 1.5))         # x s: test_bvh_hit_scene_equals_linear_scan's
N_ORACLE = 20_000                                                     # rays of a case held to the f32 oracle on the GPU

# The jitter of the grazing sets, chosen on the CPU against the oracle alone (tests/test_bvh_extremes_cpu.py asserts the
# conditions and prints the figures under pytest -s), per set because the three boundaries are not equally sharp:
#   silhouette  aim displaced by eps r g, g standard normal.  2e-6: at 1e-5 the unit cases had 38 f32/f64 flips, the offset
#               cases 24; at 2e-6 every case has 93 .. 151 of 13 000, with 49.7 .. 50.6 % of the rays hitting in f64.
#   edge        aim displaced by eps |edge| g.  2e-6: at 1e-5 the cloud had 18 flips (the triangle test is sharper than the
#               sphere test); 2e-6 is also below a needle's width (1e-5 of its length), so that an aim pushed inward does not
#               leave through the other long edge.  56 .. 96 flips of 13 000 (cloud, ratio, stacked), 209 .. 326 of 26 000
#               (flat, flat3), 1470 .. 2204 (needles); 32.7 .. 52.8 % hit in f64.
#   face        in units of the sliver's half-width L (see _face), not of r: L / r runs from 5e-4 (unit) to 4e-2 (offsets),
#               and a jitter of 2e-3 r gave 7 % hits in f64 at unit scale and 98 % under the offsets.  Even rays: aim at the
#               touching point, displaced by 1.5 L g; with those alone the offsets reached 0 .. 10 flips (stacked, offset: 0),
#               since the band of |lateral| around L in which f32 and f64 disagree is ~1e-6 r^2 / 2L wide.  Odd rays: aim at
#               the sliver's rim, touch +- L perp, displaced by EPS_RIM L g.  Together 3739 .. 4186 flips of 13 000 without
#               an offset, 384 .. 1558 with one; 49.3 .. 50.1 % hit in f64.
# No case needs a lower bar than 20 flips (MIN_FLIPS is empty).  stack: 7199 .. 7212 of 10 000 rays end in an exact tie.
# random: 9.4 % (flat, small: the quads' determinant is 1.9e-8, so only rays within 58 degrees of the normal pass the
# reference's cutoff) .. 59.9 % of the rays hit a non-giant object; 530 / 601 (cloud), 543 / 702 (ratio), 564 .. 578 / 578
# (flat), 600 / 600 (flat3), 405 / 600 (needles; 299 / 300, 335 / 337, 327 / 328 of the hittable at small, offset,
# large_offset) and 58 / 60 distinct primitives (stacked) are hit.
EPS = {f: {"silhouette": 2e-6, "face": 1.5, "edge": 2e-6} for f in FAMILIES}
EPS_RIM = 1e-3
MIN_FLIPS = {}                                                        # (family, transform, set) -> a bar below 20, with its reason

N_RAYS = {"random": 21_000, "silhouette": 13_000, "face": 13_000, "edge": 13_000, "stack": 10_000}     # 60 000 per case
N_TARGETS = 40                                                        # targets per grazing set, N_RAYS / N_TARGETS rays each


class Scene:
    """tag[n], shape f64[n, 9] (f32 values), mat_tag[n], mat f64[n, 6]; giant[n]: the spheres far larger than the rest; group[n]:
    the distinct primitive an object is a copy of; film_ggx[n]: the objects that take a GGX material for the film"""

    def __init__(self, family, transform):
        self.family, self.transform = family, transform
        self.s, off = TRANSFORMS[transform]
        self.off = np.array(off, dtype=np.float64)
        self.t_min = 1e-3 * self.s

    def __len__(self):
        return len(self.tag)

    def intervals(self):
        return [(a * self.s, b * self.s) for a, b in INTERVALS]

    def corners(self):
        """per object the points its box spans: f64[n, 3, 3] (a sphere: c - r, c, c + r)"""
        p = self.shape.reshape(-1, 3, 3).copy()
        sph = self.tag == 0
        c, r = self.shape[sph, 0:3], self.shape[sph, 3:4]
        p[sph] = np.stack([c - r, c, c + r], axis=1)
        return p

    def core_bounds(self):
        p = self.corners()[~self.giant].reshape(-1, 3)
        return p.min(axis=0), p.max(axis=0)

    def hittable(self):
        """False for a triangle no ray can hit: the reference rejects |d . (e1 x e2)| < 1e-8 with |d| = 1, which is every ray once
        |e1 x e2| < 1e-8 -- the needles at scale 2^-10 (2e-3 x 2e-8), and the needles an offset rounded to a segment."""
        v = self.shape.reshape(-1, 3, 3)
        return (self.tag == 0) | (np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1) >= 1e-8)

    def objects(self, pt, film=False):
        specs = []
        for i in range(len(self)):
            mt, mv = int(self.mat_tag[i]), list(self.mat[i])
            if film and self.film_ggx[i]:
                mt, mv = 2, [0.05 + 0.5 * ((i * 7) % 10) / 10.0, 0.9, 0.8, 0.7, float(i % 2), 1.5]
            specs.append((int(self.tag[i]), list(self.shape[i]), mt, mv))
        return pt.make_objects(specs)

    def camera(self, pt, size=32):
        """camera_look_at in the transformed frame: the whole camera goes through p -> s p + off, screen included.  (A screen
        left at distance 1 from an eye near 2^22 has all its pixels within two ulps: every ray the same direction.)"""
        cam = pt.camera_look_at((0.3, 0.6, 1.2), (0.0, -0.3, -2.0), (0.0, 1.0, 0.0), size, size, 50.0)
        for k in range(3):
            cam.origin[k] = cam.origin[k] * self.s + self.off[k]
            cam.lower_left[k] = cam.lower_left[k] * self.s + self.off[k]
            cam.horizontal[k] *= self.s
            cam.vertical[k] *= self.s
        return cam

    def film_integrators(self):
        """-> [(integrator, film must be finite)].  Every light of a flat family is coplanar with surfaces it lights; the
        reference's light sampling has cos = 0 on both ends there and its f32 film holds NaN pixels (the f32 oracle's does).
        So the light-sampling film of those families is compared NaN for NaN, and the finite, non-black film is the one by
        BSDF sampling alone (integrator 1)."""
        return [(0, False), (1, True)] if self.family.startswith("flat") else [(0, True)]

    def moved(self, seed=5):
        """The refit pose: every object translated by up to 0.2 extents per axis, 5 % of them by 3 extents (the bounds, hence the
        grid, change).  Per axis, so a plane stays a plane: flat keeps its axis of zero extent."""
        rng = np.random.default_rng(seed)
        lo, hi = self.core_bounds()
        n = len(self)
        step = rng.uniform(-0.2, 0.2, (n, 3))
        far = rng.uniform(size=n) < 0.05
        step[far] = rng.choice([-3.0, 3.0], (int(far.sum()), 3))
        step[self.giant] = 0.0
        d = step * (hi - lo)
        out = Scene(self.family, self.transform)
        out.__dict__.update(self.__dict__)
        shape = self.shape.copy()
        sph = self.tag == 0
        shape[sph, 0:3] += d[sph]
        shape[~sph] += np.tile(d[~sph], 3)
        out.shape = _f32(shape)
        return out


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _materials(rng, n, emit):
    """random_scene's materials without GGX: emissive (the first two of `emit` and a tenth), Lambert, Oren-Nayar"""
    mt, mv = np.zeros(n, dtype=np.int64), np.zeros((n, 6))
    m = rng.integers(0, 10, n)
    first = set(np.flatnonzero(emit)[:2].tolist())
    for i in range(n):
        if emit[i] and (i in first or m[i] == 0):
            mt[i], mv[i, :3] = 1, rng.uniform(2, 20, 3)
        elif m[i] == 8:
            mt[i], mv[i, :4] = 3, list(rng.uniform(0.2, 0.9, 3)) + [rng.uniform(0, 1)]
        else:
            mt[i], mv[i, :3] = 0, rng.uniform(0.1, 0.9, 3)
    return mt, mv


def _cloud(rng, n):
    prims = []
    for _ in range(n):
        if rng.integers(0, 2) == 0:
            prims.append((0, list(rng.uniform([-1, -1, -3], [1, 1, -1])) + [float(rng.uniform(0.05, 0.5))]))
        else:
            v0 = rng.uniform([-1.2, -1.2, -3.2], [1.2, 1.2, -0.8])
            prims.append((1, list(v0) + list(v0 + rng.uniform(-1, 1, 3)) + list(v0 + rng.uniform(-1, 1, 3))))
    return prims


def _quads(axis, at, lo, hi, n=17):
    """n x n quads (two triangles each, shared edges and vertices) in the plane x_axis = at over [lo, hi] of the other two axes"""
    a, b = [k for k in range(3) if k != axis]
    ua, ub = np.linspace(lo[a], hi[a], n + 1), np.linspace(lo[b], hi[b], n + 1)

    def p(i, j):
        v = np.zeros(3)
        v[axis], v[a], v[b] = at, ua[i], ub[j]
        return list(v)

    prims = []
    for i in range(n):
        for j in range(n):
            prims.append((1, p(i, j) + p(i + 1, j + 1) + p(i + 1, j)))
            prims.append((1, p(i, j) + p(i, j + 1) + p(i + 1, j + 1)))
    return prims


def scene(family, transform, seed=0):
    rng = np.random.default_rng(1000 * FAMILIES.index(family) + seed)
    giants, groups = [], None
    lo, hi = np.array([-1.2, -1.0, -3.2]), np.array([1.2, 1.0, -0.8])
    if family == "cloud":
        prims = _cloud(rng, 600) + [(0, [0.0, 0.0, -2.0, 6.0])]
        giants = [600]
    elif family == "ratio":
        prims = _cloud(rng, 600)
        low = min(min(p[1][1::3]) if p[0] else p[1][1] - p[1][3] for p in prims)
        prims += [(0, [0.0, low - 1000.0, -2.0, 1000.0]), (0, [0.0, 0.0, -2.0, 5000.0])]
        giants = [600, 601]
        for _ in range(100):
            prims.append((0, list(rng.uniform([-1, -1, -3], [1, 1, -1])) + [float(np.exp(rng.uniform(np.log(1e-3), np.log(1e-2))))]))
    elif family == "flat":
        prims = _quads(1, -1.0, lo, hi)
    elif family == "flat3":
        prims = _quads(1, -1.0, lo, hi, 10) + _quads(0, -1.2, lo, hi, 10) + _quads(2, -3.2, lo, hi, 10)
    elif family == "needles":
        prims = []
        for _ in range(300):
            v0 = rng.uniform([-1, -1, -3], [1, 1, -1])
            u = _unit(rng.normal(size=3))
            w = _unit(np.cross(u, rng.normal(size=3)))
            prims.append((1, list(v0) + list(v0 + u * rng.uniform(1.6, 2.4)) + list(v0 + w * 2e-5)))
        for _ in range(300):
            prims.append((0, list(rng.uniform([-1, -1, -3], [1, 1, -1])) + [float(rng.uniform(0.03, 0.1))]))
    else:
        base = _cloud(rng, 40)
        base = [(t, v[:3] + [float(rng.uniform(0.1, 0.4))]) if t == 0 else (t, v) for t, v in base]
        prims, groups = [], []
        for g, p in enumerate(base):
            k = int(rng.choice([1, 5, 9, 17]))
            prims += [p] * k
            groups += [g] * k
        for c in ([-0.4, 0.3, -1.6], [0.5, -0.4, -2.4]):                  # two sets of concentric spheres
            for r in np.linspace(0.05, 0.5, 10):
                prims.append((0, c + [float(r)]))
                groups.append(max(groups) + 1)
    n = len(prims)
    order = rng.permutation(n)
    sc = Scene(family, transform)
    sc.tag = np.array([prims[i][0] for i in order], dtype=np.int64)
    shape = np.zeros((n, 9))
    for k, i in enumerate(order):
        shape[k, :len(prims[i][1])] = prims[i][1]
    sph = sc.tag == 0
    shape[sph, 0:3] = shape[sph, 0:3] * sc.s + sc.off
    shape[sph, 3] *= sc.s
    shape[~sph] = shape[~sph] * sc.s + np.tile(sc.off, 3)
    sc.shape = _f32(shape)
    sc.giant = np.isin(order, giants)
    sc.group = np.arange(n) if groups is None else np.array(groups)[order]
    emit = sph & ~sc.giant if family == "needles" else ~sc.giant
    sc.mat_tag, sc.mat = _materials(rng, n, emit)
    sc.film_ggx = (rng.uniform(size=n) < 0.1) & (sc.mat_tag != 1)
    return sc


# ------------------------------------------------------------------------------------------------------------------ rays
def _pack(o, d):
    return np.concatenate([o, _f32(d)], axis=1)


def _targets(rng, idx, n, weight=None):
    """n rays over N_TARGETS of the objects idx -> the target of every ray"""
    pick = rng.choice(idx, size=min(N_TARGETS, len(idx)), replace=False, p=weight)
    return np.repeat(pick, -(-n // len(pick)))[:n]


def _random(sc, rng, n):
    lo, hi = sc.core_bounds()
    o = rng.uniform(lo, hi, (n, 3))
    d = rng.normal(size=(n, 3))
    m = n // 5                                                           # a fifth from 300 extents away, aimed at an object
    ext = (hi - lo).max()
    o[:m] = 0.5 * (lo + hi) + 300.0 * ext * _unit(rng.normal(size=(m, 3)))
    o = _f32(o)
    t = rng.choice(np.flatnonzero(~sc.giant), m)
    w = rng.dirichlet([1.0, 1.0, 1.0], m)
    p = sc.corners()[t]
    aim = np.where((sc.tag[t] == 0)[:, None], p[:, 1], (w[:, :, None] * p).sum(axis=1))
    d[:m] = aim - o[:m]
    return _pack(o, d), np.full(n, -1)


def _silhouette(sc, rng, n, eps):
    sph = np.flatnonzero((sc.tag == 0) & ~sc.giant)
    r_all = sc.shape[sph, 3]
    small = r_all < 0.02 * sc.s                                          # ratio: half of the targets among the tiny spheres
    weight = None
    if small.any():
        weight = np.where(small, 0.5 / small.sum(), 0.5 / (~small).sum())
    t = _targets(rng, sph, n, weight)
    c, r = sc.shape[t, 0:3], sc.shape[t, 3:4]
    o = _f32(c + r * rng.uniform(2.0, 6.0, (n, 1)) * _unit(rng.normal(size=(n, 3))))
    co = c - o
    D = np.linalg.norm(co, axis=1, keepdims=True)
    u = _unit(np.cross(co, rng.normal(size=(n, 3))))
    aim = c + r * D / np.sqrt(D * D - r * r) * u + r * eps * rng.normal(size=(n, 3))
    return _pack(o, aim - o), t


def _face(sc, rng, n, eps):
    """Origin on a box face of a sphere (o_k = c_k +- r as f32 computes it), d_k = 0, aimed at the touching point.  The plane the
    ray lies in is the f32 value P of c_k +- r, at r_p = |P - c_k| from the centre.  With r_p > r no ray in it hits; with
    r_p < r the sphere reaches through the plane by a sliver of half-width L = sqrt(r^2 - r_p^2), and a ray hits if it passes
    within L of the touching point: hits that exist through the rounding of one addition.  Under an offset (r_p - r up to half
    an ulp of the offset) L is mostly a hundred eps wide and nothing is left to straddle, so the targets are the N_TARGETS
    faces with the thinnest slivers: those the jitter does straddle."""
    sph = np.flatnonzero((sc.tag == 0) & ~sc.giant)
    sph = sph[np.unique(sc.group[sph], return_index=True)[1]]           # one of a set of coincident copies
    cand = np.array([(i, k, sg) for i in sph for k in range(3) for sg in (-1.0, 1.0)])
    ci, ck, cs = cand[:, 0].astype(np.int64), cand[:, 1].astype(np.int64), cand[:, 2]
    c_k, r_c = sc.shape[ci, ck], sc.shape[ci, 3]
    plane = (c_k.astype(np.float32) + (cs * r_c).astype(np.float32)).astype(np.float64)
    sliver = (r_c - np.abs(plane - c_k)) / r_c
    best = np.flatnonzero(sliver > 0.0)
    best = best[np.argsort(sliver[best], kind="stable")][:N_TARGETS]
    pick = np.repeat(best, -(-n // len(best)))[:n]
    t, k, sign = ci[pick], ck[pick], cs[pick]
    c, r = sc.shape[t, 0:3], sc.shape[t, 3:4]
    rows = np.arange(n)
    w = rng.normal(size=(n, 3))
    w[rows, k] = 0.0
    w = _unit(w)
    touch = c.copy()
    touch[rows, k] += sign * r[:, 0]
    o = _f32(touch + r * rng.uniform(2.0, 6.0, (n, 1)) * w)
    o[rows, k] = plane[pick]
    g = rng.normal(size=(n, 3))
    g[rows, k] = 0.0
    L = np.sqrt(r * r - (plane[pick] - c[rows, k])[:, None] ** 2)
    aim = touch + L * eps * g                                            # even rays: at the touching point, jitter of the sliver's size
    perp = np.cross(np.eye(3)[k], w) * rng.choice([-1.0, 1.0], (n, 1))
    rim = touch + L * perp + L * EPS_RIM * g                             # odd rays: at the sliver's rim, where hit turns into miss
    aim[1::2] = rim[1::2]
    d = aim - o
    d[rows, k] = 0.0
    return _pack(o, d), t


def _edge(sc, rng, n, eps):
    v = sc.shape.reshape(-1, 3, 3)
    tri = np.flatnonzero((sc.tag == 1) & sc.hittable())
    if len(tri) == 0:
        return None
    t = _targets(rng, tri, n)
    a = rng.integers(0, 3, n)
    b = (a + 1 + rng.integers(0, 2, n)) % 3
    va, vb = v[t, a], v[t, b]
    lam = rng.uniform(0.0, 1.0, (n, 1))
    lam[rng.uniform(size=n) < 0.2] = 0.0                                 # a fifth at the vertex itself
    p = (1.0 - lam) * va + lam * vb
    lo, hi = sc.core_bounds()
    ext = (hi - lo).max()
    nrm = _unit(np.cross(v[t, 1] - v[t, 0], v[t, 2] - v[t, 0]))
    side = rng.choice([-1.0, 1.0], (n, 1))
    o = _f32(p + ext * rng.uniform(0.1, 0.5, (n, 1)) * _unit(side * nrm + 0.7 * rng.normal(size=(n, 3))))
    length = np.linalg.norm(vb - va, axis=1, keepdims=True)
    aim = p + eps * length * rng.normal(size=(n, 3))
    return _pack(o, aim - o), t


def _inplane(sc, rng, n):
    """flat families: rays lying exactly in a plane of triangles (origin and direction), and rays that only start in one"""
    v = sc.shape.reshape(-1, 3, 3)
    t = rng.choice(np.flatnonzero(sc.tag == 1), n)
    w = rng.dirichlet([1.0, 1.0, 1.0], n)
    o = _f32((w[:, :, None] * v[t]).sum(axis=1))
    k = np.argmin(np.ptp(v[t], axis=1), axis=1)                          # the plane's axis: zero extent over the triangle
    rows = np.arange(n)
    o[rows, k] = v[t, 0][rows, k]
    d = rng.normal(size=(n, 3))
    d[rows[: n // 2], k[: n // 2]] = 0.0
    far = rows[: n // 8]                                                 # some of them from outside the quads
    lo, hi = sc.core_bounds()
    o[far] = _f32(o[far] - 3.0 * (hi - lo).max() * _unit(d[far]))
    return _pack(o, d), np.full(n, -1)


def _stack(sc, rng, n):
    t = rng.integers(0, len(sc), n)
    p = sc.corners()[t]
    w = rng.dirichlet([1.0, 1.0, 1.0], n)
    sph = (sc.tag[t] == 0)[:, None]
    r = np.where(sph[:, 0], sc.shape[t, 3], 0.0)[:, None]
    ball = _unit(rng.normal(size=(n, 3))) * rng.uniform(0.0, 0.9, (n, 1)) ** (1.0 / 3.0)
    inside = np.where(sph, p[:, 1] + r * ball, (w[:, :, None] * p).sum(axis=1))
    lo, hi = sc.core_bounds()
    o = _f32(rng.uniform(lo - 0.3 * (hi - lo), hi + 0.3 * (hi - lo), (n, 3)))
    d = inside - o
    h = n // 3                                                           # a third start inside a sphere (the concentric sets: between shells)
    s_idx = np.flatnonzero(sc.tag == 0)
    ts = rng.choice(s_idx, h)
    o[:h] = _f32(sc.shape[ts, 0:3] + sc.shape[ts, 3:4] * _unit(rng.normal(size=(h, 3))) * rng.uniform(0.0, 0.95, (h, 1)))
    d[:h] = rng.normal(size=(h, 3))
    return _pack(o, d), np.full(n, -1)


def ray_sets(sc, seed=1):
    """-> {name: (rays f64[n, 6] of f32 values, target i64[n] or -1)}"""
    rng = np.random.default_rng(seed + 17 * FAMILIES.index(sc.family))
    eps = EPS[sc.family]
    stacked = sc.family == "stacked"                                     # its stack rays come out of the random set's share
    out = {"random": _random(sc, rng, N_RAYS["random"] - (N_RAYS["stack"] if stacked else 0))}
    if ((sc.tag == 0) & ~sc.giant).any():
        out["silhouette"] = _silhouette(sc, rng, N_RAYS["silhouette"], eps["silhouette"])
        out["face"] = _face(sc, rng, N_RAYS["face"], eps["face"])
        out["edge"] = _edge(sc, rng, N_RAYS["edge"], eps["edge"])
    else:
        out["edge"] = _edge(sc, rng, N_RAYS["edge"] + N_RAYS["silhouette"], eps["edge"])
        out["inplane"] = _inplane(sc, rng, N_RAYS["face"])
    if stacked:
        out["stack"] = _stack(sc, rng, N_RAYS["stack"])
    return {k: v for k, v in out.items() if v is not None}


def all_rays(sets):
    return np.concatenate([r for r, _ in sets.values()], axis=0)


def oracle_rays(sets):
    """N_ORACLE rays of a case, every set represented"""
    per = -(-N_ORACLE // len(sets))
    return np.concatenate([r[:per] for r, _ in sets.values()], axis=0)[:N_ORACLE]
