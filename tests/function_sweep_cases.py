"""Cases of the device-function sweep (tests/test_function_sweep_cpu.py, tests/test_gpu_function_sweep.py).

Deterministic from fixed seeds, numpy only.  Every input a device function receives is an f32 value (pt_debug_* rounds its
f64 arguments), so the rows are rounded to f32 HERE and both oracle precisions and the device see the same numbers.  The
material parameters are not rounded: the f64 oracle takes them as the scene file states them (metallic 0.99 is 0.99, not the
f32 next to it, which lies ABOVE 0.99 and would take the other branch of `metallic > 0.99`).

A cell is one uploaded object.  Bsdf cells share one set of direction rows and draw words; shape cells carry their own
observers.  `bsdf_tables(pt, orc)` and `shape_tables(pt, orc)` evaluate both oracle precisions on every cell once and keep the
result for the session."""
import numpy as np

F64, F32 = 64, 32
SPHERE, TRIANGLE = 0, 1
LAMBERT, EMISSIVE, MIRROR, OREN_NAYAR = 0, 1, 2, 3

N_ROWS = 1024                     # per bsdf cell (the issue allows 2048)
AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)

# row kinds of the direction rows
AXIS, FRAME_EDGE, NORMAL_AXIS, NORMAL_GENERAL, GRAZING, MIRROR_WO, ALONG_N, WORD_EDGE, RANDOM = range(9)
KIND_NAMES = ["axis", "frame_edge", "normal_axis", "normal_general", "grazing", "mirror_wo", "along_n", "word_edge", "random"]


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _perpendicular(n, rng):
    """A random unit vector perpendicular to each row of n (for an axis n its component along n is exactly 0)."""
    t = np.cross(n, rng.normal(size=n.shape))
    return _unit(t)


class DirectionRows:
    """din, nrm (n x 3), wo (n x 3, eval only), eta_inverse (n, bool: eta = 1/ior, else ior), words (n x 4 u32), kind (n)."""

    def __init__(self, seed=20261020, n=N_ROWS):
        rng = np.random.default_rng(seed)
        nrm = _unit(rng.normal(size=(n, 3)))
        din = _unit(rng.normal(size=(n, 3)))
        kind = np.full(n, RANDOM)
        # one quarter of the normals exactly +-x, +-y, +-z
        q = n // 4
        nrm[0:q] = AXES[np.arange(q) % 6]; kind[0:q] = AXIS
        a = q
        # |n.y| over [0.9985, 0.9995]: both sides of frame_of's 0.999
        ny = np.linspace(0.9985, 0.9995, 64) * np.where(np.arange(64) % 2, -1.0, 1.0)
        phi = rng.uniform(0.0, 2.0 * np.pi, 64)
        s = np.sqrt(1.0 - ny * ny)
        nrm[a:a + 64] = np.stack([s * np.cos(phi), ny, s * np.sin(phi)], 1); kind[a:a + 64] = FRAME_EDGE
        a += 64
        nrm[a:a + 64] = AXES[np.arange(64) % 6]; kind[a:a + 64] = NORMAL_AXIS          # d = -n below
        a += 64
        kind[a:a + 64] = NORMAL_GENERAL                                                # d = -n below, any normal
        a += 64
        # grazing incidence, cos(i, n) log-uniform over [1e-7, 1e-2]; half on axis normals, where d.n = -c exactly
        c = 10.0 ** rng.uniform(-7.0, -2.0, 64)
        nrm[a:a + 32] = AXES[np.arange(32) % 6]
        t = _perpendicular(nrm[a:a + 64], rng)
        din[a:a + 64] = -(c[:, None] * nrm[a:a + 64] + np.sqrt(1.0 - c * c)[:, None] * t); kind[a:a + 64] = GRAZING
        a += 64
        # the rest as tests/tools/make_golden.py draws them: the ray arrives from the side the normal faces
        flip = (din * nrm).sum(1) > 0
        din[flip] *= -1
        nrm, din = f32(nrm), f32(din)
        ni = (kind == NORMAL_AXIS) | (kind == NORMAL_GENERAL)
        din[ni] = -nrm[ni]
        wo = _unit(rng.normal(size=(n, 3)))
        kind_eval = kind.copy()
        d_n = (din * nrm).sum(1, keepdims=True)
        wo[a:a + 64] = (din - 2.0 * d_n * nrm)[a:a + 64]; kind_eval[a:a + 64] = MIRROR_WO      # the f64 mirror direction of d
        a += 64
        wo[a:a + 64] = nrm[a:a + 64]; kind_eval[a:a + 64] = ALONG_N
        a += 64
        words = rng.integers(0, 2**32, size=(n, 4), dtype=np.uint64).astype(np.uint32)
        for j in range(6):                                   # r1, r2, lobe at 0 and at 0xFFFFFFFF
            words[a + 8 * j:a + 8 * j + 8, j // 2] = 0 if j % 2 == 0 else 0xFFFFFFFF
        kind[a:a + 48] = WORD_EDGE
        a += 48
        assert a < n - 200
        self.n, self.din, self.nrm, self.wo = n, din, nrm, f32(wo)
        self.kind, self.kind_eval, self.words = kind, kind_eval, words
        self.eta_inverse = rng.uniform(size=n) < 0.5

    def eta(self, ior):
        return f32(np.where(self.eta_inverse, 1.0 / ior, ior))

    def eval_in(self, ior=1.5):
        return np.concatenate([self.din, self.wo, self.nrm, self.eta(ior)[:, None]], 1)

    def sample_in(self, ior=1.5):
        return np.concatenate([self.din, self.nrm, self.eta(ior)[:, None]], 1)


# ------------------------------------------------------------------ material cells
ROUGHNESS = [0.0, 0.02, 0.05, 0.3, 1.0]
METALLIC_ABOVE = float(np.nextafter(np.float32(0.99), np.float32(1.0)))        # the f32 next above 0.99
METALLIC = [0.0, 0.5, 0.99, METALLIC_ABOVE, 1.0]
IOR = [0.75, 1.0, 1.33, 2.4]
GGX_COLOUR = [0.9, 0.7, 0.3]
SIGMA = [0.0, 0.35, 1.0, 10.0]
ALBEDO = [(0.7, 0.7, 0.7), (0.0, 0.0, 0.0), (1.5, 1.0, 0.2)]
LAMBERT_COLOUR = [0.8, 0.6, 0.2]
EMISSIVE_COLOUR = [15.0, 15.0, 15.0]
_UNIT_SPHERE = [0, 0, 0, 1]


class BsdfCell:
    def __init__(self, name, tag, params, ior=1.5, **key):
        self.name, self.tag, self.params, self.ior, self.key = name, tag, list(params), ior, key
        self.spec = (SPHERE, _UNIT_SPHERE, tag, self.params)


def ggx_cells():
    return [BsdfCell(f"ggx r={r:g} m={'0.99+' if m == METALLIC_ABOVE else format(m, 'g')} ior={ior:g}", MIRROR, [r] + GGX_COLOUR + [m, ior],
                     ior=ior, roughness=r, metallic=m)
            for r in ROUGHNESS for m in METALLIC for ior in IOR]


def oren_nayar_cells():
    return [BsdfCell(f"oren_nayar sigma={s:g} albedo={al}", OREN_NAYAR, list(al) + [s], sigma=s, albedo=al) for s in SIGMA for al in ALBEDO]


def lambert_cell(colour=LAMBERT_COLOUR):
    return BsdfCell(f"lambert {tuple(colour)}", LAMBERT, colour)


def emissive_cell():
    return BsdfCell("emissive", EMISSIVE, EMISSIVE_COLOUR)


def bsdf_cells():
    return ggx_cells() + oren_nayar_cells() + [lambert_cell(), emissive_cell()]


# decisions of a sample row (wo3, f3, pdf, cos): the failure tuple (mirror.rs:216: wo = n, f = 0, pdf = 1, cos = 0) and the side of wo
def failed(out, nrm):
    out = np.asarray(out, dtype=np.float64)
    return (out[:, 3:6] == 0).all(1) & (out[:, 6] == 1.0) & (out[:, 7] == 0.0) & (out[:, 0:3] == nrm).all(1)


def side(out, nrm):
    return np.sign((np.asarray(out, dtype=np.float64)[:, 0:3] * nrm).sum(1))


def same_decision(a, b, nrm):
    fa, fb = failed(a, nrm), failed(b, nrm)
    return (fa == fb) & (fa | (side(a, nrm) == side(b, nrm)))


def _row_max(e):
    e = np.where(np.isnan(e), np.inf, e)             # a NaN against a finite reference is an infinite error
    return e.reshape(len(e), int(np.prod(e.shape[1:]))).max(1, initial=0.0)


def rel_err(got, ref, floor=1e-5):
    """Per row: max over the columns of |got - ref| / max(|ref|, floor)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.abs(got - ref) / np.maximum(np.abs(ref), floor)
    return _row_max(e)


def abs_err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        e = np.abs(got - ref)
    return _row_max(e)


def quantiles(e):
    """median and 99th percentile of an error list (0, 0 for an empty one)."""
    if len(e) == 0:
        return 0.0, 0.0
    return float(np.quantile(e, 0.5, method="higher")), float(np.quantile(e, 0.99, method="higher"))


# ------------------------------------------------------------------ shape cells
# The f32 point a sampler returns is only good to half an ulp of its coordinates.  The centre lies within 0.4 of the origin so
# that this is 1.5e-8 = 3e-6 of the smallest radius, below the 1e-5 r the inside test asks of point = from + dir * dist;
# no coordinate is zero, so center - from still cancels.
SPHERE_CENTRE = np.array([0.25, -0.125, 0.375])
RADII = [0.005, 0.2, 5.0, 100.0]
AT_CENTRE, INSIDE, SKIN, OUTSIDE = "centre", "inside", "skin", "outside"
_GRID = 2.0 ** 24


def _r12(rng, n):
    k = rng.integers(0, 2**23, size=(n, 2)).astype(np.float64)
    k[0] = [0, 0]; k[1] = [2**23 - 1, 2**23 - 1]; k[2] = [0, 2**23 - 1]; k[3] = [2**23 - 1, 0]     # first and last grid points
    return (2 * k + 1) / _GRID          # the generator's open-interval grid, exact in f32


class ShapeCell:
    """frm (n x 3) observers, r12 (n x 2), target (n x 3: a point of the light, for the with-target form)."""

    def __init__(self, name, spec, frm, r12, target, scale, **key):
        self.name, self.spec, self.frm, self.r12, self.target, self.scale, self.key = name, spec, f32(frm), r12, f32(target), scale, key
        self.n = len(self.frm)


def sphere_cells(seed=20261021):
    rng = np.random.default_rng(seed)
    cells = []
    for r in f32(RADII):                  # shape records are f32 values: both oracle precisions see the same light
        for where, n in ((AT_CENTRE, 16), (INSIDE, 256), (SKIN, 256), (OUTSIDE, 256)):
            if where == AT_CENTRE:
                d = np.zeros(n)
            elif where == INSIDE:
                d = r * rng.uniform(0.1, 0.999, n)
            elif where == SKIN:
                d = r * (1.0 + 10.0 ** rng.uniform(-4.0, -2.0, n))
            else:
                d = r * (1.0 + 10.0 ** rng.uniform(-2.0, 3.0, n))
            frm = SPHERE_CENTRE + d[:, None] * _unit(rng.normal(size=(n, 3)))
            pole = np.arange(n) % 8 == 0                      # straight above / below the centre: frame_of's axis branch
            frm[pole] = SPHERE_CENTRE + d[pole, None] * np.where(np.arange(n) % 16 == 0, 1.0, -1.0)[pole, None] * AXES[2]
            target = SPHERE_CENTRE + r * _unit(rng.normal(size=(n, 3)))
            cells.append(ShapeCell(f"sphere r={r:g} {where}", (SPHERE, list(SPHERE_CENTRE) + [float(f32(r))], EMISSIVE, [36.0] * 3), frm, _r12(rng, n),
                                   target, r, radius=r, where=where))
    return cells


# All four triangles lie in an axis plane, so their unit normal is exact in every arithmetic and "in the plane" is exact too.
TRIANGLES = {
    "golden": [-0.3, 0.99, -2.3, 0.3, 0.99, -2.3, 0.3, 0.99, -1.7],
    "sliver": [-0.3, 0.99, -2.3, 0.3, 0.99, -2.3, 0.3, 0.99, -2.3 + 1e-4],            # the same base, height 1e-4
    "tiny": [0.5, 0.25, -1.5, 0.5, 0.25 + 1e-4, -1.5, 0.5, 0.25, -1.5 + 1e-4],          # 1e-4 across, in the plane x = 0.5
    "large": [-25.0, -10.0, -3.0, 25.0, -10.0, -3.0, 0.0, 33.0, -3.0],                  # edges of about 50, in the plane z = -3
}
RANDOM_OBS, IN_PLANE, NEAR_PLANE, AT_SAMPLE = "random", "in_plane", "near_plane", "at_sample"


def triangle_point(v, r12, dtype=np.float64):
    """TriangleShape::sample_surface_from_point's point (shape.rs:215-219).  dtype = float32: the f32 specification's value,
    v0 + e1*u then + e2*v with one rounding per fma (pt_oracle.hpp triangle_sample), evaluated in f64 and rounded, which is
    exact for an fma of f32 operands."""
    v = np.asarray(v, dtype=np.float64).reshape(3, 3)
    if dtype == np.float32:
        v = f32(v)
        e1, e2 = f32(v[1] - v[0]), f32(v[2] - v[0])
        s = np.sqrt(r12[:, 0].astype(np.float32)).astype(np.float64)
        u, w = f32(1.0 - s), f32(r12[:, 1] * s)
        return f32(e2 * w[:, None] + f32(e1 * u[:, None] + v[0]))
    s = np.sqrt(r12[:, 0])
    return v[0] + (v[1] - v[0]) * (1.0 - s)[:, None] + (v[2] - v[0]) * (r12[:, 1] * s)[:, None]


def triangle_cells(seed=20261022):
    rng = np.random.default_rng(seed)
    cells = []
    for name, v in TRIANGLES.items():
        v = [float(x) for x in f32(v)]
        vv = np.asarray(v).reshape(3, 3)
        e1, e2 = vv[1] - vv[0], vv[2] - vv[0]
        nrm = _unit(np.cross(e1, e2))
        edge = max(np.linalg.norm(e1), np.linalg.norm(e2), np.linalg.norm(vv[2] - vv[1]))
        reach = max(edge, 1.0)
        for where, n in ((RANDOM_OBS, 256), (IN_PLANE, 64), (NEAR_PLANE, 64), (AT_SAMPLE, 16)):
            r12 = _r12(rng, n)
            in_plane = vv[0] + rng.uniform(-2.0, 3.0, (n, 1)) * e1 + rng.uniform(-2.0, 3.0, (n, 1)) * e2
            if where == RANDOM_OBS:
                frm = vv.mean(0) + rng.uniform(-1.0, 1.0, (n, 3)) * reach
            elif where == IN_PLANE:
                frm = in_plane
            elif where == NEAR_PLANE:
                frm = in_plane + nrm * (rng.uniform(0.0, 1e-6, (n, 1)) * np.where(rng.uniform(size=(n, 1)) < 0.5, -1.0, 1.0))
            else:
                frm = triangle_point(v, r12, np.float32)          # the f32-rounded sampled point: d == 0 in exact arithmetic
            target = triangle_point(v, _r12(rng, n))
            cells.append(ShapeCell(f"triangle {name} {where}", (TRIANGLE, list(v), EMISSIVE, [15.0] * 3), frm, r12, target, edge,
                                   triangle=name, where=where))
    return cells


def shape_cells():
    return sphere_cells() + triangle_cells()


# ------------------------------------------------------------------ both oracles on every cell, once per session
class BsdfTable:
    """ev32, ev64 (n x 4), sm32, sm64 (n x 8) of one cell, its decision statistics and the f32 oracle's error quantiles."""
    pass


_TABLES = {}


def rows():
    if "rows" not in _TABLES:
        _TABLES["rows"] = DirectionRows()
    return _TABLES["rows"]


def included(kind):
    """Rows that enter a tolerance comparison: all but normal incidence on a general normal (test_function_sweep_cpu.py
    shows why: the two precisions get a different tangent-plane azimuth there, and the sampled half vector with it)."""
    return kind != NORMAL_GENERAL


def bsdf_tables(pt, orc):
    if "bsdf" in _TABLES:
        return _TABLES["bsdf"]
    R = rows()
    out = {}
    for cell in bsdf_cells():
        ob = pt.make_objects([cell.spec])
        t = BsdfTable()
        t.cell = cell
        t.eval_in, t.sample_in = R.eval_in(cell.ior), R.sample_in(cell.ior)
        t.ev64, t.ev32 = orc.bsdf_eval(ob, t.eval_in, F64), orc.bsdf_eval(ob, t.eval_in, F32)
        t.sm64, t.sm32 = orc.bsdf_sample(ob, t.sample_in, R.words, F64), orc.bsdf_sample(ob, t.sample_in, R.words, F32)
        t.agree32 = same_decision(t.sm32, t.sm64, R.nrm)
        t.share32 = float(t.agree32.mean())
        t.stable = t.share32 >= 0.99
        t.finite64 = np.isfinite(t.sm64).all(1)
        t.ev_finite64 = np.isfinite(t.ev64).all(1)
        for a in (t.ev64, t.ev32, t.sm64, t.sm32):
            a.setflags(write=False)
        out[cell.name] = t
    _TABLES["bsdf"] = out
    return out


class ShapeTable:
    pass


def shape_tables(pt, orc):
    if "shape" in _TABLES:
        return _TABLES["shape"]
    out = {}
    for cell in shape_cells():
        ob = pt.make_objects([cell.spec])
        t = ShapeTable()
        t.cell = cell
        t.s64, t.s32 = orc.shape_sample(ob, cell.frm, None, cell.r12, F64), orc.shape_sample(ob, cell.frm, None, cell.r12, F32)
        t.t64, t.t32 = orc.shape_sample(ob, cell.frm, cell.target, None, F64), orc.shape_sample(ob, cell.frm, cell.target, None, F32)
        for a in (t.s64, t.s32, t.t64, t.t32):
            a.setflags(write=False)
        out[cell.name] = t
    _TABLES["shape"] = out
    return out


# columns of orc.shape_sample (point3 normal3 pdf dir3 dist) in the order of debug_shape_sample (point3 pdf dir3 dist)
DEVICE_COLUMNS = [0, 1, 2, 6, 7, 8, 9, 10]
