"""Named inputs of the a-trous filter at the edges of what its argument checks admit: images smaller than the
step, one pixel wide, strips; every sigma exactly 0 or near FLT_MAX; variance 0, huge, denormal, not given; miss pixels,
emitters, orthogonal normals, albedo and depth under their floors; negative, large, NaN and infinite film values.

A case is (film f32[H,W,3], features f32[H,W,8], the PtDenoise fields, a variance plane f32[H,W] or None).  tests/
test_atrous_cases_cpu.py holds the table to its admission condition and to closed forms; tests/test_gpu_atrous_cases.py
holds pt_denoise_device / pt_denoise_var_device to the f64 restatement (tests/denoise_ref.py) on every case.

Conditioning.  With g_p = 0 or sigma_l = 0 the luminance stop is 1e10 per unit of L, with sigma_d = 0 the depth stop is:
a difference of one f32 ulp decides a weight.  So the inputs come from a palette: film k/64, albedo in {1/4, 1/2, 1},
depth k/8, normals (0,0,1), (0.6,0,0.8), (0,0.6,0.8) (pairwise n.n' > 0) and, where a case says so, (1,0,0), (0,0,-1) and the miss
record's 0.  A difference of two inputs is then 0 or at least 1/256, a stopped weight exactly k or exactly 0 in f32 and in f64,
and what the iterations make of the palette differs by roundings only where the values that a weight mixes differ by as
little (a weight's error e^-D 1e10 dD moves the sum by D times that, at most dD / e).

Admission condition: the restatement evaluated with every array in f32 stays within ADMIT = 2.5e-5 of its f64 evaluation
(max |a - b| / max(|b|, 1e-3) over the finite entries) with the same non-finite mask: a quarter of the 1e-4 the device is
held to.  Measured, worst per family (f32 restatement against f64 | MI355X against f64):
    size      9.7e-06 | 9.6e-06
    steps     9.6e-06 | 9.2e-06
    sigma     5.8e-06 | 5.8e-06
    variance  6.5e-06 | 6.7e-06
    features  1.0e-05 | 1.0e-05
    film      7.7e-06 | 7.5e-06
Tried and not admitted: a half of constant film (var = 0, g_p = 0) beside a noisy half, 4.4e-3.  Where g_p = 0, var' = sum w^2
var_q / (sum w)^2 takes var_q > 0 from a neighbour whose u differs from u_p by less than an f32 ulp with a weight between 0
and k that this difference decides, and the next step's stop follows: the rule itself is ill-conditioned there in f32, and
no statement about the device can be made at 1e-4.  A film of both signs is not admitted either (4.9e-4): the measure is
relative and its floor of 1e-3 is far under the values that cancel; film_negative is negative throughout.
"""
import functools
import zlib
from collections import namedtuple

import numpy as np

import denoise_ref as dr

ADMIT = 2.5e-5
Case = namedtuple("Case", "name family film feat dn var")

NORMALS = np.array([(0.0, 0.0, 1.0), (0.6, 0.0, 0.8), (0.0, 0.6, 0.8)], np.float32)
MISS = np.array([1, 1, 1, 0, 0, 0, 0, 0], np.float32)
OFF = dict(sigma_l=3.0e38, sigma_n=0.0, sigma_d=3.0e38)          # every stop off (where g_p > 0)
SIZES = [(1, 1), (1, 2), (2, 1), (1, 9), (9, 1), (2, 3), (3, 2), (5, 7), (7, 5), (7, 31), (31, 7), (9, 33), (33, 9), (8, 32),
         (32, 8), (1, 4096), (4096, 1)]                          # (H, W): both readings of "31 x 7"; grids 128 x 1 and 1 x 512


def max_rel(got, ref):
    """The project's error measure (tests/test_gpu_denoise.py: _max_rel) over the entries finite in ref."""
    ok = np.isfinite(ref)
    if not ok.any():
        return 0.0
    got, ref = np.asarray(got, np.float64)[ok], np.asarray(ref, np.float64)[ok]
    with np.errstate(invalid="ignore"):
        return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-3)))


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def palette_film(rng, H, W, lo=0, hi=64):
    return (rng.integers(lo, hi + 1, (H, W, 3)) / 64.0).astype(np.float32)


def surface(rng, H, W):
    """Surface records: albedo in {1/4, 1/2, 1} per channel, one of NORMALS, depth k/8 in [1, 3]."""
    f = np.zeros((H, W, 8), np.float32)
    f[..., 0:3] = rng.choice(np.array([0.25, 0.5, 1.0], np.float32), (H, W, 3))
    f[..., 4:7] = NORMALS[rng.integers(0, 3, (H, W))]
    f[..., 7] = rng.integers(8, 25, (H, W)) / 8.0
    return f


def checker(H, W):
    ys, xs = np.mgrid[0:H, 0:W]
    return (ys + xs) % 2 == 1


def _build():
    cases = []

    def add(name, family, film, feat, var=None, **dn):
        d = dict(iterations=5, sigma_l=4.0, sigma_n=128.0, sigma_d=0.025)
        d.update(dn)
        cases.append(Case(name, family, np.ascontiguousarray(film, np.float32), np.ascontiguousarray(feat, np.float32), d,
                          None if var is None else np.ascontiguousarray(var, np.float32)))

    def rnd(name, H, W):
        r = _rng(name)
        return r, palette_film(r, H, W), surface(r, H, W)

    # ---- sizes: default sigmas, 5 iterations (steps 1 .. 16)
    for H, W in SIZES:
        _, c, f = rnd(f"size_{H}x{W}", H, W)
        add(f"size_{H}x{W}", "size", c, f)
    # ---- steps larger than the image (step 2^15 at 16 iterations); the strips at 12: steps up to 2048 land inside
    for H, W in ((5, 7), (9, 33)):
        _, c, f = rnd(f"steps_{H}x{W}", H, W)
        for it in (6, 12, 16):
            add(f"steps_{H}x{W}_it{it}", "steps", c, f, iterations=it)
    for H, W in ((1, 4096), (4096, 1), (2, 512)):
        _, c, f = rnd(f"steps_{H}x{W}", H, W)
        add(f"steps_{H}x{W}_it12", "steps", c, f, iterations=12)
    # ---- sigmas
    sig = dict(sl0=dict(sigma_l=0.0), sn0=dict(sigma_n=0.0), sd0=dict(sigma_d=0.0), all0=dict(sigma_l=0.0, sigma_n=0.0, sigma_d=0.0),
               off=OFF, sn1=dict(sigma_n=1.0))
    for (H, W), it in (((9, 33), 5), ((5, 7), 12), ((1, 9), 5), ((1, 512), 12), ((512, 1), 12)):
        _, c, f = rnd(f"sigma_{H}x{W}", H, W)
        for k, v in sig.items():
            add(f"sigma_{k}_{H}x{W}_it{it}", "sigma", c, f, iterations=it, **v)
    # (a stop of 1e10 that lets nothing through: all luminances, or all depths, of the image differ by 1/64 or more)
    for H, W in ((5, 7), (9, 33)):
        r, c, f = rnd(f"distinct_{H}x{W}", H, W)
        k = r.permutation(H * W).reshape(H, W) + 1
        grey = np.repeat((k / 64.0)[..., None], 3, -1)
        fl = f.copy()
        fl[..., 0:3] = 0.5
        add(f"sigma_sl0_distinct_{H}x{W}", "sigma", grey, fl, sigma_l=0.0)
        fd = f.copy()
        fd[..., 7] = (k + 7) / 8.0
        add(f"sigma_sd0_distinct_{H}x{W}", "sigma", c, fd, sigma_d=0.0)
    # ---- variance
    for H, W in ((9, 33), (1, 9), (1, 4096), (4096, 1)):
        r = _rng(f"var_const_{H}x{W}")
        f = surface(r, H, W)
        f[..., 0:3] = 0.5
        add(f"var_const_{H}x{W}", "variance", np.full((H, W, 3), 0.375, np.float32), f)
    r = _rng("var_blocks3")
    f = surface(r, 9, 33)
    f[..., 0:3] = 0.5
    add("var_blocks3", "variance", np.kron(palette_film(r, 3, 11).transpose(2, 0, 1), np.ones((3, 3), np.float32)).transpose(1, 2, 0), f)
    # (g_p = 0 beside non-zero differences at every pixel and step: the all-zero planes below)
    for H, W in ((9, 33), (5, 7), (1, 9)):
        r, c, f = rnd(f"var_plane_{H}x{W}", H, W)
        mixed = (2.0 ** -r.integers(0, 12, (H, W))).astype(np.float32)
        kind = r.integers(0, 6, (H, W))
        mixed[kind == 0] = np.nan
        mixed[kind == 1] = -1.0
        mixed[kind == 2] = np.inf
        for k, v in (("zero", np.zeros((H, W))), ("1e30", np.full((H, W), 1e30)), ("denormal", np.full((H, W), 1e-42)), ("mixed", mixed)):
            add(f"var_plane_{k}_{H}x{W}", "variance", c, f, var=v)
    # ---- features
    H, W = 9, 33
    for tag, dn in (("", {}), ("_sn0", dict(sigma_n=0.0))):
        r, c, f = rnd("feat_miss_checker", H, W)
        f[checker(H, W)] = MISS
        add("feat_miss_checker" + tag, "features", c, f, **dn)
        r, c, f = rnd("feat_miss_halves", H, W)
        f[:, :16] = MISS
        add("feat_miss_halves" + tag, "features", c, f, **dn)
        r, c, f = rnd("feat_ortho_halves", H, W)
        f[:, :16, 4:7] = (1.0, 0.0, 0.0)
        f[:, 16:, 4:7] = (0.0, 0.0, 1.0)
        c[:, :16] = 0.0
        add("feat_ortho_halves" + tag, "features", c, f, **dn)
        r, c, f = rnd("feat_opposite_checker", H, W)
        f[..., 4:7] = (0.0, 0.0, 1.0)
        f[checker(H, W), 6] = -1.0
        add("feat_opposite_checker" + tag, "features", c, f, **dn)
    r, c, f = rnd("feat_emitter_quarter", H, W)
    f[2:6, 5:12, 3] = 0.25
    f[7, 20, 3] = 0.25
    add("feat_emitter_quarter", "features", c, f)
    r, c, f = rnd("feat_albedo_zero", H, W)
    f[:, 10:20, 0:3] = 0.0
    f[checker(H, W), 1] = 0.0
    add("feat_albedo_zero", "features", c, f)
    r, c, f = rnd("feat_albedo_tiny", H, W)
    f[:, 10:20, 0:3] = 5e-4
    add("feat_albedo_tiny", "features", c, f)
    r, c, f = rnd("feat_depth_zero", H, W)
    f[checker(H, W) & (np.mgrid[0:H, 0:W][1] < 16), 7] = 0.0
    add("feat_depth_zero", "features", c, f)
    r, c, f = rnd("feat_depth_tiny", H, W)
    f[:, :16, 7] = 1e-4
    f[4, 3:9, 7] = 0.0
    add("feat_depth_tiny", "features", c, f)
    # ---- film values
    r, c, f = rnd("film_negative", H, W)
    add("film_negative", "film", palette_film(r, H, W, -64, -1), f)   # (no zero crossings: the error measure is relative)
    r, c, f = rnd("film_large", H, W)
    add("film_large", "film", c * np.float32(2.0 ** r.integers(0, 5, (H, W, 1))) * np.float32(64.0), f)    # up to 2^10
    r, c, f = rnd("film_nan_surface", H, W)                       # a wall of normal (1,0,0) in columns 20 .. 23 stops the NaN
    f[:, 20:24, 4:7] = (1.0, 0.0, 0.0)
    c[4, 8, 0] = np.nan
    add("film_nan_surface", "film", c, f, iterations=2)
    add("film_nan_surface_it5", "film", c, f)
    r, c, f = rnd("film_nan_emitter", H, W)                       # a single emitter pixel among surfaces
    f[4, 8, 3] = 1.0
    c[4, 8, 1] = np.nan
    add("film_nan_emitter", "film", c, f, iterations=2)
    r, c, f = rnd("film_nan_emitter_block", H, W)                 # the centre of a 5 x 5 emitter
    f[2:7, 6:11, 3] = 1.0
    c[4, 8, 1] = np.nan
    add("film_nan_emitter_block", "film", c, f)
    r, c, f = rnd("film_nan_miss_edge", H, W)                     # a miss pixel beside a surface
    f[:, :16] = MISS
    c[4, 15, 2] = np.nan
    add("film_nan_miss_edge", "film", c, f, iterations=2)
    r, c, f = rnd("film_nan_miss_deep", H, W)                     # a miss pixel three pixels from the surface
    f[:, :16] = MISS
    c[4, 12, 2] = np.nan
    add("film_nan_miss_deep", "film", c, f)
    r, c, f = rnd("film_inf_surface", H, W)
    f[:, 20:24, 4:7] = (1.0, 0.0, 0.0)
    c[4, 8, 0] = np.inf
    add("film_inf_surface", "film", c, f, iterations=2)
    return cases


CASES = _build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
NAMES = [c.name for c in CASES]
FAMILIES = ("size", "steps", "sigma", "variance", "features", "film")


def evaluate(case, dtype=np.float64, **override):
    """The restatement on a case -> linear dtype[H,W,3]."""
    return dr.denoise(case.film, case.feat, dtype=dtype, var=case.var, **dict(case.dn, **override))


@functools.lru_cache(maxsize=None)
def reference(name):
    """The f64 restatement of case `name`, computed once (read-only)."""
    ref = evaluate(BY_NAME[name])
    ref.setflags(write=False)
    return ref


def nonfinite_mask(name):
    """The entries of the output that the rule makes NaN or infinite."""
    return ~np.isfinite(reference(name))


def untouched(case):
    """The pixels no iteration changes: emitters, and pixels without a tap of n_p.n_q > 0 anywhere (every miss pixel)."""
    f = case.feat
    return (f[..., 3] > 0) | ~(f[..., 4:7] != 0).any(-1)


def nan_footprint(case):
    """Where the rule makes the output NaN, from the rule's structure alone (no arithmetic): a NaN in L(u) makes the 3 x 3
    variance around it NaN, whatever the classes of the pixels; a pixel with at least one tap that is not excluded turns NaN
    when its own u, its g_p (the 3 x 3 of var) or the u of such a tap is NaN; an emitter and a pixel all of whose taps are
    excluded keep (u, var).  -> bool[H,W,3]"""
    def dilate(m):
        out = m.copy()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                out |= dr._shift(m, dy, dx)[0]
        return out

    f = case.feat.astype(np.float64)
    bad_u = np.isnan(case.film)
    bad_v = dilate(bad_u.any(-1))
    if case.var is not None:
        with np.errstate(invalid="ignore"):
            bad_v &= ~(np.isfinite(case.var) & (case.var >= 0))
    for i in range(case.dn["iterations"]):
        h = 1 << i
        bad_g = dilate(bad_v)
        bad_p = bad_u.any(-1)
        taps = np.zeros(bad_p.shape, bool)
        from_q = np.zeros(bad_p.shape, bool)
        var_q = np.zeros(bad_p.shape, bool)
        for j in range(-2, 3):
            for k in range(-2, 3):
                if j == 0 and k == 0:
                    continue
                out, _ = dr.excluded(f, j * h, k * h)
                taps |= ~out
                from_q |= ~out & dr._shift(bad_p, j * h, k * h)[0]
                var_q |= ~out & dr._shift(bad_v, j * h, k * h)[0]
        hit = taps & (bad_p | bad_g | from_q)
        bad_u = bad_u | hit[..., None]
        bad_v = bad_v | hit | (taps & var_q)
    return bad_u
